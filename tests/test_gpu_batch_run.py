"""-m gpu: closed-loop episodes of the MPPI batches on the device (CtkMppiBatch.closed_loop / CtkMppiMlpBatch.closed_loop; ctk_batch_run,
ctk_batch_plant_*; kernel ctk_batch_plant<ENV> between the launches of ctk_mppi_batch<ENV, LOG>).

Two kinds of comparison.  Against the ORACLE (its float32 Predictor.step with the plant's parameters), at the project's trajectory
bound rtol 1e-4 / atol 2e-5 through margins.close: the plant kernel alone (1), and every realised transition of a run (2) — a plant that
read a stale input or the wrong record fails the latter.  Against the LOOP `u = step(S); S = plant_step(S, u)` on a second batch with
the same seeds, assert_array_equal throughout (3 - 6): the contract of run().  Sizes, start states and overrides: batch_run_cases.py."""
import numpy as np
import pytest

import batch_run_cases as K
from oracle import ctk_oracle as O
from control_toolkit_amd import CtkMppiBatch, CtkMppiMlpBatch
from margins import close

pytestmark = pytest.mark.gpu


def make(env, n=K.B, materialize=False):
    return CtkMppiBatch(n, seeds=K.seeds(n), **K.batch_kwargs(env, materialize))


def loop(batch, S0, steps, u_prev=None, ids=None, plant_substeps=None):
    """the loop run() replaces, on the same entry points a caller would use"""
    n = S0.shape[0]
    states, inputs = np.empty((n, steps + 1, batch.S), np.float32), np.empty((n, steps, batch.C), np.float32)
    states[:, 0] = S0
    for k in range(steps):
        inputs[:, k] = batch.step(states[:, k], u_prev=u_prev if k == 0 else None, ids=ids)
        states[:, k + 1] = batch.closed_loop.plant_step(states[:, k], inputs[:, k], ids=ids, plant_substeps=plant_substeps)
    return states, inputs


def same_controllers(a, b, materialize, tag):
    for q in range(a.B):
        np.testing.assert_array_equal(a.read("U_NOM", q), b.read("U_NOM", q), err_msg=f"{tag}: U_NOM of problem {q}")
        np.testing.assert_array_equal(a.read("J", q), b.read("J", q), err_msg=f"{tag}: J of problem {q}")
        np.testing.assert_array_equal(a.get_state(q), b.get_state(q), err_msg=f"{tag}: state vector of problem {q}")
        assert a.rng_position(q) == b.rng_position(q), f"{tag}: Philox position of problem {q}"
        if materialize:
            np.testing.assert_array_equal(a.read("Q", q), b.read("Q", q), err_msg=f"{tag}: Q of problem {q}")
            np.testing.assert_array_equal(a.read("TRAJ", q), b.read("TRAJ", q), err_msg=f"{tag}: TRAJ of problem {q}")


def same_traces(got, want, tag):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{tag}: inputs")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{tag}: states")


def check_wiring(env, states, inputs, tag, substeps=1, own=None):
    """every realised transition against the oracle's step of (states[:, k], inputs[:, k]) with the plants' parameters"""
    lo, hi = K.limits(env)
    assert np.isfinite(inputs).all() and (inputs >= lo).all() and (inputs <= hi).all(), tag
    for k in range(inputs.shape[1]):
        close(tag, "transition", states[:, k + 1], K.oracle_step(env, states[:, k], inputs[:, k], substeps, own), **K.TRAJ_TOL)


# ---- 1. the plant kernel against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overrides", [False, True])
@pytest.mark.parametrize("substeps", K.SUBSTEPS)
@pytest.mark.parametrize("env", K.ENVS)
def test_plant_step_matches_the_oracle(env, substeps, overrides):
    batch = make(env)
    own = None
    if overrides:
        name, vals = K.override_values(env, K.B)
        batch.closed_loop.set_plant_params(name, vals)
        np.testing.assert_array_equal(batch.closed_loop.get_plant_params(name), vals)
        np.testing.assert_array_equal(batch.get_problem_params(name), np.full(K.B, vals[1], np.float32))      # the controllers keep theirs
        assert batch.params_differ() == 0
        own = {name: vals}
    before = [(batch.get_state(q), batch.rng_position(q)) for q in range(K.B)]
    for r in range(8):                                       # B rows per call: 24 states and inputs per case
        S, U = K.start_states(env, K.B, seed=r), K.uniform_inputs(env, (K.B,), seed=100 + r)
        got = batch.closed_loop.plant_step(S, U, plant_substeps=substeps)
        close(f"plant_step {env} substeps {substeps} {'own plants' if overrides else 'the modelled plant'}", "s_next", got,
              K.oracle_step(env, S, U, substeps, own), **K.TRAJ_TOL)
    # a subset, in the order of ids
    S, U = K.start_states(env, K.B, seed=9), K.uniform_inputs(env, (K.B,), seed=109)
    np.testing.assert_array_equal(batch.closed_loop.plant_step(S[[0, 2]], U[[0, 2]], ids=[0, 2], plant_substeps=substeps),
                                  batch.closed_loop.plant_step(S, U, plant_substeps=substeps)[[0, 2]])
    for q, (st, pos) in enumerate(before):                   # no controller state or Philox position moved
        np.testing.assert_array_equal(batch.get_state(q), st)
        assert batch.rng_position(q) == pos
    if overrides:
        batch.closed_loop.clear_plant_params()
        close(f"plant_step {env} substeps {substeps} overrides cleared", "s_next", batch.closed_loop.plant_step(S, U, plant_substeps=substeps),
              K.oracle_step(env, S, U, substeps), **K.TRAJ_TOL)
    batch.close()


# ---- 2. the wiring of a run -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", K.ENVS)
def test_run_transitions_match_the_oracle(env):
    batch = make(env)
    S0 = K.start_states(env, K.B)
    states, inputs = batch.closed_loop.run(S0, K.STEPS)
    assert states.shape == (K.B, K.STEPS + 1, batch.S) and inputs.shape == (K.B, K.STEPS, batch.C)
    np.testing.assert_array_equal(states[:, 0], S0)
    check_wiring(env, states, inputs, f"run {env}")
    np.testing.assert_array_equal(batch.last_run_first_bad, np.full(K.B, -1))
    np.testing.assert_array_equal(batch.closed_loop.last_run_first_bad, batch.last_run_first_bad)
    for q in range(K.B):                                     # the last input is the problem's own last output; K.STEPS draws were consumed
        np.testing.assert_array_equal(batch.get_state(q)[-batch.C:], inputs[q, -1])
        assert batch.rng_position(q) == K.STEPS
    # a finer plant than the model: 4 Euler sub-steps per dt
    states, inputs = batch.closed_loop.run(S0, K.STEPS, plant_substeps=4)
    check_wiring(env, states, inputs, f"run {env} plant substeps 4", substeps=4)
    batch.close()


# ---- 3. run == loop, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["own_u", "u_prev_given", "subset"])
@pytest.mark.parametrize("env", K.ENVS)
def test_run_is_the_loop(env, variant):
    materialize = variant != "u_prev_given"
    a, b = make(env, materialize=materialize), make(env, materialize=materialize)
    ids = [0, 2] if variant == "subset" else None
    n = len(ids) if ids else K.B
    S0 = K.start_states(env, K.B)[ids or slice(None)]
    up = K.uniform_inputs(env, (n,), seed=5) if variant == "u_prev_given" else None
    if variant == "subset":                                  # the batch has a history: every problem has stepped once
        for x in (a, b):
            x.step(K.start_states(env, K.B, seed=3))
    got, want = a.closed_loop.run(S0, K.STEPS, u_prev=up, ids=ids), loop(b, S0, K.STEPS, u_prev=up, ids=ids)
    same_traces(got, want, f"{env} {variant}")
    same_controllers(a, b, materialize, f"{env} {variant} after the run")
    check_wiring(env, got[0], got[1], f"run {env} {variant}")
    # the batch continues as if the loop had been stepped: one more step, then a second run, of all problems
    S = K.start_states(env, K.B, seed=1)
    np.testing.assert_array_equal(a.step(S), b.step(S))
    same_controllers(a, b, materialize, f"{env} {variant} after one more step")
    same_traces(a.closed_loop.run(S, K.STEPS), loop(b, S, K.STEPS), f"{env} {variant} second run")
    same_controllers(a, b, materialize, f"{env} {variant} after the second run")
    a.close(); b.close()


# ---- 4. per-problem controllers and plant overrides -------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", K.ENVS)
def test_per_problem_controllers_and_plants(env):
    name, vals = K.override_values(env, K.B)
    model = (vals[1] * np.array([1.1, 0.9, 1.05], np.float32)).astype(np.float32)        # what each controller plans with
    a, b = make(env, materialize=True), make(env, materialize=True)
    for x in (a, b):
        x.set_problem_params(name, model)
        x.closed_loop.set_plant_params(name, vals[[0, 2]], ids=[0, 2])                    # problem 1's plant: its own controller's value
        assert x.params_differ() == 1
    plant = np.array([vals[0], model[1], vals[2]], np.float32)
    np.testing.assert_array_equal(a.closed_loop.get_plant_params(name), plant)
    S0 = K.start_states(env, K.B)
    got = a.closed_loop.run(S0, K.STEPS)
    same_traces(got, loop(b, S0, K.STEPS), f"{env} per-problem")
    same_controllers(a, b, True, f"{env} per-problem after the run")
    check_wiring(env, got[0], got[1], f"run {env} per-problem", own={name: plant})
    # a controller parameter that changes between two runs moves the un-overridden plant with it, and only that one
    for x in (a, b):
        x.set_problem_params(name, model[1] * np.float32(1.2), ids=[1])
    plant2 = np.array([vals[0], model[1] * np.float32(1.2), vals[2]], np.float32)
    np.testing.assert_array_equal(a.closed_loop.get_plant_params(name), plant2)
    S1 = got[0][:, -1]
    got = a.closed_loop.run(S1, K.STEPS)
    same_traces(got, loop(b, S1, K.STEPS), f"{env} per-problem, second run")
    same_controllers(a, b, True, f"{env} per-problem after the second run")
    check_wiring(env, got[0], got[1], f"run {env} per-problem, second run", own={name: plant2})
    a.close(); b.close()


# ---- 5. splits into launches and segments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["CartPole", "Hover"])
def test_splits_and_segments_give_the_same_bits(env, monkeypatch):
    whole = make(env, K.B_SPLIT, materialize=True)
    monkeypatch.setenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH", str(K.SPLIT_PER_LAUNCH))
    split = make(env, K.B_SPLIT, materialize=True)
    monkeypatch.delenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    monkeypatch.setenv("CTK_BATCH_RUN_SEGMENT_STEPS", str(K.SEGMENT_STEPS))
    segmented = make(env, K.B_SPLIT, materialize=True)
    monkeypatch.setenv("CTK_BATCH_RUN_SEGMENT_STEPS", "100000")                          # the switch never raises the segment length
    unchanged = make(env, K.B_SPLIT, materialize=True)
    monkeypatch.delenv("CTK_BATCH_RUN_SEGMENT_STEPS")
    name, vals = K.override_values(env, K.B_SPLIT)
    S0 = K.start_states(env, K.B_SPLIT)
    up = K.uniform_inputs(env, (K.B_SPLIT,), seed=6)
    runs = []
    for x in (whole, split, segmented, unchanged):
        x.closed_loop.set_plant_params(name, vals)
        runs.append(x.closed_loop.run(S0, K.STEPS_SEGMENTS, u_prev=up))
    check_wiring(env, runs[0][0], runs[0][1], f"run {env} B {K.B_SPLIT}, {K.STEPS_SEGMENTS} steps", own={name: vals})
    for x, r, tag in zip((split, segmented, unchanged), runs[1:], ("2 + 2 + 1 launches", "4 + 4 + 2 steps", "switch above the default")):
        same_traces(r, runs[0], f"{env} {tag}")
        same_controllers(x, whole, True, f"{env} {tag}")
    # ... and the loop, which is every step a segment of its own
    fresh = make(env, K.B_SPLIT, materialize=True)
    fresh.closed_loop.set_plant_params(name, vals)
    same_traces(loop(fresh, S0, K.STEPS_SEGMENTS, u_prev=up), runs[0], f"{env} the loop")
    for x in (whole, split, segmented, unchanged, fresh):
        x.close()


# ---- 6. the MLP batch: a learned network plans, the analytic CartPole is the plant -------------------------------------------------------
def make_mlp():
    m = K.MLP
    batch = CtkMppiMlpBatch(m["B"], seeds=K.seeds(m["B"]), predictor_hidden=m["hidden"], num_rollouts=m["N"], mpc_horizon=m["H"], dt=K.DT,
                            materialize_trajectories=True)
    batch.set_problem_weights(np.stack([O.mlp_default_weights(100 + q, hidden=m["hidden"]) for q in range(m["B"])]))
    return batch


def test_mlp_batch_run_is_the_loop_against_the_analytic_plant():
    a, b = make_mlp(), make_mlp()
    n = K.MLP["B"]
    name, vals = K.override_values("CartPole", n)
    for x in (a, b):
        x.closed_loop.set_plant_params(name, vals)
    S0 = K.start_states("CartPole", n)
    got = a.closed_loop.run(S0, K.STEPS)
    np.testing.assert_array_equal(got[0][:, 0], S0)
    same_traces(got, loop(b, S0, K.STEPS), "MLP batch")
    same_controllers(a, b, True, "MLP batch after the run")
    check_wiring("CartPole", got[0], got[1], "run MLP batch", own={name: vals})
    np.testing.assert_array_equal(a.step(S0), b.step(S0))
    same_traces(a.closed_loop.run(S0, K.STEPS, plant_substeps=2), loop(b, S0, K.STEPS, plant_substeps=2), "MLP batch second run")
    same_controllers(a, b, True, "MLP batch after the second run")
    # a problem without a network is not run, and nothing moves
    bare = CtkMppiMlpBatch(2, num_rollouts=K.MLP["N"], mpc_horizon=K.MLP["H"], dt=K.DT)
    with pytest.raises(Exception, match=r"ctk_mlp_batch_run: no network weights for problem\(s\) 0, 1"):
        bare.closed_loop.run(S0, K.STEPS)
    assert bare.rng_position(0) == 0
    for x in (a, b, bare):
        x.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    batch = make("CartPole")
    S0 = K.start_states("CartPole", K.B)
    snap = [(batch.get_state(q), batch.rng_position(q)) for q in range(K.B)]
    host = np.zeros((K.B, batch.N, batch.samples_needed() // batch.N, 1), np.float32)
    dev = torch.zeros(host.size, device="cuda")
    for samples in (host, dev.data_ptr()):
        with pytest.raises(NotImplementedError, match="device Philox only"):
            batch.closed_loop.run(S0, K.STEPS, samples=samples)
    with pytest.raises(ValueError, match=r"states must have shape \(3, 4\)"):
        batch.closed_loop.run(S0[:2], K.STEPS)
    with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
        batch.closed_loop.run(S0[:1], K.STEPS, ids=[3])
    with pytest.raises(ValueError, match="at least one step"):
        batch.closed_loop.run(S0, 0)
    # the library's own checks, behind the binding's
    lib, h = batch._lib, batch._h
    out_s, out_u = np.zeros((K.B, 2, 4), np.float32), np.zeros((K.B, 1, 1), np.float32)
    ptr = lambda x: x.ctypes.data                                                         # noqa: E731
    assert lib.ctk_batch_run(h, 0, None, ptr(S0), None, 0, 0, ptr(out_s), ptr(out_u), None) == 1
    assert "at least one step" in lib.ctk_batch_last_error(h).decode()
    assert lib.ctk_batch_run(h, 0, None, ptr(S0), None, 1, -1, ptr(out_s), ptr(out_u), None) == 1
    assert "sub-step count" in lib.ctk_batch_last_error(h).decode()
    bad = np.array([0, 3], np.int32)
    assert lib.ctk_batch_run(h, 2, ptr(bad), ptr(S0), None, 1, 0, ptr(out_s), ptr(out_u), None) == 1
    assert "problem index 3 is outside 0 .. 2" in lib.ctk_batch_last_error(h).decode()
    assert lib.ctk_batch_run(h, 0, None, None, None, 1, 0, ptr(out_s), ptr(out_u), None) == 1
    for q, (st, pos) in enumerate(snap):                     # nothing moved
        np.testing.assert_array_equal(batch.get_state(q), st)
        assert batch.rng_position(q) == pos
    batch.close()
