"""-m gpu: per-problem plant and cost parameters of a CtkCemBatch (ctk_cem_problem_set_param, kernel ctk_cem_batch_pp<ENV, TRAJ>).

The contract under test extends test_gpu_cem_batch.py's: problem p of a batch behaves BIT FOR BIT like a CtkEngine("cem", "ODE",
seed=seeds[p]) created from the same configuration that received the same calls, and set_param is one of those calls -
batch.set_problem_params(name, values, ids) is handles[q].set_param(name, values[j]) for every listed q, batch.set_param(name, v) is
set_param(name, v) on every handle.  Every comparison against single handles is assert_array_equal; the only tolerances in this file are
those of tests/test_gpu_tf_goldens.py::test_cem_matches_reference_golden, which is RUN (not restated) on a problem of a batch in the
per-problem form.  The sizes are test_gpu_cem_batch.CONFIGS: the smallest at which each branch of the kernel's body is taken."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkCemBatch, CtkEngine
from helpers import env_from
import test_gpu_tf_goldens as goldens
from test_gpu_batch_params import OWN, TARGET
from test_gpu_cem_batch import (CONFIGS, SOURCES, STEPS, ProblemAsEngine, close_all, common_kw, compare, differing_states, draws_for,
                                first_states, make)

pytestmark = pytest.mark.gpu


def set_own(batch, handles, rng, name, lo, hi, ids=None):
    """one value of `name` per listed problem, drawn from [lo, hi): to the batch in one call, to each handle through set_param"""
    who = list(range(batch.B)) if ids is None else list(ids)
    vals = rng.uniform(lo, hi, len(who)).astype(np.float32)
    batch.set_problem_params(name, vals, ids=ids)
    for j, q in enumerate(who):
        handles[q].set_param(name, float(vals[j]))
        assert batch.get_problem_param(name, q) == vals[j] == np.float32(handles[q].get_param(name))
    return vals


def personalise(batch, handles, rng, ids=None):
    """a target, a plant parameter and a cost weight of its own for every listed problem"""
    for name, lo, hi in OWN[batch.environment]:
        set_own(batch, handles, rng, name, lo, hi, ids)


def step_all(batch, handles, s, ids=None):
    """one step of the listed problems on both sides; returns u after asserting the two agree"""
    who = list(range(batch.B)) if ids is None else list(ids)
    u = batch.step(s[who] if ids is not None else s, ids=ids)
    uh = np.stack([handles[q].step(s[q]) for q in who])
    np.testing.assert_array_equal(u, uh)
    assert np.all(np.isfinite(u))
    return u


def pp_name(batch, materialize):
    return f"ctk_cem_batch_pp<{batch.cfg.environment}, {'true' if materialize else 'false'}>"


# ---- 1. batch == single handles that have parameters of their own, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("B", [1, 3, 5])
def test_batch_equals_handles_with_their_own_parameters(B, config, materialize):
    """before the first step every problem gets its own target(s), one plant parameter and one cost weight; then the three sample sources
    of test_gpu_cem_batch.py, STEPS closed-loop steps each, the plant being the oracle's Predictor.step"""
    batch, handles, plant = make(config, B, materialize)
    rng = np.random.default_rng(B * 137 + len(config))
    assert batch.params_differ() == 0
    personalise(batch, handles, rng)
    assert batch.params_differ() == 1 and batch.dominant_kernel() == pp_name(batch, materialize)
    s = first_states(rng, B, batch.S)
    differing_states(batch, handles, rng)
    for source, given in SOURCES:
        for t in range(STEPS):
            up = rng.uniform(-1.0, 1.0, (B, batch.C)).astype(np.float32) if given else None
            bs, hs, keep = draws_for(source, rng, list(range(B)), batch)
            u = batch.step(s, bs, u_prev=up)
            uh = np.stack([handles[q].step(s[q], hs[q], u_prev=None if up is None else up[q]) for q in range(B)])
            np.testing.assert_array_equal(u, uh, err_msg=f"{config} B={B} {source} u_prev={'given' if given else 'None'} step {t}: u")
            assert np.all(np.isfinite(u))
            s = plant.step(s, u).astype(np.float32)
            del keep
        compare(batch, handles, range(B), materialize, f"{config} B={B} after {source}/{'given' if given else 'None'}")
    close_all(batch, handles)


# ---- 2. a new target array every step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["four_workgroups", "quad2d", "hover"])
def test_per_step_targets(config):
    """all problems on even steps, a strict subset of ids on odd steps, mirrored on the handles; every step steps every problem"""
    B = 5
    batch, handles, plant = make(config, B, True)
    rng = np.random.default_rng(16)
    personalise(batch, handles, rng)
    s = first_states(rng, B, batch.S)
    for t in range(6):
        set_own(batch, handles, rng, *TARGET[batch.environment], ids=None if t % 2 == 0 else [1, 2, 4])
        u = step_all(batch, handles, s)
        s = plant.step(s, u).astype(np.float32)
        compare(batch, handles, range(B), True, f"{config} per-step targets, step {t}")
    close_all(batch, handles)


# ---- 3. subset steps, split launches, late stepping -------------------------------------------------------------------------------------------
def test_subset_steps_and_split_launches(monkeypatch):
    """B = 5 as three launches (2 + 2 + 1); steps alternate between all problems and ids = [1, 3, 4] (launches {1, 3} and {4}: the second
    launch's first record is not problem 0, and record j is not problem j); parameters are set on problems that the next step does not
    step, which are stepped later.  Constants indexed by problem id where the launch order is required (or the reverse) fail here."""
    B, config = 5, "four_workgroups"
    monkeypatch.setenv("CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH", "2")
    batch, handles, plant = make(config, B, True)
    monkeypatch.delenv("CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    rng = np.random.default_rng(40)
    personalise(batch, handles, rng)
    s = first_states(rng, B, batch.S)
    ids, rest = [1, 3, 4], [0, 2]
    for t in range(6):
        if t % 2 == 0:
            u = step_all(batch, handles, s)
            s = plant.step(s, u).astype(np.float32)
        else:
            personalise(batch, handles, rng, ids=rest[(t // 2) % 2:])   # ... set now, not stepped in this step, stepped by the next one
            set_own(batch, handles, rng, "target_position", -0.15, 0.15, ids=[3, 4])
            u = step_all(batch, handles, s, ids=ids)
            s[ids] = plant.step(s[ids], u).astype(np.float32)
        compare(batch, handles, range(B), True, f"split launches, step {t}")
    # a problem whose parameter changes twice before it is stepped keeps the last value
    set_own(batch, handles, rng, "L", 0.15, 0.25, ids=[0, 2])
    step_all(batch, handles, s, ids=ids)
    set_own(batch, handles, rng, "L", 0.15, 0.25, ids=[0])
    step_all(batch, handles, s, ids=[0, 2, 4])
    compare(batch, handles, range(B), True, "after parameters set on problems that were stepped later")
    close_all(batch, handles)


# ---- 4. warm-up mixed with parameters -----------------------------------------------------------------------------------------------------------
def test_warmup_mixed_with_parameters():
    """after reset([2]) the next whole-batch step runs 5 iterations for problem 2 beside 2 for the others, each with its own parameters"""
    B = 4
    kw = dict(num_rollouts=64, mpc_horizon=12, dt=0.02, cem_outer_it=2, cem_best_k=8, warmup=True, warmup_iterations=5,
              cem_initial_action_stdev=0.5, cem_stdev_min=0.01)
    seeds = [21, 22, 23, 24]
    batch = CtkCemBatch(B, seeds=seeds, **kw)
    handles = [CtkEngine("cem", "ODE", seed=seeds[q], **kw) for q in range(B)]
    plant = O.Predictor("ODE", dt=0.02, env=O.EnvParams())
    per_it = 64 * 12
    rng = np.random.default_rng(4)
    personalise(batch, handles, rng)
    s = first_states(rng, B, 4)
    u = step_all(batch, handles, s)                       # the warm-up step of all four
    s = plant.step(s, u).astype(np.float32)
    batch.reset([2])
    handles[2].reset()
    set_own(batch, handles, rng, "target_position", -0.15, 0.15)
    set_own(batch, handles, rng, "L", 0.15, 0.25, ids=[2, 3])
    assert [batch.samples_needed(q) for q in range(B)] == [2 * per_it, 2 * per_it, 5 * per_it, 2 * per_it]
    # caller-supplied samples have one row length: refused before anything is consumed, and the tables stay
    tables = {n: batch.get_problem_params(n) for n in batch.param_names}
    before = [(batch.get_state(q), batch.rng_position(q)) for q in range(B)]
    with pytest.raises(ValueError, match=r"0: 2, 1: 2, 2: 5, 3: 2.*separate calls"):
        batch.step(s, np.zeros((B, 2, 64, 12, 1), np.float32))
    for q in range(B):
        np.testing.assert_array_equal(batch.get_state(q), before[q][0])
        assert batch.rng_position(q) == before[q][1]
    for n in batch.param_names:
        np.testing.assert_array_equal(batch.get_problem_params(n), tables[n], err_msg=n)
    u = step_all(batch, handles, s)                       # one launch, mixed iteration counts, every problem its own constants
    s = plant.step(s, u).astype(np.float32)
    compare(batch, handles, range(B), False, "after the mixed step")
    step_all(batch, handles, s)
    compare(batch, handles, range(B), False, "one step later")
    close_all(batch, handles)


# ---- 5. the two forms of the kernel compute the same ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["four_workgroups", "quad2d", "hover"])
def test_the_two_forms_give_the_same_bits(config):
    """two batches of the same seeds: one never touched, the other with every parameter of every problem set per problem to its default"""
    B = 3
    seeds = [21 + q for q in range(B)]
    common = common_kw(config, True)
    shared, own = CtkCemBatch(B, seeds=seeds, **common), CtkCemBatch(B, seeds=seeds, **common)
    for name in own.param_names:
        own.set_problem_params(name, np.full(B, shared.get_param(name), np.float32))
    assert shared.params_differ() == 0 and own.params_differ() == 1
    eid = shared.cfg.environment
    assert shared.dominant_kernel() == f"ctk_cem_batch<{eid}, true>" and own.dominant_kernel() == f"ctk_cem_batch_pp<{eid}, true>"
    if config == "four_workgroups":
        plain = CtkCemBatch(2, **common_kw(config, False))
        assert plain.dominant_kernel() == "ctk_cem_batch<0, false>"
        plain.close()
    plant = O.Predictor("ODE", dt=0.02, env=CONFIGS[config][6]())
    rng = np.random.default_rng(5)
    s = first_states(rng, B, shared.S)
    for t in range(4):
        u = shared.step(s)
        np.testing.assert_array_equal(own.step(s), u)
        for q in range(B):
            for buf in ("U_NOM", "STD", "J", "Q", "TRAJ", "BEST_IDX"):
                np.testing.assert_array_equal(own.read(buf, q), shared.read(buf, q), err_msg=f"{config} step {t}: {buf} of problem {q}")
            np.testing.assert_array_equal(own.get_state(q), shared.get_state(q))
            assert own.rng_position(q) == shared.rng_position(q)
        s = plant.step(s, u).astype(np.float32)
    assert shared.params_differ() == 0 and shared.dominant_kernel() == f"ctk_cem_batch<{eid}, true>"
    shared.close()
    own.close()


# ---- 6. the parameters are in the result ----------------------------------------------------------------------------------------------------------
def test_parameters_matter():
    """two problems with the same seed, state and draws and different target_position give different u and J; each equals its handle"""
    common = common_kw("four_workgroups", True)
    N, H, its = CONFIGS["four_workgroups"][1], CONFIGS["four_workgroups"][2], CONFIGS["four_workgroups"][4]
    s = np.tile(np.array([0.05, -0.1, 2.8, 0.4], np.float32), (2, 1))
    noise = np.random.default_rng(0).standard_normal((1, its, N, H, 1)).astype(np.float32)
    noise = np.concatenate([noise, noise])
    up = np.zeros((2, 1), np.float32)
    batch = CtkCemBatch(2, seeds=[9, 9], **common)
    u = batch.step(s, noise, u_prev=up)                           # same everything: same result
    assert u[0, 0] == u[1, 0]
    np.testing.assert_array_equal(batch.read("J", 0), batch.read("J", 1))
    fresh = CtkCemBatch(2, seeds=[9, 9], **common)
    handles = [CtkEngine("cem", "ODE", seed=9, **common) for _ in range(2)]
    targets = [-0.1, 0.1]
    fresh.set_problem_params("target_position", targets)
    for h, v in zip(handles, targets):
        h.set_param("target_position", v)
    u2 = fresh.step(s, noise, u_prev=up)
    uh = np.stack([handles[q].step(s[q], noise[q], u_prev=up[q]) for q in range(2)])
    np.testing.assert_array_equal(u2, uh)
    compare(fresh, handles, range(2), True, "two targets")
    assert u2[0, 0] != u2[1, 0]
    J0, J1 = fresh.read("J", 0), fresh.read("J", 1)
    assert not np.array_equal(J0, J1) and not np.array_equal(J0, batch.read("J", 0))
    batch.close()
    close_all(fresh, handles)


# ---- 7. a whole-batch set_param after the problems diverged ------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["four_workgroups", "quad2d"])
def test_whole_batch_set_param_after_divergence(config):
    B = 4
    batch, handles, plant = make(config, B, True)
    rng = np.random.default_rng(6)
    personalise(batch, handles, rng)
    s = first_states(rng, B, batch.S)
    u = step_all(batch, handles, s)
    s = plant.step(s, u).astype(np.float32)
    (tname, _, _), other = OWN[batch.environment][0], [n for n, _, _ in OWN[batch.environment][1:]]
    before = {n: batch.get_problem_params(n) for n in other}
    batch.set_param(tname, 0.07)                                  # overwrites that name for every problem ...
    for h in handles:
        h.set_param(tname, 0.07)
    assert batch.get_param(tname) == np.float32(0.07)
    np.testing.assert_array_equal(batch.get_problem_params(tname), np.full(B, 0.07, np.float32))
    for n in other:                                               # ... and leaves the other names per problem
        np.testing.assert_array_equal(batch.get_problem_params(n), before[n])
        assert len(set(before[n].tolist())) == B
    assert batch.params_differ() == 1
    for t in range(2):
        u = step_all(batch, handles, s)
        s = plant.step(s, u).astype(np.float32)
    compare(batch, handles, range(B), True, f"{config}: set_param({tname}) after divergence")
    # get_param keeps returning the last whole-batch value, whatever a problem holds
    set_own(batch, handles, rng, tname, -0.1, 0.1)
    assert batch.get_param(tname) == np.float32(0.07)
    step_all(batch, handles, s)
    compare(batch, handles, range(B), True, f"{config}: per-problem {tname} again")
    close_all(batch, handles)


# ---- 8. reset, set_state and parameters ----------------------------------------------------------------------------------------------------------
def test_reset_and_set_state_leave_the_tables_alone():
    B = 4
    batch, handles, plant = make("four_workgroups", B, True)
    rng = np.random.default_rng(7)
    personalise(batch, handles, rng)
    s = first_states(rng, B, batch.S)
    u = step_all(batch, handles, s)
    s = plant.step(s, u).astype(np.float32)
    tables = {n: batch.get_problem_params(n) for n in batch.param_names}

    def tables_unchanged(tag):
        for n in batch.param_names:
            np.testing.assert_array_equal(batch.get_problem_params(n), tables[n], err_msg=f"{tag}: {n}")
            for q in range(B):
                assert batch.get_problem_param(n, q) == np.float32(handles[q].get_param(n)), f"{tag}: {n} of problem {q}"

    batch.reset([1, 3])
    for q in (1, 3):
        handles[q].reset()
    tables_unchanged("after reset([1, 3])")
    compare(batch, handles, range(B), True, "after reset([1, 3])")
    u = step_all(batch, handles, s)
    s = plant.step(s, u).astype(np.float32)
    differing_states(batch, handles, rng)                          # set_state on both sides
    tables_unchanged("after set_state")
    assert batch.params_differ() == 1
    u = step_all(batch, handles, s)
    s = plant.step(s, u).astype(np.float32)
    batch.reset()
    for h in handles:
        h.reset()
    tables_unchanged("after reset() of all")
    step_all(batch, handles, s)
    compare(batch, handles, range(B), True, "after reset() of all and one more step")
    close_all(batch, handles)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_alone():
    B = 4
    batch, handles, plant = make("four_workgroups", B, True)
    rng = np.random.default_rng(4)
    personalise(batch, handles, rng)
    s = first_states(rng, B, batch.S)
    u = step_all(batch, handles, s)
    s = plant.step(s, u).astype(np.float32)
    tables = {n: batch.get_problem_params(n) for n in batch.param_names}
    lib, h = batch._lib, batch._h
    vals = (ctypes.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    n_params = len(batch.param_names)

    def refused(n_ids, ids, pid, values, pattern):
        assert lib.ctk_cem_problem_set_param(h, n_ids, ids, pid, values) == 1
        assert pattern in lib.ctk_cem_batch_last_error(h), lib.ctk_cem_batch_last_error(h)

    refused(0, None, n_params, vals, b"ctk_cem_problem_set_param: unknown parameter id")          # a bad parameter id
    refused(0, None, -1, vals, b"ctk_cem_problem_set_param: unknown parameter id")
    refused(1, (ctypes.c_int32 * 1)(4), 3, vals, b"ctk_cem_problem_set_param: problem index 4 is outside 0 .. 3")   # a problem out of range
    refused(2, (ctypes.c_int32 * 2)(0, -1), 3, vals, b"ctk_cem_problem_set_param: problem index -1")
    refused(2, (ctypes.c_int32 * 2)(2, 1), 3, vals, b"ctk_cem_problem_set_param: ids must be strictly ascending")     # descending ids
    refused(2, (ctypes.c_int32 * 2)(1, 1), 3, vals, b"ctk_cem_problem_set_param: ids must be strictly ascending")
    refused(5, (ctypes.c_int32 * 5)(0, 1, 2, 3, 3), 3, vals, b"ctk_cem_problem_set_param: n_ids must be 1 .. 4")
    refused(0, None, 3, None, b"ctk_cem_problem_set_param: NULL values")                            # NULL values
    refused(2, (ctypes.c_int32 * 2)(0, 3), 3, None, b"ctk_cem_problem_set_param: NULL values")
    v = ctypes.c_float(-1.0)
    assert lib.ctk_cem_problem_get_param(h, 4, 3, ctypes.byref(v)) == 1 and lib.ctk_cem_problem_get_param(h, 0, n_params, ctypes.byref(v)) == 1
    assert lib.ctk_cem_problem_get_param(h, 0, 3, None) == 1 and v.value == -1.0
    # the binding refuses the same before it asks the library
    with pytest.raises(ValueError, match="unknown parameter"):
        batch.set_problem_params("target_x", 0.1)
    with pytest.raises(ValueError, match="strictly ascending"):
        batch.set_problem_params("L", [0.2, 0.2], ids=[2, 1])
    with pytest.raises(ValueError, match=r"0 \.\. 3"):
        batch.set_problem_params("L", [0.2], ids=[4])
    with pytest.raises(ValueError, match="one value per listed problem"):
        batch.set_problem_params("L", [0.2, 0.2, 0.2])
    with pytest.raises(ValueError, match="finite"):
        batch.set_problem_params("L", [0.2, np.nan, 0.2, 0.2])
    with pytest.raises(ValueError, match=r"outside 0 \.\. 3"):
        batch.get_problem_param("L", 4)
    # nothing was written: the tables read back as before and the next step is the handles'
    for n in batch.param_names:
        np.testing.assert_array_equal(batch.get_problem_params(n), tables[n], err_msg=n)
    u = step_all(batch, handles, s)
    compare(batch, handles, range(B), True, "after the refusals")
    # a refusal on a batch that never had a parameter set leaves it in the shared form
    plain = CtkCemBatch(2, **common_kw("one_workgroup", False))
    assert lib.ctk_cem_problem_set_param(plain._h, 0, None, 99, vals) == 1
    assert plain.params_differ() == 0 and plain.dominant_kernel() == "ctk_cem_batch<0, false>"
    plain.close()
    close_all(batch, handles)


# ---- 10. the reference-recorded fixture inside a per-problem batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "quad2d"])
def test_reference_fixture_inside_a_per_problem_batch(monkeypatch, case):
    """cem_<case>.npz fed to problem 1 of B = 3 in the per-problem form: the fixture's parameters are set per problem, the neighbours
    hold other targets.  Bit-equal to a handle, and within the reference's tolerances - the body of test_cem_matches_reference_golden
    itself runs on the problem (its bounds and its elite-set rule, nothing restated)"""
    real_engine_from = goldens.engine_from
    made = []

    def batch_engine_from(d, opt, **kw):
        assert opt == "cem"
        handle = real_engine_from(d, opt, **kw)
        batch = CtkCemBatch(3, seeds=[31, 32, 33], environment=str(d["environment"]), num_rollouts=int(d["num_rollouts"]),
                            mpc_horizon=int(d["mpc_horizon"]), dt=float(d["dt"]), action_low=d["low"], action_high=d["high"], **kw)
        env = env_from(d)
        for n in env.param_names():
            batch.set_problem_params(n, float(getattr(env, n)))
        tname, lo, hi = TARGET[batch.environment]
        mine = batch.get_problem_param(tname, 1)
        batch.set_problem_params(tname, [mine + 0.5 * lo, mine + 0.5 * hi], ids=[0, 2])
        assert len(set(batch.get_problem_params(tname).tolist())) == 3 and batch.params_differ() == 1
        made.append(batch.dominant_kernel())        # the golden test closes its engine, and with it the batch
        return ProblemAsEngine(batch, 1, handle, np.random.default_rng(33))

    monkeypatch.setattr(goldens, "engine_from", batch_engine_from)
    goldens.test_cem_matches_reference_golden(monkeypatch, case, "batch")
    assert len(made) == 1 and made[0].startswith("ctk_cem_batch_pp<")


# ---- 11. a user environment ---------------------------------------------------------------------------------------------------------------------------
def test_user_environment_has_the_per_problem_form():
    """a library built with a user model (tests/envs/pendulum_env.h) carries ctk_cem_batch_pp<3, TRAJ>; the states wander by a seeded
    perturbation (no plant is needed to hold a batch against its handles)"""
    from control_toolkit_amd.build_env import register_environment
    name = register_environment(os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs", "pendulum_env.h"))
    B = 3
    common = dict(num_rollouts=128, mpc_horizon=12, dt=0.02, environment=name, materialize_trajectories=True, cem_outer_it=2, cem_best_k=16,
                  cem_initial_action_stdev=0.5, cem_stdev_min=0.01)
    batch = CtkCemBatch(B, seeds=[31 + q for q in range(B)], **common)
    handles = [CtkEngine("cem", "ODE", seed=31 + q, **common) for q in range(B)]
    assert batch.dominant_kernel() == "ctk_cem_batch<3, true>"
    rng = np.random.default_rng(31)
    for pname, lo, hi in (("target_angle", -0.3, 0.3), ("length", 0.4, 0.6), ("ang_weight", 40.0, 60.0)):
        set_own(batch, handles, rng, pname, lo, hi)
    assert batch.params_differ() == 1 and batch.dominant_kernel() == "ctk_cem_batch_pp<3, true>"
    s = rng.uniform(-0.4, 0.4, (B, 2)).astype(np.float32)
    s[:, 0] += 2.6
    for t in range(3):
        if t == 2:
            set_own(batch, handles, rng, "target_angle", -0.3, 0.3, ids=[0, 2])
        step_all(batch, handles, s)
        s = (s + rng.uniform(-0.05, 0.05, s.shape)).astype(np.float32)
    compare(batch, handles, range(B), True, "Pendulum, per-problem parameters")
    close_all(batch, handles)
