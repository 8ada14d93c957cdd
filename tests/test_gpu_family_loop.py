"""-m gpu: closed-loop runs and episodes of the CEM and RPGD batches on the device (BatchClosedLoop(cem_batch) / BatchClosedLoop(rpgd_batch);
include/ctk_hip_loop.h; kernels ctk_cem_batch_plant<ENV>, ctk_cem_batch_plant_noisy<ENV>, ctk_rpgd_batch_plant<ENV>,
ctk_rpgd_batch_plant_noisy<ENV> between the launches of ctk_cem_batch<ENV, TRAJ> / ctk_g_rpgd_batch<ENV>).

Against the LOOP `u = step(S); S = plant_step(S, u)` (1) and `U = step(Y); S, Y, c = plant_step_noisy(S, U, U_prev)` (2) on a twin batch,
assert_array_equal throughout — traces, every readable buffer, the state vector, the Philox position, and one further step: the
counters of every step record of a segment (CEM: iterations and hand-off tags; RPGD: iterations, Adam offset, resampling, population
buffer) are computed on the host ahead of the segment, and each of them gives plausible numbers when wrong.  Against the ORACLE (3):
every realised transition is the oracle's float32 step (plus sigma * the oracle's draws at the problem's noise position), every
realised cost the oracle's stage cost of (s_k, u_k, u_{k-1}) with the plant's parameters; a stale u or a wrong record fails there.
Across optimizers (4): one (S, U, U_prev) through the noisy plants of an MPPI, a CEM and an RPGD batch at one noise position gives the
same bits.  Cases: family_loop_cases.py; start states, overrides, sigmas, seeds and bounds: batch_run_cases.py / batch_episode_cases.py;
the margin helpers are test_gpu_batch_episodes.py's, used and not restated; the observed margins go through tests/margins.py
(profiles/r23_family_closed_loop.txt)."""
import numpy as np
import pytest

import batch_episode_cases as E
import batch_run_cases as K
import family_loop_cases as F
from control_toolkit_amd import BatchClosedLoop, CtkCemBatch, CtkError, CtkMppiBatch, CtkRpgdBatch, Episodes
from margins import record
from test_gpu_batch_episodes import cost_margins, same_episodes, transition_margins

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("family,case", F.FAMILY_CASES, ids=[f"{f}-{c}" for f, c in F.FAMILY_CASES])


def make(family, case, n=K.B, noise=False, reset=True):
    cls = CtkCemBatch if family == "cem" else CtkRpgdBatch
    b = cls(n, seeds=K.seeds(n), **F.batch_kwargs(family, case))
    if family == "rpgd" and reset:
        b.reset()                                             # the device Philox's draws, every problem at its own position
    if noise:
        w, v = E.sigmas(F.environment(family, case), n)
        lp = BatchClosedLoop(b)
        lp.set_noise(process=w, measurement=v)
        lp.set_noise_seeds(E.noise_seeds(n))
    return b


def positions(b):
    return [BatchClosedLoop(b).noise_position(q) for q in range(b.B)]


def last_outputs(b, ids=None):
    at = -b.C - (1 if isinstance(b, CtkCemBatch) else 2)      # behind u: count (CEM), adam_step and count (RPGD)
    return np.stack([b.get_state(q)[at:at + b.C] for q in (range(b.B) if ids is None else ids)])


def same_controllers(a, b, family, tag):
    for q in range(a.B):
        for name in F.BUFFERS[family]:
            np.testing.assert_array_equal(a.read(name, q), b.read(name, q), err_msg=f"{tag}: {name} of problem {q}")
        np.testing.assert_array_equal(a.get_state(q), b.get_state(q), err_msg=f"{tag}: state vector of problem {q}")
        assert a.rng_position(q) == b.rng_position(q), f"{tag}: Philox position of problem {q}"


def one_more_step(a, b, env, family, tag):
    """the sequence numbers and every other counter were left right: both go on stepping"""
    S = K.start_states(env, a.B, seed=1)
    np.testing.assert_array_equal(a.step(S), b.step(S), err_msg=f"{tag}: one more step")
    same_controllers(a, b, family, f"{tag}, one more step")


def run_loop(b, S0, steps, u_prev=None, ids=None, plant_substeps=None):
    """the loop run() replaces, on the entry points a caller would use"""
    n = S0.shape[0]
    states, inputs = np.empty((n, steps + 1, b.S), np.float32), np.empty((n, steps, b.C), np.float32)
    states[:, 0] = S0
    for k in range(steps):
        inputs[:, k] = b.step(states[:, k], u_prev=u_prev if k == 0 else None, ids=ids)
        states[:, k + 1] = BatchClosedLoop(b).plant_step(states[:, k], inputs[:, k], ids=ids, plant_substeps=plant_substeps)
    return states, inputs


def episode_loop(b, S0, steps, u_prev=None, ids=None, plant_substeps=None, Y0=None):
    """the loop episodes() replaces"""
    n = S0.shape[0]
    ep = Episodes(np.empty((n, steps + 1, b.S), np.float32), np.empty((n, steps + 1, b.S), np.float32),
                  np.empty((n, steps, b.C), np.float32), np.empty((n, steps), np.float32))
    ep.states[:, 0], ep.observations[:, 0] = S0, S0 if Y0 is None else Y0
    before = last_outputs(b, ids) if u_prev is None else np.asarray(u_prev, np.float32).reshape(n, b.C)
    for k in range(steps):
        ep.inputs[:, k] = b.step(ep.observations[:, k], u_prev=u_prev if k == 0 else None, ids=ids)
        ep.states[:, k + 1], ep.observations[:, k + 1], ep.costs[:, k] = BatchClosedLoop(b).plant_step_noisy(
            ep.states[:, k], ep.inputs[:, k], before if k == 0 else ep.inputs[:, k - 1], ids=ids, plant_substeps=plant_substeps)
    return ep


def check_run_against_the_oracle(env, states, inputs, tag, substeps=1, own=None):
    """every realised transition of a run against the oracle's float32 step, with the project's trajectory bound"""
    assert np.isfinite(inputs).all() and np.isfinite(states).all(), tag
    worst = 0.0
    for k in range(inputs.shape[1]):
        want = K.oracle_step(env, states[:, k], inputs[:, k], substeps, own).astype(np.float64)
        bound = K.TRAJ_TOL["atol"] + K.TRAJ_TOL["rtol"] * np.abs(want)
        worst = max(worst, float((np.abs(states[:, k + 1] - want) / bound).max()))
    print(f"{tag}: worst used of the transition bound {worst:.3f}")
    record(tag, "s_next", [worst], [0.0], atol=1.0)
    assert worst <= 1.0, f"{tag}: {worst}"


def check_episode_against_the_oracle(env, ep, tag, B, pos0, u_first, ids=None, substeps=1, own=None, noise=True):
    """every realised transition, observation and cost of an episode of the problems `ids` of a batch of B with the case sigmas and noise
    seeds: the transitions and draws with the bounds of batch_episode_cases.py at the noise positions pos0 + k, the costs of
    (s_k, u_k, u_{k-1}) with u_first before the first step"""
    rows = list(range(B)) if ids is None else list(ids)
    w, v = E.sigmas(env, B)
    if not noise:
        w, v = np.zeros_like(w), np.zeros_like(v)
    seeds = E.noise_seeds(B)
    m = transition_margins(env, ep, w[rows], v[rows], [seeds[q] for q in rows], pos0, substeps, own)
    owns = [dict() if own is None else {k: vals[j] for k, vals in own.items()} for j in range(len(rows))]
    c = cost_margins(env, ep, np.asarray(u_first, np.float32).reshape(len(rows), -1), owns)
    print(f"{tag}: worst used, states {m[:, 0].max():.3f}, observations {m[:, 1].max():.3f}, costs {c.max():.3f}")
    record(tag, "s_next", m[:, 0], np.zeros(len(rows)), atol=1.0)
    record(tag, "y - s", m[:, 1], np.zeros(len(rows)), atol=1.0)
    record(tag, "cost", c.max(axis=1), np.zeros(len(rows)), atol=1.0)
    assert np.isfinite(ep.inputs).all() and (m <= 1.0).all() and (c <= 1.0).all(), f"{tag}: {m} {c}"


def own_of(env, n, ids=None):
    name, vals = K.override_values(env, n)
    return name, vals, {name: vals if ids is None else vals[ids]}


# ---- 1. run == the loop, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["u_prev_given", "own_u", "subset", "per_problem"])
@CASES
def test_run_is_the_loop(family, case, variant):
    env = F.environment(family, case)
    a, b = make(family, case), make(family, case)
    ids = [0, 2] if variant == "subset" else None
    n = len(ids) if ids else K.B
    S0 = K.start_states(env, K.B)[ids or slice(None)]
    up = K.uniform_inputs(env, (n,), seed=5) if variant == "u_prev_given" else None
    own = None
    if variant == "subset":                                   # problem 0 has stepped once, problem 2 has not: its warm-up step lies in the run
        for x in (a, b):
            x.step(K.start_states(env, K.B, seed=3)[:1], ids=[0])
    if variant == "per_problem":                              # the un-overridden plants follow their controllers' tables
        name, vals, own = own_of(env, K.B)
        for x in (a, b):
            x.set_problem_params(name, vals)
        assert a.params_differ() == 1
    tag = f"run {family} {case} {variant}"
    states, inputs = BatchClosedLoop(a).run(S0, K.STEPS, u_prev=up, ids=ids)
    want_states, want_inputs = run_loop(b, S0, K.STEPS, u_prev=up, ids=ids)
    np.testing.assert_array_equal(states, want_states, err_msg=f"{tag}: states")
    np.testing.assert_array_equal(inputs, want_inputs, err_msg=f"{tag}: inputs")
    np.testing.assert_array_equal(states[:, 0], S0)
    np.testing.assert_array_equal(BatchClosedLoop(a).last_run_first_bad, np.full(n, -1))
    same_controllers(a, b, family, tag)
    assert positions(a) == [0] * K.B                          # a run never moves the noise positions
    check_run_against_the_oracle(env, states, inputs, tag, 1, own)
    one_more_step(a, b, env, family, tag)
    a.close(); b.close()


@pytest.mark.parametrize("differ", [False, True], ids=["shared", "per_problem"])
@CASES
def test_launch_splits_and_segments_give_the_same_bits(family, case, differ, monkeypatch):
    """B 5, 10 steps: the device loop in segments of 4 + 4 + 2 steps and, for CEM, every step as 2 + 2 + 1 launches (in the per-problem
    form each launch takes its constants from its own offset behind the segment's records) against the unsplit host loop"""
    env, n = F.environment(family, case), K.B_SPLIT
    monkeypatch.setenv(F.SEGMENT_SWITCH, str(K.SEGMENT_STEPS))
    monkeypatch.setenv(F.CEM_SPLIT_SWITCH, str(K.SPLIT_PER_LAUNCH))
    a = make(family, case, n)                                 # both switches are read at creation
    monkeypatch.delenv(F.SEGMENT_SWITCH)
    monkeypatch.delenv(F.CEM_SPLIT_SWITCH)
    b = make(family, case, n)
    own = None
    if differ:
        name, vals, own = own_of(env, n)
        for x in (a, b):
            x.set_problem_params(name, vals)
    S0, up = K.start_states(env, n), K.uniform_inputs(env, (n,), seed=6)
    tag = f"run {family} {case} B {n}, {K.STEPS_SEGMENTS} steps, {'per-problem' if differ else 'shared'} form"
    states, inputs = BatchClosedLoop(a).run(S0, K.STEPS_SEGMENTS, u_prev=up)
    want_states, want_inputs = run_loop(b, S0, K.STEPS_SEGMENTS, u_prev=up)
    np.testing.assert_array_equal(states, want_states, err_msg=f"{tag}: states")
    np.testing.assert_array_equal(inputs, want_inputs, err_msg=f"{tag}: inputs")
    same_controllers(a, b, family, tag)
    check_run_against_the_oracle(env, states, inputs, tag, 1, own)
    # the noisy plant through the same split and segments
    for x in (a, b):
        w, v = E.sigmas(env, n)
        BatchClosedLoop(x).set_noise(process=w, measurement=v)
        BatchClosedLoop(x).set_noise_seeds(E.noise_seeds(n))
    ep = BatchClosedLoop(a).episodes(states[:, -1], K.STEPS_SEGMENTS)
    same_episodes(ep, episode_loop(b, states[:, -1], K.STEPS_SEGMENTS), f"{tag}: episodes")
    check_episode_against_the_oracle(env, ep, f"episodes {tag[4:]}", n, [0] * n, inputs[:, -1], own=own)      # u_prev None: the run's last input
    same_controllers(a, b, family, f"{tag} after the episodes")
    assert positions(a) == positions(b) == [K.STEPS_SEGMENTS] * n
    one_more_step(a, b, env, family, tag)
    a.close(); b.close()


# ---- 2. episodes == the loop, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["u_prev_given", "own_u", "subset"])
@CASES
def test_episodes_are_the_loop(family, case, variant):
    env = F.environment(family, case)
    a, b = make(family, case, noise=True), make(family, case, noise=True)
    ids = [0, 2] if variant == "subset" else None
    n = len(ids) if ids else K.B
    S0 = K.start_states(env, K.B)[ids or slice(None)]
    up = K.uniform_inputs(env, (n,), seed=5) if variant == "u_prev_given" else None
    if variant != "u_prev_given":                             # the batch has a history: every problem's own last output is not 0
        for x in (a, b):
            x.step(K.start_states(env, K.B, seed=3))
        assert np.abs(last_outputs(a)).max() > 0
    tag = f"episodes {family} {case} {variant}"
    first = last_outputs(a, ids) if up is None else up         # the input before the first one
    got, want = BatchClosedLoop(a).episodes(S0, K.STEPS, u_prev=up, ids=ids), episode_loop(b, S0, K.STEPS, u_prev=up, ids=ids)
    same_episodes(got, want, tag)
    check_episode_against_the_oracle(env, got, tag, K.B, [0] * n, first, ids=ids)
    same_controllers(a, b, family, tag)
    moved = [K.STEPS if (ids is None or q in ids) else 0 for q in range(K.B)]
    assert positions(a) == positions(b) == moved              # unlisted problems' noise positions do not move
    assert not np.array_equal(got.observations[-1], got.states[-1])            # problem 2 has measurement noise: y is not s
    # it continues as if the loop had been stepped: a second episode of all problems, y and s apart
    S1, Y1 = K.start_states(env, K.B, seed=1), K.start_states(env, K.B, seed=2)
    first, pos = last_outputs(a), positions(a)
    second = BatchClosedLoop(a).episodes(S1, K.STEPS, Y0=Y1)
    same_episodes(second, episode_loop(b, S1, K.STEPS, Y0=Y1), f"{tag} second episode")
    check_episode_against_the_oracle(env, second, f"{tag} second episode", K.B, pos, first)
    same_controllers(a, b, family, f"{tag} after the second episode")
    assert positions(a) == positions(b) == [m + K.STEPS for m in moved]
    one_more_step(a, b, env, family, tag)
    a.close(); b.close()


@CASES
def test_noiseless_episodes_are_the_run(family, case):
    env = F.environment(family, case)
    a, b = make(family, case), make(family, case)
    np.testing.assert_array_equal(BatchClosedLoop(a).get_noise_seeds(), np.array(K.seeds(K.B), np.uint64))   # default: the controller's seed
    S0, first = K.start_states(env, K.B), last_outputs(a)     # u_prev None: the input before the first one is the problem's own last output
    ep, (states, inputs) = BatchClosedLoop(a).episodes(S0, K.STEPS), BatchClosedLoop(b).run(S0, K.STEPS)
    assert isinstance(ep, Episodes) and ep.costs.shape == (K.B, K.STEPS) and np.isfinite(ep.costs).all()
    np.testing.assert_array_equal(ep.states, states)
    np.testing.assert_array_equal(ep.inputs, inputs)
    np.testing.assert_array_equal(ep.observations, ep.states)
    check_episode_against_the_oracle(env, ep, f"episodes {family} {case} noiseless", K.B, [0] * K.B, first, noise=False)
    same_controllers(a, b, family, f"{family} {case} noiseless")
    assert positions(a) == [K.STEPS] * K.B and positions(b) == [0] * K.B       # the position advances whatever the sigmas
    one_more_step(a, b, env, family, f"{family} {case} noiseless")
    a.close(); b.close()


@CASES
def test_an_episode_of_a_plus_b_steps_is_two_episodes(family, case):
    env = F.environment(family, case)
    whole, parts = make(family, case, noise=True), make(family, case, noise=True)
    S0, up = K.start_states(env, K.B), K.uniform_inputs(env, (K.B,), seed=6)
    ref = BatchClosedLoop(whole).episodes(S0, K.STEPS, u_prev=up)
    a = BatchClosedLoop(parts).episodes(S0, 2, u_prev=up)
    b = BatchClosedLoop(parts).episodes(a.states[:, -1], K.STEPS - 2, Y0=a.observations[:, -1])
    joined = Episodes(np.concatenate([a.states, b.states[:, 1:]], 1), np.concatenate([a.observations, b.observations[:, 1:]], 1),
                      np.concatenate([a.inputs, b.inputs], 1), np.concatenate([a.costs, b.costs], 1))
    same_episodes(joined, ref, f"{family} {case} 2 + {K.STEPS - 2} steps")
    check_episode_against_the_oracle(env, ref, f"episodes {family} {case} {K.STEPS} steps in one", K.B, [0] * K.B, up)
    same_controllers(parts, whole, family, f"{family} {case} continued")
    assert positions(parts) == positions(whole) == [K.STEPS] * K.B
    whole.close(); parts.close()


# ---- 3. every realised transition, cost and draw against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("substeps,overrides", [(1, False), (1, True), (2, True), (4, False)])
@CASES
def test_transitions_costs_and_draws_match_the_oracle(family, case, substeps, overrides):
    env = F.environment(family, case)
    batch = make(family, case, noise=True)
    lp = BatchClosedLoop(batch)
    own, owns = None, [dict() for _ in range(K.B)]
    if overrides:
        name, vals, own = own_of(env, K.B)
        lp.set_plant_params(name, vals)
        np.testing.assert_array_equal(lp.get_plant_params(name), vals)
        owns = [{name: vals[p]} for p in range(K.B)]
        assert batch.params_differ() == 0                     # an override is the plant's alone
    lp.set_noise_position(1, 5)                               # positions are per problem
    pos0 = positions(batch)
    assert pos0 == [0, 5, 0]
    S0, up = K.start_states(env, K.B), K.uniform_inputs(env, (K.B,), seed=8)
    ep = lp.episodes(S0, K.STEPS, u_prev=up, plant_substeps=substeps)
    np.testing.assert_array_equal(ep.states[:, 0], S0)
    np.testing.assert_array_equal(ep.observations[:, 0], S0)
    assert positions(batch) == [p + K.STEPS for p in pos0] and max(positions(batch)) < E.MAX_POS
    tag = f"episodes {family} {case} substeps {substeps} {'own plants' if overrides else 'the modelled plant'}"
    w, v = E.sigmas(env, K.B)
    seeds = E.noise_seeds(K.B)
    assert np.isfinite(ep.inputs).all() and np.isfinite(ep.costs).all() and (ep.costs > 0).all(), tag
    m = transition_margins(env, ep, w, v, seeds, pos0, substeps, own)
    c = cost_margins(env, ep, up, owns)
    print(f"{tag}: worst used, states {m[:, 0].max():.3f}, observations {m[:, 1].max():.3f}, costs {c.max():.3f}")
    record(tag, "s_next", m[:, 0], np.zeros(K.B), atol=1.0)
    record(tag, "y - s", m[:, 1], np.zeros(K.B), atol=1.0)
    record(tag, "cost", c.max(axis=1), np.zeros(K.B), atol=1.0)
    assert (m <= 1.0).all(), f"{tag}: {m}"
    assert (c <= 1.0).all(), f"{tag}: {c}"
    # zero-sigma components are exactly the noiseless values: the deterministic plant kernel's on the same operands, the state itself
    for k in range(K.STEPS):
        det = lp.plant_step(ep.states[:, k], ep.inputs[:, k], plant_substeps=substeps)
        np.testing.assert_array_equal(ep.states[:, k + 1][w == 0], det[w == 0], err_msg=f"{tag}: zero process sigma, step {k}")
        np.testing.assert_array_equal(ep.observations[:, k + 1][v == 0], ep.states[:, k + 1][v == 0], err_msg=f"{tag}: zero measurement sigma, step {k}")
    # the check tells a wrong position apart: against the draws one position on, every noisy problem violates its bounds
    wrong = transition_margins(env, ep, w, v, seeds, pos0, substeps, own, shift=1)
    for p in range(K.B):
        if w[p].any():
            assert wrong[p, 0] > 1.0, f"{tag}: problem {p}'s states pass against the wrong position"
        if v[p].any():
            assert wrong[p, 1] > 1.0, f"{tag}: problem {p}'s observations pass against the wrong position"
    batch.close()


# ---- 4. common random numbers across optimizers -------------------------------------------------------------------------------------------
def test_the_three_families_share_one_disturbance():
    """An MPPI, a CEM and an RPGD batch on CartPole with equal noise seeds, positions, sigmas and plant tables.  Each controller would
    drive its own trajectory, so the shared disturbance is checked where the operands can be made equal: the same (S, U, U_prev) through
    every family's noisy plant at the same noise position gives the same next state, observation and cost, bit for bit."""
    env, n = "CartPole", K.B
    batches = {"mppi": CtkMppiBatch(n, seeds=K.seeds(n), **K.batch_kwargs(env)), "cem": make("cem", "one_workgroup"),
               "rpgd": make("rpgd", "cartpole_small")}
    w, v = E.sigmas(env, n)
    name, vals = K.override_values(env, n)
    S, U, Up = K.start_states(env, n), K.uniform_inputs(env, (n,), seed=11), K.uniform_inputs(env, (n,), seed=12)
    out = {}
    for fam, b in batches.items():
        lp = BatchClosedLoop(b)
        lp.set_noise(process=w, measurement=v)
        lp.set_noise_seeds(E.noise_seeds(n))
        lp.set_plant_params(name, vals)
        lp.set_plant_params("ccrc_weight", 40.0)              # a cost weight of the plant's: the common yardstick
        lp.set_noise_position(2, 7)
        first = lp.plant_step_noisy(S, U, Up, plant_substeps=2)
        second = lp.plant_step_noisy(first[0], Up, U, plant_substeps=2)
        det = lp.plant_step(S, U, plant_substeps=2)
        assert [lp.noise_position(q) for q in range(n)] == [2, 2, 9]
        out[fam] = (*first, *second, det)
    assert not np.array_equal(out["mppi"][0][2], out["mppi"][1][2])            # problem 2 has measurement noise
    assert not np.array_equal(out["mppi"][0][1], out["mppi"][6][1])            # problem 1 has process noise
    for fam in ("cem", "rpgd"):
        for i, what in enumerate(("S_next", "Y_next", "cost", "second S_next", "second Y_next", "second cost", "plant_step")):
            np.testing.assert_array_equal(out[fam][i], out["mppi"][i], err_msg=f"{fam} against mppi: {what}")
    for b in batches.values():
        b.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_an_rpgd_problem_that_was_never_reset_is_refused():
    case, env = "cartpole_small", "CartPole"
    a, b = make("rpgd", case, reset=False), make("rpgd", case)
    S0 = K.start_states(env, K.B)
    a.reset(ids=[0, 2])                                       # problem 1 was never reset
    before = [(a.rng_position(q), BatchClosedLoop(a).noise_position(q)) for q in range(K.B)]
    with pytest.raises(CtkError, match=r"\[ctk 5\] ctk_rpgd_batch_run: problem 1 was never reset.*nothing was launched"):
        BatchClosedLoop(a).run(S0, K.STEPS)
    with pytest.raises(CtkError, match=r"\[ctk 5\] ctk_rpgd_batch_episodes: problem 1 was never reset.*nothing was launched"):
        BatchClosedLoop(a).episodes(S0, K.STEPS)
    assert [(a.rng_position(q), BatchClosedLoop(a).noise_position(q)) for q in range(K.B)] == before
    # nothing moved, the sequence numbers included: the listed problems that were reset run as those of a batch that was never refused
    # (a consumed sequence number would leave the run waiting for a result that carries another one: CtkError)
    ids = [0, 2]
    states, inputs = BatchClosedLoop(a).run(S0[ids], K.STEPS, ids=ids)
    want_states, want_inputs = BatchClosedLoop(b).run(S0[ids], K.STEPS, ids=ids)
    np.testing.assert_array_equal(states, want_states)
    np.testing.assert_array_equal(inputs, want_inputs)
    for q in ids:
        np.testing.assert_array_equal(a.get_state(q), b.get_state(q))
    a.close(); b.close()


@pytest.mark.parametrize("family,case", [("cem", "one_workgroup"), ("rpgd", "cartpole_small")])
def test_refusals(family, case):
    batch = make(family, case)
    lp, lib, h, pre = BatchClosedLoop(batch), batch._lib, batch._h, F.PREFIX[family]
    S0 = K.start_states("CartPole", K.B)
    snap = [(batch.get_state(q), batch.rng_position(q), lp.noise_position(q)) for q in range(K.B)]
    with pytest.raises(ValueError, match="at least one step"):
        lp.run(S0, 0)
    with pytest.raises(ValueError, match="at least one step"):
        lp.episodes(S0, 0)
    with pytest.raises(ValueError, match="process noise: a standard deviation is finite and >= 0"):
        lp.set_noise(process=-1e-3)
    with pytest.raises(NotImplementedError, match="device Philox only"):
        lp.run(S0, K.STEPS, samples=np.zeros((K.B, 4), np.float32))
    # the library's own refusals, under the family's names
    ptr = lambda x: x.ctypes.data                                                         # noqa: E731
    err = lambda: getattr(lib, pre + "_last_error")(h).decode()                           # noqa: E731
    st, ob = np.zeros((K.B, 2, 4), np.float32), np.zeros((K.B, 2, 4), np.float32)
    inp, co = np.zeros((K.B, 1, 1), np.float32), np.zeros((K.B, 1), np.float32)
    f = lambda e: getattr(lib, f"{pre}_{e}")                                              # noqa: E731
    assert f("run")(h, 0, None, ptr(S0), None, 0, 0, ptr(st), ptr(inp), None) == 1 and f"{pre}_run: a run has at least one step" in err()
    assert f("episodes")(h, 0, None, ptr(S0), None, None, 0, 0, ptr(st), ptr(ob), ptr(inp), ptr(co), None) == 1
    assert f"{pre}_episodes: an episode has at least one step" in err()
    assert f("run")(h, 0, None, ptr(S0), None, 1, -1, ptr(st), ptr(inp), None) == 1 and f"{pre}_run: the plant's sub-step count" in err()
    assert f("run")(h, 0, None, None, None, 1, 0, ptr(st), ptr(inp), None) == 1 and f"{pre}_run: NULL start states or trace destination" in err()
    sg = np.full((K.B, 4), 0.01, np.float32)
    sg[1, 2] = -1e-3
    assert f("plant_set_noise")(h, 0, None, 0, ptr(sg)) == 1
    assert f"{pre}_plant_set_noise: a standard deviation is finite and >= 0" in err() and "problem 1, state 2" in err()
    assert not lp.get_noise()[0].any()                        # a refused call wrote nothing
    bad = np.array([0, 3], np.int32)
    assert f("run")(h, 2, ptr(bad), ptr(S0), None, 1, 0, ptr(st), ptr(inp), None) == 1 and f"{pre}_run: problem index 3 is outside 0 .. 2" in err()
    for q, (state, rpos, npos) in enumerate(snap):            # nothing moved
        np.testing.assert_array_equal(batch.get_state(q), state)
        assert batch.rng_position(q) == rpos and lp.noise_position(q) == npos
    batch.close()
