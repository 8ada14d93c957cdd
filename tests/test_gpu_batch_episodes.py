"""-m gpu: stochastic closed-loop episodes of the MPPI batches on the device, with the realised cost (BatchClosedLoop.episodes /
plant_step_noisy / the noise settings; ctk_batch_episodes, ctk_batch_plant_step_noisy; kernel ctk_batch_plant_noisy<ENV> between the
launches of ctk_mppi_batch<ENV, LOG>).

Against the ORACLE: every realised transition is the oracle's float32 step plus sigma_w * the oracle's device_noise at the problem's
noise position, every observation the state plus sigma_v * the other half of the same draws (2), every realised cost the oracle's stage
cost of (s_k, u_k, u_{k-1}) with the plant's parameters (4).  Against the LOOP `U = step(Y); S, Y, c = plant_step_noisy(S, U, U_prev)` and
against run(), assert_array_equal throughout (1, 3, 5 - 8): the contract.  The three ways to get the data flow wrong each fail one of 2 - 4:
a plant that advanced the observation instead of the true state fails 2 and 3, a cost or plant that read the stale u_prev fails 4, a
wrong noise position fails 2.  Cases, references and bounds: batch_episode_cases.py; the observed margins go through tests/margins.py
(profiles/r21_episode_margins.txt)."""
import ctypes

import numpy as np
import pytest

import batch_episode_cases as E
import batch_run_cases as K
from oracle import ctk_oracle as O
from control_toolkit_amd import CtkMppiBatch, CtkMppiMlpBatch, Episodes
from margins import record

pytestmark = pytest.mark.gpu


def make(env, n=K.B, materialize=False, noise=True):
    b = CtkMppiBatch(n, seeds=K.seeds(n), **K.batch_kwargs(env, materialize))
    if noise:
        set_noise(b, env, n)
    return b


def set_noise(b, env, n):
    w, v = E.sigmas(env, n)
    b.closed_loop.set_noise(process=w, measurement=v)
    b.closed_loop.set_noise_seeds(E.noise_seeds(n))


def positions(b):
    return [b.closed_loop.noise_position(q) for q in range(b.B)]


def last_outputs(b, ids=None):
    return np.stack([b.get_state(q)[-b.C:] for q in (range(b.B) if ids is None else ids)])


def loop(batch, S0, steps, u_prev=None, ids=None, plant_substeps=None, Y0=None):
    """the loop episodes() replaces, on the entry points a caller would use"""
    n = S0.shape[0]
    ep = Episodes(np.empty((n, steps + 1, batch.S), np.float32), np.empty((n, steps + 1, batch.S), np.float32),
                  np.empty((n, steps, batch.C), np.float32), np.empty((n, steps), np.float32))
    ep.states[:, 0], ep.observations[:, 0] = S0, S0 if Y0 is None else Y0
    before = last_outputs(batch, ids) if u_prev is None else np.asarray(u_prev, np.float32).reshape(n, batch.C)
    for k in range(steps):
        ep.inputs[:, k] = batch.step(ep.observations[:, k], u_prev=u_prev if k == 0 else None, ids=ids)
        ep.states[:, k + 1], ep.observations[:, k + 1], ep.costs[:, k] = batch.closed_loop.plant_step_noisy(
            ep.states[:, k], ep.inputs[:, k], before if k == 0 else ep.inputs[:, k - 1], ids=ids, plant_substeps=plant_substeps)
    return ep


def same_controllers(a, b, materialize, tag):
    for q in range(a.B):
        np.testing.assert_array_equal(a.read("U_NOM", q), b.read("U_NOM", q), err_msg=f"{tag}: U_NOM of problem {q}")
        np.testing.assert_array_equal(a.read("J", q), b.read("J", q), err_msg=f"{tag}: J of problem {q}")
        np.testing.assert_array_equal(a.get_state(q), b.get_state(q), err_msg=f"{tag}: state vector of problem {q}")
        assert a.rng_position(q) == b.rng_position(q), f"{tag}: Philox position of problem {q}"
        if materialize:
            np.testing.assert_array_equal(a.read("Q", q), b.read("Q", q), err_msg=f"{tag}: Q of problem {q}")


def same_episodes(got, want, tag):
    for name in Episodes._fields:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=f"{tag}: {name}")


def used(err, bound):
    return np.asarray(err, np.float64) / np.asarray(bound, np.float64)


def transition_margins(env, ep, w, v, seeds, pos0, substeps, own, shift=0):
    """worst |error| / bound of the states and of the observations, per problem [n, 2], against the draws of position pos0 + k + shift"""
    n, steps, S = ep.inputs.shape[0], ep.inputs.shape[1], ep.states.shape[2]
    db, out = E.draw_bound(), np.zeros((n, 2))
    for k in range(steps):
        det = K.oracle_step(env, ep.states[:, k], ep.inputs[:, k], substeps, own).astype(np.float64)
        for p in range(n):
            nz = E.expected_noise(seeds[p], pos0[p] + k + shift, S).astype(np.float64)
            want = det[p] + w[p].astype(np.float64) * nz[:S]
            bound = E.TRAJ_TOL["atol"] + E.TRAJ_TOL["rtol"] * np.abs(want) + w[p] * db
            out[p, 0] = max(out[p, 0], used(np.abs(ep.states[p, k + 1] - want), bound).max())
            y = ep.observations[p, k + 1].astype(np.float64)
            diff = y - ep.states[p, k + 1].astype(np.float64)
            noisy = v[p] > 0
            if noisy.any():
                bound = v[p] * db + 2.0 ** -23 * np.abs(y)
                out[p, 1] = max(out[p, 1], used(np.abs(diff - v[p].astype(np.float64) * nz[S:])[noisy], bound[noisy]).max())
    return out


def check_transitions(batch, env, ep, tag, pos0, substeps=1, own=None):
    n = ep.inputs.shape[0]
    w, v = E.sigmas(env, batch.B)
    w, v, seeds = w[:n], v[:n], E.noise_seeds(batch.B)[:n]
    lo, hi = K.limits(env)
    assert np.isfinite(ep.inputs).all() and (ep.inputs >= lo).all() and (ep.inputs <= hi).all(), tag
    m = transition_margins(env, ep, w, v, seeds, pos0, substeps, own)
    print(f"{tag}: worst used, states {m[:, 0].max():.3f}, observations {m[:, 1].max():.3f}")
    record(tag, "s_next", m[:, 0], np.zeros(n), atol=1.0)
    record(tag, "y - s", m[:, 1], np.zeros(n), atol=1.0)
    assert (m <= 1.0).all(), f"{tag}: {m}"
    # zero-sigma components are exactly the noiseless values: the deterministic plant kernel's on the same operands, the state itself
    for k in range(ep.inputs.shape[1]):
        det = batch.closed_loop.plant_step(ep.states[:, k], ep.inputs[:, k], plant_substeps=substeps)
        np.testing.assert_array_equal(ep.states[:, k + 1][w == 0], det[w == 0], err_msg=f"{tag}: zero process sigma, step {k}")
        np.testing.assert_array_equal(ep.observations[:, k + 1][v == 0], ep.states[:, k + 1][v == 0], err_msg=f"{tag}: zero measurement sigma, step {k}")
    # the check tells a wrong position apart: against the draws one position on, every noisy problem violates its bounds
    wrong = transition_margins(env, ep, w, v, seeds, pos0, substeps, own, shift=1)
    for p in range(n):
        if w[p].any():
            assert wrong[p, 0] > 1.0, f"{tag}: problem {p}'s states pass against the wrong position"
        if v[p].any():
            assert wrong[p, 1] > 1.0, f"{tag}: problem {p}'s observations pass against the wrong position"


# ---- 1. noiseless == run ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", K.ENVS)
def test_noiseless_episodes_are_the_run(env):
    a, b = make(env, materialize=True, noise=False), make(env, materialize=True, noise=False)
    S0 = K.start_states(env, K.B)
    np.testing.assert_array_equal(a.closed_loop.get_noise_seeds(), np.array(K.seeds(K.B), np.uint64))      # default: the controller's seed
    ep, (states, inputs) = a.closed_loop.episodes(S0, K.STEPS), b.closed_loop.run(S0, K.STEPS)
    assert isinstance(ep, Episodes) and ep.costs.shape == (K.B, K.STEPS) and np.isfinite(ep.costs).all()
    np.testing.assert_array_equal(ep.states, states)
    np.testing.assert_array_equal(ep.inputs, inputs)
    np.testing.assert_array_equal(ep.observations, ep.states)
    np.testing.assert_array_equal(a.last_run_first_bad, np.full(K.B, -1))
    same_controllers(a, b, True, f"{env} noiseless")
    assert positions(a) == [K.STEPS] * K.B and positions(b) == [0] * K.B       # the position advances whatever the sigmas
    S = K.start_states(env, K.B, seed=1)                                       # the sequence numbers agree: both go on stepping
    np.testing.assert_array_equal(a.step(S), b.step(S))
    same_controllers(a, b, True, f"{env} noiseless, one more step")
    a.close(); b.close()


# ---- 2. transitions against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overrides", [False, True])
@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("env", K.ENVS)
def test_transitions_match_the_oracle_plus_its_draws(env, substeps, overrides):
    batch = make(env)
    own = None
    if overrides:
        name, vals = K.override_values(env, K.B)
        batch.closed_loop.set_plant_params(name, vals)
        own = {name: vals}
    S0 = K.start_states(env, K.B)
    batch.closed_loop.set_noise_position(1, 5)                                 # positions are per problem
    pos0 = positions(batch)
    assert pos0 == [0, 5, 0]
    ep = batch.closed_loop.episodes(S0, K.STEPS, plant_substeps=substeps)
    np.testing.assert_array_equal(ep.states[:, 0], S0)
    np.testing.assert_array_equal(ep.observations[:, 0], S0)
    assert positions(batch) == [p + K.STEPS for p in pos0]
    check_transitions(batch, env, ep, f"episodes {env} substeps {substeps} {'own plants' if overrides else 'the modelled plant'}", pos0, substeps, own)
    batch.close()


# ---- 3. the controller sees y, not s: episodes == loop, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["u_prev_given", "own_u", "subset"])
@pytest.mark.parametrize("env", K.ENVS)
def test_episodes_are_the_loop(env, variant):
    a, b = make(env, materialize=True), make(env, materialize=True)
    ids = [0, 2] if variant == "subset" else None
    n = len(ids) if ids else K.B
    S0 = K.start_states(env, K.B)[ids or slice(None)]
    up = K.uniform_inputs(env, (n,), seed=5) if variant == "u_prev_given" else None
    if variant != "u_prev_given":                             # the batch has a history: every problem has stepped once
        for x in (a, b):
            x.step(K.start_states(env, K.B, seed=3))
    got, want = a.closed_loop.episodes(S0, K.STEPS, u_prev=up, ids=ids), loop(b, S0, K.STEPS, u_prev=up, ids=ids)
    same_episodes(got, want, f"{env} {variant}")
    same_controllers(a, b, True, f"{env} {variant} after the episode")
    moved = [K.STEPS if (ids is None or q in ids) else 0 for q in range(K.B)]
    assert positions(a) == positions(b) == moved                               # unlisted problems' noise positions do not move
    assert not np.array_equal(got.observations[-1], got.states[-1])            # problem 2 has measurement noise: y is not s
    # it continues as if the loop had been stepped: a second episode of all problems from where the first ended, y and s apart
    S1, Y1 = K.start_states(env, K.B, seed=1), K.start_states(env, K.B, seed=2)
    same_episodes(a.closed_loop.episodes(S1, K.STEPS, Y0=Y1), loop(b, S1, K.STEPS, Y0=Y1), f"{env} {variant} second episode")
    same_controllers(a, b, True, f"{env} {variant} after the second episode")
    assert positions(a) == positions(b) == [m + K.STEPS for m in moved]
    a.close(); b.close()


# ---- 4. the realised cost -----------------------------------------------------------------------------------------------------------------
def cost_margins(env, ep, u_first, owns, stale=False):
    n, steps = ep.costs.shape
    out = np.zeros((n, steps))
    for p in range(n):
        for k in range(steps):
            up = ep.inputs[p, k] if stale else (u_first[p] if k == 0 else ep.inputs[p, k - 1])
            want = float(E.stage_cost_oracle(env, owns[p], ep.states[p, k], ep.inputs[p, k], up))
            out[p, k] = abs(float(ep.costs[p, k]) - want) / float(E.cost_bound(env, want))
    return out


@pytest.mark.parametrize("variant", ["default", "own_target", "plant_cost_weight", "substeps2"])
@pytest.mark.parametrize("env", K.ENVS)
def test_realised_cost_matches_the_oracle(env, variant):
    """costs[j][k] against the oracle's stage cost of (s_k, u_k, u_{k-1}) with the PLANT's parameters.  plant_cost_weight overrides
    ccrc_weight (the weight of the input-change term) of every plant: a common yardstick the controllers do not plan with, and the
    variant in which a cost that read the stale u_prev = u_k must show — asserted as a condition on the inputs: against that reference
    the same costs exceed the bound at least ten times somewhere.  (With the default weights CartPole's input-change term, at most 4,
    is below ten times the bound at these start states' costs of ~2e4, so the other variants print the figure only.)  substeps2: the
    cost's derived constants do not depend on the plant's sub-step count."""
    batch = make(env)
    owns = [dict() for _ in range(K.B)]
    if variant == "own_target":
        tgt = "target_position" if env == "CartPole" else "target_x"
        vals = np.array([0.05, -0.1, 0.15], np.float32)
        batch.set_problem_params(tgt, vals)                                    # the un-overridden plant follows its controller
        owns = [{tgt: vals[p]} for p in range(K.B)]
    if variant == "plant_cost_weight":
        vals = np.array([40.0, 55.0, 70.0], np.float32)
        batch.closed_loop.set_plant_params("ccrc_weight", vals)
        owns = [{"ccrc_weight": vals[p]} for p in range(K.B)]
        assert batch.params_differ() == 0
    sub = 2 if variant == "substeps2" else None
    S0, up = K.start_states(env, K.B), K.uniform_inputs(env, (K.B,), seed=8)
    ep = batch.closed_loop.episodes(S0, K.STEPS, u_prev=up, plant_substeps=sub)
    assert np.isfinite(ep.costs).all() and (ep.costs > 0).all()
    m = cost_margins(env, ep, up, owns)
    stale = cost_margins(env, ep, up, owns, stale=True)
    tag = f"cost {env} {variant}"
    print(f"{tag}: worst used {m.max():.3f}; against the stale u_prev {stale.max():.1f}")
    record(tag, "cost", m.max(axis=1), np.zeros(K.B), atol=1.0)
    assert (m <= 1.0).all(), f"{tag}: {m}"
    if variant == "plant_cost_weight":
        assert stale.max() >= 10.0, f"{tag}: the inputs do not tell the stale previous input apart ({stale.max():.2f} x the bound)"
        # u_prev = None: the problem's own last output (here the episode's last input) is the first step's previous input
        S1, last = ep.states[:, -1], ep.inputs[:, -1]
        ep2 = batch.closed_loop.episodes(S1, 2, Y0=ep.observations[:, -1])
        m2 = cost_margins(env, ep2, last, owns)
        record(tag + " own last output", "cost", m2.max(axis=1), np.zeros(K.B), atol=1.0)
        assert (m2 <= 1.0).all(), f"{tag} own last output: {m2}"
        assert cost_margins(env, ep2, np.zeros_like(last), owns)[:, 0].max() > 1.0     # ... and not zero
    batch.close()


# ---- 5. replay and seeds ------------------------------------------------------------------------------------------------------------------
def test_replay_and_seeds():
    env = "Quad2D"
    batch = make(env)
    lp = batch.closed_loop
    w, v = E.sigmas(env, K.B)
    gw, gv = lp.get_noise()
    np.testing.assert_array_equal(gw, w); np.testing.assert_array_equal(gv, v)
    np.testing.assert_array_equal(lp.get_noise_seeds(), np.array(E.noise_seeds(K.B), np.uint64))
    lp.set_noise(measurement=0.5, ids=[1])                                     # one kind, a subset, a scalar; the other kind stays
    np.testing.assert_array_equal(lp.get_noise()[1][1], np.full(batch.S, 0.5, np.float32))
    np.testing.assert_array_equal(lp.get_noise()[0], w)
    lp.clear_noise()
    assert not lp.get_noise()[0].any() and not lp.get_noise()[1].any()
    np.testing.assert_array_equal(lp.get_noise_seeds(), np.array(E.noise_seeds(K.B), np.uint64))      # clear_noise keeps the seeds
    lp.set_noise(process=w, measurement=v)
    lp.set_noise_position(2, 0xFFFFFFFF)
    assert lp.noise_position(2) == 0xFFFFFFFF
    lp.set_noise_position(2, 3)
    batch.step(K.start_states(env, K.B, seed=3))
    snap = [(batch.get_state(q), batch.rng_position(q), lp.noise_position(q)) for q in range(K.B)]
    S0 = K.start_states(env, K.B)
    first = lp.episodes(S0, K.STEPS)                                           # u_prev None: the own last output, which set_state restores
    assert [lp.noise_position(q) for q in range(K.B)] == [K.STEPS, K.STEPS, 3 + K.STEPS]
    assert not np.array_equal(last_outputs(batch), np.stack([st[-batch.C:] for st, _, _ in snap]))
    for q, (st, pos, npos) in enumerate(snap):
        batch.set_state(q, st); batch.set_rng_position(q, pos); lp.set_noise_position(q, npos)
    same_episodes(lp.episodes(S0, K.STEPS), first, "replay")
    # common random numbers: problems 1 and 2 made twins (controller seed, noise seed, sigmas, position, start state) give identical rows
    twin = CtkMppiBatch(K.B, seeds=[7, 9, 9], **K.batch_kwargs(env))
    tl = twin.closed_loop
    tl.set_noise(process=w[2], measurement=v[2])
    tl.set_noise_seeds([E.noise_seeds(3)[0], E.noise_seeds(3)[2], E.noise_seeds(3)[2]])
    Sx = np.stack([S0[0], S0[1], S0[1]])
    ep = tl.episodes(Sx, K.STEPS)
    for name in Episodes._fields:
        np.testing.assert_array_equal(getattr(ep, name)[1], getattr(ep, name)[2], err_msg=f"twins: {name}")
    # ... and changing only the noise seed gives different states
    for q in range(K.B):
        twin.reset([q]); tl.set_noise_position(q, 0)
    tl.set_noise_seeds([E.noise_seeds(3)[1]], ids=[2])
    ep = tl.episodes(Sx, K.STEPS)
    assert not np.array_equal(ep.states[1, 1], ep.states[2, 1])
    batch.close(); twin.close()


# ---- 6. splits, segments, continuation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["CartPole", "Hover"])
def test_splits_segments_and_continuation_give_the_same_bits(env, monkeypatch):
    n = K.B_SPLIT
    whole = make(env, n, materialize=True)
    monkeypatch.setenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH", str(K.SPLIT_PER_LAUNCH))
    monkeypatch.setenv("CTK_BATCH_RUN_SEGMENT_STEPS", str(K.SEGMENT_STEPS))
    split = make(env, n, materialize=True)                    # both switches are read at creation
    monkeypatch.delenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    monkeypatch.delenv("CTK_BATCH_RUN_SEGMENT_STEPS")
    parts = make(env, n, materialize=True)
    name, vals = K.override_values(env, n)
    S0, up = K.start_states(env, n), K.uniform_inputs(env, (n,), seed=6)
    for x in (whole, split, parts):
        x.closed_loop.set_plant_params(name, vals)
    ref = whole.closed_loop.episodes(S0, K.STEPS_SEGMENTS, u_prev=up)
    check_transitions(whole, env, ref, f"episodes {env} B {n}, {K.STEPS_SEGMENTS} steps", [0] * n, 1, {name: vals})
    same_episodes(split.closed_loop.episodes(S0, K.STEPS_SEGMENTS, u_prev=up), ref, f"{env} 2 + 2 + 1 launches, 4 + 4 + 2 steps")
    same_controllers(split, whole, True, f"{env} split and segmented")
    assert positions(split) == positions(whole) == [K.STEPS_SEGMENTS] * n
    # episodes(10) == episodes(4) then episodes(6, Y0 = ...)
    a = parts.closed_loop.episodes(S0, 4, u_prev=up)
    b = parts.closed_loop.episodes(a.states[:, -1], 6, Y0=a.observations[:, -1])
    np.testing.assert_array_equal(b.states[:, 0], a.states[:, -1]); np.testing.assert_array_equal(b.observations[:, 0], a.observations[:, -1])
    joined = Episodes(np.concatenate([a.states, b.states[:, 1:]], 1), np.concatenate([a.observations, b.observations[:, 1:]], 1),
                      np.concatenate([a.inputs, b.inputs], 1), np.concatenate([a.costs, b.costs], 1))
    same_episodes(joined, ref, f"{env} 4 + 6 steps")
    same_controllers(parts, whole, True, f"{env} continued")
    for x in (whole, split, parts):
        x.close()


# ---- 6b. one batch, one run buffer, both layouts in turn ------------------------------------------------------------------------------------
def same_bits(got, want, tag):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag


@pytest.mark.parametrize("env", ["CartPole", "Hover"])
def test_mixed_calls_share_one_buffer(env, monkeypatch):
    """run, episodes, plant_step, plant_step_noisy and run again on ONE batch, in segments of 2 steps: the grown-on-demand run buffer
    serves the layout with and the layout without the noisy plant's parts in turn.  Against a twin stepped as the host loop, whose buffer
    only ever holds single plant steps.  Host sequencing alone: bit for bit, no tolerance."""
    monkeypatch.setenv("CTK_BATCH_RUN_SEGMENT_STEPS", "2")
    a, b = make(env), make(env)                               # the switch is read at creation
    la, lb = a.closed_loop, b.closed_loop
    S0 = K.start_states(env, K.B)
    # A: the device loops
    st1, in1 = la.run(S0, 3)
    ep = la.episodes(st1[:, -1], 3)
    s3 = la.plant_step(ep.states[:, -1], ep.inputs[:, -1])
    s4, y4, c4 = la.plant_step_noisy(s3, ep.inputs[:, -1], ep.inputs[:, -2])
    st2, in2 = la.run(s4, 2)
    # B: the same 8 controller steps and 2 single plant steps, every step a round trip
    def run_loop(S, steps):
        states, inputs = np.empty((K.B, steps + 1, b.S), np.float32), np.empty((K.B, steps, b.C), np.float32)
        states[:, 0] = S
        for k in range(steps):
            inputs[:, k] = b.step(states[:, k])
            states[:, k + 1] = lb.plant_step(states[:, k], inputs[:, k])
        return states, inputs
    wst1, win1 = run_loop(S0, 3)
    wep = loop(b, wst1[:, -1], 3)
    w3 = lb.plant_step(wep.states[:, -1], wep.inputs[:, -1])
    w4, wy4, wc4 = lb.plant_step_noisy(w3, wep.inputs[:, -1], wep.inputs[:, -2])
    wst2, win2 = run_loop(w4, 2)
    tag = f"{env} mixed calls"
    for name, got, want in (("first run's states", st1, wst1), ("first run's inputs", in1, win1), ("plant_step", s3, w3),
                            ("plant_step_noisy's states", s4, w4), ("plant_step_noisy's observations", y4, wy4),
                            ("plant_step_noisy's costs", c4, wc4), ("second run's states", st2, wst2), ("second run's inputs", in2, win2)):
        same_bits(got, want, f"{tag}: {name}")
    for name in Episodes._fields:
        same_bits(getattr(ep, name), getattr(wep, name), f"{tag}: the episode's {name}")
    assert not np.array_equal(ep.observations[2], ep.states[2])                # problem 2 has measurement noise
    for q in range(K.B):
        same_bits(a.get_state(q), b.get_state(q), f"{tag}: state vector of problem {q}")
        assert a.rng_position(q) == b.rng_position(q) == 8, f"{tag}: Philox position of problem {q}"
    assert positions(a) == positions(b) == [4] * K.B and 4 < E.MAX_POS, f"{tag}: noise positions"
    a.close(); b.close()


# ---- 7. the existing paths are blind to the noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", K.ENVS)
def test_run_and_plant_step_ignore_the_noise(env):
    a, b = make(env), make(env, noise=False)
    S0 = K.start_states(env, K.B)
    U = K.uniform_inputs(env, (K.B,), seed=11)
    np.testing.assert_array_equal(a.closed_loop.plant_step(S0, U), b.closed_loop.plant_step(S0, U))
    ra, rb = a.closed_loop.run(S0, K.STEPS), b.closed_loop.run(S0, K.STEPS)
    np.testing.assert_array_equal(ra[0], rb[0]); np.testing.assert_array_equal(ra[1], rb[1])
    a.reset(); a.closed_loop.clear_plant_params()
    assert positions(a) == [0] * K.B
    w, v = a.closed_loop.get_noise()
    np.testing.assert_array_equal(w, E.sigmas(env, K.B)[0]); np.testing.assert_array_equal(v, E.sigmas(env, K.B)[1])
    a.close(); b.close()


# ---- 8. the MLP batch: a learned network plans, the noisy analytic CartPole is the plant ----------------------------------------------------
def make_mlp():
    m = K.MLP
    batch = CtkMppiMlpBatch(m["B"], seeds=K.seeds(m["B"]), predictor_hidden=m["hidden"], num_rollouts=m["N"], mpc_horizon=m["H"], dt=K.DT,
                            materialize_trajectories=True)
    batch.set_problem_weights(np.stack([O.mlp_default_weights(100 + q, hidden=m["hidden"]) for q in range(m["B"])]))
    w, v = E.sigmas("CartPole", 3)
    batch.closed_loop.set_noise(process=w[1:], measurement=v[1:])              # problem 0: process only; problem 1: both kinds
    batch.closed_loop.set_noise_seeds(E.noise_seeds(3)[1:])
    return batch


def test_mlp_batch_episodes():
    a, b = make_mlp(), make_mlp()
    n = K.MLP["B"]
    name, vals = K.override_values("CartPole", n)
    for x in (a, b):
        x.closed_loop.set_plant_params(name, vals)
    S0, up = K.start_states("CartPole", n), K.uniform_inputs("CartPole", (n,), seed=5)
    got = a.closed_loop.episodes(S0, K.STEPS, u_prev=up)
    same_episodes(got, loop(b, S0, K.STEPS, u_prev=up), "MLP batch")
    same_controllers(a, b, True, "MLP batch after the episode")
    assert positions(a) == positions(b) == [K.STEPS] * n
    # the transitions, with the case sigmas of problems 1 and 2
    w, v = E.sigmas("CartPole", 3)
    m = transition_margins("CartPole", got, w[1:], v[1:], E.noise_seeds(3)[1:], [0] * n, 1, {name: vals})
    wrong = transition_margins("CartPole", got, w[1:], v[1:], E.noise_seeds(3)[1:], [0] * n, 1, {name: vals}, shift=1)
    record("episodes MLP batch", "s_next", m[:, 0], np.zeros(n), atol=1.0)
    record("episodes MLP batch", "y - s", m[:, 1], np.zeros(n), atol=1.0)
    assert (m <= 1.0).all() and (wrong[:, 0] > 1.0).all() and wrong[1, 1] > 1.0, (m, wrong)
    np.testing.assert_array_equal(got.observations[0], got.states[0])          # problem 0 has no measurement noise
    own = loop(b, S0, K.STEPS, plant_substeps=2)                                 # u_prev None after a history, 2 sub-steps
    same_episodes(a.closed_loop.episodes(S0, K.STEPS, plant_substeps=2), own, "MLP batch second episode")
    same_controllers(a, b, True, "MLP batch after the second episode")
    # a problem without a network is not run, and nothing moves
    bare = CtkMppiMlpBatch(2, num_rollouts=K.MLP["N"], mpc_horizon=K.MLP["H"], dt=K.DT)
    with pytest.raises(Exception, match=r"\[ctk 5\] ctk_mlp_batch_episodes: no network weights for problem\(s\) 0, 1.*nothing was launched"):
        bare.closed_loop.episodes(S0, K.STEPS)
    assert bare.rng_position(0) == 0 and bare.closed_loop.noise_position(0) == 0
    for x in (a, b, bare):
        x.close()


# ---- 9. the library's own refusals --------------------------------------------------------------------------------------------------------
def test_c_level_refusals():
    batch = make("CartPole")
    lib, h = batch._lib, batch._h
    S0 = K.start_states("CartPole", K.B)
    U = np.zeros((K.B, 1), np.float32)
    st, ob = np.zeros((K.B, 2, 4), np.float32), np.zeros((K.B, 2, 4), np.float32)
    inp, co = np.zeros((K.B, 1, 1), np.float32), np.zeros((K.B, 1), np.float32)
    sn, yn, c = np.zeros((K.B, 4), np.float32), np.zeros((K.B, 4), np.float32), np.zeros(K.B, np.float32)
    ptr = lambda x: x.ctypes.data                                                         # noqa: E731
    err = lambda: lib.ctk_batch_last_error(h).decode()                                    # noqa: E731
    snap = [(batch.get_state(q), batch.rng_position(q), batch.closed_loop.noise_position(q)) for q in range(K.B)]
    before = batch.closed_loop.get_noise()
    for bad in (-1e-3, float("nan"), float("inf")):
        sg = np.full((K.B, 4), 0.01, np.float32)
        sg[1, 2] = bad
        assert lib.ctk_batch_plant_set_noise(h, 0, None, 0, ptr(sg)) == 1
        assert "ctk_batch_plant_set_noise: a standard deviation is finite and >= 0" in err() and "problem 1, state 2" in err()
    sg = np.full((K.B, 4), 0.01, np.float32)
    for kind in (-1, 2):
        assert lib.ctk_batch_plant_set_noise(h, 0, None, kind, ptr(sg)) == 1 and "ctk_batch_plant_set_noise: kind is 0" in err()
    assert lib.ctk_batch_plant_set_noise(h, 0, None, 0, None) == 1 and "ctk_batch_plant_set_noise: NULL sigma" in err()
    assert lib.ctk_batch_plant_get_noise(h, 0, 2, ptr(sn)) == 1 and lib.ctk_batch_plant_get_noise(h, K.B, 0, ptr(sn)) == 1
    assert lib.ctk_batch_plant_set_noise_seed(h, 0, None, None) == 1 and "ctk_batch_plant_set_noise_seed: NULL seeds" in err()
    assert lib.ctk_batch_plant_noise_set_position(h, K.B, 0) == 1 and "ctk_batch_plant_noise_set_position: problem index 3" in err()
    pos = ctypes.c_uint32()
    assert lib.ctk_batch_plant_noise_get_position(h, -1, ctypes.byref(pos)) == 1
    for x, y in zip(batch.closed_loop.get_noise(), before):  # a refused call wrote nothing
        np.testing.assert_array_equal(x, y)
    ep = lambda s0, steps, sub=0, states=st, obs=ob, inputs=inp, costs=co: lib.ctk_batch_episodes(      # noqa: E731
        h, 0, None, s0, None, None, steps, sub, states, obs, inputs, costs, None)
    assert ep(ptr(S0), 0, 0, ptr(st), ptr(ob), ptr(inp), ptr(co)) == 1 and "ctk_batch_episodes: an episode has at least one step" in err()
    assert ep(ptr(S0), 1, -1, ptr(st), ptr(ob), ptr(inp), ptr(co)) == 1 and "ctk_batch_episodes: the plant's sub-step count" in err()
    for miss in range(5):
        args = [ptr(S0), 1, 0, ptr(st), ptr(ob), ptr(inp), ptr(co)]
        args[[0, 3, 4, 5, 6][miss]] = None
        assert ep(*args) == 1 and "ctk_batch_episodes: NULL start states or trace destination" in err()
    bad = np.array([0, 3], np.int32)
    assert lib.ctk_batch_episodes(h, 2, ptr(bad), ptr(S0), None, None, 1, 0, ptr(st), ptr(ob), ptr(inp), ptr(co), None) == 1
    assert "ctk_batch_episodes: problem index 3 is outside 0 .. 2" in err()
    for miss in range(6):
        args = [ptr(S0), ptr(U), ptr(U), 0, ptr(sn), ptr(yn), ptr(c)]
        args[[0, 1, 2, 4, 5, 6][miss]] = None
        assert lib.ctk_batch_plant_step_noisy(h, 0, None, *args) == 1 and "ctk_batch_plant_step_noisy: NULL" in err()
    assert lib.ctk_batch_plant_step_noisy(h, 0, None, ptr(S0), ptr(U), ptr(U), -1, ptr(sn), ptr(yn), ptr(c)) == 1
    assert "ctk_batch_plant_step_noisy: the plant's sub-step count" in err()
    for q, (state, rpos, npos) in enumerate(snap):           # nothing moved
        np.testing.assert_array_equal(batch.get_state(q), state)
        assert batch.rng_position(q) == rpos and batch.closed_loop.noise_position(q) == npos
    batch.close()
