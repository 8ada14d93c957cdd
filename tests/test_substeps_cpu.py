"""Guards the inputs of test_gpu_substeps.py (tests/substep_cases.py) without a GPU.  For every (environment, config, state, size) that
file uses, with the very inputs it uses (substep_cases.input_sets: MPPI, CEM's last iteration, random action, plain rollouts, the
CEM-GMM step, the throughput sizes):

 (1) all costs are finite;
 (2) J of the float32 oracle and J of SubstepF64 (every sub-step in float64 on the float32 state, rounded after every sub-step) agree to
     GAP_BOUND = 3e-6 relative, a tenth of the 3e-5 that the GPU file allows a kernel;
 (3) at the large states the oracle's angle column equals SubstepF64's bit for bit, and no angle update of any SUB-step is a near-tie of
     float32 rounding (large_angle_cases.near_ties on the trajectory of the sub-steps);
 (4) sub-step semantics, independent of the oracle's own loop: predict_core at (dt, k, H) equals every k-th state of predict_core at
     (dt / k, 1, k H) on inputs repeated k times.  Both are the same float32 operations in the same order, so they are compared for
     equality (k = 2, 4 as the issue asks, and the 3 of CONFIGS), all three environments;
 (5) the sub-step length a handle derives, f32(f64(f32(dt)) / k), is the float32 the oracle uses, f32(dt / k), for every pair of CONFIGS
     and of the composition check; the pairs the module's docstring excludes do differ;
 (6) the plans of the GPU file's composition check (two handles compared with each other) have no near-tie at the large states either.

A further check (test_a_miscounted_substep_loop_would_not_pass) states what the GPU file is there to catch: one sub-step too many or too few
of the right length, k steps of the whole dt, or no sub-steps at all use more than 10x the J bound at every state, H = 4 included.

Measured (worst relative gap of J between the float32 oracle and SubstepF64 over every input set of the GPU file, per sub-step form):
                      (0.02, 2)   (0.03, 3)   (0.005, 1)
  CartPole  ordinary   1.05e-06    1.66e-06    2.83e-07
            large      6.07e-07    5.75e-07    5.36e-07
  Quad2D    ordinary   5.20e-07    4.79e-07    3.70e-07
            large      5.00e-07    5.43e-07    4.45e-07
  Hover     ordinary   2.84e-07    4.35e-07    2.33e-07
            large      3.82e-07    3.81e-07    2.64e-07
The worst, 1.66e-6, leaves 18x to the 3e-5 bound.  (large_angle_cases.StepF64, which rounds once per MPC step, differs from the oracle by
5e-4 .. 1.2e-1 at the large states with 2 - 4 sub-steps: an artefact of that form, which is why SubstepF64 exists.)

States kept: the three ordinary ones and both large ones (32760.5 rad / 0.7 rad/s and 1e9 rad / 0.7 rad/s) in all three environments.
States dropped: none (substep_cases.DROPPED is empty).  With the large-angle file's own seeds seven input sets had ONE row each with a near-tie
in a sub-step's angle update at 32760.5 rad; those sets draw from another seed (substep_cases.SEEDS), every other set keeps the seeds of
large_angle_cases.PLAIN_SEED / OTHER_SEED:
  CartPole  MPPI N 100 H 20 period 5 (0.03, 3) row 91; rollout() N 128 H 20 (0.03, 3) row 127; CEM-GMM (0.005, 1) row 24;
            CEM batch, problem 1 with its own target, N 128 H 20 (0.02, 2) row 5
  Quad2D    random action N 128 H 20 (0.03, 3) row 106
  Hover     CEM N 100 H 20 (0.02, 2) row 5; MPPI N 128 H 20 period 1 (0.03, 3) row 97"""
import numpy as np
import pytest

from oracle import ctk_oracle as O
import large_angle_cases as L
import substep_cases as S

GAP_BOUND = 3e-6          # a tenth of the GPU file's rtol on J


def rel_gap(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))


def guard(tag, env, dt, k, is_large, r32, r64, own=()):
    """checks (1) - (3) of one case; returns the relative gap in J"""
    a = L.ANGLE[env]
    assert np.isfinite(r32["J"]).all() and np.isfinite(r64["J"]).all(), tag                                                                # (1)
    gap = rel_gap(r32["J"], r64["J"])
    assert gap <= GAP_BOUND, f"{tag}: J differs from the per-sub-step float64 form by {gap:.2e}"                                           # (2)
    if is_large:                                                                                                                           # (3)
        assert np.array_equal(r32["traj"][:, :, a].view(np.uint32), r64["traj"][:, :, a].view(np.uint32)), f"{tag}: angle bits differ"
        sub = S.sub_trajectory(env, r32["s"], r32["Q"], dt, k, own)
        assert np.array_equal(sub[:, ::k].view(np.uint32), r32["traj"].view(np.uint32)), tag
        ties = L.near_ties(sub, a, dt=dt, substeps=k)
        assert ties.size == 0, f"{tag}: rows {ties} have a near-tie in an angle update, choose another seed (substep_cases.SEEDS)"
    return gap


@pytest.mark.parametrize("env", L.ENVS)
def test_oracle_is_a_tight_reference_at_every_substep_case(env):
    worst = {}
    for label, H, dt, k, large, ref in S.input_sets(env):
        for name, th, om, is_large in S.states(env, large):
            gap = guard(f"{env} {label} {name} theta0 {th}", env, dt, k, is_large, ref(th, om), ref(th, om, predictor=S.SubstepF64))
            key = ("large" if is_large else "ordinary", dt, k)
            worst[key] = max(worst.get(key, 0.0), gap)
    for label, dt, k, th, om, is_large, ref in S.batch_sets(env):
        r32 = ref()
        gap = guard(f"{env} {label} theta0 {th}", env, dt, k, is_large, r32, ref(predictor=S.SubstepF64), ref.args[-1])
        key = ("large" if is_large else "ordinary", dt, k)
        worst[key] = max(worst.get(key, 0.0), gap)
    for (kind, dt, k), g in sorted(worst.items()):
        print(f"{env:8s} {kind:8s} dt {dt} k {k}: worst relative gap of J, fp32 oracle vs SubstepF64: {g:.2e}")


@pytest.mark.parametrize("dt,k", S.CONFIGS + [(0.02, 4)])
@pytest.mark.parametrize("env", L.ENVS)
def test_k_substeps_are_k_steps_of_a_kth_of_the_time_step(env, dt, k):                                                                     # (4)
    assert S.oracle_substep(dt, k) == np.float32((dt / k) / 1)
    pars = L.env_params(env)
    N, H = 128, 7
    Q = L.draws_for(env, N, H)
    for th, om in S.ORDINARY + S.LARGE:
        s = np.tile(L.base_state(env, th, om), (N, 1))
        coarse = O.Predictor("ODE", dt=dt, env=pars, intermediate_steps=k).predict_core(s, Q)
        fine = O.Predictor("ODE", dt=dt / k, env=pars, intermediate_steps=1).predict_core(s, np.repeat(Q, k, axis=1))
        assert fine.shape == (N, k * H + 1, pars.S)
        np.testing.assert_array_equal(coarse, fine[:, ::k], err_msg=f"{env} theta0 {th}")
        if k > 1:
            assert not np.array_equal(coarse[:, 1], fine[:, 1])               # ... and the sub-steps do something


@pytest.mark.parametrize("env", L.ENVS)
def test_composition_check_has_no_near_tie_at_the_large_states(env):
    """test_gpu_substeps.py::test_substeps_compose compares two handles with each other, not with the oracle; at a large angle it still
    needs plans without a near-tie, or the two handles' sin / cos (CartPole: the checked one with sub-steps, the fast one without) could
    round an angle update differently"""
    a, pars = L.ANGLE[env], L.env_params(env)
    for dt_a, k, Ha, dt_b, Hb in S.COMPOSITIONS:
        Q = np.repeat(S.composition_plans(env, 128, Ha), k, axis=1)
        for name, th, om, large in S.states(env):
            if large:
                s = np.tile(L.base_state(env, th, om), (128, 1))
                t32, t64 = (cls("ODE", dt=dt_b, env=pars).predict_core(s, Q) for cls in (O.Predictor, L.StepF64))
                assert np.array_equal(t32[:, :, a].view(np.uint32), t64[:, :, a].view(np.uint32)), (env, k, th)
                assert L.near_ties(t32, a, dt=dt_b).size == 0, (env, k, th)


@pytest.mark.parametrize("dt,k", [c for c in S.CONFIGS if c[1] > 1])
@pytest.mark.parametrize("env", L.ENVS)
def test_a_miscounted_substep_loop_would_not_pass(env, dt, k):
    """what the GPU file is there to catch: one sub-step too many or too few (of the right length), or k steps of the whole dt, move J
    far beyond the bound it asserts, at every state, at the smallest size"""
    N, H, p = S.SIZES[2]
    for name, th, om, large in S.states(env):
        want = S.mppi_ref(env, N, H, p, th, om, dt, k)["J"].astype(np.float64)
        for wrong_dt, wrong_k in [(dt * (k + 1) / k, k + 1), (dt * (k - 1) / k, k - 1), (dt * k, k), (dt, 1)]:
            got = S.mppi_ref(env, N, H, p, th, om, wrong_dt, wrong_k)["J"]
            used = np.max(np.abs(got - want) / (1e-3 + 3e-5 * np.abs(want)))
            assert used > 10.0, (env, name, wrong_dt, wrong_k, used)


def test_the_two_derivations_of_the_substep_length_agree():                                                                                # (5)
    pairs = S.CONFIGS + S.TP_CONFIGS + [(0.02, 4)] + [(da, k) for da, k, _, _, _ in S.COMPOSITIONS] + [(db, 1) for _, _, _, db, _ in S.COMPOSITIONS]
    for dt, k in pairs:
        assert S.kernel_substep(dt, k) == S.oracle_substep(dt, k), (dt, k)
    for da, k, Ha, db, Hb in S.COMPOSITIONS:                                  # the two handles of the composition check integrate at ONE length
        assert S.kernel_substep(da, k) == S.kernel_substep(db, 1) and Ha * k == Hb
    for dt, k in [(0.02, 3), (0.02, 5), (0.005, 3), (0.01, 3)]:               # why these are not in CONFIGS
        assert abs(int(S.kernel_substep(dt, k).view(np.uint32)) - int(S.oracle_substep(dt, k).view(np.uint32))) == 1, (dt, k)


def test_states_and_sizes_are_the_ones_agreed():
    assert S.CONFIGS == [(0.02, 2), (0.03, 3), (0.005, 1)]
    assert S.SIZES == [(128, 20, 1), (100, 20, 5), (128, 4, 1)] and S.CEM_SIZES == [(128, 20), (100, 20)] and (S.CEM_K, S.CEM_ITS) == (16, 2)
    assert S.ORDINARY == [(0.4, -0.7), (-2.9, 1.5), (3.1, 0.0)] and S.LARGE == [L.IN_RANGE[0], L.FAR_OUT[0]]
    for env in L.ENVS:
        kept = [(th, om) for _, th, om, large in S.states(env) if large]
        assert set(kept) | {st for e, st in S.DROPPED if e == env} == set(S.LARGE)
