"""Guards the inputs of test_gpu_large_angles.py (tests/large_angle_cases.py) without a GPU: at those start states the float32 oracle must
be a reference worth comparing a kernel with.  For every (environment, case) the GPU file uses, with the very inputs it uses (MPPI at
its four (N, H, period), CEM's last iteration at its three (N, H), the throughput sizes), built by large_angle_cases.mppi_ref / cem_ref:

 (a) the oracle's angle column equals, bit for bit in every row, that of the same oracle with each predictor step done in float64 on the
     float32 state and rounded back (StepF64) — "another association of the same arithmetic", which is what a kernel is;
 (b) J of the two agrees to rtol 2e-6 in every row (measured: <= 5.3e-7 — the GPU file allows a kernel 3e-5);
 (c) every CROSSING case first leaves the fast sin/cos range at the step it names;
 (d) all costs are finite;
 (e) for the gradient cases, rollout_cost_and_grad through the two predictors agrees to 1e-5 of the gradient's max;
 (f) no angle update of any row is a near-tie of float32 rounding (large_angle_cases.near_ties): a fused multiply-add, or a rate a few
     spacings off, could round such an angle the other way, and one spacing near 32768 rad (2e-3 .. 4e-3 rad) moves J by ~1e-4 relative.
     A first version of the GPU file showed exactly that: 1 row of 100 (Quad2D, CEM, theta0 just below the limit) and 1 row of 32832 (the
     throughput sizes) outside the J bound, every one a row this check names.  The seeds of the draws are chosen so that there is none.

A state that fails (a) or (b) is the wrong state for a tight comparison, not a reason for a wider bound: mid-range angles do fail them
(theta0 = -700.3 on Quad2D: 2 of 512 rows differ in an angle bit and J by 9.1e-6 relative; theta0 = 5000.25 on CartPole: 9.2e-5), which is
why the case lists keep away from 1e3 .. 2e4."""
import functools

import numpy as np
import pytest

from oracle import ctk_oracle as O
import large_angle_cases as L

N = 128          # the rows of the ragged N = 100 are the first 100 of these


def both(env, theta0, omega0, H, seed=None):
    """(traj, J) of plain rollouts of draws_for() through the oracle's predictor and through its float64-step form"""
    p = L.env_params(env)
    s = np.tile(L.base_state(env, theta0, omega0), (N, 1))
    Q = L.draws_for(env, N, H, seed)
    up = np.zeros(p.C, np.float32)
    out = []
    for cls in (O.Predictor, L.StepF64):
        traj = cls("ODE", dt=0.02, env=p).predict_core(s, Q)
        out.append((traj, O.Cost(p).get_trajectory_cost(traj, Q, up)))
    return out


def input_sets(env):
    """every (label, reference builder) of the GPU file for `env`: builder(theta0, omega0, predictor) -> the oracle's results"""
    sets = [(f"mppi N{n} H{h} p{p}", h, functools.partial(L.mppi_ref, env, n, h, p)) for n, h, p in L.MPPI_CONFIGS]
    sets += [(f"cem N{n} H{h}", h, functools.partial(L.cem_ref, env, n, h)) for n, h in L.CEM_SIZES]
    if env == "CartPole":
        sets += [(f"throughput p{p}", L.TP_H, functools.partial(L.mppi_ref, env, L.TP_N, L.TP_H, p)) for p in (1, 2)]
    return sets


@pytest.mark.parametrize("env", L.ENVS)
def test_oracle_is_a_tight_reference_at_every_large_angle_case(env):
    a = L.ANGLE[env]
    worst = 0.0
    for label, H, ref in input_sets(env):
        states = L.TP_STATES if label.startswith("throughput") else [(th, om) for _, th, om, _ in L.cases(env, H)]
        for th, om in states:
            r32, r64 = ref(th, om), ref(th, om, predictor=L.StepF64)
            tag = f"{env} {label} theta0 {th}"
            assert np.array_equal(r32["traj"][:, :, a].view(np.uint32), r64["traj"][:, :, a].view(np.uint32)), f"{tag}: angle bits differ"          # (a)
            assert np.isfinite(r32["J"]).all() and np.isfinite(r64["J"]).all(), tag                                                            # (d)
            worst = max(worst, float(np.max(np.abs(r32["J"].astype(np.float64) - r64["J"]) / np.abs(r64["J"]))))
            np.testing.assert_allclose(r32["J"], r64["J"], rtol=2e-6, atol=0.0, err_msg=tag)                                                   # (b)
            assert L.near_ties(r32["traj"], a).size == 0, f"{tag}: an angle update is a near-tie, choose another seed (large_angle_cases.py)"
    print(f"{env}: worst relative difference of J between the fp32 oracle and its float64-step form: {worst:.2e}")


@pytest.mark.parametrize("env", L.ENVS)
def test_crossing_cases_cross_where_they_say(env):                                                                                               # (c)
    for th, om, H, step in L.CROSSING[env]:
        (t32, _), _ = both(env, th, om, H)
        assert L.first_out_of_range_step(t32, L.ANGLE[env]) == step, (env, th, om, H)
        assert L.first_out_of_range_step(L.mppi_ref(env, N, H, 1, th, om)["traj"], L.ANGLE[env]) == step        # MPPI forms the same inputs to an ulp
        ang = np.abs(t32[:, :, L.ANGLE[env]]).max(axis=0)
        assert ang[step] >= L.LIMIT + 0.02 and (step == 0 or ang[:step].max() <= L.LIMIT - 0.02)      # an ulp in the inputs does not move it
    # the terminal-only case: no step START is out of range, so only the terminal cost's cos is beyond the fast range
    th, om, H, step = L.CROSSING[env][-1]
    assert step == H


def test_in_range_cases_stay_in_range_and_the_others_do_not():
    for env in L.ENVS:
        for th, om in L.IN_RANGE[:4]:
            (t32, _), _ = both(env, th, om, 20)
            assert L.first_out_of_range_step(t32, L.ANGLE[env]) is None, (env, th)
        for th, om in L.JUST_OUT + L.FAR_OUT:
            (t32, _), _ = both(env, th, om, 20)
            assert L.first_out_of_range_step(t32, L.ANGLE[env]) == 0, (env, th)


GRAD_CASES = L.GRAD_CASES      # what the GPU file's single-gradient and descent tests start from


@pytest.mark.parametrize("env", L.ENVS)
def test_gradient_cases_have_a_tight_reference(env):                                                                                            # (e)
    p = L.env_params(env)
    cost = O.Cost(p)
    for th, om in GRAD_CASES:
        s = np.tile(L.base_state(env, th, om), (64, 1))
        Q = L.draws_for(env, 64, 20, 3)
        up = np.zeros(p.C, np.float32)
        J1, _, g1 = O.rollout_cost_and_grad(O.Predictor("ODE", dt=0.02, env=p), cost, s, Q, up)
        J2, _, g2 = O.rollout_cost_and_grad(L.StepF64("ODE", dt=0.02, env=p), cost, s, Q, up)
        assert np.isfinite(g1).all()
        np.testing.assert_allclose(g1, g2, rtol=0.0, atol=1e-5 * np.abs(g2).max(), err_msg=f"{env} theta0 {th}")
        np.testing.assert_allclose(J1, J2, rtol=2e-6)
