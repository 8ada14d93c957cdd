"""Guards the cases of test_gpu_params.py (tests/param_cases.py) without a GPU.  For every environment and every case (one per plant or
cost parameter, and ALL), with the very plans that file rolls out (param_cases.inputs_of: MPPI at both sizes, CEM's last iteration,
random action, plain rollouts):

 (1) the float32 oracle at the perturbed parameters agrees with PlantF64 — the float64 statement from the primary parameters alone, which
     shares no derived constant with the oracle or the library, stepping the float32 state and rounding after every step — on TRAJ and J
     within A TENTH of the GPU file's bounds (J: rtol 3e-6 / atol 1e-4; TRAJ: rtol 1e-5 / atol 3e-6).  A derivation that the oracle and
     the library's derive() get wrong in the same way fails here;
 (2) sensitivity: for every single-parameter case the tensor in which the parameter shows (TRAJ for a parameter of the dynamics, J for
     one of the cost), with and without the perturbation, differs by at least 20x the GPU bound atol + rtol |want| on at least half of
     the rows (rollouts; a row of TRAJ counts by its worst element), on EVERY set of plans.  No parameter is left without such a
     case: 17 / 18 / 21 names, counted;
 (3) the oracle's hand-written reverse mode at the perturbed parameters against float64 autograd through PlantF64 (and, for the cost
     parameters, through an MLP and a GRU step written out in torch), at the bounds of test_oracle_adjoints_match_torch_autograd_fp64;
 (4) angle roundings: large_angle_cases.near_ties is a tool for angles of ~3e4 rad, where one float32 spacing of the angle moves J by 1e-4
     relative.  At the ordinary state of these cases it flags every row (the window it allows for another association, 16 spacings of
     omega, is as wide as the angle's own spacing), so it cannot be "empty" here and choosing seeds cannot make it so.  What it stands for
     is asserted instead: one spacing of every angle of every trajectory is below a hundredth of TRAJ's bound at that angle (|angle| < 8
     rad: at most 4.8e-7 against 3e-5 + 1e-4 |angle|), so an angle that rounds the other way in a kernel uses a hundredth of a bound, and
     param_cases.SEEDS stays empty.

Measured (worst share of the GPU bound that the oracle and PlantF64 differ by, over all cases and plans): CartPole J 0.043 TRAJ 0.089,
Quad2D J 0.013 TRAJ 0.069, Hover J 0.009 TRAJ 0.013.  The one case above a tenth was CartPole target_equilibrium = -1 from the state
(0.4, -0.7): 0.19 on J, through one of rollout()'s plans whose J = 4.6 is a difference of terms of ~3000; it starts from (0.2, -0.3)
instead (param_cases.STATE_FOR), where it measures 0.02."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
import large_angle_cases as L
import param_cases as P

J_TOL = dict(rtol=3e-5, atol=1e-3)             # the GPU file's
TRAJ_TOL = dict(rtol=1e-4, atol=3e-5)
SHARE = 0.1                                    # (1): a tenth of them
FACTOR = 20.0                                  # (2)


def used(got, want, rtol, atol):
    return np.abs(np.asarray(got, np.float64) - want) / (atol + rtol * np.abs(want))


@pytest.mark.parametrize("env", P.ENVS)
def test_oracle_agrees_with_the_float64_statement_at_every_case(env):                                                                    # (1)
    worst = dict(J=0.0, TRAJ=0.0)
    for own in CASES_OF(env):
        cost = O.Cost(P.params_with(env, own))
        for label, s, Q, up, traj in P.inputs_of(env, own):
            t64, J64 = P.plant_check(env, own, s, Q, up)
            uj = float(used(cost.get_trajectory_cost(traj, Q, up), J64, **J_TOL).max())
            ut = float(used(traj, t64, **TRAJ_TOL).max())
            assert np.isfinite(J64).all() and uj <= SHARE and ut <= SHARE, f"{env} {P.case_id(env, own)} {label}: J {uj:.3f} TRAJ {ut:.3f} of the GPU bound"
            worst["J"], worst["TRAJ"] = max(worst["J"], uj), max(worst["TRAJ"], ut)
    print(f"{env}: worst share of the GPU bound, fp32 oracle vs PlantF64: J {worst['J']:.3f} TRAJ {worst['TRAJ']:.3f}")


def CASES_OF(env):
    return [(), P.DEFAULTS[env]] + P.CASES[env]                 # the unperturbed parameters and the library's defaults too


def rows_moved(env, own):
    """per set of plans: the share of rows on which the perturbation moves its tensor by FACTOR bounds or more"""
    dyn = P.is_dynamics(env, own[0][0])
    base = P.params_with(env, ())
    out = []
    for label, s, Q, up, traj in P.inputs_of(env, own):
        without = O.Predictor("ODE", dt=P.DT, env=base).predict_core(np.tile(s, (Q.shape[0], 1)), Q)
        if dyn:
            u = used(without, traj, **TRAJ_TOL).reshape(Q.shape[0], -1).max(axis=1)
        else:
            assert np.array_equal(without, traj)                          # a cost parameter leaves the dynamics alone
            u = used(O.Cost(base).get_trajectory_cost(without, Q, up), O.Cost(P.params_with(env, own)).get_trajectory_cost(traj, Q, up), **J_TOL)
        out.append((label, float(np.mean(u >= FACTOR))))
    return out


@pytest.mark.parametrize("env", P.ENVS)
def test_every_parameter_has_a_case_that_shows(env):                                                                                     # (2)
    kept = set()
    for own in P.SINGLE[env]:
        (name, value), = own
        d = float(getattr(P.defaults(env), name))
        assert value not in (d, 0.0, 1.0) and value != float(getattr(P.params_with(env, ()), name))
        if d != 0.0 and own != (("target_equilibrium", -1.0),):            # (-1: the other equilibrium, a second case of its parameter)
            m = np.frexp(abs(value / d))[0]
            assert m != 0.5, f"{name}: {value} is the default times a power of two"
        for label, share in rows_moved(env, own):
            assert share >= 0.5, f"{env} {P.case_id(env, own)} {label}: only {share:.2f} of the rows move by {FACTOR}x the bound"
        kept.add(name)
    assert kept == set(P.param_names(env)) and len(kept) == {"CartPole": 17, "Quad2D": 18, "Hover": 21}[env]
    assert P.CASES[env][-1] == P.ALL[env] and len(P.CASES[env]) == len(P.SINGLE[env]) + 1
    everything = dict(P.ALL[env])
    assert set(everything) == set(P.param_names(env)) and everything["cc_weight"] != everything["R"]
    for name, value in everything.items():
        assert value not in (float(getattr(P.defaults(env), name)), 0.0, 1.0), name
    if env == "CartPole":
        assert (("target_equilibrium", -1.0),) in P.SINGLE[env]


GRAD_KINDS = [("ODE", None), ("MLP", "cost"), ("GRU", "cost")]


@pytest.mark.parametrize("kind,which", GRAD_KINDS, ids=[k for k, _ in GRAD_KINDS])
@pytest.mark.parametrize("env", P.ENVS)
def test_oracle_gradients_at_the_perturbed_parameters(env, kind, which):                                                                 # (3)
    N, H = (16, 20) if kind == "ODE" else (8, 15)
    for own in [()] + (P.CASES[env] if which is None else P.cost_cases(env)):
        J, g = P.oracle_grad(env, kind, own, N, H)
        J64, g64 = P.grad_ref(env, kind, own, N, H)
        tag = f"{env} {kind} {P.case_id(env, own)}"
        np.testing.assert_allclose(J, J64, rtol=2e-5, err_msg=tag)
        np.testing.assert_allclose(g, g64, rtol=2e-4, atol=2e-6 * max(1.0, float(np.abs(g64).max())), err_msg=tag)


@pytest.mark.parametrize("env", P.ENVS)
def test_an_angle_rounded_the_other_way_cannot_use_a_bound(env):                                                                         # (4)
    a = L.ANGLE[env]
    for own in CASES_OF(env):
        for label, s, Q, up, traj in P.inputs_of(env, own):
            ang = np.abs(traj[:, :, a]).astype(np.float64)
            share = float((np.spacing(np.abs(traj[:, :, a])) / (TRAJ_TOL["atol"] + TRAJ_TOL["rtol"] * ang)).max())
            assert share <= 0.01, f"{env} {P.case_id(env, own)} {label}: {share:.2e}"
    assert P.SEEDS == {}


def test_float64_statement_rounds_its_parameters_as_the_abi_does():
    for env in P.ENVS:
        plant = P.PlantF64(env, P.params_with(env, P.ALL[env]))
        for name, value in P.ALL[env]:
            assert getattr(plant, name) == float(np.float32(value))
        assert plant.dt == float(np.float32(0.02))


def test_sizes_and_state_are_the_ones_agreed():
    import substep_cases as S
    assert P.SIZES == [(100, 20, 5), (128, 20, 1)] and P.NET_SIZE == (48, 15) and P.STATE == S.ORDINARY[0] == (0.4, -0.7)
    assert set(P.STATE_FOR) == {("CartPole", (("target_equilibrium", -1.0),))}
