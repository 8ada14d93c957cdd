"""Guards the cases of test_gpu_hyper.py (tests/hyper_cases.py) without a GPU.

 (1) the float32 oracle against the reference recordings at hyper-parameters away from the defaults (tests/golden/*hyper*.npz), at the
     bounds of test_oracle_golden.py's test_*_matches_reference* tests;
 (2) the float32 oracle against OptimF64 — the float64 statement from the primary hyper-parameters alone — at every case, within A TENTH
     of the GPU file's bounds (J, CEM's mean and deviation, one descent iteration, the warm start) and, for u_nom, within HALF of the LBD
     rule's bound (hyper_cases.u_bound: the suite's bound times 100 / LBD below LBD = 100);
 (3) sensitivity: every single-value case moves the tensor it is compared in by at least 20 bounds on at least half of the rows, against
     the same step at the defaults;
 (4) mutations of the oracle, each of which must FAIL the comparison with the recordings: k_dd and k_uu exchanged, cc_weight dropped, the
     clipped perturbation in the correction cost, the moments shifted by shift_previous, the mean's tail refilled with 0."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from helpers import (load, mppi_oracle_from, rpgd_oracle_from, cem_oracle_from, random_oracle_from, cem_naive_grad_oracle_from, cut_is_separated)
import large_angle_cases as L
import hyper_cases as Hc
from hyper_cases import OptimF64

J_TOL = dict(rtol=3e-5, atol=1e-3)             # the GPU file's
CEM_TOL = dict(rtol=1e-4, atol=1e-5)
PLAN_TOL = dict(rtol=2e-5, atol=2e-5)          # the template kernels' (CartPole's own: rtol 1e-3 / atol 2e-3)
PLAN_TOL_TUNED = dict(rtol=1e-3, atol=2e-3)
SHARE = 0.1
FACTOR = 20.0


def used(got, want, rtol, atol):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / (atol + rtol * np.abs(want))


def u_of(o):
    return np.asarray(o.u, np.float32).reshape(-1)


# ---- (1) the oracle against the recordings ---------------------------------------------------------------------------------------------
def check_mppi_fixture(d, make=mppi_oracle_from):
    o = make(d)
    np.testing.assert_array_equal(o.u_nom, d["u_nom_init"])
    assert np.array_equal(d["u_nom_init"][0, 0], 0.5 * (d["low"] + d["high"])) and np.any(d["u_nom_init"] != 0)     # the asymmetric limits' middle
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(np.broadcast_to(u_of(o), (o.C,)), d[f"u_prev_{t}"])
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.u_run, d[f"u_run_{t}"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-5, atol=2e-6)
        o.u_nom = d[f"u_nom_{t}"].copy(); o.u = O._u_out(d[f"u_{t}"])


@pytest.mark.parametrize("case", Hc.MPPI_FIXTURES)
def test_mppi_matches_reference_away_from_the_defaults(case):
    d = load(f"mppi_{case}.npz")
    assert (float(d["cc_weight"]), float(d["R"]), float(d["LBD"]), float(d["NU"])) == (np.float32(0.37), np.float32(2.3), 30.0, 2.0)
    assert float(d["SQRTRHOINV"]) == np.float32(0.2 if "saturated" in case else 0.08)
    p, H = int(d["period_interpolation_inducing_points"]), int(d["mpc_horizon"])
    assert p > 1 and (H - 1) % p != 0 and int(d["steps"]) == 3
    if case == "hyper_saturated_cartpole":
        assert d["clipped_share"].min() > 0.5                 # more than half of the perturbed inputs sit on a limit: u and delta_u differ
    check_mppi_fixture(d)


def check_rpgd_fixture(d, make=rpgd_oracle_from):
    o = make(d)
    o.optimizer_reset(d["reset_draws"])
    np.testing.assert_allclose(o.Q, d["Q_init"], rtol=1e-6, atol=1e-7)
    tol = dict(rtol=1e-4, atol=1e-4)                          # the short descents' (test_rpgd_matches_reference)
    for t in range(int(d["steps"])):
        key = f"resample_draws_{t}"
        u = o.step(d[f"s_{t}"], d[key] if key in d.files else None)
        assert (key in d.files) == ((o.count - 1) % o.resamp_per == 0)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], **tol)
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], **tol)
        np.testing.assert_allclose(o.opt.m, d[f"m_{t}"], **tol)
        np.testing.assert_allclose(o.opt.v, d[f"v_{t}"], rtol=tol["rtol"], atol=1e-4 * float(np.abs(d[f"v_{t}"]).max()))
        np.testing.assert_array_equal(o.trajectory_ages, d[f"ages_{t}"])
        np.testing.assert_allclose(o.Q_before_warmstart, d[f"Q_logged_{t}"], **tol)
        np.testing.assert_allclose(o.J, d[f"J_logged_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_logged_{t}"], rtol=1e-4, atol=1e-5)
        assert o.opt.step_count == int(d[f"adam_step_{t}"])
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], **tol)
        o.Q = d[f"Q_{t}"].copy(); o.opt.m = d[f"m_{t}"].copy(); o.opt.v = d[f"v_{t}"].copy(); o.u = O._u_out(d[f"u_{t}"])


@pytest.mark.parametrize("case", Hc.RPGD_FIXTURES)
def test_rpgd_matches_reference_away_from_the_defaults(case):
    d = load(f"rpgd_{case}.npz")
    assert (float(d["learning_rate"]), float(d["adam_beta_1"]), float(d["adam_beta_2"]), float(d["adam_epsilon"]), float(d["gradmax_clip"])) == \
        tuple(float(np.float32(x)) for x in (0.2, 0.7, 0.9, 1e-3, 0.05))
    assert int(d["shift_previous"]) == (2 if "normal" in case else 0) and int(d["resamp_per"]) == 3
    # the clip binds on every row: every rollout's first moment after the first iteration would otherwise exceed (1 - beta1) * clip
    o = rpgd_oracle_from(d)
    o.optimizer_reset(d["reset_draws"])
    _, _, g = O.rollout_cost_and_grad(o.predictor, o.cost, np.tile(d["s_0"], (o.N, 1)), o.Q, np.zeros(o.C, np.float32))
    assert np.sqrt((g.astype(np.float64) ** 2).sum(axis=(1, 2))).min() > float(d["gradmax_clip"])
    check_rpgd_fixture(d)


def test_rpgd_keeping_every_row_matches_reference():
    """opt_keep_k_ratio 1.0: k = N.  A resampling step draws an empty block, keeps every row in order of cost with its moments and age"""
    d = load(f"rpgd_{Hc.RPGD_KEEP_ALL_FIXTURE}.npz")
    o = rpgd_oracle_from(d)
    assert o.k == o.N and d["resample_draws_0"].shape[0] == 0 and "resample_draws_3" in d.files
    check_rpgd_fixture(d)
    assert np.all(d["ages_3"] == 4.0)


def check_cem_fixture(d, make=cem_oracle_from):
    o = make(d)
    np.testing.assert_array_equal(o.dist_mue, d["dist_mue_init"])
    np.testing.assert_array_equal(o.stdev, d["stdev_init"])
    K = int(d["cem_best_k"])
    for t in range(int(d["steps"])):
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=1e-6, atol=2e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-6)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        ref_best = np.argsort(d[f"J_{t}"], kind="stable")[:K]
        assert set(o.best_idx.tolist()) == set(ref_best.tolist()) and o.best_idx[0] == ref_best[0]
        np.testing.assert_allclose(o.dist_mue, d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(o.stdev, d[f"stdev_{t}"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-6, atol=1e-6)
        o.dist_mue, o.stdev = d[f"dist_mue_{t}"].copy(), d[f"stdev_{t}"].copy()
        o.u = O._u_out(d[f"u_{t}"])


def assert_hyper_cem_header(d):
    assert (float(d["cem_initial_action_stdev"]), float(d["cem_stdev_min"]), int(d["cem_best_k"])) == (np.float32(1.3), np.float32(0.4), 2)
    assert np.any(d["low"] != -d["high"])
    assert d["clamped_share"].min() > 0.5                     # the clamp binds on most elements
    first = 0.5 * (d["low"] + d["high"]) + d["noise_0"][0] * np.float32(1.3)                      # the first population, before the clip
    assert np.mean((first <= d["low"]) | (first >= d["high"])) > 0.3                              # the initial deviation saturates
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(d[f"dist_mue_{t}"][0, -1], 0.5 * (d["low"] + d["high"]))    # the refill is the limits' middle, not 0


@pytest.mark.parametrize("case", Hc.CEM_FIXTURES)
def test_cem_matches_reference_away_from_the_defaults(case):
    d = load(f"cem_{case}.npz")
    assert_hyper_cem_header(d)
    check_cem_fixture(d)


@pytest.mark.parametrize("case", Hc.RANDOM_FIXTURES)
def test_random_action_matches_reference_between_asymmetric_limits(case):
    d = load(f"random_{case}.npz")
    assert np.any(d["low"] != -d["high"])
    o = random_oracle_from(d)
    for t in range(int(d["steps"])):
        u = o.step(d[f"s_{t}"], d[f"u01_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        assert cut_is_separated(d[f"J_{t}"], 1) and int(o.best_idx) == int(np.argmin(d[f"J_{t}"]))
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-6, atol=1e-7)
        o.u = O._u_out(d[f"u_{t}"])


@pytest.mark.parametrize("case", Hc.CEM_NAIVE_GRAD_FIXTURES)
def test_cem_naive_grad_matches_reference_away_from_the_defaults(case):
    d = load(f"cem_naive_grad_{case}.npz")
    assert_hyper_cem_header(d)
    assert (float(d["learning_rate"]), float(d["gradmax_clip"])) == (np.float32(0.3), np.float32(0.05))
    o = cem_naive_grad_oracle_from(d)
    K = int(d["cem_best_k"])
    for t in range(int(d["steps"])):
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=2e-5, atol=5e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=5e-5)
        assert cut_is_separated(d[f"J_{t}"], K)
        np.testing.assert_allclose(o.dist_mue, d[f"dist_mue_{t}"], rtol=2e-5, atol=5e-6)
        np.testing.assert_allclose(o.stdev, d[f"stdev_{t}"], rtol=5e-5, atol=5e-6)
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=2e-5, atol=5e-6)
        o.dist_mue, o.stdev = d[f"dist_mue_{t}"].copy(), d[f"stdev_{t}"].copy()
        o.u = O._u_out(d[f"u_{t}"])


# ---- (4) mutations of the oracle: each fails the comparison with the recordings -------------------------------------------------------------
class ExchangedMppi(O.MPPI):
    def mppi_correction_cost(self, u, delta_u):               # k_dd and k_uu exchanged
        f = np.float32
        t = f(0.5) * self.R * (delta_u ** 2) + self.R * u * delta_u + f(0.5) * (f(1.0) - f(1.0) / self.NU) * self.R * (u ** 2)
        return np.sum(self.cc_weight * t, axis=(1, 2), dtype=np.float32)


class NoCcMppi(O.MPPI):
    def mppi_correction_cost(self, u, delta_u):               # cc_weight dropped
        return super().mppi_correction_cost(u, delta_u) / self.cc_weight


class ClippedDeltaMppi(O.MPPI):
    def mppi_correction_cost(self, u, delta_u):               # the clipped perturbation u - u_nom in place of delta_u
        shifted = np.concatenate([self.u_nom[:, 1:, :], self.u_nom[:, -1:, :]], 1)
        return super().mppi_correction_cost(u, (u - shifted).astype(np.float32))


class MomentsShiftedWithThePlans(O.RPGD):
    def step(self, s, resample_draws=None):                   # the moments shifted by shift_previous instead of one
        sp, C = self.shift_previous, self.C
        tape = []
        core = self.predictor.predict_core

        def spy(s_t, Q):                                      # the last rollout of a step is get_action's: the moments then are the descent's
            if self.opt.m is not None:
                tape.append((self.opt.m.copy(), self.opt.v.copy()))
            return core(s_t, Q)
        self.predictor.predict_core = spy
        try:
            resampled = self.count % self.resamp_per == 0
            u = super().step(s, resample_draws)
        finally:
            del self.predictor.predict_core
        shift = lambda a: np.concatenate([a[:, sp:, :], np.zeros((a.shape[0], min(sp, a.shape[1]), C), np.float32)], 1)
        m, v = (shift(a) for a in tape[-1])
        if resampled:
            z = np.zeros((self.N - self.k, self.H, C), np.float32)
            m, v = np.concatenate([z, m[self.best_idx]], 0), np.concatenate([z, v[self.best_idx]], 0)
        self.opt.m, self.opt.v = m, v
        return u


class ZeroRefillCem(O.CEM):
    def step(self, s, noise):                                 # the mean's tail refilled with 0 instead of the limits' middle
        u = super().step(s, noise)
        self.dist_mue[:, -1, :] = 0.0
        return u


def rebuilt(cls, make):
    def f(d):
        o = make(d)
        o.__class__ = cls
        return o
    return f


# (the clipped perturbation: on the saturated recordings only, u and delta_u differ where inputs clip)
WRONG_COSTS = [(c, m) for m in (ExchangedMppi, NoCcMppi, ClippedDeltaMppi) for c in Hc.MPPI_FIXTURES if m is not ClippedDeltaMppi or "saturated" in c]


@pytest.mark.parametrize("case,mutant", WRONG_COSTS, ids=[f"{m.__name__}-{c}" for c, m in WRONG_COSTS])
def test_a_wrong_correction_cost_fails_the_recordings(case, mutant):
    with pytest.raises(AssertionError):
        check_mppi_fixture(load(f"mppi_{case}.npz"), rebuilt(mutant, mppi_oracle_from))


@pytest.mark.parametrize("case", [c for c in Hc.RPGD_FIXTURES if "normal" in c])
def test_moments_shifted_with_the_plans_fail_the_recordings(case):
    d = load(f"rpgd_{case}.npz")
    assert int(d["shift_previous"]) == 2
    with pytest.raises(AssertionError):
        check_rpgd_fixture(d, rebuilt(MomentsShiftedWithThePlans, rpgd_oracle_from))


@pytest.mark.parametrize("case", Hc.CEM_FIXTURES)
def test_a_zero_refill_of_the_mean_fails_the_recordings(case):
    with pytest.raises(AssertionError):
        check_cem_fixture(load(f"cem_{case}.npz"), rebuilt(ZeroRefillCem, cem_oracle_from))


# ---- (2) the oracle against the float64 statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", Hc.ENVS)
def test_mppi_oracle_agrees_with_the_float64_statement_at_every_case(env):
    worst = dict(J=0.0, u_nom=0.0)
    for own in [()] + Hc.MPPI_CASES:
        cfg = Hc.config_of(Hc.MPPI_DEFAULTS, own)
        lo, hi = Hc.limits_of(env, own)
        for N, H, p in Hc.MPPI_SIZES:
            r = Hc.mppi_ref(env, own, N, H, p)
            J64, u64, Q64 = OptimF64.mppi_step(env, L.env_params(env), cfg, lo, hi, H, p, r["plan0"], r["u_prev"], r["noise"], r["traj"])
            np.testing.assert_allclose(r["Q"], Q64, rtol=1e-6, atol=1e-6)
            uj = float(used(r["J"], J64, **J_TOL).max())
            uu = float(used(r["u_nom"], u64, **Hc.u_bound(cfg["LBD"])).max())
            tag = f"{env} {Hc.mppi_id(own)} N{N} p{p}"
            assert uj <= SHARE, f"{tag}: J uses {uj:.3f} of the GPU bound"
            assert uu <= (0.5 if cfg["LBD"] < 100.0 else SHARE), f"{tag}: u_nom uses {uu:.3f} of the bound at LBD {cfg['LBD']}"
            worst["J"], worst["u_nom"] = max(worst["J"], uj), max(worst["u_nom"], uu)
    print(f"{env}: worst share of the GPU bound, fp32 oracle vs OptimF64: J {worst['J']:.3f} u_nom {worst['u_nom']:.3f}")


@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_oracle_agrees_with_the_float64_statement_at_every_case(env):
    for own in [()] + Hc.CEM_CASES:
        for N, H in Hc.CEM_SIZES:
            r = Hc.cem_ref(env, own, N, H)
            kw = r["kw"]
            mu64, sd64 = OptimF64.cem_finish(r["Q"][r["best"]], kw["cem_stdev_min"], kw["cem_initial_action_stdev"], r["lo"], r["hi"])
            tag = f"{env} {Hc.cem_id(own)} N{N}"
            assert float(used(r["mu"], mu64, **CEM_TOL).max()) <= SHARE, tag
            assert float(used(r["std"], sd64, **CEM_TOL).max()) <= SHARE, tag
            if dict(own).get("cem_stdev_min") == 0.4:
                assert np.mean(r["std"][:, :-1] == np.float32(0.4)) > 0.5, f"{tag}: the clamp binds on {np.mean(r['std'][:, :-1] == np.float32(0.4)):.2f} of the elements"
            if dict(own).get("cem_initial_action_stdev") == 1.3:
                assert np.mean((r["Q"] == r["lo"]) | (r["Q"] == r["hi"])) > 0.1, tag


@pytest.mark.parametrize("env", Hc.GMM_ENVS)
def test_cem_gmm_case_has_no_near_tie_and_a_clamp_that_partly_binds(env):
    r = Hc.gmm_ref(env)
    assert r["min_margin"] >= 1e-4 and r["min_cost_gap"] >= 1e-3           # (the GPU test needs 1e-5 and 1e-4)
    clamped = float(np.mean(r["std"] == np.float32(Hc.GMM_KW["cem_stdev_min"])))
    assert 0.5 < clamped < 1.0, clamped
    first = 0.5 * (r["lo"] + r["hi"]) + r["normals"][0] * np.float32(Hc.GMM_KW["cem_initial_action_stdev"])
    assert np.mean((first <= r["lo"]) | (first >= r["hi"])) > 0.3          # the initial deviation saturates


RULES = ["torch", "keras"]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_descent_iterations_agree_with_the_float64_statement(env, rule):
    """every iteration of the first step, from the oracle's own state and gradient: clip_by_norm, the Adam rule, the limits"""
    for own in [()] + Hc.RPGD_CASES:
        kw = Hc.config_of(Hc.RPGD_DEFAULTS, own)
        o = Hc.rpgd_oracle(env, own, rule)
        d0, _ = Hc.rpgd_draws(env, own)
        o.optimizer_reset(d0)
        np.testing.assert_allclose(o.Q, OptimF64.sample(d0, kw, o.low, o.high, o.H, o.period), rtol=1e-6, atol=1e-7, err_msg=f"{env} {Hc.rpgd_id(own)}")
        o.u = O._u_out(np.full(o.C, Hc.U_PREV, np.float32))
        s_t = np.tile(Hc.rpgd_state_of(env, own), (o.N, 1))
        for t in range(1, kw["outer_its"] + 1):
            _, _, g = O.rollout_cost_and_grad(o.predictor, o.cost, s_t, o.Q, u_of(o))
            norm = np.sqrt((g.astype(np.float64) ** 2).sum(axis=(1, 2)))
            if kw["gradmax_clip"] == 0.05:
                assert norm.min() > 0.05, f"{env}: the clip does not bind on every row"
            if kw["gradmax_clip"] == 1e9:                      # never binds, where the defaults' clip binds on every row
                assert norm.max() < 1e9 and norm.min() > Hc.RPGD_DEFAULTS["gradmax_clip"], f"{env}: {norm.min():.3g} .. {norm.max():.3g}"
            m0, v0 = (np.zeros_like(o.Q), np.zeros_like(o.Q)) if o.opt.m is None else (o.opt.m, o.opt.v)
            Q64, m64, v64 = OptimF64.descent_iteration(rule, g, o.Q, m0, v0, t, kw, o.low, o.high)
            o.grad_step(s_t)
            tag = f"{env} {rule} {Hc.rpgd_id(own)} iteration {t}"
            assert float(used(o.Q, Q64, **PLAN_TOL).max()) <= SHARE, tag
            np.testing.assert_allclose(o.opt.m, m64, rtol=2e-6, atol=1e-7 * float(np.abs(m64).max()), err_msg=tag)
            np.testing.assert_allclose(o.opt.v, v64, rtol=2e-6, atol=1e-7 * float(np.abs(v64).max()), err_msg=tag)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_warm_start_agrees_with_the_float64_statement(env):
    """a step of no iterations from a state with non-zero moments, resampling and not: plans by shift_previous, moments by one"""
    for own in [()] + Hc.RPGD_CASES:
        kw = Hc.config_of(Hc.RPGD_DEFAULTS, own)
        for resample in (True, False):
            o = Hc.rpgd_oracle(env, own)
            d0, d1 = Hc.rpgd_draws(env, own)
            o.optimizer_reset(d0)
            o.step(Hc.STATE[env], d1)                          # moments, ages and a count of 1
            o.outer_its = 0
            o.count = 2 if resample else 1
            o.trajectory_ages = (o.trajectory_ages + np.arange(o.N, dtype=np.float32)).astype(np.float32)
            Q, m, v, ages = o.Q.copy(), o.opt.m.copy(), o.opt.v.copy(), o.trajectory_ages.copy()
            o.step(Hc.STATE[env], d1 if resample else None)
            fresh = OptimF64.sample(d1, kw, o.low, o.high, o.H, o.period) if resample else None
            Q64, m64, v64, a64 = OptimF64.warm_start(Q, m, v, ages, o.best_idx, fresh, kw["shift_previous"])
            tag = f"{env} {Hc.rpgd_id(own)} resample={resample}"
            np.testing.assert_allclose(o.Q, Q64, rtol=1e-6, atol=1e-7, err_msg=tag)
            np.testing.assert_array_equal(o.opt.m, m64, err_msg=tag)
            np.testing.assert_array_equal(o.opt.v, v64, err_msg=tag)
            np.testing.assert_array_equal(o.trajectory_ages, a64, err_msg=tag)


# ---- (3) sensitivity ---------------------------------------------------------------------------------------------------------------------------
def share_moved(got, want, rows, rtol, atol):
    return float(np.mean(used(got, want, rtol, atol).reshape(rows, -1).max(axis=1) >= FACTOR))


@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_mppi_case_shows(env):
    names = set()
    for own in Hc.MPPI_SINGLE:
        (name, value), = own
        for N, H, p in Hc.MPPI_SIZES:
            base, r = Hc.mppi_ref(env, (), N, H, p, Hc.is_far(own)), Hc.mppi_ref(env, own, N, H, p)
            if Hc.MPPI_SHOWS_IN[name] == "J":
                share = share_moved(base["J"], r["J"], N, **J_TOL)
            else:
                assert np.array_equal(base["J"], r["J"])      # LBD leaves J alone: it shows in the update
                share = share_moved(base["u_nom"], r["u_nom"], r["u_nom"].size, **Hc.u_bound(value))
            assert share >= 0.5, f"{env} {Hc.mppi_id(own)} N{N} p{p}: only {share:.2f} of the rows move by {FACTOR}x the bound"
        names.add(name)
    assert names == set(Hc.MPPI_DEFAULTS) | {"limits"}
    everything = dict(Hc.MPPI_ALL)
    assert all(everything[k] != v for k, v in Hc.MPPI_DEFAULTS.items()) and everything["cc_weight"] != everything["R"]
    assert 0.5 * (1 - 1 / everything["NU"]) != 0.5            # k_dd != k_uu by far


@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_cem_case_shows(env):
    for own in Hc.CEM_SINGLE:
        for N, H in Hc.CEM_SIZES:
            base, r = Hc.cem_ref(env, (), N, H), Hc.cem_ref(env, own, N, H)
            share = share_moved(base["std"], r["std"], r["std"].size, **CEM_TOL)
            assert share >= 0.5, f"{env} {Hc.cem_id(own)} N{N}: only {share:.2f} of STD's elements move by {FACTOR}x the bound"


def rpgd_moved(env, own):
    """the share of rows on which a single-value case moves the tensor it shows in, at the LOOSEST bound a kernel is held to"""
    names = dict(own)
    base, r = Hc.rpgd_ref(env, (), far=own == Hc.RPGD_CLIP_NEVER), Hc.rpgd_ref(env, own)     # the same state at the defaults
    N = Hc.RPGD_N
    a, b = base["steps"][1], r["steps"][1]                    # the second step: moments of five iterations behind it, no resampling
    if "shift_previous" in names:
        return share_moved(a["Q"], b["Q"], N, **PLAN_TOL_TUNED)
    if "SAMPLING_DISTRIBUTION" in names or "uniform_dist_min" in names:
        return share_moved(base["Q_init"], r["Q_init"], N, **PLAN_TOL_TUNED)
    if "adam_beta_1" in names or "gradmax_clip" in names:
        return share_moved(a["m"], b["m"], N, rtol=2e-3, atol=2e-4 * float(np.abs(b["m"]).max()))
    if "adam_beta_2" in names:
        return share_moved(a["v"], b["v"], N, rtol=4e-3, atol=4e-4 * float(np.abs(b["v"]).max()))
    return share_moved(a["descended"], b["descended"], N, **PLAN_TOL_TUNED)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_rpgd_case_shows(env):
    for own in Hc.RPGD_SINGLE:
        share = rpgd_moved(env, own)
        assert share >= 0.5, f"{env} {Hc.rpgd_id(own)}: only {share:.2f} of the rows move by {FACTOR}x the bound"
