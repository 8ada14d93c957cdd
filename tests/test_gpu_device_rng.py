"""-m gpu: the in-kernel Philox4x32-10 draws (samples = None, CTK_LOC_NONE) of every optimizer against the oracle.

Every case steps an engine WITHOUT samples and the oracle WITH tests/philox_cases.py: expected_samples at the engine's reported Philox
position, then compares the first tensor the draws reach (Q where materialised, PLAN after an RPGD reset / the fresh rows after a
resampling step), J, the distribution (U_NOM / STD), BEST_IDX and u at the tolerances of the same optimizer's oracle-seeded test with
host samples.  tests/test_philox_cases_cpu.py shows on the CPU that the oracle's float32 Box-Muller rounding is below a fifth of the
J tolerance on these shapes, so a failure here is a wrong stream, column block, row, call or kind, not rounding.  Each case names the
kernel it means to cover.  Comparisons go through tests/margins.py: the observed errors are kept in profiles/r13_device_rng_margins.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine
from gpu_helpers import apply_env
from margins import close, record
import philox_cases as PC
from philox_cases import SEED, expected_samples
from gmm_oracle import CEMGMM
from test_gpu_mppi import U_TOL
from test_gpu_rpgd import assert_close_mostly
from test_gpu_env import QLO, QHI, S0 as QUAD_S0, quad_env, apply_params
from test_gpu_hover import HLO, HHI, S0 as HOVER_S0, j_tol as hover_j_tol

pytestmark = pytest.mark.gpu

J_RTOL = PC.J_RTOL                      # test_gpu_mppi.py / test_gpu_cem_random.py: rtol 3e-5 (analytic predictor)
NET_J = dict(rtol=5e-5, atol=1e-3)      # test_gpu_mlp.py (MLP);  GRU: test_gpu_hover.py: j_tol
ENVS = {
    "CartPole": dict(env=lambda: O.EnvParams(terminal_weight=0.3, target_position=0.05), lo=-1.0, hi=1.0, s0=PC.S0, S=4, C=1),
    "Quad2D": dict(env=quad_env, lo=QLO, hi=QHI, s0=QUAD_S0, S=6, C=2),
    "Hover": dict(env=lambda: O.HoverParams(target_x=0.3), lo=HLO, hi=HHI, s0=HOVER_S0, S=7, C=3),
}


def weights_for(pred, envname, hidden=(32, 32)):
    S, C = ENVS[envname]["S"], ENVS[envname]["C"]
    if pred == "MLP":
        return O.mlp_default_weights(1, S + C, S, hidden) if hidden != (32, 32) else O.mlp_default_weights(1, S + C, S)
    return O.gru_default_weights(3, S + C, S) if pred == "GRU" else None


def make(opt, pred, envname, N, H, okw, ekw, hidden=(32, 32), lo=None, hi=None, **common):
    """(environment record, predictor, oracle, engine): the same configuration on both sides, seed = SEED"""
    E = ENVS[envname]
    env, w = E["env"](), weights_for(pred, envname, hidden)
    lo, hi = (E["lo"] if lo is None else lo), (E["hi"] if hi is None else hi)
    seed = common.pop("seed", SEED)
    p = O.Predictor(pred, dt=0.02, env=env, weights=w, **(dict(hidden_sizes=hidden) if hidden != (32, 32) else {}))
    cls = {"mppi": O.MPPI, "cem": O.CEM, "random_action": O.RandomAction, "rpgd": O.RPGD, "gradient": O.GradientTF,
           "cem_naive_grad": O.CEMNaiveGrad, "cem_grad_bharadhwaj": O.CEMGradBharadhwaj, "cem_gmm": CEMGMM}[opt]
    o = cls(p, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, **okw)
    e = CtkEngine(opt, pred, environment=envname, num_rollouts=N, mpc_horizon=H, dt=0.02, action_low=lo, action_high=hi, seed=seed,
                  **(dict(predictor_hidden=hidden) if hidden != (32, 32) else {}), **ekw, **common)
    (apply_env if envname == "CartPole" else apply_params)(e, env)
    if w is not None:
        e.set_predictor_weights(w)
    return E, p, o, e


def j_tol(pred, envname):
    return dict(rtol=J_RTOL) if pred == "ODE" else hover_j_tol("GRU") if pred == "GRU" else NET_J


def u_vec(u):
    return np.asarray(u, np.float32).reshape(-1)


def best_idx_check(tag, got, o_J, o_best, K, rtol, atol=0.0):
    """BEST_IDX position by position wherever the oracle's neighbouring sorted costs (the cut K-1 | K included) are further apart than
    the J tolerance on both sides (2 * (atol + rtol |J|)); otherwise, with a clear cut, the elite SET"""
    srt = np.sort(np.asarray(o_J, np.float64))[: K + 1]
    gaps = np.diff(srt) / (2 * (atol + rtol * np.abs(srt[:-1])))          # > 1: further apart than both sides' tolerance
    got, want = np.asarray(got).reshape(-1)[:K], np.asarray(o_best).reshape(-1)[:K]
    if len(gaps) == 0 or gaps.min() > 1:
        np.testing.assert_array_equal(got, want, err_msg=tag)
    elif len(srt) <= K or gaps[K - 1] > 1:
        assert set(got.tolist()) == set(want.tolist()), tag
    else:
        print(f"{tag}: the oracle's costs at the cut are within the J tolerance: BEST_IDX not compared")


def advanced(e, before):
    assert e.rng_position() == before + 1, f"Philox position {e.rng_position()} after a completed step from {before}"


# ======================================================================================================================
# MPPI
# ======================================================================================================================
def mppi_step(tag, E, p, o, e, s, pred="ODE", envname="CartPole", logging=True, off=0):
    """one device-draw step against the oracle fed expected_samples at the engine's reported position; re-pins the engine"""
    N, H, C = o.N, o.H, o.C
    pos = e.rng_position()
    z = expected_samples("mppi", dict(N=N, H=H, C=C, P=o.P, offset=off), SEED, pos)
    assert z.size == e.samples_needed()
    uo, ug = o.step(s, z.reshape(N, o.P, C)), e.step(s)
    advanced(e, pos)
    if logging:
        close(tag, "Q", e.read("Q"), o.u_run, rtol=1e-4, atol=2e-6)          # test_mppi_device_rng_matches_oracle_philox: Box-Muller rounding
    close(tag, "J", e.read("J"), o.J, **j_tol(pred, envname))
    close(tag, "U_NOM", e.read("U_NOM"), o.u_nom, **U_TOL)
    close(tag, "u", ug, u_vec(uo), **U_TOL)
    if pred == "GRU":
        e.predictor_set_hidden(p.hidden)
    e.set_state(np.concatenate([o.u_nom.reshape(-1), u_vec(uo)]).astype(np.float32))
    return uo


@pytest.mark.parametrize("mat", [True, False])
@pytest.mark.parametrize("N,H,period,off", PC.MPPI_ODE_SHAPES)
def test_mppi_ode_device_draws(N, H, period, off, mat):
    """CartPole ODE, both instantiations (logging / not), the headline shape, ragged N, P % 4 != 0, N = 1, a global row offset"""
    E, p, o, e = make("mppi", "ODE", "CartPole", N, H, dict(period_interpolation_inducing_points=period),
                      dict(period_interpolation_inducing_points=period, materialize_trajectories=mat, global_rollout_offset=off))
    name = e.dominant_kernel()
    print(f"N{N} H{H} period {period}: {name}, P = {o.P}")
    if (N, H, period) == (1024, 50, 1):
        assert name == f"ctk_mppi_rollout<0, 0, {'true' if mat else 'false'}, false>", name
    assert name.startswith(f"ctk_mppi_rollout<0, 0, {'true' if mat else 'false'}, false"), name
    if (N, H, period) == (130, 35, 10):
        assert o.P == 5 and o.P % 4 != 0 and N % 64 != 0
    assert e.rng_position() == 0
    s = E["s0"].copy()
    for t in range(3):
        uo = mppi_step(f"mppi ODE N{N} H{H} p{period} mat={mat} step {t}", E, p, o, e, s, logging=mat, off=off)
        s = p.step(s.reshape(1, 4), u_vec(uo).reshape(1, 1))[0]
    e.close()


@pytest.mark.parametrize("period", [1, 2])
def test_mppi_throughput_kernel_device_draws(period):
    """the smallest ragged N of the single-wave throughput kernel (N >= 32768), logging on and off"""
    N, H = 32768 + 3, 6
    for mat in (True, False):
        E, p, o, e = make("mppi", "ODE", "CartPole", N, H, dict(period_interpolation_inducing_points=period),
                          dict(period_interpolation_inducing_points=period, materialize_trajectories=mat))
        assert "ctk_mppi_rollout_tp" in e.dominant_kernel(), e.dominant_kernel()
        s = E["s0"].copy()
        for t in range(2):
            uo = mppi_step(f"mppi tp N{N} p{period} mat={mat} step {t}", E, p, o, e, s, logging=mat)
            s = p.step(s.reshape(1, 4), u_vec(uo).reshape(1, 1))[0]
        assert "ctk_mppi_rollout_tp" in e.dominant_kernel(), e.dominant_kernel()
        e.close()


# (predictor, environment, N, H, period, engine keywords, hidden widths, what the kernel's name must contain)
NET_CASES = [
    ("MLP", "CartPole", 130, 7, 3, {}, (32, 32), "ctk_mppi_rollout<0, 3, true"),                                 # the tuned pair kernel
    ("GRU", "CartPole", 130, 7, 3, {}, (32, 32), "ctk_mppi_rollout<0, 2, "),                               # the tuned 4-wave GRU kernel
    ("MLP", "CartPole", 130, 7, 3, {}, (64, 64), "SplitMlp64<false>"),                                     # the 64-unit MLP
    ("MLP", "CartPole", 130, 7, 3, dict(generic_kernels=True), (32, 32), "ctk_g_rollout_split<0, SplitMlp<false>, 0, true, 1>"),
    ("MLP", "CartPole", 4128, 6, 2, dict(generic_kernels=True), (32, 32), "ctk_g_rollout_split<0, SplitMlp<false>, 0, true, 2>"),   # 258 tiles: two per workgroup
    ("MLP", "Hover", 130, 7, 1, {}, (32, 32), "ctk_g_rollout_split<2, "),                                  # P*C = 21: odd, C = 3
]


@pytest.mark.parametrize("pred,envname,N,H,period,ekw,hidden,kernel", NET_CASES)
def test_mppi_network_kernels_device_draws(pred, envname, N, H, period, ekw, hidden, kernel):
    E, p, o, e = make("mppi", pred, envname, N, H, dict(period_interpolation_inducing_points=period),
                      dict(period_interpolation_inducing_points=period, materialize_trajectories=True, **ekw), hidden=hidden)
    print(f"{pred} {envname} N{N}: {e.dominant_kernel()}")
    assert kernel in e.dominant_kernel(), e.dominant_kernel()
    if envname == "Hover":
        assert (o.P * o.C) % 2 == 1 and o.C == 3
    if pred == "GRU":
        h0 = (0.2 * np.random.default_rng(0).standard_normal((2, 32))).astype(np.float32)
        e.predictor_set_hidden(h0); p.hidden = h0.copy()
    s = E["s0"].copy()
    for t in range(2):
        mppi_step(f"mppi {pred}{hidden[0]} {envname} N{N} {'template' if ekw else 'own'} step {t}", E, p, o, e, s, pred=pred, envname=envname)
        s = (s + np.resize(np.array([0.01, 0.0, -0.02, 0.01], np.float32), s.size)).astype(np.float32)
    e.close()


# ======================================================================================================================
# CEM (one launch and launch per phase), random-action
# ======================================================================================================================
def cem_state(o):
    return np.concatenate([o.dist_mue.reshape(-1), o.stdev.reshape(-1), u_vec(o.u), [getattr(o, "count", 0)]]).astype(np.float32)


def cem_step(tag, o, e, s, pred="ODE", envname="CartPole", opt="cem", seed=SEED):
    N, H, C, K = o.N, o.H, o.C, o.K
    its = o.iterations() if opt == "cem" else o.cem_outer_it
    pos = e.rng_position()
    z = expected_samples(opt, dict(N=N, H=H, C=C, its=its), seed, pos)
    assert z.size == e.samples_needed()
    uo, ug = o.step(s, z.reshape(its, N, H, C)), e.step(s)
    advanced(e, pos)
    if opt == "cem":                                  # tolerances: test_gpu_cem_random.py::test_cem_matches_oracle (test_gpu_mlp.py for the MLP)
        close(tag, "Q", e.read("Q"), o.Q, rtol=1e-5, atol=2e-6)
        close(tag, "J", e.read("J"), o.J, **j_tol(pred, envname))
        best_idx_check(tag, e.read("BEST_IDX"), o.J, o.best_idx, K, **j_tol(pred, envname))
        close(tag, "U_NOM", e.read("U_NOM"), o.dist_mue, rtol=1e-4, atol=1e-5 if pred == "ODE" else 2e-5)
        close(tag, "STD", e.read("STD"), o.stdev, rtol=1e-4, atol=1e-5 if pred == "ODE" else 2e-5)
        close(tag, "u", ug, u_vec(uo), rtol=1e-5, atol=2e-6)
    else:                                             # cem-naive-grad: test_gpu_variants.py::test_cem_naive_grad_matches_oracle
        close(tag, "Q", e.read("Q"), o.Q, rtol=1e-4, atol=2e-4)
        close(tag, "J", e.read("J"), o.J, rtol=2e-4, atol=1e-2)
        close(tag, "U_NOM", e.read("U_NOM"), o.dist_mue, rtol=1e-4, atol=1e-4)
        close(tag, "STD", e.read("STD"), o.stdev, rtol=1e-3, atol=1e-4)
        close(tag, "u", ug, u_vec(uo), rtol=1e-4, atol=1e-4)
    e.set_state(cem_state(o))
    return uo


def cem_compare(monkeypatch, form, pred, envname, N, H, K, its, steps=2, seed=SEED, mat=True):
    """the comparison of one CEM configuration in one device form ("one_launch" / "per_phase": CTK_NO_CEM_FUSED at creation)"""
    kw = dict(cem_outer_it=its, cem_best_k=K)
    if form == "per_phase":
        monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")
    try:
        E, p, o, e = make("cem", pred, envname, N, H, kw, dict(kw, materialize_trajectories=mat), seed=seed)
    finally:
        if form == "per_phase":
            monkeypatch.delenv("CTK_NO_CEM_FUSED")
    name = e.dominant_kernel()
    print(f"cem {pred} {envname} N{N} {form}: {name}")
    if pred == "ODE":
        assert name.startswith("ctk_cem_fused<" if form == "one_launch" else "ctk_affine_rollout<"), name
    else:
        assert "ctk_cem_fused" not in name, name      # the network predictors have the launch-per-phase form only
    s = E["s0"].copy()
    for t in range(steps):
        uo = cem_step(f"cem {pred} {envname} N{N} H{H} {form} step {t}", o, e, s, pred, envname, seed=seed)
        assert np.isfinite(u_vec(uo)).all()
        s = p.step(s.reshape(1, -1), u_vec(uo).reshape(1, -1))[0]
    e.close()


CEM_CASES = [(form, "ODE", "CartPole") + shape for shape in PC.CEM_ODE_SHAPES for form in ("one_launch", "per_phase")] + \
            [("per_phase", "MLP", "CartPole", 256, 12, 32, 2), ("one_launch", "ODE", "Quad2D", 130, 7, 13, 2), ("per_phase", "ODE", "Quad2D", 130, 7, 13, 2)]


@pytest.mark.parametrize("form,pred,envname,N,H,K,its", CEM_CASES)
def test_cem_device_draws(monkeypatch, form, pred, envname, N, H, K, its):
    """stream `it` for outer iteration `it`, in both device forms (the network predictors have the launch-per-phase form only)"""
    cem_compare(monkeypatch, form, pred, envname, N, H, K, its)


@pytest.mark.parametrize("envname", ["Quad2D", "Hover"])
def test_random_action_device_draws(envname):
    N, H = 65, 7
    E, p, o, e = make("random_action", "ODE", envname, N, H, {}, dict(materialize_trajectories=True))
    assert e.dominant_kernel().startswith("ctk_affine_rollout<%d, " % {"Quad2D": 1, "Hover": 2}[envname]), e.dominant_kernel()
    C = o.C
    s = E["s0"].copy()
    for t in range(3):
        pos = e.rng_position()
        u01 = expected_samples("random_action", dict(N=N, H=H, C=C), SEED, pos).reshape(N, H, C)
        uo, ug = o.step(s, u01), e.step(s)
        advanced(e, pos)
        tag = f"random {envname} step {t}"
        close(tag, "Q", e.read("Q"), (E["lo"] + u01 * (E["hi"] - E["lo"])).astype(np.float32), rtol=0, atol=1e-6)
        close(tag, "J", e.read("J"), o.J, rtol=J_RTOL)
        best_idx_check(tag, e.read("BEST_IDX"), o.J, [o.best_idx], 1, J_RTOL)
        # u = the first input of the oracle's best plan: the SAME row (the index, exactly), its value as the engine formed it (lo + u * span
        # contracts to one FMA on the device: one ulp from the oracle's two roundings where the span is no power of two; Q's bound above)
        bi = int(e.read("BEST_IDX")[0])
        np.testing.assert_array_equal(ug, e.read("Q")[bi, 0, :])
        if bi == int(o.best_idx):                                                # (best_idx_check above demands it unless the two best costs tie)
            close(tag, "u", ug, o.Q[o.best_idx, 0, :], rtol=0, atol=1e-6)
        s = p.step(s.reshape(1, -1), u_vec(uo).reshape(1, -1))[0]
    e.close()


# ======================================================================================================================
# RPGD
# ======================================================================================================================
def rpgd_state(o):
    return np.concatenate([o.Q.ravel(), o.opt.m.ravel(), o.opt.v.ravel(), o.trajectory_ages.ravel(), u_vec(o.u), [o.opt.step_count], [o.count]]).astype(np.float32)


def make_rpgd(pred, envname, N, H, period, k, kind="uniform", whole=True, its=3, resamp_per=2, lo=None, hi=None, **ekw):
    okw = dict(outer_its=its, resamp_per=resamp_per, period_interpolation_inducing_points=period, SAMPLING_DISTRIBUTION=kind, shift_previous=1,
               learning_rate=0.05, opt_keep_k_ratio=(k + 0.5) / N, gradmax_clip=5.0, sample_whole_control_space=whole, uniform_dist_min=-0.7,
               uniform_dist_max=0.6, sample_stdev=0.5, sample_mean=0.1)
    kw = dict(outer_its=its, resamp_per=resamp_per, period_interpolation_inducing_points=period, sampling_distribution=0 if kind == "uniform" else 1,
              shift_previous=1, learning_rate=0.05, opt_keep_k=k, gradmax_clip=5.0, sample_whole_control_space=int(whole), sample_min=-0.7,
              sample_max=0.6, sample_stdev=0.5, sample_mean=0.1, **ekw)
    E, p, o, e = make("rpgd", pred, envname, N, H, okw, kw, lo=lo, hi=hi)
    assert o.k == k
    return E, p, o, e


def rpgd_reset_both(tag, o, e, kind):
    """device-draw reset against the oracle's reset fed expected_samples: PLAN at 1e-6 (uniform: exact words, one affine map and the
    interpolation; normal: + the transform's rounding times sample_stdev = 0.5)"""
    N, H, C = o.N, o.H, o.C
    pos = e.rng_position()
    d0 = expected_samples("rpgd", dict(N=N, H=H, C=C, P=o.P, kind=kind), SEED, pos, "reset")
    assert d0.size == e.samples_needed_reset()
    o.optimizer_reset(d0.reshape(N, o.P, C)); e.reset()
    advanced(e, pos)
    close(tag, "PLAN", e.read("PLAN"), o.Q, rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(e.read("AGES"), 0)


@pytest.mark.parametrize("whole", [True, False])
@pytest.mark.parametrize("kind", ["uniform", "normal"])
@pytest.mark.parametrize("envname", ["CartPole", "Quad2D", "Hover"])
def test_rpgd_reset_device_draws(envname, kind, whole):
    """each sampling_distribution, sample_whole_control_space on and off (limits other than the sample range), C = 1, 2, 3"""
    lo, hi = (-0.9, 0.8) if envname == "CartPole" else (None, None)
    E, p, o, e = make_rpgd("ODE", envname, 33, 9, 4, 8, kind=kind, whole=whole, lo=lo, hi=hi)
    assert e.rng_position() == 0
    rpgd_reset_both(f"rpgd reset {envname} {kind} whole={whole}", o, e, kind)
    x = e.read("PLAN")
    if kind == "uniform" and not whole:
        assert x.min() >= -0.7 - 1e-6 and x.max() <= 0.6 + 1e-6                  # the sample range, inside every limit used here
    e.close()


# (name, predictor, environment, N, H, period, k, engine keywords, kernel name, tolerance of the descended plans)
ODE_TOL = dict(rtol=1e-3, atol=2e-3)                   # test_gpu_rpgd.py::test_rpgd_ode_matches_oracle
RPGD_FORMS = [
    ("single_launch", "ODE", "CartPole", 48, 12, 5, 8, {}, "ctk_rpgd_descent<0>", ODE_TOL),
    ("separate_launches", "ODE", "CartPole", 130, 9, 4, 13, {}, "ctk_rpgd_descent<0>", ODE_TOL),
    ("template", "ODE", "CartPole", 130, 9, 4, 13, dict(generic_kernels=True), "ctk_g_rpgd_descent<0>", ODE_TOL),
    ("template_quad2d", "ODE", "Quad2D", 48, 12, 5, 8, {}, "ctk_g_rpgd_descent<1>", ODE_TOL),
    ("template_hover_normal", "ODE", "Hover", 48, 12, 5, 8, {}, "ctk_g_rpgd_descent<2>", ODE_TOL),
    ("persistent_mlp", "MLP", "CartPole", 72, 20, 5, 18, {}, "ctk_rpgd_mlp_persistent", dict(rtol=2e-4, atol=2e-4)),   # test_gpu_net_shapes.py
]


def rpgd_steps(name, pred, envname, N, H, period, k, ekw, kernel, tol):
    kind = "normal" if name.endswith("normal") else "uniform"
    E, p, o, e = make_rpgd(pred, envname, N, H, period, k, kind=kind, **ekw)
    print(f"rpgd {name}: {e.dominant_kernel()}")
    assert e.dominant_kernel() == kernel, e.dominant_kernel()
    if name == "single_launch":
        assert N <= 64 and not ekw                     # one workgroup holds the population: descent, keep-k and warm start in one launch
    C = o.C
    rpgd_reset_both(f"rpgd {name} reset", o, e, kind)
    s = E["s0"].copy()
    for t in range(4):                                 # resamp_per = 2: steps 0 and 2 resample
        tag = f"rpgd {name} step {t}"
        pos = e.rng_position()
        assert pos == t + 1
        resample = t % 2 == 0
        assert (e.samples_needed() > 0) == resample
        dr = expected_samples("rpgd", dict(N=N, H=H, C=C, P=o.P, k=k, kind=kind), SEED, pos).reshape(N - k, o.P, C) if resample else None
        assert dr is None or dr.size == e.samples_needed()
        uo, ug = o.step(s, dr), e.step(s)
        advanced(e, pos)                               # a step that does not resample moves the position too
        plan = e.read("PLAN")
        if resample:
            close(tag, "PLAN fresh", plan[: N - k], o.Q[: N - k], rtol=1e-6, atol=1e-6)
        record(tag, "PLAN", plan, o.Q, **tol)
        assert_close_mostly(plan, o.Q, max_outliers=max(4, o.Q.size // 400), **tol)       # keepers: the descent behind them
        np.testing.assert_array_equal(e.read("AGES"), o.trajectory_ages)
        assert (e.read("AGES").min() == 1.0) == resample
        close(tag, "J", e.read("J"), o.J, rtol=2e-3, atol=1e-2)
        close(tag, "u", ug, u_vec(uo), rtol=1e-3, atol=2e-3)
        best_idx_check(tag, e.read("BEST_IDX"), o.J, o.best_idx, k, rtol=2e-3, atol=1e-2)
        e.set_state(rpgd_state(o))
        s = (s + np.resize(np.array([0.01, 0.0, -0.02, 0.01], np.float32), s.size)).astype(np.float32)
    e.close()


@pytest.mark.parametrize("name,pred,envname,N,H,period,k,ekw,kernel,tol", RPGD_FORMS, ids=[f[0] for f in RPGD_FORMS])
def test_rpgd_step_device_draws(name, pred, envname, N, H, period, k, ekw, kernel, tol):
    """reset, then four steps with resamp_per = 2: the fresh rows after each resampling step, every row against the oracle, the ages"""
    rpgd_steps(name, pred, envname, N, H, period, k, ekw, kernel, tol)


def test_rpgd_single_launch_size_with_separate_launches():
    """CTK_NO_RPGD_FUSED is read once per process: the (48, 12) case again, in a fresh child process, as the launch-per-phase form"""
    env = dict(os.environ, CTK_NO_RPGD_FUSED="1", CTK_MARGINS_OUT=os.devnull)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_rpgd_step_device_draws and single_launch"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "failed" not in r.stdout


# ======================================================================================================================
# gradient, cem-naive-grad, cem-grad-bharadhwaj
# ======================================================================================================================
def grad_state(o):
    return np.concatenate([o.Q.ravel(), o.opt.m.ravel(), o.opt.v.ravel(), np.zeros(o.N, np.float32), u_vec(o.u), [o.opt.step_count], [o.count]]).astype(np.float32)


GRAD_KW = dict(learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-7, gradmax_clip=5.0)
# Quad2D with limits whose spans are powers of two: lo + u * (hi - lo) then rounds once, fused or not, so "exactly" is a fair demand
GRAD_QLO, GRAD_QHI = np.array([-1.0, -0.5], np.float32), np.array([1.0, 0.5], np.float32)


@pytest.mark.parametrize("envname,N,H,its", [("CartPole", 40, 9, 3), ("CartPole", 100, 8, 1), ("Quad2D", 40, 9, 3)])
def test_gradient_device_draws(envname, N, H, its):
    """the reset's uniform plans, then the fresh tail input of every plan after each step = lo + u * (hi - lo) of word c of block 0, exactly"""
    lim = dict(lo=GRAD_QLO, hi=GRAD_QHI) if envname == "Quad2D" else {}
    E, p, o, e = make("gradient", "ODE", envname, N, H, dict(gradient_steps=its, **GRAD_KW), dict(outer_its=its, **GRAD_KW), **lim)
    print(f"gradient {envname} N{N}: {e.dominant_kernel()}")
    assert e.dominant_kernel() == ("ctk_rpgd_descent<0>" if envname == "CartPole" else "ctk_g_rpgd_descent<1>"), e.dominant_kernel()
    C = o.C
    cfg = dict(N=N, H=H, C=C)
    lo, hi = (np.float32(-1), np.float32(1)) if envname == "CartPole" else (GRAD_QLO, GRAD_QHI)
    assert e.rng_position() == 0
    d0 = expected_samples("gradient", cfg, SEED, 0, "reset").reshape(N, H, C)
    o.optimizer_reset(d0); e.reset()
    assert e.rng_position() == 1
    close(f"gradient {envname} N{N} reset", "PLAN", e.read("PLAN"), o.Q, rtol=1e-6, atol=1e-7)
    s = E["s0"].copy()
    tol = dict(rtol=5e-4, atol=5e-4)                   # test_gpu_variants.py::test_gradient_matches_oracle
    for t in range(3):
        tag = f"gradient {envname} N{N} step {t}"
        pos = e.rng_position()
        tail = expected_samples("gradient", cfg, SEED, pos)
        assert tail.size == e.samples_needed() == N * C
        uo, ug = o.step(s, tail.reshape(N, 1, C)), e.step(s)
        advanced(e, pos)
        plan = e.read("PLAN")
        np.testing.assert_array_equal(plan[:, -1, :], (lo + tail.reshape(N, C) * (hi - lo)).astype(np.float32))
        np.testing.assert_array_equal(plan[:, -1, :], o.Q[:, -1, :])
        record(tag, "Q", e.read("Q"), o.Q_refined, **tol); record(tag, "PLAN", plan, o.Q, **tol)
        assert_close_mostly(e.read("Q"), o.Q_refined, **tol)
        assert_close_mostly(plan, o.Q, **tol)
        close(tag, "J", e.read("J"), o.J, rtol=2e-3, atol=2e-2)
        close(tag, "u", ug, u_vec(uo), rtol=1e-3, atol=1e-3)
        e.set_state(grad_state(o))
        s = p.step(s.reshape(1, -1), u_vec(uo).reshape(1, -1))[0]
    e.close()


NAIVE_KW = dict(cem_initial_action_stdev=0.5, cem_stdev_min=0.1, learning_rate=0.1, gradmax_clip=10.0)


@pytest.mark.parametrize("pred,N,H,K,its", [("ODE", 130, 11, 13, 2), ("MLP", 128, 20, 16, 2)])
def test_cem_naive_grad_device_draws(pred, N, H, K, its):
    """ctk_sample_plans: stream `it`, column block (step * C + input) / 4 of the flat row"""
    kw = dict(cem_outer_it=its, cem_best_k=K, **NAIVE_KW)
    E, p, o, e = make("cem_naive_grad", pred, "CartPole", N, H, kw, kw)
    print(f"cem_naive_grad {pred}: {e.dominant_kernel()}")
    assert ("ctk_rpgd_descent<0>" if pred == "ODE" else "ctk_rpgd_mlp") in e.dominant_kernel(), e.dominant_kernel()
    s = E["s0"].copy()
    for t in range(3):
        cem_step(f"cem_naive_grad {pred} N{N} step {t}", o, e, s, pred, "CartPole", opt="cem_naive_grad")
    e.close()


def test_cem_naive_grad_device_draws_two_inputs():
    """C = 2: the column block of a flat [H*C] row is (h*C + c) >> 2, not (h >> 2)"""
    N, H, K, its = 66, 7, 11, 2
    kw = dict(cem_outer_it=its, cem_best_k=K, **NAIVE_KW)
    E, p, o, e = make("cem_naive_grad", "ODE", "Quad2D", N, H, kw, kw)
    assert e.dominant_kernel() == "ctk_g_rpgd_descent<1>", e.dominant_kernel()
    for t in range(2):
        cem_step(f"cem_naive_grad Quad2D N{N} step {t}", o, e, E["s0"], "ODE", "Quad2D", opt="cem_naive_grad")
    e.close()


BH_KW = dict(cem_initial_action_stdev=2.0, cem_stdev_min=1e-6, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-8,
             gradmax_clip=5.0)


def bh_split(z, N, H, C, K, its):
    return z[: K * H * C].reshape(K, H, C), z[K * H * C:].reshape(its, N - K, H, C)


@pytest.mark.parametrize("pred,N,H,K,its", [("ODE", 32, 20, 8, 2), ("MLP", 64, 16, 16, 2)])
def test_cem_grad_bharadhwaj_device_draws(pred, N, H, K, its):
    """ctk_cem_build_population: the initial elites on rows [0, K) of stream 0, the rest of iteration `it` on rows K.. of stream `it`"""
    kw = dict(cem_outer_it=its, cem_best_k=K, **BH_KW)
    E, p, o, e = make("cem_grad_bharadhwaj", pred, "CartPole", N, H, kw, kw)
    print(f"cem_grad_bharadhwaj {pred}: {e.dominant_kernel()}")
    assert ("ctk_rpgd_descent<0>" if pred == "ODE" else "ctk_rpgd_mlp") in e.dominant_kernel(), e.dominant_kernel()
    s = E["s0"].copy()
    tol = dict(rtol=5e-4, atol=5e-4)                   # test_gpu_variants.py::test_cem_grad_bharadhwaj_matches_oracle
    for t in range(3):
        tag = f"cem_grad_bharadhwaj {pred} N{N} step {t}"
        pos = e.rng_position()
        z = expected_samples("cem_grad_bharadhwaj", dict(N=N, H=H, C=1, K=K, its=its), SEED, pos)
        assert z.size == e.samples_needed()
        el, rest = bh_split(z, N, H, 1, K, its)
        uo, ug = o.step(s, el, rest), e.step(s)
        advanced(e, pos)
        record(tag, "Q", e.read("Q"), o.Q, **tol)
        assert_close_mostly(e.read("Q"), o.Q, **tol)
        assert_close_mostly(e.read("ADAM_M"), o.opt.m, **tol)
        close(tag, "U_NOM", e.read("U_NOM"), o.dist_mue, rtol=1e-3, atol=1e-3)
        close(tag, "STD", e.read("STD"), o.stdev, rtol=5e-3, atol=1e-3)
        close(tag, "u", ug, u_vec(uo), rtol=1e-3, atol=1e-3)
        e.set_state(np.concatenate([o.dist_mue.ravel(), o.stdev.ravel(), [float(o.u)], [o.count], o.opt.m.ravel(), o.opt.v.ravel(),
                                    [o.opt.step_count]]).astype(np.float32))
    e.close()


# ======================================================================================================================
# the transform itself
# ======================================================================================================================
# The allowance is a multiple of the float32 oracle's own worst deviation from the float64 transform on the same words (measured in the
# test; ~3.4e-7).  The device's logf / sincosf are a couple of ulp like NumPy's: 4x.  A (0,1] / [0,1) mix-up in u1 moves the draws with
# u1 < 1e-3 by more than 1.6e-5, over ten times this bound.  Observed on an MI355X: 1.60x (MPPI, whose Q carries one more rounding,
# z * stdev) and 1.20x (CEM, std a power of two): profiles/r13_device_rng_margins.txt.
TRANSFORM_FACTOR = 4.0


def transform_check(tag, z_dev, unclipped, stream, N, cols):
    f64n = PC.normal_f64(SEED, stream, 0, 0, N, cols)
    own = np.abs(O.device_noise(SEED, stream, 0, 0, N, cols, "normal").astype(np.float64) - f64n).max()
    small = PC.small_u1(SEED, stream, 0, 0, N, cols) & unclipped
    err = np.abs(z_dev[unclipped] - f64n[unclipped])
    print(f"{tag}: oracle float32 vs float64 {own:.3e}; device vs float64 {err.max():.3e} = {err.max() / own:.2f} x; "
          f"{int(unclipped.sum())} of {unclipped.size} draws unclipped, {int(small.sum())} of them with u1 < 1e-3")
    assert unclipped.mean() > 0.99 and small.sum() >= 20
    allowed = TRANSFORM_FACTOR * own
    assert allowed <= 2e-6                             # never above the inherited bound (rtol 1e-4 / atol 2e-6)
    close(tag, "z", z_dev[unclipped], f64n[unclipped], rtol=0.0, atol=allowed)


def test_transform_mppi_first_step_against_float64():
    """u_nom = 0, period 1: Q = clip(z * stdev): the affine map divided out of the unclipped elements, against normal_f64"""
    N, H = 1024, 50
    E, p, o, e = make("mppi", "ODE", "CartPole", N, H, dict(period_interpolation_inducing_points=1),
                      dict(period_interpolation_inducing_points=1, materialize_trajectories=True))
    e.step(E["s0"])
    Q = e.read("Q")[:, :, 0].astype(np.float64)
    unclipped = np.abs(Q) < 1.0
    transform_check("transform mppi", Q / np.float64(o.stdev), unclipped, 0, N, H)
    e.close()


def test_transform_cem_first_iteration_against_float64():
    """one iteration from mu = 0, std = 0.125 (a power of two: Q = z / 8 exactly, and |z| < 8 is never clipped)"""
    N, H = 1024, 50
    kw = dict(cem_outer_it=1, cem_best_k=100, cem_initial_action_stdev=0.125)
    E, p, o, e = make("cem", "ODE", "CartPole", N, H, kw, dict(kw, materialize_trajectories=True))
    assert e.dominant_kernel().startswith("ctk_cem_fused<"), e.dominant_kernel()
    e.step(E["s0"])
    Q = e.read("Q")[:, :, 0].astype(np.float64)
    transform_check("transform cem", Q * 8.0, np.abs(Q) < 1.0, 0, N, H)
    e.close()


# ======================================================================================================================
# the Philox position
# ======================================================================================================================
POS_CASES = {   # opt -> (oracle keywords, engine keywords); one outer iteration where there are any: Q is then the draws' first tensor
    "mppi": (dict(period_interpolation_inducing_points=3), dict(period_interpolation_inducing_points=3, materialize_trajectories=True)),
    "cem": (dict(cem_outer_it=1, cem_best_k=9), dict(cem_outer_it=1, cem_best_k=9, materialize_trajectories=True)),
    "random_action": ({}, dict(materialize_trajectories=True)),
    "cem_naive_grad": (dict(cem_outer_it=1, cem_best_k=9, **NAIVE_KW), dict(cem_outer_it=1, cem_best_k=9, **NAIVE_KW)),
    "cem_grad_bharadhwaj": (dict(cem_outer_it=1, cem_best_k=9, **BH_KW), dict(cem_outer_it=1, cem_best_k=9, **BH_KW)),
    "cem_gmm": (dict(cem_outer_it=1, cem_best_k=9), dict(cem_outer_it=1, cem_best_k=9, materialize_trajectories=True)),
    "gradient": (dict(gradient_steps=2, **GRAD_KW), dict(outer_its=2, **GRAD_KW)),
}
POS_N, POS_H = 70, 7


def make_pos(opt):
    if opt == "rpgd":
        return make_rpgd("ODE", "CartPole", POS_N, POS_H, 3, 10)
    return make(opt, "ODE", "CartPole", POS_N, POS_H, *POS_CASES[opt])


def first_tensor_at(opt, E, o, e, k):
    """the next call's draws are those of call = k: the first tensor they reach against the oracle fed expected_samples(position = k)"""
    N, H = POS_N, POS_H
    s = E["s0"]
    tag = f"position {opt} call {k}"
    if opt in ("rpgd", "gradient"):
        cfg = dict(N=N, H=H, C=1, P=getattr(o, "P", H))
        d0 = expected_samples(opt, cfg, SEED, k, "reset")
        o.optimizer_reset(d0.reshape(N, -1, 1)); e.reset()
        close(tag, "PLAN", e.read("PLAN"), o.Q, rtol=1e-6, atol=1e-6)
    elif opt == "mppi":
        o.optimizer_reset(); e.reset(); e.set_state(np.zeros(H + 1, np.float32)); o.u = O._u_out(np.zeros(1, np.float32))
        z = expected_samples(opt, dict(N=N, H=H, C=1, P=o.P), SEED, k)
        o.step(s, z.reshape(N, o.P, 1)); e.step(s)
        close(tag, "Q", e.read("Q"), o.u_run, rtol=1e-4, atol=2e-6)
    elif opt == "random_action":
        u01 = expected_samples(opt, dict(N=N, H=H, C=1), SEED, k).reshape(N, H, 1)
        e.step(s)
        close(tag, "Q", e.read("Q"), (np.float32(-1) + u01 * np.float32(2)).astype(np.float32), rtol=0, atol=1e-6)
    elif opt == "cem_gmm":
        o.optimizer_reset(); e.reset(); e.set_state(o.state())
        z = expected_samples(opt, dict(N=N, H=H, C=1, its=1), SEED, k)
        o.step(s, z[: N * H].reshape(1, N, H, 1), z[N * H:].reshape(1, N)); e.step(s)
        close(tag, "Q", e.read("Q"), o.Q, rtol=1e-5, atol=2e-6)
    elif opt == "cem_grad_bharadhwaj":          # (the variants' resets leave u and the Adam moments alone: pin them to the oracle's)
        o.optimizer_reset(); e.reset()
        zero = np.zeros(N * H, np.float32)
        m, v = (zero, zero) if o.opt.m is None else (o.opt.m.ravel(), o.opt.v.ravel())
        e.set_state(np.concatenate([o.dist_mue.ravel(), o.stdev.ravel(), [float(o.u)], [o.count], m, v, [o.opt.step_count]]).astype(np.float32))
        z = expected_samples(opt, dict(N=N, H=H, C=1, K=9, its=1), SEED, k)
        el, rest = bh_split(z, N, H, 1, 9, 1)
        o.step(s, el, rest); e.step(s)
        record(tag, "Q", e.read("Q"), o.Q, rtol=5e-4, atol=5e-4)
        assert_close_mostly(e.read("Q"), o.Q, rtol=5e-4, atol=5e-4)
    else:                                              # cem, cem_naive_grad
        o.optimizer_reset(); e.reset(); e.set_state(cem_state(o))
        z = expected_samples(opt, dict(N=N, H=H, C=1, its=1), SEED, k)
        o.step(s, z.reshape(1, N, H, 1)); e.step(s)
        close(tag, "Q", e.read("Q"), o.Q, **(dict(rtol=1e-5, atol=2e-6) if opt == "cem" else dict(rtol=1e-4, atol=2e-4)))


@pytest.mark.parametrize("opt", PC.OPTIMIZERS)
def test_position_counts_every_completed_step_and_drawing_reset(opt):
    """0 on a fresh handle; +1 after a reset that draws (RPGD, gradient: the others' resets draw nothing and leave it); +1 after EVERY
    completed step, RPGD's non-resampling steps included; unchanged by a refused call; set_rng_position(k) makes the next draws those of
    call = k"""
    E, p, o, e = make_pos(opt)
    s = E["s0"]
    assert e.rng_position() == 0
    draws_on_reset = opt in ("rpgd", "gradient")
    if draws_on_reset:
        with pytest.raises(Exception, match="ctk_reset"):
            e.step(s)                                  # refused: RPGD before its reset
        assert e.rng_position() == 0
        with pytest.raises(ValueError):
            e._check(e._lib.ctk_reset(e._h, None, 1))  # refused: CTK_LOC_HOST without a buffer
        assert e.rng_position() == 0
    e.reset()
    assert e.rng_position() == (1 if draws_on_reset else 0)
    base = e.rng_position()
    for t in range(3):                                 # (RPGD: resamp_per = 2, so step 1 draws nothing and still counts)
        if opt == "rpgd":
            assert (e.samples_needed() > 0) == (t % 2 == 0)
        e.step(s)
        assert e.rng_position() == base + t + 1
    pos = e.rng_position()
    if opt == "rpgd":
        e.step(s); pos += 1                            # ... so that the next step is one that takes samples
    need = e.samples_needed()
    assert need > 0
    with pytest.raises(ValueError):
        e.step(s, np.zeros(need + 1, np.float32))      # refused: wrong sample shape
    assert e.rng_position() == pos
    rc = e._lib.ctk_step(e._h, e._s_p, None, None, 1, e._u_p)       # refused by the library: CTK_LOC_HOST without a buffer
    assert rc == 1 and e.rng_position() == pos
    assert e.samples_needed() == need
    e.step(s, np.zeros(need, np.float32))             # a step fed from the caller's buffer is a completed step as well
    assert e.rng_position() == pos + 1
    for k in (1000, 0xFFFFFFFE):
        e.set_rng_position(k)
        assert e.rng_position() == k
        first_tensor_at(opt, E, o, e, k)
        assert e.rng_position() == k + 1
    e.close()


RESUME = ["rpgd", "gradient", "cem_naive_grad", "cem_grad_bharadhwaj"]


@pytest.mark.parametrize("opt", RESUME)
def test_state_and_position_resume_a_single_handle_bit_for_bit(opt):
    """ctk_get_state + ctk_rng_get_position carried into a fresh handle: the next steps are the same, bit for bit"""
    two = dict(cem_outer_it=2, cem_best_k=9)
    def fresh():
        if opt == "rpgd":
            return make_rpgd("ODE", "CartPole", POS_N, POS_H, 3, 10)[3]
        okw, ekw = POS_CASES[opt]
        return make(opt, "ODE", "CartPole", POS_N, POS_H, dict(okw, **two) if opt.startswith("cem") else okw,
                    dict(ekw, **two) if opt.startswith("cem") else ekw)[3]
    a = fresh()
    s = PC.S0.copy()
    plant = O.Predictor("ODE", dt=0.02, env=O.EnvParams())
    if opt in ("rpgd", "gradient"):
        a.reset()
    for _ in range(3):
        s = plant.step(s.reshape(1, 4), a.step(s).reshape(1, 1))[0]
    st, pos = a.get_state(), a.rng_position()
    assert pos == (4 if opt in ("rpgd", "gradient") else 3)
    b = fresh()
    b.set_state(st); b.set_rng_position(pos)
    names = ("PLAN", "ADAM_M", "ADAM_V", "AGES", "J") if opt in ("rpgd", "gradient") else ("Q", "J", "U_NOM", "STD")
    for _ in range(3):
        ua, ub = a.step(s), b.step(s)
        np.testing.assert_array_equal(ua, ub)
        for n in names:
            np.testing.assert_array_equal(a.read(n), b.read(n), err_msg=n)
        assert a.rng_position() == b.rng_position()
        s = plant.step(s.reshape(1, 4), ua.reshape(1, 1))[0]
    a.close(); b.close()


def test_resident_read_ahead_honours_a_position_set_between_steps():
    """the resident kernel with read_ahead may prepare the next step's inputs early: a ctk_rng_set_position between two steps must still
    give what the launched handle gives, bit for bit"""
    kw = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1, seed=SEED)
    a, b = CtkEngine("mppi", "ODE", **kw), CtkEngine("mppi", "ODE", **kw)
    b.resident_enable(True, idle_us=100000.0, read_ahead=True)
    s = PC.S0.copy()
    for t in range(6):
        if t == 3:
            a.set_rng_position(77); b.set_rng_position(77)
        np.testing.assert_array_equal(b.step(s), a.step(s))
        if t == 2:
            assert b.dominant_kernel().startswith("ctk_mppi_resident<0, "), b.dominant_kernel()
        s = s + np.array([0.01, 0.0, -0.02, 0.01], np.float32)
    assert a.rng_position() == b.rng_position() == 80
    np.testing.assert_array_equal(b.read("U_NOM"), a.read("U_NOM"))
    np.testing.assert_array_equal(b.read("J"), a.read("J"))
    a.close(); b.close()
