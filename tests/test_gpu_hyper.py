"""-m gpu: the optimizers' hyper-parameters (the fields of ctk_config) away from their defaults, on every kernel family.

The hyper-parameters are fixed at ctk_create, so every case is a handle of its own.  Two references:
  * the recordings of the unmodified reference at these values (tests/golden/*hyper*.npz), at the bounds of the existing golden tests;
  * the float32 oracle at the cases of tests/hyper_cases.py, which tests/test_hyper_cases_cpu.py holds to OptimF64 (a float64 statement
    from the primary hyper-parameters alone) and shows to move the compared tensor by 20 bounds or more.

Bounds, all the project's own (every comparison goes through margins.close with a tag that starts "hyper"):
  J  rtol 3e-5 / atol 1e-3 (recordings: rtol 1e-5; network predictors: + atol 1e-3);  TRAJ  rtol 1e-4 / atol 3e-5 (recordings 2e-5);
  u, U_NOM  U_TOL (recordings: rtol 1e-5 / atol 1e-5) times 100 / LBD below LBD = 100 (hyper_cases.u_bound: the soft-min turns a cost
  error dJ into a relative weight error dJ / LBD, and the suite's bound assumes LBD = 100);  CEM's Q, mu, STD, u  check_cem's;
  RPGD  CartPole's own kernels rtol 1e-3 / atol 2e-3, the template's rtol 2e-5 / atol 2e-5 (test_gpu_large_angles.check_rpgd_descent),
  through assert_close_mostly: Adam's normalised update moves an input whose gradient is within rounding of zero by up to 2 lr per
  iteration whatever the gradient's size, so the outliers are bounded by 2 lr its and their number by max(4, size / 400).
  ADAM_M  rtol 2e-3 / atol 2e-4 of the largest moment, ADAM_V  twice that (a square): the single-gradient tests' bound on g.
  A recording through the MLP: the same 2e-5, with assert_close_mostly's derived outlier count (rpgd_recording says why).
Each test names the kernel it means to run and checks dominant_kernel().  Shapes stay at N <= 128 and H <= 20 but for the throughput
kernels' TP_N / TP_H and for the two-tile form of the template's split MLP rollout, which starts at 258 full tiles: N = 4128, run at H = 10."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkMppiMlpBatch, CtkCemBatch, CtkRpgdBatch
from helpers import load, env_from, rpgd_kwargs_from
import large_angle_cases as L
import hyper_cases as Hc
from margins import close
from test_gpu_mppi import U_TOL
from test_gpu_rpgd import count_outliers
from test_gpu_large_angles import J_TOL, CEM_TOL, ENV_ID, FORMS, FORM_IDS, TP_N, TP_H
from test_gpu_tf_goldens import elite_sets_agree

pytestmark = pytest.mark.gpu

TRAJ_TOL = dict(rtol=1e-4, atol=3e-5)
GOLDEN_J_RTOL = 1e-5
NET_TOL = dict(rtol=2e-4, atol=2e-4)         # the network kernels' RPGD plans (test_cartpole_mppi_and_rpgd_on_64_unit_mlp_match_oracle, test_gpu_gru_grad.py)
FORMS_P = pytest.mark.parametrize("env,generic", FORMS, ids=FORM_IDS)


def form_id(env, generic):
    return FORM_IDS[FORMS.index((env, generic))]


def set_params(e, pars):
    for n in pars.param_names():
        e.set_param(n, float(getattr(pars, n)))


def lim(a):
    return float(a[0]) if np.size(a) == 1 else np.asarray(a, np.float32)


def engine_from(d, opt, **kw):
    """a handle for a recording: its environment, parameters, limits and network"""
    pred = str(d["predictor"])
    e = CtkEngine(opt, pred, environment=str(d["environment"]), num_rollouts=int(d["num_rollouts"]), mpc_horizon=int(d["mpc_horizon"]), dt=float(d["dt"]),
                  action_low=lim(d["low"]), action_high=lim(d["high"]), **kw)
    set_params(e, env_from(d))
    if pred == "MLP":
        e.set_predictor_weights(d["mlp_weights"])
    return e


def case_engine(opt, env, own, pred="ODE", **kw):
    """a handle for a case of hyper_cases: the environment's parameters of the large-angle file, the case's limits"""
    lo, hi = Hc.limits_of(env, own)
    e = CtkEngine(opt, pred, environment=env, dt=Hc.DT, action_low=lim(lo), action_high=lim(hi), **kw)
    set_params(e, L.env_params(env))
    return e


def mostly(tag, tensor, got, want, rtol, atol, outlier_atol):
    """test_gpu_rpgd.assert_close_mostly with its derived outlier count, the margin of the rest recorded"""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.abs(got - want) > atol + rtol * np.abs(want)
    assert int(bad.sum()) <= max(4, got.size // 400), f"{tag} {tensor}: {int(bad.sum())} outliers of {got.size} elements"
    assert np.abs(got - want).max() <= outlier_atol, f"{tag} {tensor}: an outlier of {np.abs(got - want).max():.3g}"
    close(tag, tensor, got[~bad], want[~bad], rtol=rtol, atol=atol)
    assert count_outliers(got, want, rtol, atol) == int(bad.sum())


# =====================================================================================================================================
# the recordings on the device
# =====================================================================================================================================
@pytest.mark.parametrize("materialize", [True, False])
@pytest.mark.parametrize("case", Hc.MPPI_FIXTURES)
def test_mppi_recordings(case, materialize):
    """ctk_mppi_rollout<ENV, PRED, LOG>: CartPole's ODE and MLP kernels, the template on Quad2D (C = 2) and Hover (C = 3)"""
    d = load(f"mppi_{case}.npz")
    env, H, C = str(d["environment"]), int(d["mpc_horizon"]), len(d["low"])
    LBD = float(d["LBD"])
    e = engine_from(d, "mppi", period_interpolation_inducing_points=int(d["period_interpolation_inducing_points"]), materialize_trajectories=materialize,
                    cc_weight=float(d["cc_weight"]), R=float(d["R"]), LBD=LBD, NU=float(d["NU"]), SQRTRHOINV=float(d["SQRTRHOINV"]))
    np.testing.assert_array_equal(e.read("U_NOM"), d["u_nom_init"])
    net = str(d["predictor"]) == "MLP"
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"noise_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"hyper recording mppi_{case} log={materialize} step {t}"
        if materialize:
            close(tag, "u_run", e.read("Q"), d[f"u_run_{t}"], rtol=1e-6, atol=1e-6)
            close(tag, "traj", e.read("TRAJ"), d[f"traj_{t}"], rtol=1e-4, atol=2e-5)
        close(tag, "J", e.read("J"), d[f"J_{t}"], rtol=GOLDEN_J_RTOL, atol=1e-3 if net else 0.0)
        close(tag, "u_nom", e.read("U_NOM"), d[f"u_nom_{t}"], **Hc.u_bound(LBD, 1e-5, 1e-5))
        close(tag, "u", u, d[f"u_{t}"], **Hc.u_bound(LBD, 1e-5, 1e-5))
        e.set_state(np.concatenate([d[f"u_nom_{t}"].reshape(H * C), d[f"u_{t}"].reshape(C)]))
    k = e.dominant_kernel()
    e.close()
    log = "true" if materialize else "false"
    assert k.startswith(f"ctk_mppi_rollout<{ENV_ID[env]}, ") and (net or k.startswith(f"ctk_mppi_rollout<{ENV_ID[env]}, 0, {log}, false")), k


@pytest.mark.parametrize("form", ["one_launch", "launch_per_phase"])
@pytest.mark.parametrize("case", Hc.CEM_FIXTURES)
def test_cem_recordings(monkeypatch, case, form):
    """ctk_cem_fused and the launch per phase: asymmetric limits, a saturating initial deviation, a clamp that binds"""
    d = load(f"cem_{case}.npz")
    env, H, K, C = str(d["environment"]), int(d["mpc_horizon"]), int(d["cem_best_k"]), len(d["low"])
    if form == "launch_per_phase":
        monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")
    e = engine_from(d, "cem", cem_outer_it=int(d["cem_outer_it"]), cem_best_k=K, cem_initial_action_stdev=float(d["cem_initial_action_stdev"]),
                    cem_stdev_min=float(d["cem_stdev_min"]), materialize_trajectories=True)
    monkeypatch.delenv("CTK_NO_CEM_FUSED", raising=False)
    np.testing.assert_array_equal(e.read("U_NOM"), d["dist_mue_init"])
    np.testing.assert_array_equal(e.read("STD"), d["stdev_init"])
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"noise_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"hyper recording cem_{case} {form} step {t}"
        close(tag, "Q", e.read("Q"), d[f"Q_{t}"], rtol=1e-5, atol=2e-6)
        close(tag, "J", e.read("J"), d[f"J_{t}"], rtol=GOLDEN_J_RTOL)
        close(tag, "traj", e.read("TRAJ"), d[f"traj_{t}"], rtol=1e-4, atol=4e-5)
        assert elite_sets_agree(d[f"J_{t}"], e.read("BEST_IDX"), K, GOLDEN_J_RTOL) == 0
        close(tag, "dist_mue", e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6)
        close(tag, "stdev", e.read("STD"), d[f"stdev_{t}"], rtol=5e-5, atol=2e-6)
        close(tag, "u", u, d[f"u_{t}"], rtol=1e-5, atol=2e-6)
        e.set_state(np.concatenate([d[f"dist_mue_{t}"].reshape(H * C), d[f"stdev_{t}"].reshape(H * C), d[f"u_{t}"].reshape(C), [t + 1]]).astype(np.float32))
    k = e.dominant_kernel()
    e.close()
    assert k == f"ctk_cem_fused<{ENV_ID[env]}, true>" if form == "one_launch" else k.startswith(f"ctk_affine_rollout<{ENV_ID[env]},"), k


@pytest.mark.parametrize("case", Hc.RANDOM_FIXTURES)
def test_random_action_recordings(case):
    """ctk_affine_rollout<ENV, 0, true>: the uniform map onto asymmetric limits"""
    d = load(f"random_{case}.npz")
    e = engine_from(d, "random_action", materialize_trajectories=True)
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"u01_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"hyper recording random_{case} step {t}"
        close(tag, "Q", e.read("Q"), d[f"Q_{t}"], rtol=1e-6, atol=1e-7)
        close(tag, "J", e.read("J"), d[f"J_{t}"], rtol=GOLDEN_J_RTOL)
        close(tag, "traj", e.read("TRAJ"), d[f"traj_{t}"], rtol=1e-4, atol=4e-5)
        assert int(e.read("BEST_IDX")[0]) == int(np.argmin(d[f"J_{t}"]))
        close(tag, "u", u, d[f"u_{t}"], rtol=1e-6, atol=1e-7)
        e.set_state(d[f"u_{t}"].astype(np.float32))
    k = e.dominant_kernel()
    e.close()
    assert k == f"ctk_affine_rollout<{ENV_ID[str(d['environment'])]}, 0, true>", k


@pytest.mark.parametrize("case", Hc.CEM_NAIVE_GRAD_FIXTURES)
def test_cem_naive_grad_recordings(case):
    """ctk_rpgd_descent<0> and ctk_g_rpgd_descent<1>: learning_rate 0.3 with a clip of 0.05 that binds, the clamp, asymmetric limits (bounds:
    test_cem_naive_grad_matches_reference_golden's)"""
    d = load(f"cem_naive_grad_{case}.npz")
    H, K, C = int(d["mpc_horizon"]), int(d["cem_best_k"]), len(d["low"])
    e = engine_from(d, "cem_naive_grad", cem_outer_it=int(d["cem_outer_it"]), cem_best_k=K, cem_initial_action_stdev=float(d["cem_initial_action_stdev"]),
                    cem_stdev_min=float(d["cem_stdev_min"]), learning_rate=float(d["learning_rate"]), gradmax_clip=float(d["gradmax_clip"]))
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"noise_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"hyper recording cem_naive_grad_{case} step {t}"
        close(tag, "Q", e.read("Q"), d[f"Q_{t}"], rtol=2e-5, atol=2e-5)
        close(tag, "J", e.read("J"), d[f"J_{t}"], rtol=GOLDEN_J_RTOL)
        assert elite_sets_agree(d[f"J_{t}"], e.read("BEST_IDX"), K, GOLDEN_J_RTOL) == 0
        close(tag, "dist_mue", e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=1e-5)
        close(tag, "stdev", e.read("STD"), d[f"stdev_{t}"], rtol=1e-4, atol=1e-5)
        close(tag, "u", u, d[f"u_{t}"], rtol=1e-5, atol=1e-5)
        e.set_state(np.concatenate([d[f"dist_mue_{t}"].reshape(H * C), d[f"stdev_{t}"].reshape(H * C), d[f"u_{t}"].reshape(C), [t + 1]]).astype(np.float32))
    k = e.dominant_kernel()
    e.close()
    env = str(d["environment"])
    assert k == (RPGD_OWN if env == "CartPole" else f"ctk_g_rpgd_descent<{ENV_ID[env]}>"), k


RPGD_OWN = "ctk_rpgd_descent<0>"                # CartPole's own descent through the ODE (with ctk_rpgd_warmstart)


def rpgd_kernel(env, generic):
    return f"ctk_g_rpgd_descent<{ENV_ID[env]}>" if (generic or env != "CartPole") else RPGD_OWN


def rpgd_engine_from(d, generic, **kw):
    k = rpgd_kwargs_from(d)
    N = int(d["num_rollouts"])
    return engine_from(d, "rpgd", generic_kernels=generic, period_interpolation_inducing_points=k["period_interpolation_inducing_points"],
                       outer_its=k["outer_its"], resamp_per=k["resamp_per"], shift_previous=k["shift_previous"],
                       opt_keep_k=int(max(int(N * k["opt_keep_k_ratio"]), 1)), sampling_distribution=0 if k["SAMPLING_DISTRIBUTION"] == "uniform" else 1,
                       sample_whole_control_space=int(k["sample_whole_control_space"]), sample_stdev=k["sample_stdev"], sample_mean=k["sample_mean"],
                       sample_min=k["uniform_dist_min"], sample_max=k["uniform_dist_max"], learning_rate=k["learning_rate"], gradmax_clip=k["gradmax_clip"],
                       adam_beta_1=k["adam_beta_1"], adam_beta_2=k["adam_beta_2"], adam_epsilon=k["adam_epsilon"], **kw)


def rpgd_recording(case, generic):
    """every step pinned to the reference's own state, at the short descents' bound of the existing golden tests (rtol 2e-5 / atol 2e-5).
    Returns the recording and the handle's kernel."""
    d = load(f"rpgd_{case}.npz")
    e = rpgd_engine_from(d, generic)
    e.reset(d["reset_draws"])
    tag0 = f"hyper recording rpgd_{case} {'template' if generic else 'own'}"
    close(tag0 + " step reset", "plan", e.read("PLAN"), d["Q_init"], rtol=1e-6, atol=1e-6)
    tol = dict(rtol=2e-5, atol=2e-5)
    # A recording through the MLP keeps the 2e-5, with assert_close_mostly's derived outlier count (max(4, size / 400)) on the plans and the
    # moments, as test_hover_rpgd_matches_reference_golden does: an input's step lr m^ / (sqrt(v^) + eps) has the slope lr / (sqrt(v^) + eps)
    # in m^, up to 200 at lr 0.2 / eps 1e-3 on gradients clipped to norm 0.05, and a network gradient differs between two float32 evaluations
    # in its last digits.  The float32 CPU oracle itself has ONE plan element of 576 at 0.74 of the bound at step 0 and none other above 0.25.
    net = str(d["predictor"]) == "MLP"
    out = 2.0 * float(d["learning_rate"]) * int(d["outer_its"])
    for t in range(int(d["steps"])):
        key = f"resample_draws_{t}"
        draws = d[key] if key in d.files and d[key].size else None
        assert e.samples_needed() == (0 if draws is None else draws.size)
        u = e.step(d[f"s_{t}"], draws, u_prev=d[f"u_prev_{t}"])
        tag = f"{tag0} step {t}"
        close(tag, "u_nom", e.read("U_NOM"), d[f"u_nom_{t}"], **tol)
        close(tag, "u", u, d[f"u_{t}"], **tol)
        mmax, vmax = float(np.abs(d[f"m_{t}"]).max()), float(np.abs(d[f"v_{t}"]).max())
        vtol = dict(rtol=tol["rtol"], atol=tol["atol"] * vmax)
        if net:
            mostly(tag, "plan", e.read("PLAN"), d[f"Q_{t}"], outlier_atol=out, **tol)
            mostly(tag, "adam_m", e.read("ADAM_M"), d[f"m_{t}"], outlier_atol=mmax, **tol)
            mostly(tag, "adam_v", e.read("ADAM_V"), d[f"v_{t}"], outlier_atol=vmax, **vtol)
        else:
            close(tag, "plan", e.read("PLAN"), d[f"Q_{t}"], **tol)
            close(tag, "adam_m", e.read("ADAM_M"), d[f"m_{t}"], **tol)
            close(tag, "adam_v", e.read("ADAM_V"), d[f"v_{t}"], **vtol)
        np.testing.assert_array_equal(e.read("AGES"), d[f"ages_{t}"])
        e.set_state(np.concatenate([d[f"Q_{t}"].ravel(), d[f"m_{t}"].ravel(), d[f"v_{t}"].ravel(), d[f"ages_{t}"].ravel(), d[f"u_{t}"].ravel(),
                                    [int(d[f"adam_step_{t}"])], [t + 1]]).astype(np.float32))
    k = e.dominant_kernel()
    e.close()
    return d, k


@pytest.mark.parametrize("generic", [False, True], ids=["own", "template"])
@pytest.mark.parametrize("case", Hc.RPGD_FIXTURES)
def test_rpgd_recordings(case, generic):
    """ctk_rpgd_descent<0> + ctk_rpgd_warmstart (CartPole's own) and ctk_g_rpgd_descent<ENV>; through the MLP the one-launch (persistent)
    descents ctk_rpgd_mlp_persistent and ctk_g_rpgd_persist<0, false>: every Adam scalar moved, a clip that binds on every row,
    shift_previous 2 and 0, resamp_per 3, both sampling maps with their constants moved"""
    d, k = rpgd_recording(case, generic)
    env = str(d["environment"])
    if str(d["predictor"]) == "ODE":
        assert k == rpgd_kernel(env, generic), k
    else:
        assert k == ("ctk_g_rpgd_persist<0, false>" if generic else "ctk_rpgd_mlp_persistent"), k


@pytest.mark.parametrize("generic", [False, True], ids=["own", "template"])
def test_rpgd_keeping_every_row(generic):
    """opt_keep_k == num_rollouts: a resampling step needs no draws (samples_needed() == 0), launches the warm start with no fresh rows and
    keeps every row in order of cost with its moments (shifted by one) and its age — as the reference does (the recording)"""
    d, k = rpgd_recording(Hc.RPGD_KEEP_ALL_FIXTURE, generic)
    assert int(d["num_rollouts"]) == int(max(int(int(d["num_rollouts"]) * float(d["opt_keep_k_ratio"])), 1))
    assert str(d["predictor"]) == "ODE" and k == rpgd_kernel(str(d["environment"]), generic), k


# =====================================================================================================================================
# MPPI: the cases against the oracle
# =====================================================================================================================================
def mppi_kw(own, N, H, p, materialize):
    return dict(num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, materialize_trajectories=materialize, **Hc.config_of(Hc.MPPI_DEFAULTS, own))


def mppi_start(ref):
    return np.concatenate([ref["plan0"].ravel(), ref["u_prev"]]).astype(np.float32)


def check_mppi(tag, own, ref, u, read, materialize, traj=True):
    LBD = Hc.config_of(Hc.MPPI_DEFAULTS, own)["LBD"]
    close(tag, "J", read("J"), ref["J"], **J_TOL)
    close(tag, "u_nom", read("U_NOM"), ref["u_nom"], **Hc.u_bound(LBD, **U_TOL))
    close(tag, "u", u, ref["u"], **Hc.u_bound(LBD, **U_TOL))
    if materialize:
        close(tag, "u_run", read("Q"), ref["Q"], rtol=1e-6, atol=1e-6)
        if traj:
            close(tag, "traj", read("TRAJ"), ref["traj"], **TRAJ_TOL)


@pytest.mark.parametrize("materialize", [True, False])
@FORMS_P
def test_mppi_four_wave_kernel(env, generic, materialize):
    """ctk_mppi_rollout<ENV, 0, LOG>, CartPole's own and the template: every single-value case, ALL and the saturated case, period 1 and 5"""
    log = "true" if materialize else "false"
    for N, H, p in Hc.MPPI_SIZES:
        for own in [()] + Hc.MPPI_CASES:
            ref = Hc.mppi_ref(env, own, N, H, p)
            e = case_engine("mppi", env, own, generic_kernels=generic, **mppi_kw(own, N, H, p, materialize))
            e.set_state(mppi_start(ref))
            u = e.step(ref["s"], ref["noise"], u_prev=ref["u_prev"])
            check_mppi(f"hyper mppi {form_id(env, generic)} log={log} step {Hc.mppi_id(own)} N{N} p{p}", own, ref, u, e.read, materialize)
            k = e.dominant_kernel()
            e.close()
            assert k.startswith(f"ctk_mppi_rollout<{ENV_ID[env]}, 0, {log}, false"), k


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
@pytest.mark.parametrize("kernel,p,generic", [("ctk_mppi_rollout_tps<", 1, False), ("ctk_mppi_rollout_tp<", 2, False), ("ctk_g_rollout", 1, True)],
                         ids=["streaming", "whole-tile", "template"])
def test_mppi_throughput_kernels(kernel, p, generic, own):
    """at the smallest N that selects them (the one large shape of the file)"""
    env = "CartPole"
    ref = Hc.mppi_ref(env, own, TP_N, TP_H, p)
    for log in (True, False):
        e = case_engine("mppi", env, own, generic_kernels=generic, **mppi_kw(own, TP_N, TP_H, p, log))
        e.set_state(mppi_start(ref))
        u = e.step(ref["s"], ref["noise"], u_prev=ref["u_prev"])
        check_mppi(f"hyper mppi {kernel.rstrip('<')} log={log} step {Hc.mppi_id(own)}", own, ref, u, e.read, log)
        k = e.dominant_kernel()
        e.close()
        assert kernel in k, k


NET_FORMS = [("CartPole", "MLP", (32, 32)), ("CartPole", "GRU", (32, 32)), ("CartPole", "MLP", (64, 64)), ("Quad2D", "MLP", (32, 32)), ("Hover", "MLP", (32, 32)),
             ("Quad2D", "GRU", (32, 32))]


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
@pytest.mark.parametrize("env,kind,hidden", NET_FORMS, ids=[f"{e}-{k}{h[0]}" for e, k, h in NET_FORMS])
def test_mppi_network_kernels(env, kind, hidden, own):
    """CartPole's own MLP and GRU kernels, the 64-unit MLP, the template's split network kernels (one tile in a workgroup) on Quad2D and Hover"""
    N, H, p = Hc.NET_SIZE
    ref = Hc.net_mppi_ref(env, kind, own, hidden)
    C = ref["u_prev"].size
    extra = dict(predictor_hidden=hidden) if hidden != (32, 32) else {}
    e = case_engine("mppi", env, own, kind, **extra, **mppi_kw(own, N, H, p, True))
    e.set_predictor_weights(ref["weights"])
    e.set_state(mppi_start(ref))
    if kind == "GRU":
        e.predictor_set_hidden(None)
    u = e.step(ref["s"], ref["noise"], u_prev=ref["u_prev"])
    tag = f"hyper mppi {kind}{hidden[0]} {env} step {Hc.mppi_id(own)}"
    LBD = Hc.config_of(Hc.MPPI_DEFAULTS, own)["LBD"]
    close(tag, "u_run", e.read("Q"), ref["Q"], rtol=1e-6, atol=1e-6)
    # test_network_mppi_cost_parameters' bounds; the 64-unit form: test_cartpole_mppi_and_rpgd_on_64_unit_mlp_match_oracle's rtol 5e-5
    close(tag, "J", e.read("J"), ref["J"], rtol=J_TOL["rtol"] if hidden == (32, 32) else 5e-5, atol=J_TOL["atol"])
    close(tag, "u_nom", e.read("U_NOM"), ref["u_nom"], **Hc.u_bound(LBD, **U_TOL))
    close(tag, "u", u, ref["u"], **Hc.u_bound(LBD, **U_TOL))
    k = e.dominant_kernel()
    e.close()
    if hidden != (32, 32):
        assert "NetMlpWideT" in k or "SplitMlp64" in k, k
    else:
        policy = "SplitGru" if kind == "GRU" else "SplitMlp<true>" if env == "Hover" else "SplitMlp<false>"
        assert k.startswith("ctk_mppi_rollout<0, ") if env == "CartPole" else k == f"ctk_g_rollout_split<{ENV_ID[env]}, {policy}, 0, true, 1>", k


@pytest.mark.parametrize("materialize", [True, False])
def test_mppi_split_mlp_kernel_with_two_tiles_in_a_workgroup(materialize):
    """ctk_g_rollout_split<1, SplitMlp<false>, 0, LOG, 2>: ALL on Quad2D's MLP at the smallest population that takes the form (258 full
    tiles).  The kernel takes MppiK as an argument and has its own LDS carve and record index per half of the workgroup."""
    env, own, (N, H, p) = "Quad2D", Hc.MPPI_ALL, Hc.TWO_TILE_SIZE
    assert N % 16 == 0 and N // 16 == 258
    ref = Hc.net_mppi_ref(env, "MLP", own, (32, 32), Hc.TWO_TILE_SIZE)
    e = case_engine("mppi", env, own, "MLP", **mppi_kw(own, N, H, p, materialize))
    e.set_predictor_weights(ref["weights"])
    e.set_state(mppi_start(ref))
    u = e.step(ref["s"], ref["noise"], u_prev=ref["u_prev"])
    check_mppi(f"hyper mppi MLP32 two tiles {env} log={materialize} step ALL", own, ref, u, e.read, materialize, traj=False)
    k = e.dominant_kernel()
    e.close()
    assert k == f"ctk_g_rollout_split<1, SplitMlp<false>, 0, {'true' if materialize else 'false'}, 2>", k


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_mppi_resident_form(env, own):
    """ctk_mppi_resident<ENV>: the constants reach the resident kernel's arguments in device memory"""
    import torch
    N, H, p = Hc.MPPI_SIZES[1]
    ref = Hc.mppi_ref(env, own, N, H, p)
    e = case_engine("mppi", env, own, **mppi_kw(own, N, H, p, False))
    e.resident_enable(True, idle_us=100000.0)
    noise = torch.from_numpy(ref["noise"]).to("cuda")
    torch.cuda.synchronize()
    tag = f"hyper mppi resident {env} step {Hc.mppi_id(own)}"
    LBD = Hc.config_of(Hc.MPPI_DEFAULTS, own)["LBD"]
    for rep in range(2):                                                   # the second step finds the kernel resident
        e.set_state(mppi_start(ref))
        u = np.array(e.step(ref["s"], noise.data_ptr(), u_prev=ref["u_prev"]), np.float32).copy()
        assert e.dominant_kernel().startswith(f"ctk_mppi_resident<{ENV_ID[env]}, "), e.dominant_kernel()
        close(tag, "u", u, ref["u"], **Hc.u_bound(LBD, **U_TOL))
    check_mppi(tag + ", read", own, ref, u, e.read, False)                 # (the reads end residency)
    e.close()


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
@pytest.mark.parametrize("env", ["CartPole", "Quad2D"])
def test_mppi_three_shards(env, own):
    """ctk_mppi_step_begin / ctk_mppi_step_end at 3 shards: neg_inv_lbd reaches ctk_mppi_merge / merge_partial and the update kernels with
    LBD != 100.  Against the oracle's single step of the whole population."""
    import torch
    N, H, p = 96, 20, 5
    G, NL = 3, 32
    ref = Hc.mppi_ref(env, own, N, H, p)
    sh = [case_engine("mppi", env, own, global_rollout_offset=i * NL, **mppi_kw(own, NL, H, p, False)) for i in range(G)]
    rec = sh[0].mppi_partial_size()
    buf = torch.zeros(G * rec, dtype=torch.float32, device="cuda")
    for i, e in enumerate(sh):
        e.set_state(mppi_start(ref))
        e.mppi_step_begin(ref["s"], buf.data_ptr() + 4 * i * rec, ref["noise"][i * NL:(i + 1) * NL], u_prev=ref["u_prev"])
    torch.cuda.synchronize()
    us = [e.mppi_step_end(buf.data_ptr(), G) for e in sh]
    tag = f"hyper mppi shards {env} step {Hc.mppi_id(own)}"
    LBD = Hc.config_of(Hc.MPPI_DEFAULTS, own)["LBD"]
    for i, e in enumerate(sh):
        np.testing.assert_array_equal(us[i], us[0])
        close(tag, "J", e.read("J"), ref["J"][i * NL:(i + 1) * NL], **J_TOL)
        close(tag, "u_nom", e.read("U_NOM"), ref["u_nom"], **Hc.u_bound(LBD, **U_TOL))
    close(tag, "u", us[0], ref["u"], **Hc.u_bound(LBD, **U_TOL))
    k = sh[0].dominant_kernel()
    for e in sh:
        e.close()
    assert k.startswith(f"ctk_mppi_rollout<{ENV_ID[env]}, 0, false"), k


B = 3


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_mppi_batch(env, own):
    """ctk_mppi_batch<ENV, true> at B = 3: every problem bit for bit a single handle of the same configuration, problem 1 against the oracle"""
    N, H, p = Hc.MPPI_SIZES[0]
    ref = Hc.mppi_ref(env, own, N, H, p)
    lo, hi = Hc.limits_of(env, own)
    kw = mppi_kw(own, N, H, p, True)
    batch = CtkMppiBatch(B, seeds=[1, 2, 3], environment=env, dt=Hc.DT, action_low=lim(lo), action_high=lim(hi), **kw)
    set_params(batch, L.env_params(env))
    noise = np.stack([ref["noise"][::-1].copy(), ref["noise"], -ref["noise"]])
    for q in range(B):
        batch.set_state(q, mppi_start(ref))
    u = np.array(batch.step(np.stack([ref["s"]] * B), noise, u_prev=np.stack([ref["u_prev"]] * B))).copy()
    check_mppi(f"hyper mppi batch {env} step {Hc.mppi_id(own)} problem 1", own, ref, u[1], lambda name: batch.read(name, 1), True)
    for q in range(B):
        h = case_engine("mppi", env, own, seed=q + 1, **kw)
        h.set_state(mppi_start(ref))
        uh = h.step(ref["s"], noise[q], u_prev=ref["u_prev"])
        np.testing.assert_array_equal(u[q], uh)
        for name in ("J", "U_NOM", "Q", "TRAJ"):
            got = batch.read(name, q)
            np.testing.assert_array_equal(got, h.read(name).reshape(got.shape), err_msg=f"{name} of problem {q}")
        h.close()
    k = batch.dominant_kernel()
    batch.close()
    assert k == f"ctk_mppi_batch<{ENV_ID[env]}, true>", k


@pytest.mark.parametrize("own", [Hc.MPPI_ALL, Hc.MPPI_SATURATED], ids=Hc.mppi_id)
def test_mppi_mlp_batch(own):
    """ctk_mppi_batch_mlp<true> at B = 3: bit for bit the single MLP handles, problem 1 against the oracle"""
    env, (N, H, p) = "CartPole", Hc.NET_SIZE
    ref = Hc.net_mppi_ref(env, "MLP", own)
    lo, hi = Hc.limits_of(env, own)
    kw = mppi_kw(own, N, H, p, True)
    batch = CtkMppiMlpBatch(B, seeds=[1, 2, 3], dt=Hc.DT, action_low=lim(lo), action_high=lim(hi), **kw)
    set_params(batch, L.env_params(env))
    batch.set_weights(ref["weights"])
    noise = np.stack([ref["noise"][::-1].copy(), ref["noise"], -ref["noise"]])
    for q in range(B):
        batch.set_state(q, mppi_start(ref))
    u = np.array(batch.step(np.stack([ref["s"]] * B), noise, u_prev=np.stack([ref["u_prev"]] * B))).copy()
    check_mppi(f"hyper mppi batch_mlp step {Hc.mppi_id(own)} problem 1", own, ref, u[1], lambda name: batch.read(name, 1), True, traj=False)
    for q in range(B):
        h = case_engine("mppi", env, own, "MLP", seed=q + 1, **kw)
        h.set_predictor_weights(ref["weights"])
        h.set_state(mppi_start(ref))
        uh = h.step(ref["s"], noise[q], u_prev=ref["u_prev"])
        np.testing.assert_array_equal(u[q], uh)
        for name in ("J", "U_NOM", "Q"):
            got = batch.read(name, q)
            np.testing.assert_array_equal(got, h.read(name).reshape(got.shape), err_msg=f"{name} of problem {q}")
        h.close()
    k = batch.dominant_kernel()
    batch.close()
    assert k == "ctk_mppi_batch_mlp<true>", k


# =====================================================================================================================================
# CEM: the clamp that binds, the saturating deviation, asymmetric limits, ALL
# =====================================================================================================================================
def check_cem(tag, ref, u, read):
    close(tag, "J", read("J"), ref["J"], **J_TOL)
    close(tag, "Q", read("Q"), ref["Q"], rtol=1e-5, atol=2e-6)
    close(tag, "mu", read("U_NOM"), ref["mu"], **CEM_TOL)
    close(tag, "std", read("STD"), ref["std"], **CEM_TOL)
    close(tag, "u", u, ref["u"], rtol=1e-5, atol=2e-6)
    close(tag, "traj", read("TRAJ"), ref["traj"], **TRAJ_TOL)


@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "launch-per-phase"])
@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_kernels(env, fused, monkeypatch):
    """ctk_cem_fused<ENV, true> and the per-phase kernels (ctk_affine_rollout, ctk_select_topk, ctk_cem_refit, the finish)"""
    for N, H in Hc.CEM_SIZES:
        for own in [()] + Hc.CEM_CASES:
            ref = Hc.cem_ref(env, own, N, H)
            if not fused:
                monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")           # read when the handle is created
            e = case_engine("cem", env, own, num_rollouts=N, mpc_horizon=H, materialize_trajectories=True, **ref["kw"])
            monkeypatch.delenv("CTK_NO_CEM_FUSED", raising=False)
            e.reset()
            u = e.step(ref["s"], ref["noise"], u_prev=np.zeros(e.C, np.float32))
            check_cem(f"hyper cem {'fused' if fused else 'phases'} {env} step {Hc.cem_id(own)} N{N}", ref, u, e.read)
            k = e.dominant_kernel()
            e.close()
            assert k == f"ctk_cem_fused<{ENV_ID[env]}, true>" if fused else k.startswith(f"ctk_affine_rollout<{ENV_ID[env]},"), k


@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_batch(env):
    """ctk_cem_batch<ENV, true> at B = 3: every case, every problem against the oracle's step with that problem's draws (the problems differ
    in their draws' order and sign)"""
    N, H = Hc.CEM_SIZES[1]
    for own in Hc.CEM_CASES:
        refs = [Hc.cem_ref(env, own, N, H, q) for q in range(B)]
        ref = refs[0]
        lo, hi = Hc.limits_of(env, own)
        batch = CtkCemBatch(B, seeds=[1, 2, 3], environment=env, num_rollouts=N, mpc_horizon=H, dt=Hc.DT, action_low=lim(lo), action_high=lim(hi),
                            materialize_trajectories=True, **ref["kw"])
        set_params(batch, L.env_params(env))
        batch.reset()
        u = np.array(batch.step(np.stack([ref["s"]] * B), np.stack([r["noise"] for r in refs]), u_prev=np.zeros((B, batch.C), np.float32))).copy()
        for q in range(B):
            check_cem(f"hyper cem batch {env} step {Hc.cem_id(own)} problem {q}", refs[q], u[q], lambda name: batch.read(name, q))
        k = batch.dominant_kernel()
        batch.close()
        assert k == f"ctk_cem_batch<{ENV_ID[env]}, true>", k


@pytest.mark.parametrize("env", Hc.GMM_ENVS)
def test_cem_gmm_between_asymmetric_limits(env):
    """ctk_affine_rollout_mix<ENV, true>, ctk_gmm_refit and the finish: a saturating initial deviation, asymmetric limits (the mixture's initial
    means are their middle), a clamp that binds on most but not all of the mixture's deviations.  Bounds: test_cem_gmm_matches_restatement's."""
    from gmm_oracle import pack_draws
    ref = Hc.gmm_ref(env)
    assert ref["min_margin"] >= 1e-5 and ref["min_cost_gap"] >= 1e-4       # the restatement's own labels and elite set have no near-tie
    e = case_engine("cem_gmm", env, (("limits", "asym"),), num_rollouts=128, mpc_horizon=20, materialize_trajectories=True, **Hc.GMM_KW)
    u = np.array(e.step(ref["s"], pack_draws(ref["normals"], ref["uniforms"]), u_prev=np.zeros(e.C, np.float32)), np.float32).copy()
    tag = f"hyper cem_gmm {env} step ALL"
    close(tag, "Q", e.read("Q"), ref["Q"], rtol=1e-5, atol=2e-6)
    close(tag, "J", e.read("J"), ref["J"], **J_TOL)
    np.testing.assert_array_equal(e.read("BEST_IDX"), ref["best"])
    np.testing.assert_array_equal(e.read("MIX_LABEL"), ref["labels"].astype(np.float32))
    np.testing.assert_array_equal(e.read("MIX_PROB"), ref["probs"])
    close(tag, "mix_mu", np.moveaxis(e.read("MIX_MU"), 0, -1), ref["mu"], rtol=1e-4, atol=1e-5)
    close(tag, "mix_std", np.moveaxis(e.read("MIX_STD"), 0, -1), ref["std"], rtol=1e-4, atol=1e-5)
    close(tag, "u", u, ref["u"], rtol=1e-5, atol=2e-6)
    k = e.dominant_kernel()
    e.close()
    assert k == f"ctk_affine_rollout_mix<{ENV_ID[env]}, true>", k


# =====================================================================================================================================
# the RPGD family
# =====================================================================================================================================
def rpgd_cfg(own, k, rule="torch", **over):
    kw = dict(Hc.config_of(Hc.RPGD_DEFAULTS, own), **over)
    return dict(outer_its=kw["outer_its"], resamp_per=kw["resamp_per"], shift_previous=kw["shift_previous"], opt_keep_k=k,
                sampling_distribution=0 if kw["SAMPLING_DISTRIBUTION"] == "uniform" else 1, sample_whole_control_space=int(kw["sample_whole_control_space"]),
                sample_stdev=kw["sample_stdev"], sample_mean=kw["sample_mean"], sample_min=kw["uniform_dist_min"], sample_max=kw["uniform_dist_max"],
                learning_rate=kw["learning_rate"], gradmax_clip=kw["gradmax_clip"], adam_beta_1=kw["adam_beta_1"], adam_beta_2=kw["adam_beta_2"],
                adam_epsilon=kw["adam_epsilon"], adam_rule=1 if rule == "keras" else 0)


def rpgd_vec(b):
    """the state before a step of hyper_cases.rpgd_ref, as set_state takes it"""
    z = np.zeros_like(b["Q"])
    return np.concatenate([b["Q"].ravel(), (z if b["m"] is None else b["m"]).ravel(), (z if b["v"] is None else b["v"]).ravel(), b["ages"].ravel(), b["u"],
                           [b["adam_step"]], [b["count"]]]).astype(np.float32)


def check_rpgd(tag, own, ref, t, u, read, tuned, tol=None):
    """the state after step t: plans, moments, ages and u.  The fresh rows of a resampling step come from the draws alone: 1e-6."""
    st, kw = ref["steps"][t], Hc.config_of(Hc.RPGD_DEFAULTS, own)
    tol = tol if tol is not None else dict(rtol=1e-3, atol=2e-3) if tuned else dict(rtol=2e-5, atol=2e-5)
    out = 2.0 * kw["learning_rate"] * kw["outer_its"]
    n_new = st["Q"].shape[0] - ref["k"] if t == 0 else 0
    plan, m, v = read("PLAN"), read("ADAM_M"), read("ADAM_V")
    if n_new:
        close(tag, "fresh", plan[:n_new], st["Q"][:n_new], rtol=1e-6, atol=1e-6)
        assert np.all(m[:n_new] == 0.0) and np.all(v[:n_new] == 0.0)
    mostly(tag, "plan", plan[n_new:], st["Q"][n_new:], outlier_atol=out, **tol)
    mostly(tag, "adam_m", m[n_new:], st["m"][n_new:], rtol=2e-3, atol=2e-4 * float(np.abs(st["m"]).max()), outlier_atol=float(np.abs(st["m"]).max()))
    mostly(tag, "adam_v", v[n_new:], st["v"][n_new:], rtol=4e-3, atol=4e-4 * float(np.abs(st["v"]).max()), outlier_atol=float(np.abs(st["v"]).max()))
    assert np.all(m[:, -1, :] == 0.0) and np.all(v[:, -1, :] == 0.0)       # the moments move by ONE step, whatever shift_previous is
    np.testing.assert_array_equal(read("AGES"), st["ages"])
    close(tag, "u", u, st["u"], **tol)


def rpgd_two_steps(tag, env, own, e, ref, tuned, tol=None, before_step=None):
    for t in range(2):
        e.set_state(rpgd_vec(ref["steps"][t]["before"]))                   # pinned to the oracle's state
        if before_step is not None:
            before_step()
        draws = ref["resample_draws"] if t == 0 else None
        assert e.samples_needed() == (0 if draws is None else draws.size)
        u = e.step(ref["s"], draws, u_prev=ref["steps"][t]["before"]["u"])
        check_rpgd(f"{tag} step {Hc.rpgd_id(own)} t{t}", own, ref, t, u, e.read, tuned, tol)


@FORMS_P
def test_rpgd_kernels(env, generic):
    """ctk_rpgd_descent + ctk_rpgd_warmstart (CartPole's own) and ctk_g_rpgd_descent<ENV>: every Adam, clip, shift and sampling case and ALL;
    a resampling step and one that keeps every row"""
    tuned = env == "CartPole" and not generic
    for own in [()] + Hc.RPGD_CASES:
        ref = Hc.rpgd_ref(env, own)
        e = case_engine("rpgd", env, own, generic_kernels=generic, num_rollouts=Hc.RPGD_N, mpc_horizon=Hc.RPGD_H,
                        period_interpolation_inducing_points=Hc.RPGD_P, **rpgd_cfg(own, ref["k"]))
        e.reset(ref["reset_draws"])
        close(f"hyper rpgd {form_id(env, generic)} step {Hc.rpgd_id(own)} reset", "plan", e.read("PLAN"), ref["Q_init"], rtol=1e-6, atol=1e-6)
        rpgd_two_steps(f"hyper rpgd {form_id(env, generic)}", env, own, e, ref, tuned)
        k = e.dominant_kernel()
        e.close()
        assert k == rpgd_kernel(env, generic), k


@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_keras_rule(env):
    """adam_rule 1 (the published Keras rule) at ALL, on the template and on CartPole's own kernels: against the oracle's KerasAdam, which
    test_hyper_cases_cpu.py holds to OptimF64.adam_keras"""
    own = Hc.RPGD_ALL
    ref = Hc.rpgd_ref(env, own, "keras")
    for generic in ([False, True] if env == "CartPole" else [False]):
        e = case_engine("rpgd", env, own, generic_kernels=generic, num_rollouts=Hc.RPGD_N, mpc_horizon=Hc.RPGD_H,
                        period_interpolation_inducing_points=Hc.RPGD_P, **rpgd_cfg(own, ref["k"], "keras"))
        e.reset(ref["reset_draws"])
        rpgd_two_steps(f"hyper rpgd keras {form_id(env, generic)}", env, own, e, ref, env == "CartPole" and not generic)
        assert e.dominant_kernel() == rpgd_kernel(env, generic), e.dominant_kernel()
        e.close()


RPGD_NETS = [("CartPole", "MLP", "ctk_rpgd_mlp_persistent"), ("CartPole", "GRU", "ctk_g_rpgd_descent_split<0, SplitGru>"),
             ("Quad2D", "MLP", "ctk_g_rpgd_persist<1, false>"), ("Hover", "GRU", "ctk_g_rpgd_descent_split<2, SplitGru>")]


@pytest.mark.parametrize("env,kind,kernel", RPGD_NETS, ids=[f"{e}-{k}" for e, k, _ in RPGD_NETS])
def test_rpgd_network_kernels(env, kind, kernel):
    """ALL on the reverse kernels of the network predictors: CartPole's one-launch (persistent) MLP descent, the template's one-launch MLP
    descent on Quad2D, the template's split GRU descent on CartPole (the gradient family's GRU runs on the template) and Hover"""
    own = Hc.RPGD_ALL
    ref = Hc.rpgd_ref(env, own, "torch", kind)
    e = case_engine("rpgd", env, own, kind, num_rollouts=ref["N"], mpc_horizon=Hc.RPGD_H, period_interpolation_inducing_points=Hc.RPGD_P,
                    **rpgd_cfg(own, ref["k"]))
    e.set_predictor_weights(ref["weights"])
    e.reset(ref["reset_draws"])
    rpgd_two_steps(f"hyper rpgd {kind} {env}", env, own, e, ref, False, NET_TOL, (lambda: e.predictor_set_hidden(None)) if kind == "GRU" else None)
    k = e.dominant_kernel()
    e.close()
    assert k == kernel, k


@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_batch(env):
    """ctk_g_rpgd_batch<ENV> at B = 3 and ALL: every problem against the oracle's steps with that problem's own draws"""
    own = Hc.RPGD_ALL
    refs = [Hc.rpgd_ref(env, own, seed=Hc.RPGD_SEED + q) for q in range(B)]
    ref = refs[0]
    lo, hi = Hc.limits_of(env, own)
    batch = CtkRpgdBatch(B, seeds=[1, 2, 3], environment=env, num_rollouts=Hc.RPGD_N, mpc_horizon=Hc.RPGD_H, dt=Hc.DT, action_low=lim(lo), action_high=lim(hi),
                         period_interpolation_inducing_points=Hc.RPGD_P, **rpgd_cfg(own, ref["k"]))
    set_params(batch, L.env_params(env))
    batch.reset(np.stack([r["reset_draws"] for r in refs]))
    for t in range(2):
        for q in range(B):
            batch.set_state(q, rpgd_vec(refs[q]["steps"][t]["before"]))
        draws = np.stack([r["resample_draws"] for r in refs]) if t == 0 else None
        u = np.array(batch.step(np.stack([ref["s"]] * B), draws, u_prev=np.stack([r["steps"][t]["before"]["u"] for r in refs]))).copy()
        for q in range(B):
            check_rpgd(f"hyper rpgd batch {env} step ALL t{t} problem {q}", own, refs[q], t, u[q], lambda name: batch.read(name, q), False)
    k = batch.dominant_kernel()
    batch.close()
    assert k == f"ctk_g_rpgd_batch<{ENV_ID[env]}>", k


def test_gradient_variant_away_from_the_defaults():
    """`gradient` on ctk_rpgd_descent<0> (Keras rule, no resampling): every Adam scalar moved and a clip that binds, against the oracle's
    GradientTF"""
    env, N, H, its = "CartPole", 40, 20, 3
    kw = dict(learning_rate=0.2, adam_beta_1=0.7, adam_beta_2=0.9, adam_epsilon=1e-3, gradmax_clip=0.05)
    lo, hi = Hc.ASYM[env]
    pars = L.env_params(env)
    e = CtkEngine("gradient", "ODE", num_rollouts=N, mpc_horizon=H, dt=Hc.DT, outer_its=its, action_low=lim(lo), action_high=lim(hi), **kw)
    set_params(e, pars)
    o = O.GradientTF(O.Predictor("ODE", dt=Hc.DT, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, gradient_steps=its, **kw)
    rng = np.random.default_rng(N)
    d0, tail = rng.random((N, H, 1), dtype=np.float32), rng.random((N, 1, 1), dtype=np.float32)
    e.reset(d0)
    o.optimizer_reset(d0)
    s = Hc.STATE[env]
    uo, ug = o.step(s, tail), np.array(e.step(s, tail, u_prev=np.zeros(1, np.float32)), np.float32).copy()
    tag, tol = "hyper gradient CartPole step ALL", dict(rtol=5e-4, atol=5e-4)      # test_gradient_matches_oracle's
    mostly(tag, "Q", e.read("Q"), o.Q_refined, outlier_atol=2.0 * kw["learning_rate"] * its, **tol)
    close(tag, "J", e.read("J"), o.J, rtol=2e-3, atol=2e-2)
    mostly(tag, "adam_m", e.read("ADAM_M"), o.opt.m, outlier_atol=float(np.abs(o.opt.m).max()), **tol)
    vmax = float(np.abs(o.opt.v).max())
    mostly(tag, "adam_v", e.read("ADAM_V"), o.opt.v, rtol=4e-3, atol=4e-4 * vmax, outlier_atol=vmax)     # check_rpgd's: 1 - beta_2 directly
    close(tag, "u", ug[0], uo, rtol=1e-3, atol=1e-3)
    assert np.all(np.abs(e.read("ADAM_M")).reshape(N, -1).max(axis=1) > 0)
    k = e.dominant_kernel()
    e.close()
    assert k == RPGD_OWN, k


def test_cem_grad_bharadhwaj_variant_away_from_the_defaults():
    """`cem_grad_bharadhwaj` on ctk_rpgd_descent<0>: Keras rule with every scalar moved, a clip that binds, asymmetric limits and a clamp,
    against the oracle"""
    env, N, H, K, its = "CartPole", 32, 20, 8, 2
    kw = dict(cem_outer_it=its, cem_best_k=K, cem_initial_action_stdev=1.3, cem_stdev_min=0.4, learning_rate=0.2, adam_beta_1=0.7, adam_beta_2=0.9,
              adam_epsilon=1e-3, gradmax_clip=0.05)
    lo, hi = Hc.ASYM[env]
    pars = L.env_params(env)
    e = CtkEngine("cem_grad_bharadhwaj", "ODE", num_rollouts=N, mpc_horizon=H, dt=Hc.DT, action_low=lim(lo), action_high=lim(hi), **kw)
    set_params(e, pars)
    o = O.CEMGradBharadhwaj(O.Predictor("ODE", dt=Hc.DT, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, **kw)
    rng = np.random.default_rng(N * H)
    el, rest = rng.standard_normal((K, H, 1)).astype(np.float32), rng.standard_normal((its, N - K, H, 1)).astype(np.float32)
    e.reset()
    s = Hc.STATE[env]
    uo, ug = o.step(s, el, rest), np.array(e.step(s, np.concatenate([el.ravel(), rest.ravel()]), u_prev=np.zeros(1, np.float32)), np.float32).copy()
    tag, tol = "hyper cem_grad_bharadhwaj CartPole step ALL", dict(rtol=5e-4, atol=5e-4)   # test_cem_grad_bharadhwaj_matches_oracle's
    mostly(tag, "Q", e.read("Q"), o.Q, outlier_atol=2.0 * kw["learning_rate"] * its, **tol)
    mostly(tag, "adam_m", e.read("ADAM_M"), o.opt.m, outlier_atol=float(np.abs(o.opt.m).max()), **tol)
    vmax = float(np.abs(o.opt.v).max())
    mostly(tag, "adam_v", e.read("ADAM_V"), o.opt.v, rtol=4e-3, atol=4e-4 * vmax, outlier_atol=vmax)
    close(tag, "mu", e.read("U_NOM"), o.dist_mue, rtol=1e-3, atol=1e-3)
    close(tag, "std", e.read("STD"), o.stdev, rtol=5e-3, atol=1e-3)
    close(tag, "u", ug[0], uo, rtol=1e-3, atol=1e-3)
    assert np.mean(o.stdev[:, :-1] == np.float32(0.4)) > 0.5              # the clamp binds
    k = e.dominant_kernel()
    e.close()
    assert k == RPGD_OWN, k
