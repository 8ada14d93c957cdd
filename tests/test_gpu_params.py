"""-m gpu: every plant and cost parameter moved away from its default, on every kernel, against the float32 oracle at the same parameters.

Every kernel consumes float32 constants that the library derives from the primary parameters (derive_constants, Env<ENV>::derive, the
batches' per-problem derivation) and that ctk_set_param refreshes: the handle's copy, the packed launch-argument block of the MPPI
step, the resident kernel's arguments in device memory.  The rest of the suite runs at the defaults, where cc_weight = R = 1,
target_equilibrium = ccrc_weight = 1, target_z = 1 and targets of 0 hide a missing or doubled factor, and it never steps a handle,
changes a parameter and steps again.  The cases are tests/param_cases.py's (one per parameter, and ALL), guarded on the CPU by
tests/test_param_cases_cpu.py: there the oracle itself is held against PlantF64, a float64 statement of the plants and costs from the
primary parameters alone, so a derivation that the oracle and the library share cannot hide, and every case is shown to move the tensor
it is compared in by 20 bounds or more.

THE SEQUENCE on every handle (sweep() below): created with the library's defaults; one step at the defaults, kept; then for every case
set_param the case's values, the zero plan, one step, compared, get_param returns what was set, the defaults again; at the end one more
step at the defaults, which must equal the first BIT FOR BIT: nothing stale survives set_param.  The steps at the defaults are compared
with the oracle as well.

Bounds, all the project's own (every comparison goes through margins.close with a tag that starts "params"):
  J  rtol 3e-5 / atol 1e-3;  TRAJ  rtol 1e-4 / atol 3e-5;  u, U_NOM  U_TOL;  CEM's Q, mu, STD, u  test_gpu_large_angles.check_cem's;
  ADAM_M  test_rpgd_single_gradient_matches_oracle's (CartPole's own kernel: rtol 2e-4 / atol 1e-6, on gradients clipped to norm 5 as
  there, see rpgd_bounds) and test_hover_single_gradient_matches_oracle_adjoint's (template and network kernels: rtol 2e-3, GRU 3e-3 /
  atol 2e-4, GRU 3e-4, of the largest gradient).
Each test names the kernel it means to run and checks dominant_kernel() after a step."""
import functools

import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkCemBatch, CtkRpgdBatch
import large_angle_cases as L
import param_cases as P
from margins import close
from test_gpu_mppi import U_TOL
from test_gpu_rpgd import assert_close_mostly
from test_gpu_large_angles import J_TOL, ENV_ID, FORMS, FORM_IDS, TP_N, TP_H, limits, rpgd_kernel_ok
from test_gpu_substeps import mppi_check, cem_check

pytestmark = pytest.mark.gpu

TRAJ_TOL = dict(rtol=1e-4, atol=3e-5)
FORMS_P = pytest.mark.parametrize("env,generic", FORMS, ids=FORM_IDS)


def form_id(env, generic):
    return FORM_IDS[FORMS.index((env, generic))]


def zeros(env):
    return np.zeros(L.LIMITS[env][0].size, np.float32)


def apply(x, env, own):
    """the parameters of a case on a handle or a whole batch: every name, through set_param; get_param returns what was set"""
    pars = P.params_with(env, own)
    for n in pars.param_names():
        x.set_param(n, float(getattr(pars, n)))
    for n in pars.param_names():
        assert np.float32(x.get_param(n)) == np.float32(getattr(pars, n)), n


def sweep(x, env, cases, at):
    """THE SEQUENCE.  at(own) -> the tensors of one step from a clean optimizer state at the parameters that are set (and compares them
    with the oracle's at `own`); x is created with the library's defaults"""
    for n, v in P.DEFAULTS[env]:                                          # premise: the handle was created with the defaults
        assert np.float32(x.get_param(n)) == np.float32(v), n
    first = at(P.DEFAULTS[env])
    for own in cases:
        apply(x, env, own)
        at(own)
        apply(x, env, P.DEFAULTS[env])
    again = at(P.DEFAULTS[env])
    assert len(first) == len(again) and len(first) > 0
    for a, b in zip(first, again):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg="a step at the defaults after the sweep differs from the one before it")


def engine(opt, env, pred="ODE", **kw):
    lo, hi = limits(env)
    return CtkEngine(opt, pred, environment=env, dt=P.DT, action_low=lo, action_high=hi, **kw)


# ---- MPPI: the four-wave kernel ---------------------------------------------------------------------------------------------------------
def mppi_at(e, env, tag, N, H, p, materialize, own):
    ref = P.mppi_ref(env, N, H, p, own)
    C = ref["Q"].shape[2]
    e.set_state(np.zeros(H * C + C, np.float32))
    u = np.array(e.step(ref["s"], ref["noise"], u_prev=np.zeros(C, np.float32)), np.float32).copy()
    mppi_check(f"{tag} step {P.case_id(env, own)} N{N} H{H} p{p}", env, ref, u, e.read, materialize, False)
    return [u, e.read("J").copy(), e.read("U_NOM").copy()] + ([e.read("TRAJ").copy()] if materialize else [])


@pytest.mark.parametrize("materialize", [True, False])
@FORMS_P
def test_mppi_four_wave_kernel(env, generic, materialize):
    eid, log = ENV_ID[env], "true" if materialize else "false"
    for N, H, p in P.SIZES:
        e = engine("mppi", env, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, materialize_trajectories=materialize,
                   generic_kernels=generic)
        sweep(e, env, P.CASES[env], functools.partial(mppi_at, e, env, f"params mppi {form_id(env, generic)} log={log}", N, H, p, materialize))
        k = e.dominant_kernel()
        e.close()
        assert k.startswith(f"ctk_mppi_rollout<{eid}, 0, {log}, false"), k


@pytest.mark.parametrize("env", P.ENVS)
def test_mppi_resident_form(env):
    """ALL: a resident step at the defaults, set_param while the kernel is resident, a resident step, the defaults, a resident step.  (The
    reads end residency, so the first step keeps u alone; set_param itself must reach the kernel's arguments in device memory.)"""
    import torch
    C, N, H, p = L.LIMITS[env][0].size, 128, 20, 1
    e = engine("mppi", env, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    e.resident_enable(True, idle_us=100000.0)
    bufs = {}

    def resident_step(own):
        ref = P.mppi_ref(env, N, H, p, own)
        if own not in bufs:
            bufs[own] = torch.from_numpy(ref["noise"]).to("cuda")
            torch.cuda.synchronize()
        e.set_state(np.zeros(H * C + C, np.float32))
        u = np.array(e.step(ref["s"], bufs[own].data_ptr(), u_prev=np.zeros(C, np.float32)), np.float32).copy()
        assert e.dominant_kernel().startswith(f"ctk_mppi_resident<{ENV_ID[env]}, "), e.dominant_kernel()
        close(f"params mppi resident {env} step {P.case_id(env, own)}", "u", u, ref["u"], **U_TOL)
        return ref, u

    _, u0 = resident_step(P.DEFAULTS[env])
    ref, u = resident_step(P.DEFAULTS[env])                               # the kernel is resident now: the parameters change under it
    np.testing.assert_array_equal(u, u0)
    apply(e, env, P.ALL[env])
    ref, u = resident_step(P.ALL[env])
    apply(e, env, P.DEFAULTS[env])
    ref, u = resident_step(P.DEFAULTS[env])
    np.testing.assert_array_equal(u, u0)
    apply(e, env, P.ALL[env])
    ref, u = resident_step(P.ALL[env])
    mppi_check(f"params mppi resident {env} step ALL, read", env, ref, u, e.read, False, False)        # (the reads end residency)
    e.close()


@pytest.mark.parametrize("kernel,p,generic", [("ctk_mppi_rollout_tps<", 1, False), ("ctk_mppi_rollout_tp<", 2, False), ("ctk_g_rollout", 1, True)],
                         ids=["streaming", "whole-tile", "template"])
def test_mppi_throughput_kernels(kernel, p, generic):
    """ALL, at the smallest N that selects them (the one large shape of the file)"""
    env = "CartPole"
    for log in (True, False):
        e = engine("mppi", env, num_rollouts=TP_N, mpc_horizon=TP_H, period_interpolation_inducing_points=p, materialize_trajectories=log,
                   generic_kernels=generic)
        sweep(e, env, [P.ALL[env]], functools.partial(mppi_at, e, env, f"params mppi {kernel.rstrip('<')} log={log}", TP_N, TP_H, p, log))
        assert kernel in e.dominant_kernel(), e.dominant_kernel()
        e.close()


# ---- CEM: the one-launch step and the launch per phase; CEM-GMM ---------------------------------------------------------------------------
def cem_at(e, env, tag, N, H, own):
    ref = P.cem_ref(env, N, H, own)
    e.reset()
    u = np.array(e.step(ref["s"], ref["noise"], u_prev=zeros(env)), np.float32).copy()
    cem_check(f"{tag} step {P.case_id(env, own)} N{N} H{H}", env, ref, u, e.read, False)
    return [u, e.read("J").copy(), e.read("U_NOM").copy(), e.read("STD").copy(), e.read("TRAJ").copy()]


@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "launch-per-phase"])
@pytest.mark.parametrize("env", P.ENVS)
def test_cem_kernels(env, fused, monkeypatch):
    eid = ENV_ID[env]
    for N, H in P.CEM_SIZES:
        if not fused:
            monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")           # read when the handle is created
        e = engine("cem", env, num_rollouts=N, mpc_horizon=H, cem_outer_it=L.CEM_ITS, cem_best_k=L.CEM_K, materialize_trajectories=True)
        monkeypatch.delenv("CTK_NO_CEM_FUSED", raising=False)
        sweep(e, env, P.CASES[env], functools.partial(cem_at, e, env, f"params cem {'fused' if fused else 'phases'} {env}", N, H))
        k = e.dominant_kernel()
        e.close()
        assert k == f"ctk_cem_fused<{eid}, true>" if fused else k.startswith(f"ctk_affine_rollout<{eid},"), k


@pytest.mark.parametrize("env", P.S.GMM_ENVS)
def test_cem_gmm_in_rollout_sampling(env):
    """ALL: ctk_affine_rollout_mix, one outer iteration from the initial mixture"""
    from gmm_oracle import pack_draws
    e = engine("cem_gmm", env, num_rollouts=128, mpc_horizon=20, cem_outer_it=1, cem_best_k=16, cem_initial_action_stdev=0.5, cem_stdev_min=0.01,
               materialize_trajectories=True)

    def at(own):
        ref = P.gmm_ref(env, own)
        e.reset()
        u = np.array(e.step(ref["s"], pack_draws(ref["normals"], ref["uniforms"]), u_prev=zeros(env)), np.float32).copy()
        tag = f"params cem_gmm {env} step {P.case_id(env, own)}"
        close(tag, "Q", e.read("Q"), ref["Q"], rtol=1e-5, atol=2e-6)
        close(tag, "J", e.read("J"), ref["J"], **J_TOL)
        close(tag, "u", u, ref["u"], rtol=1e-5, atol=2e-6)
        return [u, e.read("J").copy(), e.read("Q").copy()]

    sweep(e, env, [P.ALL[env]], at)
    assert e.dominant_kernel() == f"ctk_affine_rollout_mix<{ENV_ID[env]}, true>", e.dominant_kernel()
    e.close()


# ---- random action and plain rollout() --------------------------------------------------------------------------------------------------
@FORMS_P
def test_random_action_and_plain_rollout(env, generic):
    eid, form = ENV_ID[env], form_id(env, generic)
    for N, H in P.ROLLOUT_SIZES:
        e = engine("random_action", env, num_rollouts=N, mpc_horizon=H, materialize_trajectories=True, generic_kernels=generic)

        def at(own):
            r = P.rollout_ref(env, N, H, own)                        # plans beyond the limits, taken as given
            tag = f"params rollout {form} step {P.case_id(env, own)} N{N} H{H}"
            traj, J = e.rollout(r["s"], r["Q"], u_prev=r["u_prev"])
            close(tag, "J", J, r["J"], **J_TOL)
            close(tag, "traj", traj, r["traj"], **TRAJ_TOL)
            ref = P.random_ref(env, N, H, own)
            u = np.array(e.step(ref["s"], ref["u01"], u_prev=zeros(env)), np.float32).copy()
            tag = f"params random_action {form} step {P.case_id(env, own)} N{N} H{H}"
            close(tag, "Q", e.read("Q"), ref["Q"], rtol=1e-6, atol=1e-7)
            close(tag, "J", e.read("J"), ref["J"], **J_TOL)
            close(tag, "traj", e.read("TRAJ"), ref["traj"], **TRAJ_TOL)
            assert int(e.read("BEST_IDX")[0]) == ref["best_idx"]
            close(tag, "u", u, ref["u"], rtol=1e-6, atol=1e-7)
            return [np.array(traj).copy(), np.array(J).copy(), u, e.read("J").copy(), e.read("TRAJ").copy()]

        sweep(e, env, P.CASES[env], at)
        k = e.dominant_kernel()
        e.close()
        assert k == f"ctk_affine_rollout<{eid}, 0, true>", k


# ---- the reverse sweeps: one Adam iteration from zero moments, ADAM_M == (1 - beta1) g ----------------------------------------------------
GRAD_N, GRAD_H = 64, 20


def rpgd_common(env, N, H, clip):
    lo, hi = limits(env)
    return dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=P.DT, period_interpolation_inducing_points=1, outer_its=1, resamp_per=1000,
                shift_previous=1, opt_keep_k=16, sampling_distribution=0, sample_whole_control_space=1, learning_rate=0.05, adam_beta_1=0.9,
                adam_beta_2=0.999, adam_epsilon=1e-8, gradmax_clip=clip, action_low=lo, action_high=hi)


def rpgd_state(Q0, up):
    """plans Q0, zero moments, zero ages, u_prev, Adam step 0, count 1 (no resampling in the step)"""
    return np.concatenate([Q0.ravel(), np.zeros(2 * Q0.size + Q0.shape[0], np.float32), up, [0], [1]]).astype(np.float32)


def rpgd_bounds(kind, tuned_cartpole, g):
    """(what ADAM_M is compared with, rtol, atol).  Template and network kernels: the moments of the unclipped gradient at
    test_hover_single_gradient_matches_oracle_adjoint's bounds.  CartPole's own kernel: test_rpgd_single_gradient_matches_oracle's
    rtol 2e-4 / atol 1e-6 are stated for gradients clipped to norm 5 per rollout (gradmax_clip of its fixture), so the moments of BOTH
    sides are scaled to that norm before they are compared: the same bound on the same scale, whatever the parameters make of |g|."""
    if not tuned_cartpole:
        return None, (3e-3 if kind == "GRU" else 2e-3), (3e-4 if kind == "GRU" else 2e-4) * float(np.abs(g).max())
    norm = np.sqrt((g.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True))
    return (5.0 / np.maximum(norm, 5.0)), 2e-4, 1e-6


def grad_at(read, env, kind, tag, tuned_cartpole, own, N, H):
    _, g = P.oracle_grad(env, kind, own, N, H)
    m = read("ADAM_M")                  # after the warm start: shifted by one step, tail zero-filled
    scale, rtol, atol = rpgd_bounds(kind, tuned_cartpole, g)
    got, want = m[:, :-1, :], 0.1 * g[:, 1:, :]
    if scale is not None:
        got, want = got * scale, want * scale
    close(f"{tag} step {P.case_id(env, own)}", "adam_m", got, want, rtol=rtol, atol=atol)
    assert np.all(m[:, -1, :] == 0.0)
    return [m.copy()]


@FORMS_P
def test_rpgd_single_gradient(env, generic):
    """ctk_rpgd_descent (CartPole's own) and ctk_g_rpgd_descent<ENV> (the template: CartPole, Quad2D, Hover)"""
    N, H, C = GRAD_N, GRAD_H, L.LIMITS[env][0].size
    e = CtkEngine("rpgd", "ODE", generic_kernels=generic, **rpgd_common(env, N, H, 1e9))
    e.reset(np.random.default_rng(3).random((N, H, C), dtype=np.float32))
    tuned = env == "CartPole" and not generic

    def at(own):
        s, Q0, up = P.grad_inputs(env, N, H, own)
        e.set_state(rpgd_state(Q0, up))
        e.step(s, None, u_prev=up)
        return grad_at(e.read, env, "ODE", f"params rpgd gradient {form_id(env, generic)}", tuned, own, N, H)

    sweep(e, env, P.CASES[env], at)
    assert rpgd_kernel_ok(e.dominant_kernel(), env, generic), e.dominant_kernel()
    e.close()


# ---- the variants (gradient, cem_naive_grad, cem_grad_bharadhwaj): ALL, one step, against their oracle classes -----------------------------
# (their reset() leaves u and Adam's moments alone, as the reference's does: every step starts from the state a fresh handle has)
def test_gradient_variant():
    env, N, H, its = "CartPole", 40, 20, 3
    e = CtkEngine("gradient", "ODE", num_rollouts=N, mpc_horizon=H, dt=P.DT, outer_its=its, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999,
                  adam_epsilon=1e-7, gradmax_clip=5.0)
    rng = np.random.default_rng(N)
    d0, tail = rng.random((N, H, 1), dtype=np.float32), rng.random((N, 1, 1), dtype=np.float32)
    e.reset(d0)
    clean = e.get_state().copy()

    def at(own):
        pars = P.params_with(env, own)
        o = O.GradientTF(O.Predictor("ODE", dt=P.DT, env=pars), O.Cost(pars), num_rollouts=N, mpc_horizon=H, gradient_steps=its, learning_rate=0.05,
                         adam_epsilon=1e-7, gradmax_clip=5.0)
        o.optimizer_reset(d0)
        e.set_state(clean)
        s = P.base_state(env, own)
        uo, ug = o.step(s, tail), np.array(e.step(s, tail, u_prev=zeros(env)), np.float32).copy()
        tag, tol = f"params gradient {env} step {P.case_id(env, own)}", dict(rtol=5e-4, atol=5e-4)      # test_gradient_matches_oracle's
        assert_close_mostly(e.read("Q"), o.Q_refined, **tol)
        close(tag, "J", e.read("J"), o.J, rtol=2e-3, atol=2e-2)
        assert_close_mostly(e.read("ADAM_M"), o.opt.m, **tol)
        close(tag, "u", ug[0], uo, rtol=1e-3, atol=1e-3)
        return [ug, e.read("J").copy(), e.read("ADAM_M").copy()]

    sweep(e, env, [P.ALL[env]], at)
    e.close()


def test_cem_naive_grad_variant():
    env, N, H, K, its = "CartPole", 128, 12, 32, 2
    kw = dict(cem_outer_it=its, cem_best_k=K, cem_initial_action_stdev=0.5, cem_stdev_min=0.1, learning_rate=0.1, gradmax_clip=10.0)
    e = CtkEngine("cem_naive_grad", "ODE", num_rollouts=N, mpc_horizon=H, dt=P.DT, **kw)
    noise = np.random.default_rng(N + H).standard_normal((its, N, H, 1)).astype(np.float32)
    e.reset()
    clean = e.get_state().copy()

    def at(own):
        pars = P.params_with(env, own)
        o = O.CEMNaiveGrad(O.Predictor("ODE", dt=P.DT, env=pars), O.Cost(pars), num_rollouts=N, mpc_horizon=H, **kw)
        e.set_state(clean)
        s = P.base_state(env, own)
        uo, ug = o.step(s, noise), np.array(e.step(s, noise, u_prev=zeros(env)), np.float32).copy()
        tag = f"params cem_naive_grad {env} step {P.case_id(env, own)}"                                  # test_cem_naive_grad_matches_oracle's
        close(tag, "Q", e.read("Q"), o.Q, rtol=1e-4, atol=2e-4)
        close(tag, "J", e.read("J"), o.J, rtol=2e-4, atol=1e-2)
        close(tag, "mu", e.read("U_NOM"), o.dist_mue, rtol=1e-4, atol=1e-4)
        close(tag, "std", e.read("STD"), o.stdev, rtol=1e-3, atol=1e-4)
        close(tag, "u", ug[0], uo, rtol=1e-4, atol=1e-4)
        return [ug, e.read("J").copy(), e.read("Q").copy()]

    sweep(e, env, [P.ALL[env]], at)
    e.close()


def test_cem_grad_bharadhwaj_variant():
    env, N, H, K, its = "CartPole", 32, 20, 8, 2
    kw = dict(cem_outer_it=its, cem_best_k=K, cem_initial_action_stdev=2.0, cem_stdev_min=1e-6, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999,
              adam_epsilon=1e-8, gradmax_clip=5.0)
    e = CtkEngine("cem_grad_bharadhwaj", "ODE", num_rollouts=N, mpc_horizon=H, dt=P.DT, **kw)
    rng = np.random.default_rng(N * H)
    el, rest = rng.standard_normal((K, H, 1)).astype(np.float32), rng.standard_normal((its, N - K, H, 1)).astype(np.float32)
    e.reset()
    clean = e.get_state().copy()

    def at(own):
        pars = P.params_with(env, own)
        o = O.CEMGradBharadhwaj(O.Predictor("ODE", dt=P.DT, env=pars), O.Cost(pars), num_rollouts=N, mpc_horizon=H, **kw)
        e.set_state(clean)
        s = P.base_state(env, own)
        uo, ug = o.step(s, el, rest), np.array(e.step(s, np.concatenate([el.ravel(), rest.ravel()]), u_prev=zeros(env)), np.float32).copy()
        tag, tol = f"params cem_grad_bharadhwaj {env} step {P.case_id(env, own)}", dict(rtol=5e-4, atol=5e-4)   # test_cem_grad_bharadhwaj_matches_oracle's
        assert_close_mostly(e.read("Q"), o.Q, **tol)
        assert_close_mostly(e.read("ADAM_M"), o.opt.m, **tol)
        close(tag, "mu", e.read("U_NOM"), o.dist_mue, rtol=1e-3, atol=1e-3)
        close(tag, "std", e.read("STD"), o.stdev, rtol=5e-3, atol=1e-3)
        close(tag, "u", ug[0], uo, rtol=1e-3, atol=1e-3)
        return [ug, e.read("Q").copy(), e.read("ADAM_M").copy()]

    sweep(e, env, [P.ALL[env]], at)
    e.close()


# ---- the batch families: B = 3, every problem against the oracle ---------------------------------------------------------------------------
B = 3
BATCH_FORMS = pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per-problem"])


def batch_sweep(batch, env, per_problem, at):
    """THE SEQUENCE on a batch.  shared: set_param(ALL) on the whole batch.  per-problem: set_problem_params, problem 1 holds ALL and the
    others the defaults.  at(owns) steps all problems once and compares problem q with the oracle at owns[q]."""
    dflt, everything = P.DEFAULTS[env], P.ALL[env]
    vals = {n: [float(getattr(P.params_with(env, own), n)) for own in (dflt, everything, dflt)] for n in batch.param_names}
    if per_problem:                                                       # the per-problem form of the kernel from the first step on
        for n in batch.param_names:
            batch.set_problem_params(n, [vals[n][0]] * B)
    first = at([dflt] * B)
    if per_problem:
        for n in batch.param_names:
            batch.set_problem_params(n, vals[n])
        for n in batch.param_names:
            for q in range(B):
                assert batch.get_problem_param(n, q) == np.float32(vals[n][q]), (n, q)
        at([dflt, everything, dflt])
        for n in batch.param_names:
            batch.set_problem_params(n, [vals[n][0]] * B)
        again = at([dflt] * B)
    else:
        apply(batch, env, everything)
        at([everything] * B)
        apply(batch, env, dflt)
        again = at([dflt] * B)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b, err_msg="a batch step at the defaults after the sweep differs from the one before it")


@BATCH_FORMS
@pytest.mark.parametrize("env", P.ENVS)
def test_mppi_batch(env, per_problem):
    C, eid = L.LIMITS[env][0].size, ENV_ID[env]
    lo, hi = limits(env)
    for N, H, p in P.SIZES:
        batch = CtkMppiBatch(B, seeds=[1, 2, 3], environment=env, num_rollouts=N, mpc_horizon=H, dt=P.DT, period_interpolation_inducing_points=p,
                             action_low=lo, action_high=hi, materialize_trajectories=True)

        def at(owns):
            refs = [P.mppi_ref(env, N, H, p, own) for own in owns]
            for q in range(B):
                batch.set_state(q, np.zeros(H * C + C, np.float32))
            u = np.array(batch.step(np.stack([r["s"] for r in refs]), np.stack([r["noise"] for r in refs]), u_prev=np.zeros((B, C), np.float32))).copy()
            out = [u]
            for q in range(B):
                tag = f"params mppi batch{'_pp' if per_problem else ''} {env} step problem {q} {P.case_id(env, owns[q])} N{N} p{p}"
                mppi_check(tag, env, refs[q], u[q], lambda name: batch.read(name, q), True, False)
                out += [batch.read("J", q).copy(), batch.read("TRAJ", q).copy()]
            return out

        batch_sweep(batch, env, per_problem, at)
        if per_problem:
            assert batch.params_differ() == 1
        assert batch.dominant_kernel() == f"ctk_mppi_batch{'_pp' if per_problem else ''}<{eid}, true>", batch.dominant_kernel()
        batch.close()


@BATCH_FORMS
@pytest.mark.parametrize("env", P.ENVS)
def test_cem_batch(env, per_problem):
    C, eid, (N, H) = L.LIMITS[env][0].size, ENV_ID[env], P.CEM_SIZES[1]
    lo, hi = limits(env)
    batch = CtkCemBatch(B, seeds=[1, 2, 3], environment=env, num_rollouts=N, mpc_horizon=H, dt=P.DT, action_low=lo, action_high=hi,
                        materialize_trajectories=True, cem_outer_it=L.CEM_ITS, cem_best_k=L.CEM_K, cem_initial_action_stdev=0.5, cem_stdev_min=0.01)

    def at(owns):
        refs = [P.cem_ref(env, N, H, own) for own in owns]
        batch.reset()
        u = np.array(batch.step(np.stack([r["s"] for r in refs]), np.stack([r["noise"] for r in refs]), u_prev=np.zeros((B, C), np.float32))).copy()
        out = [u]
        for q in range(B):
            tag = f"params cem batch{'_pp' if per_problem else ''} {env} step problem {q} {P.case_id(env, owns[q])}"
            cem_check(tag, env, refs[q], u[q], lambda name: batch.read(name, q), False)
            out += [batch.read("J", q).copy(), batch.read("TRAJ", q).copy()]
        return out

    batch_sweep(batch, env, per_problem, at)
    assert batch.dominant_kernel() == f"ctk_cem_batch{'_pp' if per_problem else ''}<{eid}, true>", batch.dominant_kernel()
    batch.close()


@BATCH_FORMS
@pytest.mark.parametrize("env", P.ENVS)
def test_rpgd_batch(env, per_problem):
    """the single gradient of test_rpgd_single_gradient in every problem of ctk_g_rpgd_batch / ctk_g_rpgd_batch_pp"""
    N, H, C, eid = GRAD_N, GRAD_H, L.LIMITS[env][0].size, ENV_ID[env]
    batch = CtkRpgdBatch(B, seeds=[1, 2, 3], **rpgd_common(env, N, H, 1e9))
    batch.reset(np.random.default_rng(9).random((B, N, batch.samples_needed_reset() // (N * C), C), dtype=np.float32))

    def at(owns):
        ins = [P.grad_inputs(env, N, H, own) for own in owns]
        for q, (s, Q0, up) in enumerate(ins):
            batch.set_state(q, rpgd_state(Q0, up))
        batch.step(np.stack([s for s, _, _ in ins]), None, u_prev=np.stack([up for _, _, up in ins]))
        out = []
        for q in range(B):
            out += grad_at(lambda name: batch.read(name, q), env, "ODE", f"params rpgd batch{'_pp' if per_problem else ''} {env} problem {q}", False,
                           owns[q], N, H)
        return out

    batch_sweep(batch, env, per_problem, at)
    assert batch.dominant_kernel() == f"ctk_g_rpgd_batch{'_pp' if per_problem else ''}<{eid}>", batch.dominant_kernel()
    batch.close()


@pytest.mark.parametrize("env", P.ENVS)
def test_batch_plant_step(env):
    """ctk_batch_plant<ENV> with plant parameters of its own (set_plant_params) against PlantF64: problem 1's plant holds the case, the
    others follow their controllers (the defaults).  Every case that moves the dynamics, and ALL."""
    C = L.LIMITS[env][0].size
    lo, hi = limits(env)
    batch = CtkMppiBatch(B, seeds=[1, 2, 3], environment=env, num_rollouts=64, mpc_horizon=10, dt=P.DT, action_low=lo, action_high=hi)
    loop = batch.closed_loop
    S0 = np.stack([P.base_state(env)] * B)
    S0[2] = -S0[2]
    U = L.draws_for(env, B, 1)[:, 0, :]
    dflt = P.DEFAULTS[env]
    first = loop.plant_step(S0, U)
    for own in [c for c in P.CASES[env] if c == P.ALL[env] or P.is_dynamics(env, c[0][0])]:
        pars = P.params_with(env, own)
        for n in batch.param_names:
            loop.set_plant_params(n, [float(getattr(pars, n))], ids=[1])
            assert loop.get_plant_params(n)[1] == np.float32(getattr(pars, n))
        got = loop.plant_step(S0, U)
        for q, o in enumerate((dflt, own, dflt)):
            want = P.PlantF64(env, P.params_with(env, o)).step(S0[q:q + 1], U[q:q + 1]).numpy()[0]
            close(f"params batch plant {env} step problem {q} {P.case_id(env, own)}", "s_next", got[q], want, **TRAJ_TOL)
        loop.clear_plant_params()
    np.testing.assert_array_equal(loop.plant_step(S0, U), first)
    batch.close()


# ---- network predictors: they replace the dynamics but evaluate the cost in code of their own ---------------------------------------------
NETS = pytest.mark.parametrize("kind", ["MLP", "GRU"])


@NETS
@pytest.mark.parametrize("env", P.ENVS)
def test_network_mppi_cost_parameters(env, kind):
    """forward: CartPole's own MLP / GRU kernels, the template's split kernels on Quad2D and Hover; cost parameters and ALL"""
    N, H = P.NET_SIZE
    C = L.LIMITS[env][0].size
    e = engine("mppi", env, kind, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=1, materialize_trajectories=True)
    e.set_predictor_weights(P.net_weights(env, kind))

    def at(own):
        ref = P.net_mppi_ref(env, kind, own)
        e.set_state(np.zeros(H * C + C, np.float32))
        if kind == "GRU":
            e.predictor_set_hidden(None)
        u = np.array(e.step(ref["s"], ref["noise"], u_prev=np.zeros(C, np.float32)), np.float32).copy()
        tag = f"params mppi {kind} {env} step {P.case_id(env, own)}"
        close(tag, "J", e.read("J"), ref["J"], **J_TOL)
        close(tag, "u_nom", e.read("U_NOM"), ref["u_nom"], **U_TOL)
        close(tag, "u", u, ref["u"], **U_TOL)
        return [u, e.read("J").copy(), e.read("U_NOM").copy()]

    sweep(e, env, P.cost_cases(env), at)
    k = e.dominant_kernel()
    e.close()
    assert (k.startswith("ctk_mppi_rollout<0, ") and "ctk_g_" not in k) if env == "CartPole" else ("ctk_g_" in k and f"<{ENV_ID[env]}," in k), k


@NETS
@pytest.mark.parametrize("env", P.ENVS)
def test_network_rpgd_cost_parameters(env, kind):
    """reverse: one Adam iteration from zero moments through the network's vector-Jacobian product and the cost's gradient"""
    N, H = P.NET_SIZE
    C = L.LIMITS[env][0].size
    e = CtkEngine("rpgd", kind, **rpgd_common(env, N, H, 1e9))
    e.set_predictor_weights(P.net_weights(env, kind))
    e.reset(np.random.default_rng(3).random((N, H, C), dtype=np.float32))

    def at(own):
        s, Q0, up = P.grad_inputs(env, N, H, own)
        e.set_state(rpgd_state(Q0, up))
        if kind == "GRU":
            e.predictor_set_hidden(None)
        e.step(s, None, u_prev=up)
        return grad_at(e.read, env, kind, f"params rpgd gradient {kind} {env}", False, own, N, H)

    sweep(e, env, P.cost_cases(env), at)
    k = e.dominant_kernel()
    e.close()
    assert "rpgd" in k and (env == "CartPole" or f"<{ENV_ID[env]}," in k), k
