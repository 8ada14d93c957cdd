"""-m gpu: every analytic rollout kernel at LARGE pole / body / craft angles, against the float32 oracle fed the same draws.

Each of these kernels takes sin / cos of the angle in two ways (csrc/ctk_device.h): ctk_sincosf_fast, a two-term Cody-Waite reduction
without a range check, documented for |x| <= CTK_SINCOS_FAST_LIMIT = 32768; and, where max |angle| over the horizon was beyond that in
any lane of the wave (or workgroup), a SECOND PASS over the whole horizon with the checked ctk_sincosf, which has to start again from
the initial state, zero the cost and input-cost sums, restore u_prev, rewrite Q / TRAJ and (four-wave kernels) keep every barrier
matched.  The rest of the suite feeds |theta| <= ~3 rad: reduction quotients -2 .. 2, and no second pass outside one MLP test.

The start states are tests/large_angle_cases.py's, guarded on the CPU by tests/test_large_angles_cpu.py:
  IN_RANGE   the fast path at quotients ~ +-20 000;
  JUST_OUT   the second pass, where the fast formula would still have been right: they show that the second pass is correct;
  CROSSING   the limit is passed inside the horizon (at H - 1, at 15 and 16 = either side of the four-wave kernels' S1 split, and at the
             terminal state only), so that amax first trips at a range boundary; they pass whether or not the kernel re-runs;
  FAR_OUT    1e9 and -3e8 rad, where the fast formula is wrong by O(1).  THESE ARE THE ONLY CASES THAT FAIL WHEN A RANGE CHECK IS
             MISSING OR WITHOUT EFFECT — they are not duplicates of JUST_OUT; do not prune them.

Bounds (every comparison goes through margins.close, so the share of each bound that is used lands in the parity-margins table):
  J      rtol 3e-5 (the figure at the top of test_gpu_mppi.py) / atol 1e-3, every row: 60x what the oracle differs from its own
         float64-step form by (5.3e-7), 4 - 5 orders below a stale sum, a skipped second pass at 1e9 or a wrong quadrant;
  TRAJ   the angle column within ONE float32 spacing of the oracle's value (an rtol at 3e4 rad would mean nothing), the other columns
         rtol 1e-4 / atol 3e-5; with logging, Q at rtol 1e-6 and every row of TRAJ present, row H included;
  u, U_NOM, mu, STD, PLAN, ADAM_M   the bounds of the existing oracle test of the same kernel.
Network predictors (MLP, GRU) keep the J / TRAJ bounds of their own oracle tests (test_gpu_mlp.py, test_gpu_gru.py): tanh / sigmoid by
v_exp / v_rcp and the MFMA summation order are theirs, not the angle's.

Each test names the kernel it means to run and checks it through dominant_kernel() AFTER a step (the handle then names what ran).
Switches that the library reads once per process (CTK_MPPI_LATE_U, CTK_MPPI_NO_PAIR) run the same tests in a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkCemBatch, CtkRpgdBatch
import large_angle_cases as L
import margins
from margins import close
from test_gpu_mppi import U_TOL
from test_gpu_rpgd import assert_close_mostly

pytestmark = pytest.mark.gpu

J_TOL = dict(rtol=3e-5, atol=1e-3)
ENV_ID = {"CartPole": 0, "Quad2D": 1, "Hover": 2}
FORMS = [("CartPole", False), ("CartPole", True), ("Quad2D", False), ("Hover", False)]           # (environment, generic_kernels)
FORM_IDS = ["CartPole", "CartPole-template", "Quad2D", "Hover"]
# (N, H, period): two full tiles and a ragged population; H = 4 serves the crossings at H - 1 and at the terminal state
MPPI_CONFIGS = L.MPPI_CONFIGS


def limits(env):
    lo, hi = L.LIMITS[env]
    return (float(lo[0]), float(hi[0])) if lo.size == 1 else (lo, hi)


def set_params(e, pars, own=None):
    for n in pars.param_names():
        e.set_param(n, float(getattr(pars, n)))


def engine(opt, env, pred="ODE", **kw):
    lo, hi = limits(env)
    e = CtkEngine(opt, pred, environment=env, dt=0.02, action_low=lo, action_high=hi, **kw)
    set_params(e, L.env_params(env))
    return e


def check_traj(tag, env, got, want):
    a = L.ANGLE[env]
    assert got.shape == want.shape                                       # every row, row H included
    sp = np.spacing(np.abs(want[:, :, a]))
    close(tag, "angle/ulp", (got[:, :, a].astype(np.float64) - want[:, :, a]) / sp, np.zeros(sp.shape), atol=1.0)
    rest = [i for i in range(want.shape[2]) if i != a]
    close(tag, "traj", got[:, :, rest], want[:, :, rest], rtol=1e-4, atol=3e-5)


def check_crossing(env, N, step, traj):
    """the CROSSING cases' premise, for the inputs large_angle_cases.draws_for gives at N = 128 (other N, other inputs: elsewhere)"""
    if step is not None and N == 128:
        assert L.first_out_of_range_step(traj, L.ANGLE[env]) == step


# ---- MPPI: the four-wave kernel ctk_mppi_rollout<ENV, ODE, LOG, P2P>, its batch forms and the resident form ---------------------------
def check_mppi(tag, env, ref, u, read, materialize):
    close(tag, "J", read("J"), ref["J"], **J_TOL)
    close(tag, "u_nom", read("U_NOM"), ref["u_nom"], **U_TOL)
    close(tag, "u", u, ref["u"], **U_TOL)
    if materialize:
        close(tag, "u_run", read("Q"), ref["Q"], rtol=1e-6, atol=1e-6)
        check_traj(tag, env, read("TRAJ"), ref["traj"])


@pytest.mark.parametrize("materialize", [True, False])
@pytest.mark.parametrize("env,generic", FORMS, ids=FORM_IDS)
def test_mppi_four_wave_kernel(env, generic, materialize):
    """CTK_MPPI_LATE_U in the environment (the child process of test_mppi_late_u_order): the same cases on the late order of u"""
    C, eid = L.LIMITS[env][0].size, ENV_ID[env]
    log = "true" if materialize else "false"
    for N, H, p in MPPI_CONFIGS:
        e = engine("mppi", env, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, materialize_trajectories=materialize,
                   generic_kernels=generic)
        for name, th, om, step in L.cases(env, H):
            ref = L.mppi_ref(env, N, H, p, th, om)
            if p == 1:
                check_crossing(env, N, step, ref["traj"])
            e.set_state(np.zeros(H * C + C, np.float32))
            u = e.step(ref["s"], ref["noise"], u_prev=np.zeros(C, np.float32))
            check_mppi(f"large_angles mppi {FORM_IDS[FORMS.index((env, generic))]} log={log} step {name} N{N} H{H} p{p}", env, ref, u, e.read, materialize)
        k = e.dominant_kernel()
        e.close()
        early = eid == 0 and not materialize and not os.environ.get("CTK_MPPI_LATE_U")        # one control input, no logging: u published early
        assert k == f"ctk_mppi_rollout<{eid}, 0, {log}, false>" if (early or eid != 0 or materialize) else k.startswith(f"ctk_mppi_rollout<0, 0, {log}, false, "), k


def run_child(switch, select, tmp_path):
    """the tests of this file selected by `select`, in a child process with the once-per-process switch set; the child writes its margins
    to a table of its own, whose rows join this process's table with the switch in their name"""
    out = str(tmp_path / "margins.txt")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select],
                       env=dict(os.environ, CTK_MARGINS_OUT=out, **{switch: "1"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
    rows = [line.rsplit(None, 6) for line in open(out) if line.startswith("large_angles")]
    assert rows
    for tag, tensor, ab, rel, rtol, atol, used in rows:
        margins._rows[(f"{tag.strip()} [{switch}]", tensor)] = dict(abs=float(ab), rel=float(rel), used=float(used), rtol=float(rtol), atol=float(atol), n=1)


def test_mppi_late_u_order(tmp_path):
    """the order in which CartPole's non-logging kernel publishes u is a once-per-process switch: the late order in a child process.  (Its own
    handle only: a generic_kernels handle names its kernel without the form, so there the order cannot be confirmed by name.)"""
    run_child("CTK_MPPI_LATE_U", "test_mppi_four_wave_kernel and CartPole and False and not template", tmp_path)


@pytest.mark.parametrize("env", L.ENVS)
def test_mppi_resident_form(env):
    import torch
    C, N, H, p = L.LIMITS[env][0].size, 128, 20, 1
    e = engine("mppi", env, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    e.resident_enable(True, idle_us=100000.0)
    for name, th, om, step in L.cases(env, H):
        ref = L.mppi_ref(env, N, H, p, th, om)
        e.set_state(np.zeros(H * C + C, np.float32))
        buf = torch.from_numpy(ref["noise"]).to("cuda")
        torch.cuda.synchronize()
        u = e.step(ref["s"], buf.data_ptr(), u_prev=np.zeros(C, np.float32))
        assert e.dominant_kernel().startswith(f"ctk_mppi_resident<{ENV_ID[env]}, "), e.dominant_kernel()     # (before the reads: they end it)
        check_mppi(f"large_angles mppi resident {env} step {name}", env, ref, u, e.read, False)
    e.close()


BATCH_OWN = {"CartPole": ("target_position", [0.0, 0.05, -0.04, 0.08]), "Quad2D": ("target_x", [0.1, 0.3, -0.2, 0.25]),
             "Hover": ("target_x", [0.2, -0.1, 0.35, 0.05])}


def mixed_states(B=4):
    """problems 0 and 2 in range, 1 just out, 3 (B = 4) far out: one launch holds workgroups that redo next to workgroups that do not"""
    return [L.IN_RANGE[0], L.JUST_OUT[0], L.IN_RANGE[1], L.FAR_OUT[0]][:B] if B == 4 else [L.IN_RANGE[0], L.JUST_OUT[2], L.FAR_OUT[1]]


@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per-problem"])
@pytest.mark.parametrize("env", L.ENVS)
def test_mppi_batch_mixed_problems(env, per_problem):
    B, C, eid = 4, L.LIMITS[env][0].size, ENV_ID[env]
    lo, hi = limits(env)
    pname, pvals = BATCH_OWN[env]
    for N, H, p in [(128, 20, 1), (100, 20, 5)]:
        common = dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, action_low=lo, action_high=hi,
                      materialize_trajectories=True)
        batch = CtkMppiBatch(B, seeds=[1, 2, 3, 4], **common)
        handles = [CtkEngine("mppi", "ODE", seed=1 + q, **common) for q in range(B)]
        for x in [batch] + handles:
            set_params(x, L.env_params(env))
        own = [((pname, pvals[q]),) if per_problem else () for q in range(B)]
        if per_problem:
            batch.set_problem_params(pname, pvals)
            for q in range(B):
                handles[q].set_param(pname, pvals[q])
        refs = [L.mppi_ref(env, N, H, p, th, om, own[q]) for q, (th, om) in enumerate(mixed_states())]
        for q in range(B):
            batch.set_state(q, np.zeros(H * C + C, np.float32))
            handles[q].set_state(np.zeros(H * C + C, np.float32))
        S = np.stack([r["s"] for r in refs])
        u = batch.step(S, np.stack([r["noise"] for r in refs]), u_prev=np.zeros((B, C), np.float32))
        assert batch.dominant_kernel() == f"ctk_mppi_batch{'_pp' if per_problem else ''}<{eid}, true>", batch.dominant_kernel()
        for q in range(B):
            tag = f"large_angles mppi batch{'_pp' if per_problem else ''} {env} step problem {q} N{N} p{p}"
            check_mppi(tag, env, refs[q], u[q], lambda name: batch.read(name, q), True)
            uh = handles[q].step(refs[q]["s"], refs[q]["noise"], u_prev=np.zeros(C, np.float32))
            np.testing.assert_array_equal(u[q], uh)
            for name in ("J", "U_NOM", "Q", "TRAJ"):
                np.testing.assert_array_equal(batch.read(name, q), handles[q].read(name), err_msg=f"{name} of problem {q}")
        batch.close()
        for h in handles:
            h.close()


# ---- MPPI: the throughput kernels (N >= 32768) ----------------------------------------------------------------------------------------
TP_N, TP_H = L.TP_N, L.TP_H
TP_STATES = L.TP_STATES


@pytest.mark.parametrize("isteps", [1, 2])
@pytest.mark.parametrize("kernel,p,generic", [("ctk_mppi_rollout_tps<", 1, False), ("ctk_mppi_rollout_tp<", 2, False), ("ctk_g_rollout", 1, True)],
                         ids=["streaming", "whole-tile", "template"])
def test_mppi_throughput_kernels(kernel, p, generic, isteps):
    """the smallest N that selects them, H = 6 as in test_mppi_throughput_variants_match_oracle: the streaming kernel (period 1, draws in a
    buffer; its second pass re-reads the draws from global memory and rebuilds the four input sums another way), the whole-tile kernel
    (P < H) and the template's one-wave kernel; intermediate_steps = 2 always takes the checked recurrence (true of CartPole, the only
    environment these kernels are run for here: Quad2D and Hover keep their sub-step loop inside the fast path, test_gpu_substeps.py)"""
    env = "CartPole"
    engines = [engine("mppi", env, num_rollouts=TP_N, mpc_horizon=TP_H, period_interpolation_inducing_points=p, intermediate_steps=isteps,
                      materialize_trajectories=log, generic_kernels=generic) for log in (True, False)]
    for th, om in TP_STATES:
        ref = L.mppi_ref(env, TP_N, TP_H, p, th, om, (), isteps)
        for e, log in zip(engines, (True, False)):
            e.set_state(np.zeros(TP_H + 1, np.float32))
            u = e.step(ref["s"], ref["noise"], u_prev=np.zeros(1, np.float32))
            check_mppi(f"large_angles mppi {kernel.rstrip('<')} isteps={isteps} log={log} step theta0 {th}", env, ref, u, e.read, log)
    for e in engines:
        assert kernel in e.dominant_kernel(), e.dominant_kernel()
        e.close()


# ---- CEM: the one-launch step, the launch per phase, the batch forms ------------------------------------------------------------------
CEM_K, CEM_ITS = L.CEM_K, L.CEM_ITS
CEM_TOL = dict(rtol=1e-4, atol=1e-5)          # test_gpu_cem_random.py::test_cem_matches_oracle: mu / STD


def check_cem(tag, env, ref, u, read):
    close(tag, "J", read("J"), ref["J"], **J_TOL)
    close(tag, "Q", read("Q"), ref["Q"], rtol=1e-5, atol=2e-6)
    close(tag, "mu", read("U_NOM"), ref["mu"], **CEM_TOL)
    close(tag, "std", read("STD"), ref["std"], **CEM_TOL)
    close(tag, "u", u, ref["u"], rtol=1e-5, atol=2e-6)
    check_traj(tag, env, read("TRAJ"), ref["traj"])


@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "launch-per-phase"])
@pytest.mark.parametrize("env", L.ENVS)
def test_cem_kernels(env, fused, monkeypatch):
    C, eid = L.LIMITS[env][0].size, ENV_ID[env]
    for N, H in L.CEM_SIZES:
        if not fused:
            monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")           # read when the handle is created
        e = engine("cem", env, num_rollouts=N, mpc_horizon=H, cem_outer_it=CEM_ITS, cem_best_k=CEM_K, materialize_trajectories=True)
        monkeypatch.delenv("CTK_NO_CEM_FUSED", raising=False)
        for name, th, om, step in L.cases(env, H):
            ref = L.cem_ref(env, N, H, th, om)
            e.reset()
            u = e.step(ref["s"], ref["noise"], u_prev=np.zeros(C, np.float32))
            check_cem(f"large_angles cem {'fused' if fused else 'phases'} {env} step {name} N{N} H{H}", env, ref, u, e.read)
        k = e.dominant_kernel()
        e.close()
        assert k == f"ctk_cem_fused<{eid}, true>" if fused else k.startswith(f"ctk_affine_rollout<{eid},"), k


@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per-problem"])
@pytest.mark.parametrize("env", L.ENVS)
def test_cem_batch_mixed_problems(env, per_problem):
    """a problem whose workgroups redo the horizon must not disturb the problems that wait beside it in the launch's hand-offs"""
    B, C, eid, N, H = 4, L.LIMITS[env][0].size, ENV_ID[env], 128, 20
    lo, hi = limits(env)
    pname, pvals = BATCH_OWN[env]
    common = dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, action_low=lo, action_high=hi, materialize_trajectories=True,
                  cem_outer_it=CEM_ITS, cem_best_k=CEM_K, cem_initial_action_stdev=0.5, cem_stdev_min=0.01)
    batch = CtkCemBatch(B, seeds=[1, 2, 3, 4], **common)
    handles = [CtkEngine("cem", "ODE", seed=1 + q, **common) for q in range(B)]
    for x in [batch] + handles:
        set_params(x, L.env_params(env))
    own = [((pname, pvals[q]),) if per_problem else () for q in range(B)]
    if per_problem:
        batch.set_problem_params(pname, pvals)
        for q in range(B):
            handles[q].set_param(pname, pvals[q])
    refs = [L.cem_ref(env, N, H, th, om, own[q]) for q, (th, om) in enumerate(mixed_states())]
    u = batch.step(np.stack([r["s"] for r in refs]), np.stack([r["noise"] for r in refs]), u_prev=np.zeros((B, C), np.float32))
    assert batch.dominant_kernel() == f"ctk_cem_batch{'_pp' if per_problem else ''}<{eid}, true>", batch.dominant_kernel()
    for q in range(B):
        check_cem(f"large_angles cem batch{'_pp' if per_problem else ''} {env} step problem {q}", env, refs[q], u[q], lambda name: batch.read(name, q))
        uh = handles[q].step(refs[q]["s"], refs[q]["noise"], u_prev=np.zeros(C, np.float32))
        np.testing.assert_array_equal(u[q], uh)
        for name in ("J", "U_NOM", "STD", "Q", "TRAJ"):
            got = batch.read(name, q)
            np.testing.assert_array_equal(got, handles[q].read(name).reshape(got.shape), err_msg=f"{name} of problem {q}")
    batch.close()
    for h in handles:
        h.close()


# ---- random action, plain rollout(), CEM-GMM's in-rollout sampling ---------------------------------------------------------------------
@pytest.mark.parametrize("env", L.ENVS)
def test_random_action_and_plain_rollout(env):
    pars = L.env_params(env)
    lo, hi = L.LIMITS[env]
    C, eid = lo.size, ENV_ID[env]
    pred, cost = O.Predictor("ODE", dt=0.02, env=pars), O.Cost(pars)
    for N, H in [(128, 20), (100, 20), (128, 4)]:
        e = engine("random_action", env, num_rollouts=N, mpc_horizon=H, materialize_trajectories=True)
        Q = L.draws_for(env, N, H)                                        # rollout(): the crossings lie where CROSSING says
        u01 = np.random.default_rng(N + H).random((N, H, C), dtype=np.float32)
        up = np.full(C, 0.1, np.float32)
        for name, th, om, step in L.cases(env, H):
            s = L.base_state(env, th, om)
            tag = f"large_angles rollout {env} step {name} N{N} H{H}"
            traj, J = e.rollout(s, Q, u_prev=up)
            want = pred.predict_core(np.tile(s, (N, 1)), Q)
            check_crossing(env, N, step, want)
            close(tag, "J", J, cost.get_trajectory_cost(want, Q, up), **J_TOL)
            check_traj(tag, env, traj, want)
            o = O.RandomAction(pred, cost, lo, hi, num_rollouts=N, mpc_horizon=H)
            uo = np.asarray(o.step(s, u01), np.float32).reshape(-1)
            ug = e.step(s, u01, u_prev=np.zeros(C, np.float32))
            tag = f"large_angles random_action {env} step {name} N{N} H{H}"
            close(tag, "Q", e.read("Q"), o.Q, rtol=1e-6, atol=1e-7)
            close(tag, "J", e.read("J"), o.J, **J_TOL)
            check_traj(tag, env, e.read("TRAJ"), o.rollout_trajectories)
            assert int(e.read("BEST_IDX")[0]) == int(o.best_idx)
            close(tag, "u", ug, uo, rtol=1e-6, atol=1e-7)              # test_quad2d_cem_and_random_match_oracle
        assert e.dominant_kernel() == f"ctk_affine_rollout<{eid}, 0, true>", e.dominant_kernel()
        e.close()


@pytest.mark.parametrize("env", ["CartPole", "Quad2D"])
def test_cem_gmm_in_rollout_sampling(env):
    """ctk_affine_rollout_mix against tests/gmm_oracle.py: one outer iteration from the initial mixture, so that the plans and their costs
    do not depend on cluster labels (near-ties of labels are test_gpu_cem_gmm.py's subject, not the angle's)"""
    from gmm_oracle import CEMGMM, pack_draws
    pars = L.env_params(env)
    lo, hi = L.LIMITS[env]
    N, H, K = 128, 20, 16
    e = engine("cem_gmm", env, num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=K, cem_initial_action_stdev=0.5, cem_stdev_min=0.01,
               materialize_trajectories=True)
    rng = np.random.default_rng(5)
    normals, uniforms = rng.standard_normal((1, N, H, lo.size)).astype(np.float32), rng.random((1, N), dtype=np.float32)
    for name, th, om, step in L.cases(env, H):
        o = CEMGMM(O.Predictor("ODE", dt=0.02, env=pars), O.Cost(pars), *limits(env), num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=K)
        s = L.base_state(env, th, om)
        uo = o.step(s, normals, uniforms)
        e.reset()
        ug = e.step(s, pack_draws(normals, uniforms), u_prev=np.zeros(lo.size, np.float32))
        tag = f"large_angles cem_gmm {env} step {name}"
        close(tag, "Q", e.read("Q"), o.Q, rtol=1e-5, atol=2e-6)
        close(tag, "J", e.read("J"), o.J, **J_TOL)
        close(tag, "u", ug, np.asarray(uo).reshape(-1), rtol=1e-5, atol=2e-6)
    assert e.dominant_kernel() == f"ctk_affine_rollout_mix<{ENV_ID[env]}, true>", e.dominant_kernel()
    e.close()


# ---- RPGD: CartPole's own kernels, the template, the batch ------------------------------------------------------------------------------
def rpgd_engine(env, generic, N, H, p, its, K, cls=None, **kw):
    lo, hi = limits(env)
    common = dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, outer_its=its, resamp_per=1000,
                  shift_previous=1, opt_keep_k=K, sampling_distribution=0, sample_whole_control_space=1, learning_rate=0.05, adam_beta_1=0.9,
                  adam_beta_2=0.999, adam_epsilon=1e-8, action_low=lo, action_high=hi, **kw)
    e = CtkEngine("rpgd", "ODE", generic_kernels=generic, **common) if cls is None else cls(**common)
    set_params(e, L.env_params(env))
    return e


def rpgd_kernel_ok(name, env, generic):
    return name == f"ctk_g_rpgd_descent<{ENV_ID[env]}>" if (generic or env != "CartPole") else ("ctk_g_" not in name and "rpgd" in name)


@pytest.mark.parametrize("env,generic", FORMS, ids=FORM_IDS)
def test_rpgd_single_gradient(env, generic):
    """one Adam iteration from zero moments: m = (1 - beta1) * dJ/dQ, as test_quad2d_single_gradient_matches_oracle_adjoint builds it
    and at its bounds — the forward tape and the adjoint take ctk_sincosf (and beyond 32768 its branch to the library's Payne-Hanek
    path) at an in-range, a just-out and a far-out state"""
    pars = L.env_params(env)
    pred, cost = O.Predictor("ODE", dt=0.02, env=pars), O.Cost(pars)
    N, H, C = 64, 20, L.LIMITS[env][0].size
    e = rpgd_engine(env, generic, N, H, 1, 1, 16, gradmax_clip=1e9)
    e.reset(np.random.default_rng(3).random((N, H, C), dtype=np.float32))
    Q0 = e.read("PLAN")
    up = np.full(C, 0.05, np.float32)
    for th, om in L.GRAD_CASES:
        s = L.base_state(env, th, om)
        e.set_state(np.concatenate([Q0.ravel(), np.zeros(2 * N * H * C + N, np.float32), up, [0], [1]]).astype(np.float32))   # count 1: no resampling
        e.step(s, None, u_prev=up)
        J, _, g = O.rollout_cost_and_grad(pred, cost, np.tile(s, (N, 1)), Q0, up)
        tag = f"large_angles rpgd gradient {FORM_IDS[FORMS.index((env, generic))]} step theta0 {th}"
        m = e.read("ADAM_M")            # after the warm start: shifted by one step, tail zero-filled
        close(tag, "adam_m", m[:, :-1, :], 0.1 * g[:, 1:, :], rtol=2e-3, atol=2e-4 * float(np.abs(g).max()))
        assert np.all(m[:, -1, :] == 0.0)
    assert rpgd_kernel_ok(e.dominant_kernel(), env, generic), e.dominant_kernel()
    e.close()


def rpgd_state(o):
    m, v = (np.zeros_like(o.Q), np.zeros_like(o.Q)) if o.opt.m is None else (o.opt.m, o.opt.v)
    return np.concatenate([o.Q.ravel(), m.ravel(), v.ravel(), o.trajectory_ages.ravel(), np.asarray(o.u, np.float32).reshape(-1),
                           [o.opt.step_count], [o.count]]).astype(np.float32)


def rpgd_oracle(env, N, H, p, its, pars=None):
    pars = L.env_params(env) if pars is None else pars
    lo, hi = L.LIMITS[env]
    return O.RPGD(O.Predictor("ODE", dt=0.02, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, outer_its=its, resamp_per=1000,
                  period_interpolation_inducing_points=p, SAMPLING_DISTRIBUTION="uniform", shift_previous=1, learning_rate=0.05,
                  opt_keep_k_ratio=0.25, gradmax_clip=5.0)


def check_rpgd_descent(tag, env, o, s, read, u, tuned_cartpole):
    """after one step of `its` Adam iterations.  J is held to the file's bound through the device's OWN refined plans (the buffer Q: the
    population the cost pass ran on, before the warm start): the oracle's cost of those plans — the cost pass, with its NaN-signalled re-run,
    alone; then J, PLAN, ADAM_M and u against the oracle's descent at the bounds of the kernel's own oracle test"""
    pars = o.cost.env
    Qd = read("Q")
    traj = o.predictor.predict_core(np.tile(s, (o.N, 1)), Qd)
    close(tag, "J_own_Q", read("J"), o.cost.get_trajectory_cost(traj, Qd, np.zeros(o.C, np.float32)), **J_TOL)
    if tuned_cartpole:       # test_rpgd_ode_matches_oracle
        close(tag, "J", read("J"), o.J, rtol=2e-3, atol=1e-2)
        close(tag, "plan", read("PLAN"), o.Q, rtol=1e-3, atol=2e-3)
        close(tag, "u", u, np.asarray(o.u, np.float32).reshape(-1), rtol=1e-3, atol=2e-3)
    else:                    # test_quad2d_rpgd_matches_oracle (short descents)
        tol = dict(rtol=2e-5, atol=2e-5)
        close(tag, "J", read("J"), o.J, rtol=2e-3, atol=1e-3)
        assert_close_mostly(read("PLAN"), o.Q, max_outliers=max(4, o.Q.size // 400), **tol)
        assert_close_mostly(read("ADAM_M"), o.opt.m, max_outliers=max(4, o.Q.size // 400), **tol)
        close(tag, "u", u, np.asarray(o.u, np.float32).reshape(-1), **tol)
    np.testing.assert_array_equal(read("AGES"), o.trajectory_ages)


@pytest.mark.parametrize("env,generic", FORMS, ids=FORM_IDS)
def test_rpgd_three_iteration_descent(env, generic):
    N, H, p, its, C = 64, 20, 5, 3, L.LIMITS[env][0].size
    e = rpgd_engine(env, generic, N, H, p, its, 16, gradmax_clip=5.0)
    for th, om in L.GRAD_CASES:
        o = rpgd_oracle(env, N, H, p, its)
        d0 = np.random.default_rng(7).random((N, o.P, C), dtype=np.float32)
        o.optimizer_reset(d0)
        o.count = 1                                   # no resampling in this step (resamp_per 1000, count 1)
        e.reset(d0)
        e.set_state(rpgd_state(o))
        s = L.base_state(env, th, om)
        o.step(s, None)
        u = e.step(s, None, u_prev=np.zeros(C, np.float32))
        check_rpgd_descent(f"large_angles rpgd descent {FORM_IDS[FORMS.index((env, generic))]} step theta0 {th}", env, o, s, e.read, u,
                           env == "CartPole" and not generic)
    assert rpgd_kernel_ok(e.dominant_kernel(), env, generic), e.dominant_kernel()
    e.close()


@pytest.mark.parametrize("env", L.ENVS)
def test_rpgd_batch_mixed_problems(env):
    B, N, H, p, its, C = 3, 64, 20, 5, 3, L.LIMITS[env][0].size
    batch = rpgd_engine(env, True, N, H, p, its, 16, cls=functools.partial(CtkRpgdBatch, B, seeds=[1, 2, 3]), gradmax_clip=5.0)
    handles = [rpgd_engine(env, True, N, H, p, its, 16, gradmax_clip=5.0, seed=1 + q) for q in range(B)]
    states = [L.base_state(env, th, om) for th, om in mixed_states(3)]
    orc = []
    d0 = np.random.default_rng(9).random((B, N, batch.samples_needed_reset() // (N * C), C), dtype=np.float32)
    batch.reset(d0)
    for q in range(B):
        o = rpgd_oracle(env, N, H, p, its)
        o.optimizer_reset(d0[q])
        o.count = 1
        handles[q].reset(d0[q])
        handles[q].set_state(rpgd_state(o))
        batch.set_state(q, rpgd_state(o))
        o.step(states[q], None)
        orc.append(o)
    u = batch.step(np.stack(states), None, u_prev=np.zeros((B, C), np.float32))
    assert batch.dominant_kernel() == f"ctk_g_rpgd_batch<{ENV_ID[env]}>", batch.dominant_kernel()
    for q in range(B):
        check_rpgd_descent(f"large_angles rpgd batch {env} step problem {q}", env, orc[q], states[q], lambda name: batch.read(name, q), u[q], False)
        uh = handles[q].step(states[q], None, u_prev=np.zeros(C, np.float32))
        np.testing.assert_array_equal(u[q], uh)
        for name in ("Q", "J", "PLAN", "ADAM_M", "ADAM_V", "AGES"):
            got = batch.read(name, q)
            np.testing.assert_array_equal(got, handles[q].read(name).reshape(got.shape), err_msg=f"{name} of problem {q}")
    batch.close()
    for h in handles:
        h.close()


# ---- network predictors: the cost's cos of the predicted angle (ctk_mlp.h, ctk_gru.h) --------------------------------------------------
@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("theta0", [40000.25, L.FAR_OUT[0][0]], ids=["just-out", "far-out"])
def test_mppi_mlp_large_angle(theta0, materialize):
    """the pair form (two waves per tile: every wave of the workgroup takes the checked pass together) and, with CTK_MPPI_NO_PAIR in the
    environment (the child process of test_mppi_mlp_one_wave_form), the one-wave form (ctk_mlp.h: rollout_mlp); the initial angle itself is
    out of range, so every trajectory sees it.  J / TRAJ / u at the bounds of test_mppi_mlp_matches_oracle."""
    pars = O.EnvParams(terminal_weight=0.25)
    w = O.mlp_default_weights(1)
    pred = O.Predictor("MLP", dt=0.02, env=pars, weights=w)
    N, H, p = 96, 9, 3
    o = O.MPPI(pred, O.Cost(pars), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    e = CtkEngine("mppi", "MLP", num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=materialize)
    set_params(e, pars)
    e.set_predictor_weights(w)
    s = np.array([0.1, -0.2, theta0, 0.7], np.float32)
    noise = np.random.default_rng(3).standard_normal((N, o.P, 1)).astype(np.float32)
    uo, ug = o.step(s, noise), e.step(s, noise)
    one_wave = bool(os.environ.get("CTK_MPPI_NO_PAIR"))
    tag = f"large_angles mppi mlp {'one-wave' if one_wave else 'pair'} log={materialize} step theta0 {theta0}"
    assert np.isfinite(o.J).all()
    close(tag, "J", e.read("J"), o.J, rtol=5e-5, atol=1e-3)
    close(tag, "u_nom", e.read("U_NOM"), o.u_nom, **U_TOL)
    close(tag, "u", ug[0], uo, **U_TOL)
    if materialize:
        close(tag, "traj", e.read("TRAJ"), o.rollout_trajectories, rtol=1e-4, atol=3e-5)
    assert e.dominant_kernel() == f"ctk_mppi_rollout<0, {1 if one_wave else 3}, {'true' if materialize else 'false'}, false>", e.dominant_kernel()
    e.close()


def test_mppi_mlp_one_wave_form(tmp_path):
    run_child("CTK_MPPI_NO_PAIR", "test_mppi_mlp_large_angle", tmp_path)


@pytest.mark.parametrize("way", ["flag-set", "cleared-by-state", "cleared-by-bound"])
def test_mppi_gru_fast_cos_flag(way):
    """CartPole's GRU kernel (ctk_gru.h) takes the unchecked cos where the host can bound every angle the cost will see
    (ctk_api.hip: fast_cos_ok): |s[2]| <= 32768 AND max_g (sum_j |Wo[g, j]| + |bo[g]|) <= 32768.  Default weights and a small angle set
    the flag; theta0 = 40000.25 clears it by the state; an output bias of 40000 on the cart-velocity row (which no cost term reads and
    whose value the bounds below still resolve: scaling all of Wo that far would put 6e-3 of absolute rounding on every predicted
    state) clears it by the bound, with every angle small.  All three at test_gpu_gru.py's bounds."""
    pars = O.EnvParams(terminal_weight=0.25)
    w = O.gru_default_weights(1).copy()
    if way == "cleared-by-bound":
        w[w.size - 4 + 1] = 40000.0                # bo[1]
    pred = O.Predictor("GRU", dt=0.02, env=pars, weights=w)
    N, H, p = 128, 20, 5
    o = O.MPPI(pred, O.Cost(pars), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    e = CtkEngine("mppi", "GRU", num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=True)
    set_params(e, pars)
    e.set_predictor_weights(w)
    s = np.array([0.1, -0.2, 40000.25 if way == "cleared-by-state" else 2.5, 0.7], np.float32)
    noise = np.random.default_rng(4).standard_normal((N, o.P, 1)).astype(np.float32)
    uo, ug = o.step(s, noise), e.step(s, noise)
    tag = f"large_angles mppi gru step {way}"
    close(tag, "traj", e.read("TRAJ"), o.rollout_trajectories, rtol=2e-4, atol=5e-5)
    close(tag, "J", e.read("J"), o.J, rtol=1e-4, atol=2e-3)
    close(tag, "u_nom", e.read("U_NOM"), o.u_nom, **U_TOL)
    close(tag, "u", ug[0], uo, **U_TOL)
    assert e.dominant_kernel() == "ctk_mppi_rollout<0, 2, true, false>", e.dominant_kernel()
    e.close()
