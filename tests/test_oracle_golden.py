"""CPU tests: the oracle (oracle/ctk_oracle.py) against the golden fixtures recorded from the
unmodified reference (tests/golden/make_golden.py).  This is what pins the oracle."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from helpers import (cem_oracle_from, random_oracle_from, cem_naive_grad_oracle_from, cut_is_separated, CEM_CASES, RANDOM_CASES,
                     CEM_NAIVE_GRAD_CASES)
from helpers import load, env_from, mppi_oracle_from, rpgd_oracle_from, MPPI_CASES, RPGD_CASES, MPPI_QUAD_CASES, RPGD_QUAD_CASES, MPPI_HOVER_CASES, RPGD_HOVER_CASES


def test_interpolator_matches_reference():
    d = load("interpolator.npz")
    keys = sorted(k[:-2] for k in d.files if k.endswith("_y"))
    assert len(keys) == 18
    for k in keys:
        H, p, C = (int(t[1:]) for t in k.split("_"))
        M = O.interpolation_matrix(H, p, C)
        np.testing.assert_array_equal(M, d[k + "_mat"])          # bit-exact matrix (Interpolator.py:53-77)
        out = O.interpolate(d[k + "_y"], M)
        np.testing.assert_allclose(out, d[k + "_out"], rtol=1e-6, atol=1e-6)
        assert O.num_inducing_points(H, p) == d[k + "_y"].shape[1]


def test_interpolation_table_is_the_matrix():
    for (H, p) in [(10, 1), (50, 10), (41, 10), (5, 10), (12, 3), (100, 10), (1, 1), (2, 5)]:
        M = O.interpolation_matrix(H, p, 1)[:, :, 0]
        i0, w0, w1 = O.interpolation_table(H, p)
        P = M.shape[0]
        R = np.zeros_like(M)
        for t in range(H):
            R[i0[t], t] += w0[t]
            if P > 1:
                R[i0[t] + 1, t] += w1[t]
        np.testing.assert_array_equal(R, M)


def test_interpolator_properties():
    # period 1 is the identity; period >= H is a straight line between 2 points
    y = np.random.default_rng(0).standard_normal((3, 9, 1)).astype(np.float32)
    np.testing.assert_array_equal(O.interpolate(y, O.interpolation_matrix(9, 1, 1)), y)
    M = O.interpolation_matrix(5, 10, 1)
    assert M.shape[0] == 2
    y2 = np.array([[[0.0], [10.0]]], np.float32)
    np.testing.assert_allclose(O.interpolate(y2, M)[0, :, 0], [0, 1, 2, 3, 4], rtol=1e-6)
    # the reference quirk: when (H-1) % p == 0 the closing step gets weight 1/p
    Mq = O.interpolation_matrix(41, 10, 1)
    assert Mq[-1, -1, 0] == np.float32(0.1)


def test_cost_aggregation_matches_reference():
    d = load("cost_aggregation.npz")
    J = O.aggregate_trajectory_cost(d["stage"], d["terminal"])
    np.testing.assert_allclose(J, d["J"], rtol=1e-6, atol=1e-4)
    # divides by H+1 (Cost_Functions/__init__.py:92)
    H = d["stage"].shape[1]
    np.testing.assert_allclose(J, (d["stage"].sum(1) + d["terminal"]) / (H + 1), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(d["stage"].sum(1), d["J_summed"], rtol=1e-5, atol=1e-3)
    cost = O.Cost(env_from(d), float(d["dt"]))
    Jfull = cost.get_trajectory_cost(d["traj"], d["inputs"], np.array([d["u_prev"]], np.float32))
    np.testing.assert_allclose(Jfull, d["J_full"], rtol=2e-6)


@pytest.mark.parametrize("case", MPPI_CASES)
def test_mppi_matches_reference(case):
    d = load(f"mppi_{case}.npz")
    o = mppi_oracle_from(d)
    np.testing.assert_array_equal(o.u_nom, d["u_nom_init"])
    for t in range(int(d["steps"])):
        assert np.float32(o.u) == d[f"u_prev_{t}"]
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.u_run, d[f"u_run_{t}"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(u, d[f"u_{t}"][0], rtol=1e-5, atol=2e-6)
        if f"traj_{t}" in d.files:
            np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        # the recorded closed loop continues from the reference's own state
        o.u_nom = d[f"u_nom_{t}"].copy(); o.u = np.float32(d[f"u_{t}"][0])


def test_mppi_properties():
    d = load("mppi_tiny_ode.npz")
    o = mppi_oracle_from(d)
    J = np.array([3.0, 1.0, 2.0, 1.5], np.float32)
    du = np.random.default_rng(0).standard_normal((4, o.H, 1)).astype(np.float32)
    b0 = o.reward_weighted_average(J, du)
    b1 = o.reward_weighted_average(J + np.float32(1000.0), du)      # shift invariance (optimizer_mppi.py:164-167)
    np.testing.assert_allclose(b0, b1, rtol=1e-5, atol=1e-6)
    o.LBD = 1e-6                                                     # LBD -> 0: arg-min perturbation
    np.testing.assert_allclose(o.reward_weighted_average(J, du), du[1], rtol=1e-6)
    # shard merge reproduces the global weighting
    o = mppi_oracle_from(d)
    J = np.random.default_rng(1).uniform(0, 500, 64).astype(np.float32)
    du = np.random.default_rng(2).standard_normal((64, o.H, 1)).astype(np.float32)
    parts = [o.mppi_partials(J[i:i + 16], du[i:i + 16]) for i in range(0, 64, 16)]
    _, _, b = O.merge_mppi_partials([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], o.LBD)
    np.testing.assert_allclose(b, o.reward_weighted_average(J, du), rtol=2e-5, atol=1e-6)


def test_adam_matches_reference():
    d = load("adam.npz")
    a = O.Adam(0.05, 0.9, 0.999, 1e-8)
    var = d["var0"]
    for t in range(3):
        var = a.apply(d[f"grad_{t}"], var)
        np.testing.assert_allclose(var, d[f"var_{t}"], rtol=1e-6, atol=1e-7)
    assert a.step_count == int(d["step"])
    np.testing.assert_allclose(a.m, d["m"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(a.v, d["v"], rtol=1e-6, atol=1e-10)


@pytest.mark.parametrize("case", RPGD_CASES)
def test_rpgd_matches_reference(case):
    d = load(f"rpgd_{case}.npz")
    o = rpgd_oracle_from(d)
    o.optimizer_reset(d["reset_draws"])
    np.testing.assert_allclose(o.Q, d["Q_init"], rtol=1e-6, atol=1e-7)
    many_its = int(d["outer_its"]) >= 20
    for t in range(int(d["steps"])):
        assert np.float32(o.u) == d[f"u_prev_{t}"]
        key = f"resample_draws_{t}"
        u = o.step(d[f"s_{t}"], d[key] if key in d.files else None)
        assert (key in d.files) == ((o.count - 1) % o.resamp_per == 0)
        # SURVEY 8c tolerance: rtol 1e-3 on Q after 20 Adam iterations (error compounds through
        # m_hat/(sqrt(v_hat)+eps)); tighter for short runs
        tol = dict(rtol=1e-3, atol=2e-3) if many_its else dict(rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], **tol)
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], **tol)
        np.testing.assert_allclose(o.opt.m, d[f"m_{t}"], rtol=tol["rtol"], atol=tol["atol"])
        np.testing.assert_allclose(o.opt.v, d[f"v_{t}"], rtol=tol["rtol"], atol=tol["atol"])
        np.testing.assert_array_equal(o.trajectory_ages, d[f"ages_{t}"])
        # what the reference logs (optimizer_rpgd.py:428-433): the descended population, get_action's costs and trajectories
        np.testing.assert_allclose(o.Q_before_warmstart, d[f"Q_logged_{t}"], **tol)
        np.testing.assert_allclose(o.J, d[f"J_logged_{t}"], rtol=1e-3 if many_its else 2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_logged_{t}"], rtol=2e-3 if many_its else 1e-4, atol=1e-2 if many_its else 1e-5)   # (20 Adam iterations: plans to 2e-3, integrated over the horizon)
        # :382-386: summed stage cost of the best plan = get_summed_stage_cost (no terminal term, Cost_Functions/__init__.py:71-72)
        tr = o.predictor.predict_core(d[f"s_{t}"].reshape(1, -1), d[f"u_nom_{t}"])
        np.testing.assert_allclose(tr, d[f"optimal_trajectory_{t}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o.cost.get_summed_stage_cost(tr, d[f"u_nom_{t}"], np.asarray(d[f"u_prev_{t}"], np.float32).reshape(-1)),
                                   d[f"summed_stage_cost_{t}"], rtol=2e-5)
        assert o.opt.step_count == int(d[f"adam_step_{t}"])
        np.testing.assert_allclose(u, d[f"u_{t}"][0], **tol)
        # continue from the reference's own state so steps are pinned one at a time
        o.Q = d[f"Q_{t}"].copy(); o.opt.m = d[f"m_{t}"].copy(); o.opt.v = d[f"v_{t}"].copy()
        o.u = np.float32(d[f"u_{t}"][0])


def test_rpgd_keepers_are_last_k_sorted():
    # keepers occupy the last k rows sorted by ascending cost (optimizer_rpgd.py:454-455)
    d = load("rpgd_ode_small.npz")
    o = rpgd_oracle_from(d)
    o.optimizer_reset(d["reset_draws"])
    Qb = None
    o.step(d["s_0"], d["resample_draws_0"])
    k = o.k
    best = o.best_idx
    sp = o.shift_previous
    Qb = o.Q_before_warmstart
    shifted = np.concatenate([Qb[:, sp:], np.tile(Qb[:, -1:], (1, sp, 1))], 1)
    np.testing.assert_array_equal(o.Q[-k:], shifted[best])
    assert np.all(np.diff(o.J[best]) >= 0)
    assert np.all(o.trajectory_ages[:-k] == 1.0)


@pytest.mark.parametrize("case", CEM_CASES)
def test_cem_matches_reference(case):
    """optimizer_cem_tf.py:54-117 as the unmodified module computed it (tests/golden/make_golden.py: record_tf_only_optimizers)"""
    d = load(f"cem_{case}.npz")
    o = cem_oracle_from(d)
    np.testing.assert_array_equal(o.dist_mue, d["dist_mue_init"])
    np.testing.assert_array_equal(o.stdev, d["stdev_init"])
    K = int(d["cem_best_k"])
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(np.broadcast_to(np.asarray(o.u, np.float32).reshape(-1), d[f"u_prev_{t}"].shape), d[f"u_prev_{t}"])
        noise = d[f"noise_{t}"]
        assert noise.shape[0] == o.iterations()           # warm-up switch (:92): the reference drew this many populations
        u = o.step(d[f"s_{t}"], noise)
        # Q of the LAST iteration = mu + noise * std of the iteration before: it matching to 2e-6 says every earlier refit matched
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=1e-6, atol=2e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-6)
        if f"traj_{t}" in d.files:
            np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        ref_best = np.argsort(d[f"J_{t}"], kind="stable")[:K]
        assert set(o.best_idx.tolist()) == set(ref_best.tolist()) and o.best_idx[0] == ref_best[0]
        np.testing.assert_allclose(o.dist_mue, d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(o.stdev, d[f"stdev_{t}"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-6, atol=1e-6)
        # the recorded closed loop continues from the reference's own distribution
        o.dist_mue, o.stdev = d[f"dist_mue_{t}"].copy(), d[f"stdev_{t}"].copy()
        o.u = O._u_out(d[f"u_{t}"])
    assert o.count == int(d["steps"])


@pytest.mark.parametrize("case", RANDOM_CASES)
def test_random_action_matches_reference(case):
    """optimizer_random_action_tf.py:38-86 as the unmodified module computed it; `cfg1` is BASELINE configs[0] (N 32, H 10)"""
    d = load(f"random_{case}.npz")
    o = random_oracle_from(d)
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(np.broadcast_to(np.asarray(o.u, np.float32).reshape(-1), d[f"u_prev_{t}"].shape), d[f"u_prev_{t}"])
        u = o.step(d[f"s_{t}"], d[f"u01_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        assert cut_is_separated(d[f"J_{t}"], 1)
        assert int(o.best_idx) == int(np.argmin(d[f"J_{t}"]))
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-6, atol=1e-7)
        o.u = O._u_out(d[f"u_{t}"])


@pytest.mark.parametrize("case", CEM_NAIVE_GRAD_CASES)
def test_cem_naive_grad_matches_reference(case):
    """optimizer_cem_naive_grad_tf.py:58-119 as the unmodified module computed it (tf.GradientTape -> torch autograd in the stand-in):
    pins the variant's statement order — gradient at the CLIPPED samples, one clipped-norm SGD step, clip, re-rollout, refit, and
    `u` = the refitted MEAN's first input (:103)"""
    d = load(f"cem_naive_grad_{case}.npz")
    o = cem_naive_grad_oracle_from(d)
    K = int(d["cem_best_k"])
    for t in range(int(d["steps"])):
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=2e-5, atol=5e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=5e-5)
        if cut_is_separated(d[f"J_{t}"], K):
            np.testing.assert_allclose(o.dist_mue, d[f"dist_mue_{t}"], rtol=2e-5, atol=5e-6)
            np.testing.assert_allclose(o.stdev, d[f"stdev_{t}"], rtol=5e-5, atol=5e-6)
            np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=2e-5, atol=5e-6)
        o.dist_mue, o.stdev = d[f"dist_mue_{t}"].copy(), d[f"stdev_{t}"].copy()
        o.u = O._u_out(d[f"u_{t}"])


def test_cem_properties():
    pred = O.Predictor("ODE")
    cost = O.Cost(pred.env)
    N, H = 64, 8
    c = O.CEM(pred, cost, num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=N)
    noise = np.random.default_rng(0).standard_normal((1, N, H, 1)).astype(np.float32)
    s = np.array([0.1, 0, 0.3, 0], np.float32)
    mu_before = c.dist_mue.copy()
    c.step(s, noise)
    # cem_best_k == N => mu == mean(Q); compare the pre-shift mean
    np.testing.assert_allclose(c.dist_mue[0, :-1, 0], c.Q.mean(0)[1:, 0], rtol=1e-5, atol=1e-6)
    assert c.dist_mue[0, -1, 0] == 0.0 and c.stdev[0, -1, 0] == np.float32(0.5)
    assert np.all(c.stdev >= np.float32(0.01))
    assert c.u == c.Q[np.argmin(c.J), 0, 0]
    assert np.all(np.abs(c.Q) <= 1.0)


def test_random_action_cfg1():
    # BASELINE config 1: random-action, N=32, H=10, 4-state analytic predictor (CPU plumbing)
    pred = O.Predictor("ODE")
    r = O.RandomAction(pred, O.Cost(pred.env), num_rollouts=32, mpc_horizon=10)
    u01 = np.random.default_rng(3).random((32, 10, 1), dtype=np.float32)
    u = r.step(np.array([0.0, 0.1, 0.5, -0.2], np.float32), u01)
    assert u == r.Q[np.argmin(r.J), 0, 0] and -1 <= u < 1
    assert r.rollout_trajectories.shape == (32, 11, 4)


def test_philox_known_answer():
    # Random123 known-answer vectors for philox4x32-10 (kat_vectors: zero and all-ones/pi cases)
    z = O.philox4x32(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert [hex(int(v)) for v in z] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    f = O.philox4x32(np.full(4, 0xFFFFFFFF, np.uint32), np.full(2, 0xFFFFFFFF, np.uint32))
    assert [hex(int(v)) for v in f] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    p = O.philox4x32(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], np.uint32),
                     np.array([0xa4093822, 0x299f31d0], np.uint32))
    assert [hex(int(v)) for v in p] == ["0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"]


def test_device_noise_statistics_and_sharding():
    a = O.device_noise(seed=7, stream=0, call=3, first_row=0, rows=4096, cols=50, kind="normal")
    assert abs(a.mean()) < 0.01 and abs(a.std() - 1) < 0.01 and np.isfinite(a).all()
    # shard invariance: rows generated by any shard equal the same global rows
    b = O.device_noise(seed=7, stream=0, call=3, first_row=1024, rows=1024, cols=50, kind="normal")
    np.testing.assert_array_equal(a[1024:2048], b)
    u = O.device_noise(seed=7, stream=1, call=0, first_row=0, rows=1024, cols=7, kind="uniform")
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.02


def test_torch_cpu_restatement_matches_the_numpy_oracle():
    """bench.py's second CPU leg (oracle/ctk_oracle_torch.py) is the pinned NumPy oracle's MPPI step in torch ops."""
    from oracle.ctk_oracle_torch import TorchMPPI
    env = O.EnvParams(terminal_weight=0.2)
    pred = O.Predictor("ODE", env=env)
    for (N, H, p) in [(64, 12, 5), (200, 30, 1)]:
        o = O.MPPI(pred, O.Cost(env), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
        t = TorchMPPI(O.MPPI(pred, O.Cost(env), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p))
        rng = np.random.default_rng(N)
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        for _ in range(3):
            noise = rng.standard_normal((N, o.P, 1)).astype(np.float32)
            uo, ut = float(o.step(s, noise)), t.step(s, noise)
            np.testing.assert_allclose(t.J.numpy(), o.J, rtol=2e-5)
            np.testing.assert_allclose(t.u_nom.numpy(), o.u_nom.reshape(-1), rtol=1e-4, atol=2e-5)
            assert abs(uo - ut) < 2e-5


# ---- second environment (Quad2D, C = 2): the same reference optimizers, recorded by tests/golden/make_golden.py -------------
@pytest.mark.parametrize("case", MPPI_QUAD_CASES + MPPI_HOVER_CASES)
def test_mppi_two_inputs_matches_reference(case):
    d = load(f"mppi_{case}.npz")
    o = mppi_oracle_from(d)
    assert (o.S, o.C) == ((6, 2) if case.startswith("quad") else (7, 3))
    np.testing.assert_array_equal(o.u_nom, d["u_nom_init"])
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(np.broadcast_to(np.asarray(o.u, np.float32).reshape(-1), (o.C,)), d[f"u_prev_{t}"])
        u = o.step(d[f"s_{t}"], d[f"noise_{t}"])
        np.testing.assert_allclose(o.u_run, d[f"u_run_{t}"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_{t}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(u, d[f"u_{t}"], rtol=1e-5, atol=2e-6)
        o.u_nom = d[f"u_nom_{t}"].copy(); o.u = d[f"u_{t}"].copy()


@pytest.mark.parametrize("case", RPGD_QUAD_CASES + RPGD_HOVER_CASES)
def test_rpgd_two_inputs_matches_reference(case):
    d = load(f"rpgd_{case}.npz")
    o = rpgd_oracle_from(d)
    o.optimizer_reset(d["reset_draws"])
    np.testing.assert_allclose(o.Q, d["Q_init"], rtol=1e-6, atol=1e-7)
    many_its = int(d["outer_its"]) >= 20
    tol = dict(rtol=1e-3, atol=2e-3) if many_its else dict(rtol=1e-4, atol=1e-4)
    for t in range(int(d["steps"])):
        key = f"resample_draws_{t}"
        u = o.step(d[f"s_{t}"], d[key] if key in d.files else None)
        np.testing.assert_allclose(o.u_nom, d[f"u_nom_{t}"], **tol)
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], **tol)
        np.testing.assert_allclose(o.opt.m, d[f"m_{t}"], **tol)
        np.testing.assert_allclose(o.opt.v, d[f"v_{t}"], **tol)
        np.testing.assert_array_equal(o.trajectory_ages, d[f"ages_{t}"])
        # what the reference logs (optimizer_rpgd.py:428-433): the descended population, get_action's costs and trajectories
        np.testing.assert_allclose(o.Q_before_warmstart, d[f"Q_logged_{t}"], **tol)
        np.testing.assert_allclose(o.J, d[f"J_logged_{t}"], rtol=1e-3 if many_its else 2e-5)
        np.testing.assert_allclose(o.rollout_trajectories, d[f"traj_logged_{t}"], rtol=2e-3 if many_its else 1e-4, atol=1e-2 if many_its else 1e-5)   # (20 Adam iterations: plans to 2e-3, integrated over the horizon)
        # :382-386: summed stage cost of the best plan = get_summed_stage_cost (no terminal term, Cost_Functions/__init__.py:71-72)
        tr = o.predictor.predict_core(d[f"s_{t}"].reshape(1, -1), d[f"u_nom_{t}"])
        np.testing.assert_allclose(tr, d[f"optimal_trajectory_{t}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o.cost.get_summed_stage_cost(tr, d[f"u_nom_{t}"], np.asarray(d[f"u_prev_{t}"], np.float32).reshape(-1)),
                                   d[f"summed_stage_cost_{t}"], rtol=2e-5)
        assert o.opt.step_count == int(d[f"adam_step_{t}"])
        np.testing.assert_allclose(u, d[f"u_{t}"], **tol)
        o.Q = d[f"Q_{t}"].copy(); o.opt.m = d[f"m_{t}"].copy(); o.opt.v = d[f"v_{t}"].copy(); o.u = d[f"u_{t}"].copy()


# ---- the oracle's hand-written reverse modes against torch autograd in fp64 (build container and GPU box: torch-CPU) ------------
@pytest.mark.parametrize("kind,envname", [("ODE", "CartPole"), ("MLP", "CartPole"), ("GRU", "CartPole"), ("GRU", "Quad2D"), ("MLP", "Quad2D"), ("ODE", "Quad2D"), ("ODE", "Hover"), ("MLP", "Hover"), ("GRU", "Hover")])
def test_oracle_adjoints_match_torch_autograd_fp64(kind, envname):
    """d(sum_n J_n)/dQ from rollout_cost_and_grad (what the HIP reverse sweeps are tested against) == autograd through a
    float64 torch restatement of the same rollout and cost (what the reference does at optimizer_rpgd.py:329-333).  CartPole's ODE
    step and cost are param_cases.PlantF64's: the float64 statement from the primary parameters alone."""
    import torch
    from param_cases import PlantF64
    env = O.ENVIRONMENTS[envname](terminal_weight=0.3)
    S, C = env.S, env.C
    weights = None if kind == "ODE" else (O.gru_default_weights(4, S + C, S) if kind == "GRU" else O.mlp_default_weights(4, S + C, S))
    pred = O.Predictor(kind, env=env, weights=weights)
    cost = O.Cost(env)
    rng = np.random.default_rng(0)
    N, H = 6, 9
    if kind == "GRU":
        pred.hidden = (0.3 * rng.standard_normal((2, 32))).astype(np.float32)
    Q = rng.uniform(-1, 1, (N, H, C)).astype(np.float32)
    s0 = (rng.standard_normal(S) * 0.3).astype(np.float32)
    up = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    J, traj, g = O.rollout_cost_and_grad(pred, cost, np.tile(s0, (N, 1)), Q, up)

    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    Qt = T(Q).requires_grad_(True)
    k = {kk: float(v) for kk, v in O.derived_constants(env, 0.02, 1).items()}
    plant = PlantF64(envname, env)

    def step(s, u, hid):
        if kind == "ODE" and envname == "CartPole":
            return plant.step(s, u), hid
        if kind == "MLP":
            W1, b1, W2, b2, W3, b3 = (T(a) for a in O.mlp_unpack(weights, S + C, S))
            x = torch.cat([s, u], 1)
            return torch.tanh(torch.tanh(x @ W1.T + b1) @ W2.T + b2) @ W3.T + b3, hid
        if kind == "GRU":
            layers, Wo, bo = O.gru_unpack(weights, S + C, S)
            x = torch.cat([s, u], 1)
            new = []
            for (Wi, Wh, bi, bh), hprev in zip(layers, hid):
                gi, gh = x @ T(Wi).T + T(bi), hprev @ T(Wh).T + T(bh)
                r, z = torch.sigmoid(gi[:, :32] + gh[:, :32]), torch.sigmoid(gi[:, 32:64] + gh[:, 32:64])
                n = torch.tanh(gi[:, 64:] + r * gh[:, 64:])
                x = (1 - z) * n + z * hprev
                new.append(x)
            return x @ T(Wo).T + T(bo), new
        if envname == "Hover":                                            # hovercraft ODE
            x_, vx, y_, vy, th, om, w = s.unbind(1)
            fb, fl = k["aF"] * u[:, 0], k["aL"] * u[:, 1]
            ax = fb * torch.cos(th) - fl * torch.sin(th) - k["c_v"] * vx
            ay = fb * torch.sin(th) + fl * torch.cos(th) - k["c_v"] * vy
            al, aw = -k["kT"] * u[:, 2] - k["c_w"] * om, k["kW"] * u[:, 2] - k["c_ww"] * w
            dt = k["dt"]
            return torch.stack([x_ + dt * vx, vx + dt * ax, y_ + dt * vy, vy + dt * ay, th + dt * om, om + dt * al, w + dt * aw], 1), hid
        x_, vx, z_, vz, th, om = s.unbind(1)                              # Quad2D ODE
        aF, aM = k["g"] + k["kF"] * (u[:, 0] + u[:, 1]), k["kM"] * (u[:, 0] - u[:, 1])
        ax, az, al = -aF * torch.sin(th) - k["c_v"] * vx, aF * torch.cos(th) - k["g"] - k["c_v"] * vz, aM - k["c_w"] * om
        dt = k["dt"]
        return torch.stack([x_ + dt * vx, vx + dt * ax, z_ + dt * vz, vz + dt * az, th + dt * om, om + dt * al], 1), hid

    def stage(s, u, upv):
        e = env
        if kind in ("ODE", "MLP") and envname == "CartPole":
            return plant.stage_cost(s, u, upv), plant.state_cost(s)
        if envname == "Hover":
            pos = k["pos_c"] * ((s[:, 0] - e.target_x) ** 2 + (s[:, 2] - e.target_y) ** 2) + e.ang_weight * (1 - torch.cos(s[:, 4]))
            return (pos + e.vel_weight * (s[:, 1] ** 2 + s[:, 3] ** 2) + e.angvel_weight * s[:, 5] ** 2 + e.wheel_weight * s[:, 6] ** 2
                    + k["ccR"] * (u ** 2).sum(1) + e.ccrc_weight * ((u - upv) ** 2).sum(1)), pos
        if envname == "Quad2D":
            pos = k["pos_c"] * ((s[:, 0] - e.target_x) ** 2 + (s[:, 2] - e.target_z) ** 2) + e.ang_weight * (1 - torch.cos(s[:, 4]))
            return (pos + e.vel_weight * (s[:, 1] ** 2 + s[:, 3] ** 2) + e.angvel_weight * s[:, 5] ** 2
                    + k["ccR"] * (u ** 2).sum(1) + e.ccrc_weight * ((u - upv) ** 2).sum(1)), pos
        dd = e.dd_weight * ((s[:, 0] - e.target_position) * k["inv_xs"]) ** 2
        ep = k["ep_c"] * (1 - torch.cos(s[:, 2])) ** 2
        return dd + ep + e.ekp_weight * s[:, 3] ** 2 + k["ccR"] * u[:, 0] ** 2 + e.ccrc_weight * (u[:, 0] - upv[:, 0]) ** 2, dd + ep

    s = T(np.tile(s0, (N, 1)))
    hid = [T(np.tile(pred.hidden[i:i + 1], (N, 1))) for i in range(2)] if kind == "GRU" else None
    upv = T(np.tile(up, (N, 1)))
    tot = 0.0
    for h in range(H):
        c, _ = stage(s, Qt[:, h, :], upv)
        tot = tot + c
        s, hid = step(s, Qt[:, h, :], hid)
        upv = Qt[:, h, :]
    _, term = stage(s, Qt[:, 0, :] * 0, upv * 0)
    Jt = (tot + env.terminal_weight * term) / (H + 1)
    Jt.sum().backward()
    np.testing.assert_allclose(J, Jt.detach().numpy(), rtol=2e-5)
    scale = np.abs(Qt.grad.numpy()).max()
    np.testing.assert_allclose(g, Qt.grad.numpy(), rtol=2e-4, atol=2e-6 * max(1.0, scale))
