"""CPU: the float64 merge references of tests/shard_refs.py against the pinned oracle.  The population of one oracle step is cut
into G groups, each group's record is built from the oracle's own costs and plans, and the reference's merge of those records must
give what the oracle computed on the whole population.  Pure gathers, shifts and ages compare exactly; means, std and the soft-min
at the tolerances tests/test_oracle_golden.py uses for the same quantities (fp32 oracle against a float64 statement)."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
import shard_refs as R

# tests/test_oracle_golden.py: u_nom / u of the fp32 oracle against the recorded reference (test_mppi_oracle_matches_reference_golden)
MPPI_U_TOL = dict(rtol=1e-5, atol=2e-6)
# tests/test_oracle_golden.py: dist_mue and stdev of the fp32 oracle against the recorded reference (the CEM golden test)
CEM_MU_TOL = dict(rtol=1e-5, atol=2e-6)
CEM_STD_TOL = dict(rtol=2e-5, atol=2e-6)

QLO, QHI = np.array([-1.0, -0.8], np.float32), np.array([1.0, 0.9], np.float32)
START = {"CartPole": np.array([0.05, -0.1, 2.8, 0.4], np.float32), "Quad2D": np.array([0.3, -0.2, 0.7, 0.1, 0.25, -0.4], np.float32)}
# (n_ranks, k) of the record-level RPGD cases of tests/test_gpu_shards.py, N_local = 16
RPGD_CASES = [(3, 5), (3, 16), (3, 24), (4, 61), (8, 24), (8, 128), (8, 127)]


def plant(envname, kind="ODE"):
    env = O.EnvParams(terminal_weight=0.3) if envname == "CartPole" else O.Quad2DParams(terminal_weight=0.4, target_x=0.1)
    lo, hi = (-1.0, 1.0) if envname == "CartPole" else (QLO, QHI)
    return O.Predictor(kind, dt=0.02, env=env), env, lo, hi


def groups(N, G):
    """G contiguous groups, ragged when G does not divide N"""
    cuts = np.linspace(0, N, G + 1).astype(int)
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_mppi_end_ref_reproduces_the_oracle_step(envname, G):
    pred, env, lo, hi = plant(envname)
    N, H, p = 100, 12, 5
    o = O.MPPI(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    rng = np.random.default_rng(G)
    s = START[envname]
    for t in range(3):
        u_nom_in = o.u_nom[0].copy()
        noise = rng.standard_normal((N, o.P, o.C)).astype(np.float32)
        u = o.step(s, noise)
        J, scaled = o.J.astype(np.float64), (noise * o.stdev).astype(np.float64)
        parts = []
        for a, b in groups(N, G):
            rho = J[a:b].min()
            e = np.exp(-(J[a:b] - rho) / o.LBD)
            parts.append(np.concatenate([[rho, e.sum()], np.sum(e[:, None, None] * scaled[a:b], axis=0).reshape(-1)]))
        u_nom, u_ref = R.mppi_end_ref(np.stack(parts), u_nom_in, o.M, o.LBD, o.low, o.high)
        np.testing.assert_allclose(u_nom, o.u_nom[0], **MPPI_U_TOL)
        np.testing.assert_allclose(u_ref, np.asarray(u).reshape(-1), **MPPI_U_TOL)
        s = pred.step(s.reshape(1, -1), np.asarray(u, np.float32).reshape(1, -1))[0]


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
@pytest.mark.parametrize("G,K", [(1, 13), (3, 13), (8, 13), (3, 1), (3, 40)])
def test_topk_refit_ref_reproduces_the_oracle_iteration(envname, G, K):
    pred, env, lo, hi = plant(envname)
    N, H, its = 120, 6, 3
    o = O.CEM(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=its, cem_best_k=K)
    rng = np.random.default_rng(10 * G + K)
    s_t = np.tile(START[envname].reshape(1, -1), (N, 1))
    for it in range(its):
        Q, elite, J, _, best = o.update_distribution(s_t, rng.standard_normal((N, H, o.C)).astype(np.float32))
        cands = np.concatenate([R.topk_records(J[a:b], Q[a:b], K, a) for a, b in groups(N, G)])
        idx, mu, sd = R.topk_refit_ref(cands, K)
        np.testing.assert_array_equal(cands[idx, 1].copy().view(np.int32), best)       # through the records' global-index field
        np.testing.assert_array_equal(cands[idx, 2:].reshape(K, H, o.C), elite)
        np.testing.assert_allclose(mu.reshape(1, H, o.C), o.dist_mue, **CEM_MU_TOL)
        np.testing.assert_allclose(sd.reshape(1, H, o.C), o.stdev, **CEM_STD_TOL)


def test_topk_refit_ref_k1_is_the_random_action_pick():
    pred, env, lo, hi = plant("Quad2D")
    N, H = 90, 4
    o = O.RandomAction(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H)
    u = o.step(START["Quad2D"], np.random.default_rng(3).random((N, H, 2), dtype=np.float32))
    cands = np.concatenate([R.topk_records(o.J[a:b], o.Q[a:b], 1, a) for a, b in groups(N, 5)])
    idx, mu, sd = R.topk_refit_ref(cands, 1)
    assert int(cands[idx[0], 1].view(np.int32)) == int(o.best_idx)
    np.testing.assert_array_equal(mu[:2], u)
    np.testing.assert_array_equal(sd, 0.0)


def test_cem_finish_ref_is_the_oracle_post_loop():
    pred, env, lo, hi = plant("Quad2D")
    N, H, K = 64, 5, 7
    o = O.CEM(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=K, cem_stdev_min=0.3)
    noise = np.random.default_rng(8).standard_normal((1, N, H, 2)).astype(np.float32)
    s_t = np.tile(START["Quad2D"].reshape(1, -1), (N, 1))
    o2 = O.CEM(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=K, cem_stdev_min=0.3)
    o2.update_distribution(s_t, noise[0])
    o.step(START["Quad2D"], noise)
    mu, sd = R.cem_finish_ref(o2.dist_mue.reshape(-1), o2.stdev.reshape(-1), H, 2, 0.3, 0.5, lo, hi)
    np.testing.assert_array_equal(mu.astype(np.float32), o.dist_mue[0])
    np.testing.assert_array_equal(sd.astype(np.float32), o.stdev[0])
    assert (o2.stdev < 0.3).any()                      # the clip did something


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
@pytest.mark.parametrize("G,k", RPGD_CASES)
def test_rpgd_end_ref_reproduces_the_oracle_keep_k(envname, G, k):
    pred, env, lo, hi = plant(envname)
    Nl, H, p, its = 16, (7 if envname == "CartPole" else 5), (3 if envname == "CartPole" else 1), 2
    N = G * Nl
    o = O.RPGD(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, outer_its=its, resamp_per=2,
               period_interpolation_inducing_points=p, shift_previous=1, opt_keep_k_ratio=k / N)
    o.k = k
    C = o.C
    rng = np.random.default_rng(G * 1000 + k)
    o.optimizer_reset(rng.random((N, o.P, C), dtype=np.float32))
    s = START[envname]
    s_t = np.tile(s.reshape(1, -1), (N, 1))
    o.first_iter_count = 0                               # the descent is run here, so that the state BEFORE the keep-k step is in hand
    o.outer_its = 0
    for t in range(3):                                   # resampling, non-resampling, resampling
        for _ in range(its):
            o.grad_step(s_t)
        Q, m, v, ages = o.Q.copy(), o.opt.m.copy(), o.opt.v.copy(), o.trajectory_ages.copy()
        J = o.cost.get_trajectory_cost(o.predictor.predict_core(s_t, Q), Q, np.asarray(o.u, np.float32).reshape(C))
        resample = t % 2 == 0
        draws = rng.random((N - k, o.P, C), dtype=np.float32) if resample else None
        fresh_all = o.sample_actions(draws) if resample else None
        u = o.step(s, draws)
        np.testing.assert_array_equal(o.J, J)            # the oracle's get_action saw the population recorded above
        kl = min(k, Nl)
        recs = np.concatenate([R.rpgd_records(J[g * Nl:(g + 1) * Nl], Q[g * Nl:(g + 1) * Nl], m[g * Nl:(g + 1) * Nl],
                                              v[g * Nl:(g + 1) * Nl], ages[g * Nl:(g + 1) * Nl], kl, g * Nl) for g in range(G)])
        out = []
        for g in range(G):
            off = g * Nl
            nf = R.rpgd_fresh_rows_ref(k, G, Nl, off, resample)
            sl = slice(off, off + Nl)
            out.append(R.rpgd_end_ref(recs, k, G, Nl, off, resample, 1, fresh_all[off:off + nf] if resample else None, C=C,
                                      own=(Q[sl], m[sl], v[sl], ages[sl])))
            assert out[-1][6] == nf
            np.testing.assert_array_equal(out[-1][4], o.u_nom[0])
            np.testing.assert_array_equal(out[-1][5], np.asarray(u).reshape(-1))
        assert sum(x[6] for x in out) == (N - k if resample else 0)
        for j, want in enumerate((o.Q, o.opt.m, o.opt.v, o.trajectory_ages)):
            np.testing.assert_array_equal(np.concatenate([x[j] for x in out]), want)
        s = pred.step(s.reshape(1, -1), np.asarray(u, np.float32).reshape(1, -1))[0]
        s_t = np.tile(s.reshape(1, -1), (N, 1))
