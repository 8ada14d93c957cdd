"""-m gpu: the sharded entry points (ctk_mppi_step_begin/_end, ctk_shard_iter_begin/_end/_finish, ctk_rpgd_step_begin/_end) at 3-8
shards in ONE process.

 a. record level: between *_begin and *_end the gathered record buffer is the caller's own device tensor, so the test writes any
    records into it and holds *_end against the float64 NumPy statement of the merge (tests/shard_refs.py) on exactly those records —
    no rollout is involved, and world sizes / record counts no real shard count could reach are reached through the API;
 b. end to end: G shards of a small N_local + the record exchange == one handle of G * N_local (and the oracle for CEM / random-action);
 c. refusals: calls out of order and impossible sizes raise the documented error and leave the handle's state vector unchanged."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine
from control_toolkit_amd._capi import CtkError
from gpu_helpers import apply_env
from margins import close
from test_gpu_mppi import U_TOL
from test_gpu_env import apply_params, quad_env, QLO, QHI, S0 as QUAD_S0
import shard_refs as R

pytestmark = pytest.mark.gpu

ENVS = {"CartPole": dict(lo=-1.0, hi=1.0, C=1, S=4, s0=np.array([0.05, -0.1, 2.8, 0.4], np.float32)),
        "Quad2D": dict(lo=QLO, hi=QHI, C=2, S=6, s0=QUAD_S0)}
LBD = 100.0                      # the engine's default MPPI temperature (control_toolkit_amd/_capi.py)
STD_MIN, INIT_STD = 0.01, 0.5    # the engine's default CEM constants
# test_sharded_topk_two_shards_equal_one_handle (tests/test_gpu_cem_random.py): shards against the full handle
TOPK_U_TOL, TOPK_MU_TOL, TOPK_STD_TOL = dict(rtol=1e-6, atol=1e-7), dict(rtol=1e-5, atol=1e-6), dict(rtol=1e-4, atol=1e-6)
# test_cem_matches_oracle (tests/test_gpu_cem_random.py): device against the fp32 oracle
ORACLE_J_RTOL, ORACLE_DIST_TOL, ORACLE_U_TOL = 3e-5, dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-5, atol=2e-6)
# test_sharded_rpgd_two_shards_equal_one_handle (tests/test_gpu_rpgd.py): shards against the full handle, and fresh rows
RPGD_TOL = dict(rtol=1e-6, atol=1e-7)
NL_RPGD = 16
# (n_ranks, k) at N_local = 16 and what each covers
RPGD_CASES = [(3, 5),      # the straddle inside the last shard
              (3, 16),     # a shard with n_fresh == 0 (the last: all keepers); the others have n_fresh == N_local
              (3, 24),     # k > N_local; shard 1 straddles; shard 2 has keeper_base 8 > 0
              (4, 61),     # shard 0 straddles
              (8, 24),     # six shards with n_fresh == N_local
              (8, 128)]    # opt_keep_k == the whole population (a single handle accepts it: test_rpgd_shards_equal_one_handle runs it)


def limits(envname):
    e = ENVS[envname]
    C = e["C"]
    return np.broadcast_to(np.asarray(e["lo"], np.float32), (C,)), np.broadcast_to(np.asarray(e["hi"], np.float32), (C,))


def plant(envname, kind="ODE", weights=None):
    env = O.EnvParams(terminal_weight=0.3) if envname == "CartPole" else quad_env()
    return O.Predictor(kind, dt=0.02, env=env, weights=weights), env


def engine(opt, envname, N, kind="ODE", env=None, weights=None, **kw):
    e = CtkEngine(opt, kind, environment=envname, num_rollouts=N, dt=0.02, action_low=ENVS[envname]["lo"], action_high=ENVS[envname]["hi"], **kw)
    if env is not None:
        (apply_env if envname == "CartPole" else apply_params)(e, env)
    if weights is not None:
        e.set_predictor_weights(weights)
    return e


def device_buffer(floats):
    import torch
    return torch.zeros(int(floats), dtype=torch.float32, device="cuda")


def overwrite(buf, recs):
    """the begin kernels (engine stream) have written their record: wait, then replace the whole buffer with the crafted records"""
    import torch
    torch.cuda.synchronize()
    flat = np.ascontiguousarray(recs, np.float32).ravel()
    assert flat.size == buf.numel()
    buf.copy_(torch.from_numpy(flat))
    torch.cuda.synchronize()


def sync():
    import torch
    torch.cuda.synchronize()


# =====================================================================================================================================
# a. record level — MPPI
# =====================================================================================================================================
def staged_floats(P, n):
    """LDS floats of a merge with all n records of P columns staged (csrc/ctk_mppi_merge.h: merge_lds_staged):
    (8 + P + 1 + min(n, 1024)) + n * (2 + P) + 256; the merge stages while that stays <= 64 KiB"""
    return (8 + P + 1 + min(n, 1024)) + n * (2 + P) + 256


def last_staged(P):
    n = 1
    while 4 * staged_floats(P, n + 1) <= 64 * 1024:
        n += 1
    return n


def mppi_records(rng, n, PC, regime):
    a = rng.uniform(1.0, 40.0, n)
    b = rng.standard_normal((n, PC)) * 0.3 * a[:, None]
    rho0 = 37.5
    if regime == "equal":
        rho = np.full(n, rho0)
    elif regime == "within_3_lambda":
        rho = rho0 + rng.uniform(0.0, 3.0 * LBD, n)
    else:                                # "alone": every other weight underflows to 0, the result is that one record's b / a
        rho = np.full(n, rho0 + 200.0 * LBD)
        rho[rng.integers(n)] = rho0
    return np.concatenate([rho[:, None], a[:, None], b], 1).astype(np.float32)


def mppi_plan_near_limits(rng, H, C, lo, hi):
    u = rng.uniform(-0.5, 0.5, (H, C)).astype(np.float32)
    for c in range(C):
        u[3:6, c] = hi[c] - np.float32(1e-4)       # a few columns a hair inside a limit: the clip is exercised
        u[min(9, H - 1):min(12, H), c] = lo[c] + np.float32(1e-4)
    return u


def mppi_record_case(envname, H, p, counts):
    C, s0 = ENVS[envname]["C"], ENVS[envname]["s0"]
    lo, hi = limits(envname)
    e = engine("mppi", envname, 64, mpc_horizon=H, period_interpolation_inducing_points=p)
    rec = e.mppi_partial_size()
    P = O.num_inducing_points(H, p)
    assert rec == 2 + P * C
    M = O.interpolation_matrix(H, p, C)
    rng = np.random.default_rng(1000 * H + len(envname))
    clipped = 0
    for n in counts:
        buf = device_buffer(n * rec)
        for regime in ("equal", "within_3_lambda", "alone"):
            u_nom_in = mppi_plan_near_limits(rng, H, C, lo, hi)
            e.set_state(np.concatenate([u_nom_in.ravel(), np.zeros(C, np.float32)]))
            e.mppi_step_begin(s0, buf.data_ptr(), rng.standard_normal((64, P, C)).astype(np.float32))   # any draws: the step is pending
            parts = mppi_records(rng, n, P * C, regime)
            overwrite(buf, parts)
            u = e.mppi_step_end(buf.data_ptr(), n)
            want_nom, want_u = R.mppi_end_ref(parts, u_nom_in, M, LBD, lo, hi)
            got = e.read("U_NOM")[0]
            clipped += int(((want_nom == lo) | (want_nom == hi)).sum())
            tag = f"shards mppi_end {envname} H={H} p={p} n={n} {regime}"
            if regime == "alone":
                assert np.isfinite(got).all() and np.isfinite(u).all()
            close(tag, "u_nom", got, want_nom, **U_TOL)
            close(tag, "u", u, want_u, **U_TOL)
    assert clipped > 0
    e.close()


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
def test_mppi_end_against_float64_few_records(envname):
    """CartPole: the tuned merge ctk_mppi_merge<true>; Quad2D: ctk_g_mppi_update (C = 2).  H = 50, p = 1: P = 50 columns per input"""
    mppi_record_case(envname, 50, 1, [1, 3, 16, 65])


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
def test_mppi_end_against_float64_at_the_staging_limit(envname):
    """the largest record count whose staged merge fits 64 KiB of LDS, and one more: the UNSTAGED MERGE of the tuned merge (records
    read from memory, !merge_can_stage).  The staged count is also above 128 narrow records: it takes the sliced column sums"""
    P = 50 * ENVS[envname]["C"]
    n = last_staged(P)
    assert 4 * staged_floats(P, n) <= 64 * 1024 < 4 * staged_floats(P, n + 1)
    assert (envname, n) in (("CartPole", 303), ("Quad2D", 155))
    mppi_record_case(envname, 50, 1, [n, n + 1])


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
def test_mppi_end_against_float64_beyond_one_chunk(envname):
    """1100 > 1024 records.  CartPole: the SECOND MERGE CHUNK of the tuned merge (MERGE_CHUNK = 1024 rescale factors per pass).
    Quad2D: the PRE-MERGE ABOVE G_UPD_MAX_PARTS (ctk_launch_mppi_merge_partial into one record before ctk_g_mppi_update)"""
    mppi_record_case(envname, 50, 1, [1100])


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
def test_mppi_end_against_float64_interpolated(envname):
    """H = 12, p = 5: P = 4 inducing points, the update interpolates; 200 staged narrow records take the sliced column sums"""
    mppi_record_case(envname, 12, 5, [3, 200])


# =====================================================================================================================================
# a. record level — CEM / random-action
# =====================================================================================================================================
def topk_lists(n_ranks, K, N_local, H, envname, ties, seed0):
    """per-rank candidate lists as *_begin leaves them (best K of N_local rows, sorted by (J, index), global indices), concatenated
    rank-major.  ties: J on a grid of whole numbers, and a seed at which the K-th and (K+1)-th record in sorted order have EQUAL J
    and sit in DIFFERENT ranks' lists — the tie rule then decides the elite set.  Otherwise all J distinct."""
    lo, hi = limits(envname)
    C = ENVS[envname]["C"]
    for seed in range(seed0, seed0 + 400):
        rng = np.random.default_rng(seed)
        lists = []
        distinct = (1.0 + 0.005 * rng.permutation(n_ranks * N_local)).astype(np.float32).reshape(n_ranks, N_local)
        for r in range(n_ranks):
            J = np.round(rng.uniform(1.0, 100.0, N_local)).astype(np.float32) if ties else distinct[r]
            Q = rng.uniform(lo, hi, (N_local, H, C)).astype(np.float32)
            lists.append(R.topk_records(J, Q, K, r * N_local))
        cands = np.concatenate(lists)
        order = np.argsort(cands[:, 0], kind="stable")
        if not ties:
            if len(np.unique(cands[:, 0])) == len(cands):
                return cands
        elif cands[order[K - 1], 0] == cands[order[K], 0] and order[K - 1] // K != order[K] // K:
            return cands
    raise AssertionError("no seed gives the wanted cost pattern")


TOPK_CASES = [(1, 1, 64, None), (3, 13, 64, None), (8, 40, 64, None), (5, 1, 64, None),
              (8, 2050, 2112, 2)]   # M = 16 400 > 16 * 1024: every selection wave takes a SECOND CHUNK pass, over records of STRIDE 2 + HC


@pytest.mark.parametrize("envname,H", [("CartPole", 6), ("Quad2D", 4)])
@pytest.mark.parametrize("n_ranks,K,N_local,H_big", TOPK_CASES)
def test_cem_iter_end_and_finish_against_float64(envname, H, n_ranks, K, N_local, H_big):
    H = H_big or H
    C, s0 = ENVS[envname]["C"], ENVS[envname]["s0"]
    lo, hi = limits(envname)
    e = engine("cem", envname, N_local, mpc_horizon=H, cem_outer_it=1, cem_best_k=K)
    rs = 2 + H * C
    assert e.shard_candidates_size() == K * rs and e.shard_iterations() == 1
    buf = device_buffer(n_ranks * K * rs)
    rng = np.random.default_rng(K)
    for ties in ([False, True] if n_ranks > 1 else [False]):       # one list cannot hold a tie that straddles ranks
        cands = topk_lists(n_ranks, K, N_local, H, envname, ties, seed0=7 * K + n_ranks)
        if ties:   # CROSS-RANK TIE AT THE CUT: "positional tie-break == global index" (ctk_shard_iter_end)
            order = np.argsort(cands[:, 0], kind="stable")
            assert cands[order[K - 1], 0] == cands[order[K], 0] and order[K - 1] // K != order[K] // K
        mu0 = rng.uniform(-0.3, 0.3, H * C).astype(np.float32)
        e.set_state(np.concatenate([mu0, np.full(H * C, 0.4, np.float32), np.zeros(C, np.float32), [1.0]]))
        e.shard_iter_begin(s0, buf.data_ptr(), rng.standard_normal((N_local, H, C)).astype(np.float32))
        overwrite(buf, cands)
        e.shard_iter_end(buf.data_ptr(), n_ranks)
        idx, mu, sd = R.topk_refit_ref(cands, K)
        tag = f"shards cem_end {envname} H={H} ranks={n_ranks} K={K} ties={ties}"
        close(tag, "mu", e.read("U_NOM").ravel(), mu, **TOPK_MU_TOL)
        close(tag, "std", e.read("STD").ravel(), sd, **TOPK_STD_TOL)
        u = e.shard_finish()
        np.testing.assert_array_equal(u, cands[idx[0], 2:2 + C])           # a copy of the best record's first input
        mu_f, sd_f = R.cem_finish_ref(mu, sd, H, C, STD_MIN, INIT_STD, lo, hi)
        close(tag, "mu_fin", e.read("U_NOM")[0], mu_f, **TOPK_MU_TOL)
        close(tag, "std_fin", e.read("STD")[0], sd_f, **TOPK_STD_TOL)
    e.close()


@pytest.mark.parametrize("envname,H", [("CartPole", 6), ("Quad2D", 4)])
@pytest.mark.parametrize("n_ranks", [1, 3, 5, 8])
def test_random_action_finish_is_the_best_record(envname, H, n_ranks):
    C, s0 = ENVS[envname]["C"], ENVS[envname]["s0"]
    e = engine("random_action", envname, 64, mpc_horizon=H)
    rs = 2 + H * C
    assert e.shard_candidates_size() == rs and e.shard_iterations() == 1
    buf = device_buffer(n_ranks * rs)
    rng = np.random.default_rng(n_ranks)
    for ties in ([False, True] if n_ranks > 1 else [False]):
        cands = topk_lists(n_ranks, 1, 64, H, envname, ties, seed0=n_ranks)
        e.shard_iter_begin(s0, buf.data_ptr(), rng.random((64, H, C), dtype=np.float32))
        overwrite(buf, cands)
        e.shard_iter_end(buf.data_ptr(), n_ranks)
        idx, _, _ = R.topk_refit_ref(cands, 1)
        np.testing.assert_array_equal(e.shard_finish(), cands[idx[0], 2:2 + C])
    e.close()


# =====================================================================================================================================
# a. record level — RPGD
# =====================================================================================================================================
def rpgd_state(Q, m, v, ages, u, adam_step, count):
    return np.concatenate([Q.ravel(), m.ravel(), v.ravel(), ages.ravel(), np.asarray(u, np.float32).ravel(), [adam_step], [count]]).astype(np.float32)


def rpgd_population(rng, N, H, envname):
    lo, hi = limits(envname)
    C = ENVS[envname]["C"]
    return (rng.uniform(lo, hi, (N, H, C)).astype(np.float32), (0.1 * rng.standard_normal((N, H, C))).astype(np.float32),
            rng.uniform(0.0, 0.01, (N, H, C)).astype(np.float32), rng.integers(1, 10, N).astype(np.float32))


def rpgd_lists(n_ranks, k, H, envname, ties, seed0):
    """per-rank keeper lists (best min(k, N_local) of N_local rows, sorted, global indices, ages 1..9, random plans and moments);
    ties: whole-number costs with the k-th and (k+1)-th record of the sorted union equal and in different ranks' lists (where the
    union has a (k+1)-th record)"""
    kl = min(k, NL_RPGD)
    for seed in range(seed0, seed0 + 400):
        rng = np.random.default_rng(seed)
        lists = []
        distinct = (1.0 + 0.25 * rng.permutation(n_ranks * NL_RPGD)).astype(np.float32).reshape(n_ranks, NL_RPGD)
        for r in range(n_ranks):
            J = np.round(rng.uniform(1.0, 40.0, NL_RPGD)).astype(np.float32) if ties else distinct[r]
            lists.append(R.rpgd_records(J, *rpgd_population(rng, NL_RPGD, H, envname), kl, r * NL_RPGD))
        recs = np.concatenate(lists)
        order = np.argsort(recs[:, 0], kind="stable")
        if not ties:
            if len(np.unique(recs[:, 0])) == len(recs):
                return recs
        elif k == len(recs):
            if len(np.unique(recs[:, 0])) < len(recs) // 2:
                return recs
        elif recs[order[k - 1], 0] == recs[order[k], 0] and order[k - 1] // kl != order[k] // kl:
            return recs
    raise AssertionError("no seed gives the wanted cost pattern")


def rpgd_kw(envname, k, off, its=1):
    H, p = (7, 3) if envname == "CartPole" else (5, 1)
    return dict(mpc_horizon=H, period_interpolation_inducing_points=p, outer_its=its, resamp_per=2, shift_previous=1, opt_keep_k=k,
                sampling_distribution=0, sample_whole_control_space=1, learning_rate=0.05, gradmax_clip=5.0, global_rollout_offset=off)


def rpgd_sampler(envname, H, p):
    pred, env = plant(envname)
    return O.RPGD(pred, O.Cost(env), ENVS[envname]["lo"], ENVS[envname]["hi"], num_rollouts=NL_RPGD, mpc_horizon=H,
                  period_interpolation_inducing_points=p, sample_whole_control_space=True)


def rpgd_record_step(e, buf, recs, envname, n_ranks, k, off, count, rng, sampler, tag):
    C, s0 = ENVS[envname]["C"], ENVS[envname]["s0"]
    H = e.H
    Q, m, v, ages = rpgd_population(rng, NL_RPGD, H, envname)
    e.set_state(rpgd_state(Q, m, v, ages, np.zeros(C), 3, count))
    e.rpgd_step_begin(s0, buf.data_ptr())
    sync()
    own = tuple(e.read(n) for n in ("PLAN", "ADAM_M", "ADAM_V", "AGES"))      # this shard's rows after the descent
    overwrite(buf, recs)
    resample = count % 2 == 0
    nf = R.rpgd_fresh_rows_ref(k, n_ranks, NL_RPGD, off, resample)
    assert e.rpgd_fresh_rows(n_ranks) == nf
    draws = rng.random((nf, sampler.P, C), dtype=np.float32) if nf else None
    u = e.rpgd_step_end(buf.data_ptr(), n_ranks, draws)
    fresh = sampler.sample_actions(draws) if nf else None
    want = R.rpgd_end_ref(recs, k, n_ranks, NL_RPGD, off, resample, 1, fresh, C=C, own=own)
    assert want[6] == nf
    got = [e.read(n) for n in ("PLAN", "ADAM_M", "ADAM_V", "AGES")]
    for name, g, w in zip(("PLAN", "ADAM_M", "ADAM_V", "AGES"), got, want[:4]):
        np.testing.assert_array_equal(g[nf:], w[nf:], err_msg=f"{tag} {name} keeper rows")      # copies
    close(tag, "fresh", got[0][:nf], want[0][:nf], **RPGD_TOL)
    np.testing.assert_array_equal(got[1][:nf], 0.0)
    np.testing.assert_array_equal(got[2][:nf], 0.0)
    np.testing.assert_array_equal(got[3][:nf], 1.0)
    np.testing.assert_array_equal(e.read("U_NOM")[0], want[4])
    np.testing.assert_array_equal(u, want[5])
    return nf


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
@pytest.mark.parametrize("n_ranks,k", RPGD_CASES)
def test_rpgd_end_against_float64_every_shard_role(envname, n_ranks, k):
    """one handle per global_rollout_offset in turn: the records are crafted, so no other shard is needed"""
    C = ENVS[envname]["C"]
    H, p = (7, 3) if envname == "CartPole" else (5, 1)
    sampler = rpgd_sampler(envname, H, p)
    kl = min(k, NL_RPGD)
    buf = device_buffer(n_ranks * kl * (3 + 3 * H * C))
    lists = {ties: rpgd_lists(n_ranks, k, H, envname, ties, seed0=100 * n_ranks + k) for ties in (False, True)}
    rng = np.random.default_rng(n_ranks * 1000 + k)
    fresh_rows = []
    for r in range(n_ranks):
        e = engine("rpgd", envname, NL_RPGD, **rpgd_kw(envname, k, r * NL_RPGD))
        assert e.rpgd_keepers_size() == kl * (3 + 3 * H * C)
        for ties in (False, True):
            nf = rpgd_record_step(e, buf, lists[ties], envname, n_ranks, k, r * NL_RPGD, 0, rng, sampler,
                                  f"shards rpgd_end {envname} ranks={n_ranks} k={k}")
        fresh_rows.append(nf)
        e.close()
    assert sum(fresh_rows) == n_ranks * NL_RPGD - k
    # the roles the table promises
    first_keeper = n_ranks * NL_RPGD - k
    assert fresh_rows == [int(np.clip(first_keeper - r * NL_RPGD, 0, NL_RPGD)) for r in range(n_ranks)]
    if (n_ranks, k) == (3, 16):
        assert fresh_rows == [16, 16, 0]           # n_fresh == N_local twice, n_fresh == 0 once
    if (n_ranks, k) == (3, 24):
        assert fresh_rows == [16, 8, 0] and 2 * NL_RPGD - first_keeper == 8    # k > N_local; shard 2: keeper_base 8 > 0
    if (n_ranks, k) == (8, 24):
        assert fresh_rows[:6] == [16] * 6


@pytest.mark.parametrize("envname", ["CartPole", "Quad2D"])
def test_rpgd_end_against_float64_without_resampling(envname):
    """(3, 24) on a NON-resampling step (count = 1, resamp_per = 2): every shard keeps its own rows, shifted; u_nom still comes from the records"""
    n_ranks, k = 3, 24
    C = ENVS[envname]["C"]
    H, p = (7, 3) if envname == "CartPole" else (5, 1)
    sampler = rpgd_sampler(envname, H, p)
    buf = device_buffer(n_ranks * NL_RPGD * (3 + 3 * H * C))
    recs = rpgd_lists(n_ranks, k, H, envname, True, seed0=11)
    rng = np.random.default_rng(5)
    for r in range(n_ranks):
        e = engine("rpgd", envname, NL_RPGD, **rpgd_kw(envname, k, r * NL_RPGD))
        nf = rpgd_record_step(e, buf, recs, envname, n_ranks, k, r * NL_RPGD, 1, rng, sampler, f"shards rpgd_end {envname} no resampling")
        assert nf == 0
        e.close()


# =====================================================================================================================================
# a. record level — one handle at 1, then 3, then 2 gathered ranks: the index buffer of *_end grows once (1 -> 3) and is then reused
# (3 -> 2); every result bit for bit that of a fresh handle at that rank count
# =====================================================================================================================================
RANK_COUNTS = (1, 3, 2)


def cem_end_at(e, n_ranks, K, N_local, H):
    C, s0 = ENVS["CartPole"]["C"], ENVS["CartPole"]["s0"]
    rng = np.random.default_rng(n_ranks)
    buf = device_buffer(n_ranks * K * (2 + H * C))
    cands = topk_lists(n_ranks, K, N_local, H, "CartPole", False, seed0=7 * K + n_ranks)
    e.set_state(np.concatenate([rng.uniform(-0.3, 0.3, H * C).astype(np.float32), np.full(H * C, 0.4, np.float32), np.zeros(C, np.float32), [1.0]]))
    e.shard_iter_begin(s0, buf.data_ptr(), rng.standard_normal((N_local, H, C)).astype(np.float32))
    overwrite(buf, cands)
    e.shard_iter_end(buf.data_ptr(), n_ranks)
    refit = [e.read("U_NOM"), e.read("STD")]
    return refit + [e.shard_finish(), e.read("U_NOM"), e.read("STD"), e.get_state()]


def test_cem_iter_end_index_buffer_grows_once_and_is_reused():
    K, N_local, H = 13, 64, 6
    kw = dict(mpc_horizon=H, cem_outer_it=1, cem_best_k=K)
    e = engine("cem", "CartPole", N_local, **kw)
    for n_ranks in RANK_COUNTS:
        got = cem_end_at(e, n_ranks, K, N_local, H)
        fresh = engine("cem", "CartPole", N_local, **kw)
        want = cem_end_at(fresh, n_ranks, K, N_local, H)
        fresh.close()
        for i, (g, w) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(g, w, err_msg=f"shards cem_end reused handle, ranks={n_ranks}, result {i}")
    e.close()


def rpgd_end_at(e, n_ranks, k):
    C, s0 = ENVS["CartPole"]["C"], ENVS["CartPole"]["s0"]
    H = e.H
    rng = np.random.default_rng(n_ranks)
    buf = device_buffer(n_ranks * min(k, NL_RPGD) * (3 + 3 * H * C))
    recs = rpgd_lists(n_ranks, k, H, "CartPole", False, seed0=100 * n_ranks + k)
    e.set_state(rpgd_state(*rpgd_population(rng, NL_RPGD, H, "CartPole"), np.zeros(C), 3, 0))      # count 0: a resampling step
    e.rpgd_step_begin(s0, buf.data_ptr())
    overwrite(buf, recs)
    nf = e.rpgd_fresh_rows(n_ranks)
    assert nf == R.rpgd_fresh_rows_ref(k, n_ranks, NL_RPGD, 0, True) and nf > 0
    u = e.rpgd_step_end(buf.data_ptr(), n_ranks, rng.random((nf, e.inducing_points(), C), dtype=np.float32))
    return [u] + [e.read(n) for n in ("PLAN", "ADAM_M", "ADAM_V", "AGES", "U_NOM")] + [e.get_state()]


def test_rpgd_step_end_index_buffer_grows_once_and_is_reused():
    k = 5                                       # <= the records of ONE rank, so that every rank count is accepted
    kw = rpgd_kw("CartPole", k, 0)
    e = engine("rpgd", "CartPole", NL_RPGD, **kw)
    for n_ranks in RANK_COUNTS:
        got = rpgd_end_at(e, n_ranks, k)
        fresh = engine("rpgd", "CartPole", NL_RPGD, **kw)
        want = rpgd_end_at(fresh, n_ranks, k)
        fresh.close()
        for i, (g, w) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(g, w, err_msg=f"shards rpgd_end reused handle, ranks={n_ranks}, result {i}")
    e.close()


# =====================================================================================================================================
# b. end to end: G shards == one handle (and the oracle)
# =====================================================================================================================================
NL = 40


@pytest.mark.parametrize("envname,kind", [("CartPole", "ODE"), ("Quad2D", "ODE")])
@pytest.mark.parametrize("G", [3, 4, 8])
def test_mppi_shards_equal_one_handle(envname, kind, G):
    mppi_shards_equal_one_handle(envname, kind, G)


def test_mppi_gru_three_shards_equal_one_handle():
    """every handle carries its own hidden state across the steps (ctk_mppi_step_end advances it like ctk_step)"""
    mppi_shards_equal_one_handle("CartPole", "GRU", 3)


def mppi_shards_equal_one_handle(envname, kind, G):
    C, S, s = ENVS[envname]["C"], ENVS[envname]["S"], ENVS[envname]["s0"].copy()
    H, p, N = 12, 5, G * NL
    w = O.gru_default_weights(1) if kind == "GRU" else None
    pred, env = plant(envname)          # the closed loop advances on the analytic plant, whatever model the controller predicts with
    kw = dict(mpc_horizon=H, period_interpolation_inducing_points=p, kind=kind, env=env, weights=w)
    full = engine("mppi", envname, N, **kw)
    sh = [engine("mppi", envname, NL, global_rollout_offset=i * NL, **kw) for i in range(G)]
    rec = full.mppi_partial_size()
    P = (rec - 2) // C
    buf = device_buffer(G * rec)
    rng = np.random.default_rng(G)
    for t in range(3):
        noise = rng.standard_normal((N, P, C)).astype(np.float32)
        u_full = full.step(s, noise)
        for i, e in enumerate(sh):
            e.mppi_step_begin(s, buf.data_ptr() + 4 * i * rec, noise[i * NL:(i + 1) * NL])
        sync()
        us = [e.mppi_step_end(buf.data_ptr(), G) for e in sh]
        for u in us[1:]:
            np.testing.assert_array_equal(u, us[0])
        tag = f"shards mppi {envname} {kind} G={G} step {t}"
        # test_mppi_sharded_begin_end_equals_single_step / two_shards_equal_one_handle: U_TOL
        close(tag, "u", us[0], u_full, **U_TOL)
        for e in sh:
            close(tag, "u_nom", e.read("U_NOM"), full.read("U_NOM"), **U_TOL)
        if kind == "GRU":
            for e in sh:   # test_mppi_gru_matches_oracle (tests/test_gpu_gru.py): the carried state, rtol 1e-4 / atol 2e-5
                close(tag, "hidden", e.predictor_get_hidden(), full.predictor_get_hidden(), rtol=1e-4, atol=2e-5)
        s = pred.step(s.reshape(1, S), u_full.reshape(1, C))[0]
    for e in sh + [full]:
        e.close()


class GapCEM(O.CEM):
    """O.CEM that records the relative cost gap at the elite cut of every iteration.  With K = 1 the refit stdev is exactly 0, so from
    the second iteration of a step on every plan IS the mean: no seed can open a gap there and none is needed, since whichever rows
    are chosen the elites are the same plan — such an iteration is recorded as inf after checking that the plans are identical."""
    def update_distribution(self, s_t, noise):
        out = super().update_distribution(s_t, noise)
        Q, srt = out[0], np.sort(out[2])
        gap = float((srt[self.K] - srt[self.K - 1]) / abs(srt[self.K - 1]))
        self.gaps = getattr(self, "gaps", []) + [np.inf if (Q == Q[:1]).all() else gap]
        return out


# start states near the targets: there the cost of a 6-step plan depends on the plan (far away it is one large constant + a sliver, and
# no seed separates the K-th from the (K+1)-th cost by 1e-4 relative)
TOPK_START = {"CartPole": np.array([0.0, 0.0, 0.1, 0.0], np.float32), "Quad2D": np.array([0.12, 0.05, 1.02, -0.05, 0.05, 0.1], np.float32)}
# rng seeds at which the ORACLE's relative cost gap at the elite cut exceeds 1e-4 in every iteration of the 3 steps (found on the CPU
# with the oracle alone; the test asserts the gap): (optimizer, environment, G, K, variant) -> seed
TOPK_SEEDS = {("cem", "CartPole", 4, 1, ""): 2, ("cem", "CartPole", 8, 40, ""): 2, ("cem", "Quad2D", 3, 13, ""): 2, ("cem", "Quad2D", 4, 40, ""): 2,
              ("random_action", "Quad2D", 4, 1, ""): 2, ("cem", "Quad2D", 3, 13, "u_prev"): 2}   # every other case: seed 1 (smallest gap 3.7e-4)


def topk_shards_equal_one_handle(opt, envname, G, K, warmup=False, with_u_prev=False, philox=False):
    C, S, s = ENVS[envname]["C"], ENVS[envname]["S"], TOPK_START[envname].copy()
    H, its, N = 6, 2, G * NL
    pred, env = plant(envname)
    lo, hi = ENVS[envname]["lo"], ENVS[envname]["hi"]
    kw = dict(mpc_horizon=H, env=env, seed=31)
    if opt == "cem":
        kw.update(cem_outer_it=its, cem_best_k=K, warmup=int(warmup), warmup_iterations=3 if warmup else 0)
        o = GapCEM(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=its, cem_best_k=K, warmup=warmup, warmup_iterations=3)
    else:
        o = O.RandomAction(pred, O.Cost(env), lo, hi, num_rollouts=N, mpc_horizon=H)
    full = engine(opt, envname, N, **kw)
    sh = [engine(opt, envname, NL, global_rollout_offset=i * NL, **kw) for i in range(G)]
    rec = sh[0].shard_candidates_size()
    assert rec == (K if opt == "cem" else 1) * (2 + H * C)
    buf = device_buffer(G * rec)
    rng = np.random.default_rng(TOPK_SEEDS.get((opt, envname, G, K, "warmup" if warmup else "u_prev" if with_u_prev else ""), 1))
    u_prev = None
    for t in range(3):
        n_it = sh[0].shard_iterations()
        assert n_it == ((3 if (warmup and t == 0) else its) if opt == "cem" else 1)
        if with_u_prev:
            u_prev = rng.uniform(-0.5, 0.5, C).astype(np.float32)
        draws = None
        if not philox:
            draws = (rng.standard_normal((n_it, N, H, C)) if opt == "cem" else rng.random((n_it, N, H, C))).astype(np.float32)
        u_full = full.step(s, None if philox else (draws if opt == "cem" else draws[0]), u_prev=u_prev)
        for it in range(n_it):
            for i, e in enumerate(sh):
                e.shard_iter_begin(s, buf.data_ptr() + 4 * i * rec, None if philox else draws[it, i * NL:(i + 1) * NL], u_prev=u_prev)
            sync()
            for e in sh:
                e.shard_iter_end(buf.data_ptr(), G)
        us = [e.shard_finish() for e in sh]
        for u in us[1:]:
            np.testing.assert_array_equal(u, us[0])
        tag = f"shards {opt} {envname} G={G} K={K} step {t}"
        close(tag, "u", us[0], u_full, **TOPK_U_TOL)
        close(tag, "J", np.concatenate([e.read("J") for e in sh]), full.read("J"), rtol=ORACLE_J_RTOL)
        if opt == "cem":
            for e in sh:
                close(tag, "mu", e.read("U_NOM"), full.read("U_NOM"), **TOPK_MU_TOL)
                close(tag, "std", e.read("STD"), full.read("STD"), **TOPK_STD_TOL)
        if not philox:
            # the fp32 oracle on the whole population (test_cem_matches_oracle / test_random_action_matches_oracle figures)
            if with_u_prev:
                o.u = O._u_out(u_prev)
            uo = o.step(s, draws if opt == "cem" else draws[0])
            if opt == "cem":
                assert len(o.gaps) >= n_it and min(o.gaps[-n_it:]) > 1e-4, o.gaps      # precondition: no elite decided by fp32 rounding
            else:
                srt = np.sort(o.J)
                assert (srt[1] - srt[0]) > 1e-4 * abs(srt[0])
            close(tag, "J_oracle", np.concatenate([e.read("J") for e in sh]), o.J, rtol=ORACLE_J_RTOL)
            close(tag, "u_oracle", us[0], np.asarray(uo).reshape(-1), **ORACLE_U_TOL)
            if opt == "cem":
                close(tag, "mu_oracle", sh[0].read("U_NOM"), o.dist_mue, **ORACLE_DIST_TOL)
                close(tag, "std_oracle", sh[-1].read("STD"), o.stdev, **ORACLE_DIST_TOL)
        s = pred.step(s.reshape(1, S), u_full.reshape(1, C))[0]
    for e in sh + [full]:
        e.close()


@pytest.mark.parametrize("envname,G,K", [("CartPole", G, K) for G in (3, 4, 8) for K in (1, 13, 40)] + [("Quad2D", 3, 13), ("Quad2D", 4, 40), ("Quad2D", 8, 1)])
def test_cem_shards_equal_one_handle_and_oracle(envname, G, K):
    """K = 40 = N_local: every row of every shard is a candidate"""
    topk_shards_equal_one_handle("cem", envname, G, K)


@pytest.mark.parametrize("envname,G", [("CartPole", 3), ("CartPole", 8), ("Quad2D", 4)])
def test_random_action_shards_equal_one_handle_and_oracle(envname, G):
    topk_shards_equal_one_handle("random_action", envname, G, 1)


def test_cem_shards_with_warmup_iterations():
    topk_shards_equal_one_handle("cem", "CartPole", 3, 13, warmup=True)      # shard_iterations() 3, then 2


def test_cem_shards_with_u_prev_given():
    topk_shards_equal_one_handle("cem", "Quad2D", 3, 13, with_u_prev=True)


@pytest.mark.parametrize("opt,envname", [("cem", "CartPole"), ("cem", "Quad2D"), ("random_action", "CartPole")])
def test_topk_shards_with_device_draws_equal_one_handle(opt, envname):
    """samples = None: every shard draws its rows of the GLOBAL Philox stream (same seed, global_rollout_offset set)"""
    topk_shards_equal_one_handle(opt, envname, 4, 13, philox=True)


@pytest.mark.parametrize("envname,kind,G,k,philox", [("CartPole", "ODE", G, k, False) for G, k in RPGD_CASES]
                         + [("Quad2D", "ODE", G, k, False) for G, k in RPGD_CASES]
                         + [("CartPole", "MLP", 3, 24, False), ("CartPole", "MLP", 8, 24, False),
                            ("CartPole", "ODE", 3, 24, True), ("Quad2D", "ODE", 4, 61, True)])
def test_rpgd_shards_equal_one_handle(envname, kind, G, k, philox):
    C, S, s = ENVS[envname]["C"], ENVS[envname]["S"], ENVS[envname]["s0"].copy()
    N = G * NL_RPGD
    w = O.mlp_default_weights(3) if kind == "MLP" else None
    pred, env = plant(envname, kind, w)
    kw = dict(rpgd_kw(envname, k, 0, its=2), kind=kind, env=env, weights=w, seed=21)
    full = engine("rpgd", envname, N, **kw)
    sh = [engine("rpgd", envname, NL_RPGD, **dict(kw, global_rollout_offset=i * NL_RPGD)) for i in range(G)]
    H = full.H
    P = full.inducing_points()
    rng = np.random.default_rng(G * 100 + k)
    d0 = None if philox else rng.random((N, P, C), dtype=np.float32)
    full.reset(d0)
    for i, e in enumerate(sh):
        e.reset(None if philox else d0[i * NL_RPGD:(i + 1) * NL_RPGD])
    np.testing.assert_array_equal(np.concatenate([e.read("PLAN") for e in sh]), full.read("PLAN"))
    rec = sh[0].rpgd_keepers_size()
    assert rec == min(k, NL_RPGD) * (3 + 3 * H * C)
    buf = device_buffer(G * rec)
    for t in range(3):
        resample = t % 2 == 0
        fresh = [e.rpgd_fresh_rows(G) for e in sh]
        assert fresh == [R.rpgd_fresh_rows_ref(k, G, NL_RPGD, i * NL_RPGD, resample) for i in range(G)]
        dr = rng.random((N - k, P, C), dtype=np.float32) if (resample and not philox and N > k) else None
        u_full = full.step(s, dr)
        for i, e in enumerate(sh):
            e.rpgd_step_begin(s, buf.data_ptr() + 4 * i * rec)
        sync()
        us = [e.rpgd_step_end(buf.data_ptr(), G, None if (dr is None or fresh[i] == 0) else dr[i * NL_RPGD: i * NL_RPGD + fresh[i]])
              for i, e in enumerate(sh)]
        for u in us[1:]:
            np.testing.assert_array_equal(u, us[0])
        tag = f"shards rpgd {envname} {kind} G={G} k={k} step {t}"
        # test_sharded_rpgd_two_shards_equal_one_handle: rtol 1e-6 / atol 1e-7 on u and on the concatenated population
        close(tag, "u", us[0], u_full, **RPGD_TOL)
        for name in ("PLAN", "ADAM_M", "ADAM_V", "AGES"):
            close(tag, name, np.concatenate([e.read(name) for e in sh]), full.read(name), **RPGD_TOL)
        s = pred.step(s.reshape(1, S), u_full.reshape(1, C))[0]
    for e in sh + [full]:
        e.close()


# =====================================================================================================================================
# c. refusals: the documented error, and the state vector as it was
# =====================================================================================================================================
def refused(e, exc, match, call):
    before = e.get_state()
    with pytest.raises(exc, match=match):
        call()
    np.testing.assert_array_equal(e.get_state(), before)


def test_mppi_shard_calls_out_of_order_are_refused():
    e = engine("mppi", "CartPole", 64, mpc_horizon=12, period_interpolation_inducing_points=5)
    buf = device_buffer(e.mppi_partial_size())
    s0 = ENVS["CartPole"]["s0"]
    refused(e, CtkError, "no sharded step pending", lambda: e.mppi_step_end(buf.data_ptr(), 1))
    e.mppi_step_begin(s0, buf.data_ptr())
    refused(e, CtkError, "previous sharded step not ended", lambda: e.mppi_step_begin(s0, buf.data_ptr()))
    sync()
    assert np.isfinite(e.mppi_step_end(buf.data_ptr(), 1)).all()       # the pending step is still good
    e.close()


@pytest.mark.parametrize("opt", ["cem", "random_action"])
def test_topk_shard_calls_out_of_order_are_refused(opt):
    kw = dict(cem_outer_it=2, cem_best_k=5) if opt == "cem" else {}
    e = engine(opt, "CartPole", 64, mpc_horizon=6, **kw)
    buf = device_buffer(e.shard_candidates_size())
    s0 = ENVS["CartPole"]["s0"]
    refused(e, CtkError, "no iteration pending", lambda: e.shard_iter_end(buf.data_ptr(), 1))
    refused(e, CtkError, "no completed iteration", e.shard_finish)
    e.shard_iter_begin(s0, buf.data_ptr())
    refused(e, CtkError, "previous iteration not ended", lambda: e.shard_iter_begin(s0, buf.data_ptr()))
    refused(e, CtkError, "no completed iteration", e.shard_finish)     # an iteration is pending, none is complete
    sync()
    e.shard_iter_end(buf.data_ptr(), 1)
    assert np.isfinite(e.shard_finish()).all()
    e.close()


def test_rpgd_shard_calls_out_of_order_and_too_few_candidates_are_refused():
    e = engine("rpgd", "CartPole", NL_RPGD, **rpgd_kw("CartPole", 40, 0))       # global k = 40 > N_local: 16 records per shard
    e.reset()
    buf = device_buffer(3 * e.rpgd_keepers_size())
    s0 = ENVS["CartPole"]["s0"]
    refused(e, CtkError, "no sharded RPGD step pending", lambda: e.rpgd_step_end(buf.data_ptr(), 3))
    e.rpgd_step_begin(s0, buf.data_ptr())
    sync()
    refused(e, CtkError, "previous sharded step not ended", lambda: e.rpgd_step_begin(s0, buf.data_ptr()))
    # opt_keep_k 40 > n_ranks * min(k, N_local) = 2 * 16
    refused(e, ValueError, "opt_keep_k exceeds the gathered candidates", lambda: e.rpgd_step_end(buf.data_ptr(), 2))
    e.close()


def test_cem_shard_needs_best_k_within_its_own_rollouts():
    """K is global and N is local: a CEM shard cannot contribute more candidates than it has rollouts (include/ctk_hip.h: ctk_shard_*)"""
    with pytest.raises(ValueError, match="cem_best_k <= num_rollouts"):
        engine("cem", "CartPole", 32, mpc_horizon=6, cem_outer_it=1, cem_best_k=33)


def test_cem_gmm_handle_is_refused_by_the_shard_calls():
    e = engine("cem_gmm", "CartPole", 64, mpc_horizon=6, cem_outer_it=1, cem_best_k=8)
    buf = device_buffer(8 * 8)
    refused(e, CtkError, "CEM-GMM handle cannot be sharded", lambda: e.shard_iter_begin(ENVS["CartPole"]["s0"], buf.data_ptr()))
    e.close()
