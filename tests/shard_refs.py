"""Float64 NumPy statements of the three record merges behind the sharded entry points, written from the record layouts and formulas
documented in include/ctk_hip.h (ctk_mppi_step_end, ctk_shard_iter_end / ctk_shard_finish, ctk_rpgd_step_end) — not from the kernels.

  MPPI partial record   {rho_r, a_r, b_r[P*C]}                       b column i*C + c = inducing point i of input c
  best-K candidate      {J, global index (int32 bits), Q[H*C]}
  RPGD keeper           {J, global index (int32 bits), age, Q[H*C], m[H*C], v[H*C]}

tests/test_shard_refs_cpu.py holds them against the pinned oracle; tests/test_gpu_shards.py holds the device against them on records
the test wrote itself."""
import numpy as np


def mppi_end_ref(parts, u_nom_in, interp, lam, lo, hi):
    """parts [n, 2+P*C]; u_nom_in [H, C]; interp [P, H, C] (oracle.interpolation_matrix); lam = LBD; lo / hi scalars or [C].
    rho = min rho_r; w_r = exp(-(rho_r - rho)/lam); a = sum a_r w_r; b = sum b_r w_r;
    u_nom_out[h] = clip(u_nom_in[min(h+1, H-1)] + interp(b)[h] / a, lo, hi); u = u_nom_out[0].  Returns (u_nom_out [H, C], u [C])."""
    parts = np.asarray(parts, np.float64)
    u_nom_in = np.asarray(u_nom_in, np.float64)
    M = np.asarray(interp, np.float64)
    P, H, C = M.shape
    assert parts.ndim == 2 and parts.shape[1] == 2 + P * C and u_nom_in.shape == (H, C)
    rho = parts[:, 0].min()
    w = np.exp(-(parts[:, 0] - rho) / float(lam))
    a = np.sum(parts[:, 1] * w)
    b = np.sum(parts[:, 2:] * w[:, None], axis=0).reshape(P, C)
    shifted = u_nom_in[np.minimum(np.arange(H) + 1, H - 1)]
    out = np.clip(shifted + np.einsum("pc,phc->hc", b, M) / a, np.asarray(lo, np.float64), np.asarray(hi, np.float64))
    return out, out[0].copy()


def topk_refit_ref(cands, K):
    """cands [M, 2+H*C]: idx = first K of the stable argsort of the cost column (ties by position); mu = mean of the K plans,
    sd = their population std (ddof 0).  Returns (idx [K], mu [H*C], sd [H*C]); K = 1 is the random-action pick."""
    cands = np.asarray(cands)
    idx = np.argsort(cands[:, 0], kind="stable")[:K]
    plans = np.asarray(cands[idx, 2:], np.float64)
    return idx, plans.mean(axis=0), plans.std(axis=0)


def cem_finish_ref(mu, sd, H, C, std_min, init_std, lo, hi, std_max=1.0e8):
    """the post-loop of CEM as O.CEM.step states it: clip sd to [std_min, std_max], shift mu and sd by one step, refill the tail
    with the mid-range input / the initial stdev.  mu, sd [H*C] -> ([H, C], [H, C])"""
    mu = np.asarray(mu, np.float64).reshape(H, C)
    sd = np.clip(np.asarray(sd, np.float64).reshape(H, C), std_min, std_max)
    mid = 0.5 * (np.broadcast_to(np.asarray(lo, np.float64), (C,)) + np.broadcast_to(np.asarray(hi, np.float64), (C,)))
    return np.concatenate([mu[1:], mid[None]], 0), np.concatenate([sd[1:], np.full((1, C), float(init_std))], 0)


def rpgd_fresh_rows_ref(k, n_ranks, N_local, offset, resample=True):
    """fresh rows of the shard at `offset`: clamp(first_keeper - offset, 0, N_local), first_keeper = n_ranks*N_local - k"""
    if not resample:
        return 0
    return int(min(max(n_ranks * N_local - k - offset, 0), N_local))


def rpgd_end_ref(recs, k, n_ranks, N_local, offset, resample, shift_previous, fresh_plans, C=1, own=None):
    """recs [M, 3+3*H*C], rank-major, each rank's list sorted.  Global sorted keeper list = first k of the stable argsort of the
    cost column; first_keeper = n_ranks*N_local - k.  Resampling step: shard row i (global row g = offset + i) is a fresh plan
    (fresh_plans [n_fresh, H, C], moments 0, age 0) if g < first_keeper, else keeper g - first_keeper: plan shifted by
    shift_previous with the last input repeated, moments shifted by ONE step and zero-filled, age kept.  Non-resampling step: the
    shard's own rows (own = (PLAN, ADAM_M, ADAM_V, AGES)) shifted the same way.  Then every age += 1.  u_nom = the plan of the
    globally best record, unshifted; u = its first input.
    Returns (PLAN, ADAM_M, ADAM_V [N_local, H, C], AGES [N_local], U_NOM [H, C], u [C], n_fresh)."""
    recs = np.asarray(recs, np.float64)
    HC = (recs.shape[1] - 3) // 3
    H = HC // C
    assert recs.shape[1] == 3 + 3 * HC and H * C == HC
    keep = np.argsort(recs[:, 0], kind="stable")[:k]
    sp = int(shift_previous)
    shift_q = lambda q: q[:, np.minimum(np.arange(H) + sp, H - 1)]
    shift_1 = lambda a: np.concatenate([a[:, 1:], np.zeros((a.shape[0], 1, C))], 1)
    u_nom = recs[keep[0], 3:3 + HC].reshape(H, C).copy()
    n_fresh = rpgd_fresh_rows_ref(k, n_ranks, N_local, offset, resample)
    if resample:
        first_keeper = n_ranks * N_local - k
        rows = keep[offset + np.arange(n_fresh, N_local) - first_keeper]           # keeper g - first_keeper for global row g
        fresh = np.zeros((0, H, C)) if n_fresh == 0 else np.asarray(fresh_plans, np.float64).reshape(n_fresh, H, C)
        z = np.zeros((n_fresh, H, C))
        Q = np.concatenate([fresh, shift_q(recs[rows, 3:3 + HC].reshape(-1, H, C))], 0)
        m = np.concatenate([z, shift_1(recs[rows, 3 + HC:3 + 2 * HC].reshape(-1, H, C))], 0)
        v = np.concatenate([z, shift_1(recs[rows, 3 + 2 * HC:].reshape(-1, H, C))], 0)
        ages = np.concatenate([np.zeros(n_fresh), recs[rows, 2]])
    else:
        Q0, m0, v0, a0 = (np.asarray(x, np.float64) for x in own)
        Q, m, v = shift_q(Q0.reshape(N_local, H, C)), shift_1(m0.reshape(N_local, H, C)), shift_1(v0.reshape(N_local, H, C))
        ages = a0.reshape(N_local).copy()
    return Q, m, v, ages + 1.0, u_nom, u_nom[0].copy(), n_fresh


# ---- record builders (what the *_begin calls leave behind, from plain arrays) ------------------------------------------------------
def index_bits(idx):
    """global indices as the records carry them: the int32 bit pattern in a float32 slot"""
    return np.asarray(idx, np.int32).view(np.float32)


def topk_records(J, Q, K, offset):
    """a shard's candidate list [min(K, N), 2+H*C]: its best K rows sorted by (J, index), with global indices"""
    J = np.asarray(J)
    best = np.argsort(J, kind="stable")[:K]
    rec = np.zeros((len(best), 2 + Q[0].size), np.float32)
    rec[:, 0] = J[best]
    rec[:, 1] = index_bits(best + offset)
    rec[:, 2:] = np.asarray(Q).reshape(len(J), -1)[best]
    return rec


def rpgd_records(J, Q, m, v, ages, k_local, offset):
    """a shard's keeper list [k_local, 3+3*H*C]: its best k_local rows sorted by (J, index)"""
    J = np.asarray(J)
    N = len(J)
    best = np.argsort(J, kind="stable")[:k_local]
    HC = np.asarray(Q).reshape(N, -1).shape[1]
    rec = np.zeros((len(best), 3 + 3 * HC), np.float32)
    rec[:, 0] = J[best]
    rec[:, 1] = index_bits(best + offset)
    rec[:, 2] = np.asarray(ages)[best]
    for j, a in enumerate((Q, m, v)):
        rec[:, 3 + j * HC:3 + (j + 1) * HC] = np.asarray(a).reshape(N, -1)[best]
    return rec
