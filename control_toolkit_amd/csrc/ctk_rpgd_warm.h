// ctk_rpgd_warm.h — the RPGD warm start (optimizer_rpgd.py:275-296, :377-379, :426, :449-516, :523) as device functions: one element of the
// new population (rpgd_warm_element) and the keep-k selection + warm start that a descent launch whose ONE workgroup holds the whole
// population runs as its tail (rpgd_fused_tail).  Shared by the CartPole kernels (ctk_rpgd.hip), the batch reset launch there and the
// batched template step (ctk_generic.hip: ctk_g_rpgd_batch).
#pragma once
#include "ctk_device.h"

constexpr int RPGD_TAIL_BLOCK = 256;   // threads of a workgroup that runs rpgd_fused_tail (RP_BLOCK, GR_BLOCK)

// ---------------------------------------------------------------------------------------------
// warm start / resampling / reset.  One thread per (row, h) of the NEW population.
//   new row i <  n_new : fresh sample (sample_actions :275-296), moments 0, age 0
//   new row i >= n_new : keeper idx[i - n_new] (or row i itself when gather == 0): plan shifted
//                        by shift_previous repeating the last input (:377-379), moments shifted by
//                        ONE and zero-filled (:465,:501), age kept; then every age += 1 (:514)
// ---------------------------------------------------------------------------------------------
struct WarmArgs {
    int N, H, P, n_new, gather, shift_previous, sampling_distribution, reset;
    float sample_stdev, sample_mean, sample_min, sample_max;   // sample_min/max < lo/hi only when sample_whole_control_space is off;
                                                               // otherwise the per-channel limits a.lo / a.hi are the range (whole_space)
    int whole_space;
    // sharded step: keepers and the best plan come from the all-gathered keeper records
    // {J, global index, age, Q[H], m[H], v[H]} instead of this handle's own rows
    const float* recs;     // nullptr: single-handle step
    int rs;                // record stride (3 + 3H)
    int keeper_base;       // index (in the global sorted keeper list) of the first keeper this shard hosts
    int fresh_tail;        // gradient_tf: the shifted-in tail input is a fresh U[lo,hi) draw per plan
                           // (optimizer_gradient_tf.py:137-144) instead of a repeat of the last input
};

// per-problem limits where they lie in device memory (ctk_g_rpgd_batch_hp): read as lim.lo[c] / lim.hi[c], like a RolloutArgs'.  A
// local copy indexed by a lane's c would live in scratch; these are loads from the element the host wrote, as the other forms' are
// loads from the kernel-argument segment
struct RpgdLimits { const float* lo; const float* hi; };

// pointers of one warm start (old population -> new population)
struct WarmPtrs {
    const float* draws; const int* idx; const float* Q_old; const float* m_old; const float* v_old; const float* ages_old;
    float* Q_new; float* m_new; float* v_new; float* ages_new; const InterpEntry* interp; float* u_nom; float* u_dev; float* u_host;
    uint32_t seq;
};

// element `gid` (= (row * H + h) * C + c) of the new population [N,H,C]; elements 0..H*C-1 also copy the best plan out and
// element 0 publishes u.  C = a.C control inputs: the reference's tensors are [N,H,C] throughout (optimizer_rpgd.py:275-296,
// :377-379, :454-513), a step is C contiguous floats.
// lim: whose limits lo / hi are read — a RolloutArgs (a itself; the batch kernels pass their shared kernel argument, see
// ctk_g_rpgd_body.inc) or, in the batch form with per-problem limits, two pointers into device memory (RpgdLimits)
template <class Lim>
CTK_DEV void rpgd_warm_element(const WarmArgs& w, const RolloutArgs& a, const Lim& lim, const WarmPtrs& p, int gid) {
    const float* __restrict__ draws = p.draws; const int* __restrict__ idx = p.idx;
    const float* __restrict__ Q_old = p.Q_old; const float* __restrict__ m_old = p.m_old; const float* __restrict__ v_old = p.v_old;
    const float* __restrict__ ages_old = p.ages_old;
    float* __restrict__ Q_new = p.Q_new; float* __restrict__ m_new = p.m_new; float* __restrict__ v_new = p.v_new;
    float* __restrict__ ages_new = p.ages_new; const InterpEntry* __restrict__ interp = p.interp;
    float* __restrict__ u_nom = p.u_nom; float* __restrict__ u_dev = p.u_dev; float* __restrict__ u_host = p.u_host;
    const uint32_t seq = p.seq;
    const int H = w.H, C = a.C, HC = H * C, PC = w.P * C;
    if (gid < w.N * HC) {
        const int i = gid / HC, hc = gid - i * HC, h = hc / C, c = hc - h * C;
        float q, mm = 0.0f, vv = 0.0f;
        if (i < w.n_new) {
            const InterpEntry e = interp[h];
            const float smin = w.whole_space ? lim.lo[c] : w.sample_min, smax = w.whole_space ? lim.hi[c] : w.sample_max;
            float y[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = min(e.i0 + j, w.P - 1) * C + c;      // column of the [P,C] draw block of this row
                float d;
                if (draws != nullptr) {
                    d = draws[(size_t)i * PC + col];
                } else {
                    float d4[4];
                    draw4(a, (uint32_t)(a.global_row0 + i), (uint32_t)(col >> 2), w.sampling_distribution == 0 ? 1 : 0, d4);
                    d = d4[col & 3];
                }
                const float raw = w.sampling_distribution == 0 ? d * (smax - smin) + smin                           // uniform
                                                                : d * w.sample_stdev + w.sample_mean;                // normal
                y[j] = fminf(fmaxf(raw, lim.lo[c]), lim.hi[c]);                                                          // :292
            }
            q = y[0] * e.w0 + (e.i0 + 1 < w.P ? y[1] * e.w1 : 0.0f);                                                 // :294
        } else if (w.gather && w.recs) {
            const float* rec = w.recs + (size_t)idx[w.keeper_base + i - w.n_new] * w.rs;
            const int hs = min(h + w.shift_previous, H - 1);
            q = rec[3 + hs * C + c];
            if (h + 1 < H) { mm = rec[3 + HC + hc + C]; vv = rec[3 + 2 * HC + hc + C]; }
        } else {
            const int src = w.gather ? idx[i - w.n_new] : i;
            const int hs = min(h + w.shift_previous, H - 1);
            q = Q_old[(size_t)src * HC + hs * C + c];
            if (w.fresh_tail && h + w.shift_previous >= H) {
                float d;
                if (draws != nullptr) {
                    d = draws[(size_t)i * C + c];
                } else {
                    float d4[4];
                    draw4(a, (uint32_t)(a.global_row0 + i), 0u, 1, d4);
                    d = d4[c & 3];
                }
                q = d * (lim.hi[c] - lim.lo[c]) + lim.lo[c];
            }
            if (h + 1 < H) { mm = m_old[(size_t)src * HC + hc + C]; vv = v_old[(size_t)src * HC + hc + C]; }
        }
        Q_new[gid] = q; m_new[gid] = mm; v_new[gid] = vv;
        if (hc == 0) {
            float age = 0.0f;
            if (i >= w.n_new) {
                if (w.gather && w.recs) age = w.recs[(size_t)idx[w.keeper_base + i - w.n_new] * w.rs + 2];
                else age = ages_old[w.gather ? idx[i - w.n_new] : i];
            }
            ages_new[i] = w.reset ? 0.0f : age + 1.0f;
        }
    }
    if (!w.reset && gid < HC) {
        // u_nom = Q_tf[best_idx[0]] BEFORE the warm start (:426)
        const float q = w.recs ? w.recs[(size_t)idx[0] * w.rs + 3 + gid] : Q_old[(size_t)idx[0] * HC + gid];
        u_nom[gid] = q;
        if (C == 1) {
            if (gid == 0) publish_u_launched(u_dev, u_host, q, seq);   // :523
        } else if (gid == 0) {
            // one thread publishes the whole input vector: u[c] first (floats 4..), then the {u[0], seq} word the host polls
            for (int cc = 0; cc < C; ++cc) {
                const float uc = w.recs ? w.recs[(size_t)idx[0] * w.rs + 3 + cc] : Q_old[(size_t)idx[0] * HC + cc];
                u_dev[cc] = uc;
                __hip_atomic_store(u_host + 4 + cc, uc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            host_words_drain();                      // the vector lands before the flag (ctk_device.h: publish_u_launched)
            const unsigned long long pv = ((unsigned long long)seq << 32) | (unsigned long long)__builtin_bit_cast(unsigned, q);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(u_host), pv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
CTK_DEV void rpgd_warm_element(const WarmArgs& w, const RolloutArgs& a, const WarmPtrs& p, int gid) { rpgd_warm_element(w, a, a, p, gid); }

// Single-workgroup RPGD step (N <= 64, the reference's default is 32): keep-k selection and the warm start run as the tail
// of the descent launch — the whole optimizer_rpgd.py:388-524 step in ONE launch instead of three.
struct FusedWarm {
    int enabled, K;
    int* idx_out;          // [K] best indices (ascending cost), as ctk_select_topk writes them
    WarmArgs w;
    WarmPtrs p;            // p.idx is ignored (the tail's own selection is used)
};

// keep-k selection + warm start as the tail of a descent launch whose ONE workgroup holds the whole population.  HC = H * a.C floats per
// plan; g_s: 128 dead words of LDS (the gradient tile, running into the clip scales behind it when HC == 1)
template <class Lim>
CTK_DEV void rpgd_fused_tail(const RolloutArgs& a, const Lim& lim, const FusedWarm& fw, float* g_s, int t, int HC) {
    __threadfence();
    __syncthreads();                                   // Q, m, v, J of this launch are visible to every thread of the block
    uint32_t* key_s = reinterpret_cast<uint32_t*>(g_s);   // g_s is dead: [64] keys, then [64] indices
    int* idx_s = reinterpret_cast<int*>(g_s) + 64;
    if (t < 64) {
        const float Jt = t < a.N ? __hip_atomic_load(a.J + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : INFINITY;
        const uint32_t u = __builtin_bit_cast(uint32_t, Jt);
        key_s[t] = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);   // order-preserving map (ctk_sampled.hip:f32_sortable)
    }
    __syncthreads();
    if (t < a.N) {                                      // rank under the total order (J, index): ctk_select_topk
        const uint32_t ki = key_s[t];
        int rk = 0;
        for (int j = 0; j < a.N; ++j) { const uint32_t kj = key_s[j]; rk += (kj < ki) | ((kj == ki) & (j < t)); }
        if (rk < fw.K) { idx_s[rk] = t; fw.idx_out[rk] = t; }
    }
    __syncthreads();
    WarmPtrs p = fw.p;
    p.idx = idx_s;
    for (int gid = t; gid < max(fw.w.N * HC, HC); gid += RPGD_TAIL_BLOCK) rpgd_warm_element(fw.w, a, lim, p, gid);
}
CTK_DEV void rpgd_fused_tail(const RolloutArgs& a, const FusedWarm& fw, float* g_s, int t, int HC) { rpgd_fused_tail(a, a, fw, g_s, t, HC); }
