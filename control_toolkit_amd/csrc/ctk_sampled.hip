// ctk_sampled.hip — rollouts whose inputs are an affine map of per-step samples, and the
// selection / refit kernels around them:
//   CEM            Q = clip(mu[h] + eps[n,h]*std[h])          optimizer_cem_tf.py:64-66
//   random-action  Q = lo + u01[n,h]*(hi-lo)                  optimizer_random_action_tf.py:56-61
//   plain rollout  Q given (base 0, scale 1, no clip)         predictor.predict_core(s, Q)
// plus smallest-K selection under the total order (J, index) (tf.argsort at
// optimizer_cem_tf.py:73 / optimizer_rpgd.py:345 with ties fixed by index), the CEM elite
// refit (:77-78) and the post-loop shift (:99-102).
#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_mlp.h"
#include "ctk_gru.h"
#include "ctk_launch.h"
#include "ctk_affine_body.h"   // affine_rollout_body, its anatomy and LDS carve (also wrapped by ctk_batch_rollout.hip)

template <int ENV, int PRED, bool WTRAJ>
// (argument order: see ctk_mppi_rollout — the leading 14 dwords are preloaded into SGPRs at wave launch)
__global__ __launch_bounds__(SAMP_BLOCK) void ctk_affine_rollout(const float* __restrict__ samples, const float* __restrict__ base,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ wperm, int rng_kind, int N_, int H_,
                                                                 int P_, uint32_t pmagic_, RolloutArgs a_in, typename Env<ENV>::K k, BestArgs best) {
    affine_rollout_body<ENV, PRED, WTRAJ, false>(samples, base, scale, wperm, rng_kind, N_, H_, P_, pmagic_, a_in, k, best, nullptr, 0u);
}

// the same rollout drawing from the two-component mixture of a CEM-GMM handle (MIX above); mix = mu[2][HC] | std[2][HC] | probs[2]
template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(SAMP_BLOCK) void ctk_affine_rollout_mix(const float* __restrict__ normals, const float* __restrict__ mix,
                                                                     const float* __restrict__ uniforms, uint32_t ustream, int N_, int H_,
                                                                     int P_, uint32_t pmagic_, RolloutArgs a_in, typename Env<ENV>::K k) {
    const BestArgs none{nullptr, 0u, nullptr, nullptr, nullptr};
    affine_rollout_body<ENV, CTK_PRED_ODE, WTRAJ, true>(normals, mix, mix + 2 * P_, nullptr, 0, N_, H_, P_, pmagic_, a_in, k, none, uniforms, ustream);
}

// predictor.update(s, Q0) for the GRU (optimizer_mppi.py:195-197): one workgroup of four waves (the split
// step of ctk_gru.h); all 16 MFMA columns carry the same (s, u); wave 0's lanes of column 0 write the new
// hidden state back in place (table | hidden, see ctk_api.hip:permute_gru_weights).
__global__ __launch_bounds__(GRU_BLOCK) void ctk_gru_advance(float s0, float s1, float s2, float s3, const float* __restrict__ u_dev,
                                                             float u_val, float* __restrict__ wperm) {
    __shared__ __attribute__((aligned(16))) float ex[GRU_EX_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    float* hidden = wperm + GRU_TABLE_FLOATS;
    const GruW w = gru_load_weights(wperm, wave, lane);
    GruState st = gru_load_state(hidden, g);
    const float sv = g == 0 ? s0 : (g == 1 ? s1 : (g == 2 ? s2 : s3));
    const float u = u_dev ? *u_dev : u_val;
    (void)gru_step(w, st, sv, u, g, ex, wave, lane);   // its barriers order every wave's loads of `hidden` before the stores below
    if (wave == 0 && c == 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                hidden[16 * m + 4 * g + r] = st.h1[m][r];
                hidden[32 + 16 * m + 4 * g + r] = st.h2[m][r];
            }
    }
}

hipError_t ctk_launch_gru_advance(hipStream_t st, const float* s, const float* u_dev, float u_val, float* wperm) {
    hipLaunchKernelGGL(ctk_gru_advance, dim3(1), dim3(GRU_BLOCK), 0, st, s[0], s[1], s[2], s[3], u_dev, u_val, wperm);
    return hipGetLastError();
}

// The same advance for the GRU batch (include/ctk_hip.h: ctk_gru_batch_*), behind the rollout launches of a step: one workgroup per step
// record, ctk_gru_advance's statements around the record's state, its problem's own last output (desc[id].u_dev, which the step's
// rollout launch published) and its problem's block of wbase (ctk_gru.h: GRU_BATCH_BLOCK_FLOATS; table | hidden, as a handle's d_wperm).
// A problem appears in at most one record of a launch, so no two workgroups touch one hidden state; the fast-cosine word behind it stays.
__global__ __launch_bounds__(GRU_BLOCK) void ctk_gru_advance_batch(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                   float* __restrict__ wbase) {
    __shared__ __attribute__((aligned(16))) float ex[GRU_EX_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const CtkBatchStep& q = steps[blockIdx.x];
    float* wperm = wbase + (size_t)q.id * GRU_BATCH_BLOCK_FLOATS;
    float* hidden = wperm + GRU_TABLE_FLOATS;
    const GruW w = gru_load_weights(wperm, wave, lane);
    GruState st = gru_load_state(hidden, g);
    const float sv = g == 0 ? q.s[0] : (g == 1 ? q.s[1] : (g == 2 ? q.s[2] : q.s[3]));
    const float u = *desc[q.id].u_dev;
    (void)gru_step(w, st, sv, u, g, ex, wave, lane);   // its barriers order every wave's loads of `hidden` before the stores below
    if (wave == 0 && c == 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                hidden[16 * m + 4 * g + r] = st.h1[m][r];
                hidden[32 + 16 * m + 4 * g + r] = st.h2[m][r];
            }
    }
}

hipError_t ctk_launch_gru_advance_batch(hipStream_t st, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_records, float* w_dev) {
    if (n_records < 1 || w_dev == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctk_gru_advance_batch, dim3(n_records), dim3(GRU_BLOCK), 0, st, desc_dev, steps_dev, w_dev);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// rank-by-counting selection: rank(i) = #{ j : (J_j, j) < (J_i, i) }, a permutation under the total
// order (cost, index), so idx_out[rank] = i for rank < K is a race-free scatter and idx_out comes
// out sorted ascending — what tf.argsort gives, ties fixed by index.
// Work N^2 comparisons, spread over N/16 blocks x 16 waves (256 blocks at N = 4096: the whole
// chip): a block owns 16 rows; wave w scans the j-slice [w*L, (w+1)*L); lane (r = lane & 15,
// q = lane >> 4) compares row r against the j = 4t + q of the slice, the slice staged in LDS as
// sortable 32-bit keys (coalesced load; 4 distinct addresses per LDS read, broadcast within 16 lanes).
// ---------------------------------------------------------------------------------------------
constexpr int SEL_WAVES = 16;
constexpr int SEL_ROWS = 16;
constexpr int SEL_CHUNK = 1024;   // keys per wave and pass (LDS: 16 waves x 1024 x 4 B = 64 KiB)


// J_i = J[i * ldj] (ldj = 1 for a plain cost vector; candidate records of the sharded path are strided)
__global__ __launch_bounds__(64 * SEL_WAVES) void ctk_select_topk(const float* __restrict__ J, int ldj, int N, int K,
                                                                  int* __restrict__ idx_out) {
    __shared__ uint32_t key_s[SEL_WAVES][SEL_CHUNK];
    __shared__ int cnt_s[SEL_WAVES][SEL_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int i = blockIdx.x * SEL_ROWS + r;
    const uint32_t ki = f32_sortable((i < N) ? J[(size_t)i * ldj] : INFINITY);
    const int L = (N + SEL_WAVES - 1) / SEL_WAVES;
    const int j0 = wave * L, j1 = min(N, j0 + L);
    int cnt = 0;
    for (int jb = j0; jb < j1; jb += SEL_CHUNK) {
        const int n = min(SEL_CHUNK, j1 - jb);
        for (int t = lane; t < n; t += 64) key_s[wave][t] = f32_sortable(J[(size_t)(jb + t) * ldj]);
        // wave-private slice: LDS ops of one wave complete in order, no barrier needed
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        for (int t = q; t < n; t += 4) {
            const uint32_t kj = key_s[wave][t];
            const int j = jb + t;
            cnt += (kj < ki) | ((kj == ki) & (j < i));
        }
    }
    cnt += __shfl_xor(cnt, 16, 64);
    cnt += __shfl_xor(cnt, 32, 64);
    if (lane < SEL_ROWS) cnt_s[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && lane < SEL_ROWS && i < N) {
        int rk = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) rk += cnt_s[w][lane];
        if (rk < K) idx_out[rk] = i;
    }
}

// elite refit: one block per horizon step h; mu = mean_k Q[idx[k],h]; sd = population std.
// Q row r = Q[r * ldq .. + H) (ldq = H for the plan matrix; 2+H with Q pointing at column 2 of candidate records)
__global__ __launch_bounds__(256) void ctk_cem_refit(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int K, int H,
                                                     float* __restrict__ mu, float* __restrict__ sd) {
    __shared__ float red[4];
    const int h = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    float s = 0.0f;
    for (int kk = t; kk < K; kk += 256) s += Q[(size_t)idx[kk] * ldq + h];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)K;
    __syncthreads();
    float v = 0.0f;
    for (int kk = t; kk < K; kk += 256) {
        const float d = Q[(size_t)idx[kk] * ldq + h] - mean;
        v += d * d;
    }
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (t == 0) {
        mu[h] = mean;
        sd[h] = sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K);   // tf.math.reduce_std: ddof = 0
    }
}

// plans of a CEM-with-gradient iteration, without rolling them out (the descent kernel does that)
__global__ __launch_bounds__(256) void ctk_sample_plans(RolloutArgs a, const float* __restrict__ samples,
                                                        const float* __restrict__ mu, const float* __restrict__ sd,
                                                        float* __restrict__ Q) {
    const int H = a.H * a.C;                  // a row of [N,H,C] is H*C contiguous floats; h below is the flat (step, input) column
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= a.N * H) return;
    const int n = gid / H, h = gid - n * H;   // gid ranges over N*H: beyond the exactness range of the p_magic trick
    const int c = h % a.C;
    float e;
    if (samples != nullptr) {
        e = samples[gid];
    } else {
        float d4[4];
        draw4(a, (uint32_t)(a.global_row0 + n), (uint32_t)(h >> 2), 0, d4);
        e = d4[h & 3];
    }
    Q[gid] = fminf(fmaxf(mu[h] + e * sd[h], a.lo[c]), a.hi[c]);
}

hipError_t ctk_launch_sample_plans(hipStream_t st, const RolloutArgs& a, const float* samples, const float* mu, const float* sd, float* Q) {
    const int total = a.N * a.H * a.C;
    hipLaunchKernelGGL(ctk_sample_plans, dim3((total + 255) / 256), dim3(256), 0, st, a, samples, mu, sd, Q);
    return hipGetLastError();
}

// population of one cem-grad-bharadhwaj iteration (optimizer_cem_grad_bharadhwaj_tf.py:94-97):
// rows [0,K) = the elites (first iteration: fresh samples, :158; afterwards the previous iteration's best K of
// the refined population, :118-119), rows [K,N) = fresh samples mu + std*eps; everything clipped.
__global__ __launch_bounds__(256) void ctk_cem_build_population(RolloutArgs a, int K, int first, const float* __restrict__ Q_prev,
                                                                const int* __restrict__ idx, const float* __restrict__ eps_elite,
                                                                const float* __restrict__ eps_rest, const float* __restrict__ mu,
                                                                const float* __restrict__ sd, float* __restrict__ Q) {
    const int H = a.H * a.C;                  // flat (step, input) columns of a row, as in ctk_sample_plans
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= a.N * H) return;
    const int n = gid / H, h = gid - n * H;   // gid ranges over N*H: beyond the exactness range of the p_magic trick
    const int c = h % a.C;
    float q;
    if (n < K && !first) {
        q = Q_prev[(size_t)idx[n] * H + h];
    } else {
        const float* src = n < K ? eps_elite : eps_rest;
        float e;
        if (src != nullptr) {
            e = src[(size_t)(n < K ? n : n - K) * H + h];
        } else {   // Philox: stream_id separates the iterations, elites of the first iteration use the same row space
            float d4[4];
            draw4(a, (uint32_t)(a.global_row0 + n), (uint32_t)(h >> 2), 0, d4);
            e = d4[h & 3];
        }
        q = mu[h] + sd[h] * e;                                   // :122-128
    }
    Q[gid] = fminf(fmaxf(q, a.lo[c]), a.hi[c]);                        // :96
}

hipError_t ctk_launch_cem_build_population(hipStream_t st, const RolloutArgs& a, int K, int first, const float* Q_prev, const int* idx,
                                           const float* eps_elite, const float* eps_rest, const float* mu, const float* sd, float* Q) {
    const int total = a.N * a.H * a.C;
    hipLaunchKernelGGL(ctk_cem_build_population, dim3((total + 255) / 256), dim3(256), 0, st, a, K, first, Q_prev, idx, eps_elite, eps_rest,
                       mu, sd, Q);
    return hipGetLastError();
}

// sharded selection: this shard's best K plans as records {J, global index (int bits), Q[H]},
// sorted ascending by (J, index) — what is all-gathered; the global top-K is the top-K of their union.
__global__ __launch_bounds__(256) void ctk_pack_candidates(const float* __restrict__ J, const float* __restrict__ Q,
                                                           const int* __restrict__ idx, int K, int H, int global_offset,
                                                           float* __restrict__ cand) {
    const int rs = 2 + H;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K * rs; i += gridDim.x * blockDim.x) {
        const int kk = i / rs, f = i - kk * rs, src = idx[kk];
        float v;
        if (f == 0) v = J[src];
        else if (f == 1) v = __builtin_bit_cast(float, global_offset + src);
        else v = Q[(size_t)src * H + (f - 2)];
        cand[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// step log: four contiguous copies in one launch; blockIdx.y selects the job, float4 body + scalar tail
struct CopyJobs { CopyJob j[4]; };
__global__ __launch_bounds__(256) void ctk_log_copy(CopyJobs jobs) {
    const CopyJob job = jobs.j[blockIdx.y];
    const unsigned n = job.n;
    const unsigned tid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (((reinterpret_cast<uintptr_t>(job.src) | reinterpret_cast<uintptr_t>(job.dst)) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(job.src);
        float4* d4 = reinterpret_cast<float4*>(job.dst);
        const unsigned n4 = n >> 2;
        for (unsigned i = tid; i < n4; i += stride) d4[i] = s4[i];
        for (unsigned i = (n4 << 2) + tid; i < n; i += stride) job.dst[i] = job.src[i];
    } else {
        for (unsigned i = tid; i < n; i += stride) job.dst[i] = job.src[i];
    }
}

hipError_t ctk_launch_copy4(hipStream_t st, const CopyJob (&jobs)[4]) {
    CopyJobs cj;
    unsigned nmax = 0;
    for (int i = 0; i < 4; ++i) { cj.j[i] = jobs[i]; nmax = jobs[i].n > nmax ? jobs[i].n : nmax; }
    if (nmax == 0) return hipSuccess;
    unsigned blocks = (nmax / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks);
    hipLaunchKernelGGL(ctk_log_copy, dim3(blocks, 4), dim3(256), 0, st, cj);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// template arguments <environment, predictor, materialise>
const char* ctk_affine_rollout_name(int pred, bool log) {
    if (pred == CTK_PRED_ODE) return log ? "ctk_affine_rollout<0, 0, true>" : "ctk_affine_rollout<0, 0, false>";
    if (pred == CTK_PRED_GRU) return log ? "ctk_affine_rollout<0, 2, true>" : "ctk_affine_rollout<0, 2, false>";
    return log ? "ctk_affine_rollout<0, 1, true>" : "ctk_affine_rollout<0, 1, false>";
}
const char* ctk_affine_rollout_env_name(int env, bool log) {
    return ctk_kernel_name("ctk_affine_rollout<%d, 0, %4$s>", env, 0, 0, log ? "true" : "false");
}

// one launch of ctk_affine_rollout<ENV, PRED, log>: `a` as the kernel takes it (a.P sample columns per row, a.p_magic their divisor);
// bst (analytic predictor only): the in-launch arg-min tail
template <int ENV, int PRED>
static void launch_affine(hipStream_t st, dim3 grid, size_t lds, const RolloutArgs& a, const typename Env<ENV>::K& k, const float* samples, int rng_kind,
                          const float* base, const float* scale, const float* wperm, bool log, hipEvent_t e0, hipEvent_t e1, const AffineBest* bst) {
    BestArgs bargs{nullptr, 0u, nullptr, nullptr, nullptr};
    if (bst && bst->ll) bargs = BestArgs{bst->ll, bst->seq, bst->u_dev, bst->u_host, bst->idx_out};
    ctk_with_bool(log, [&](auto log_c) {
        CTK_LAUNCH((ctk_affine_rollout<ENV, PRED, decltype(log_c)::value>), grid, dim3(SAMP_BLOCK), lds, st, e0, e1, samples, base, scale, wperm, rng_kind,
                   a.N, a.H, a.P, a.p_magic, a, k, bargs);
    });
}

// CartPole, any predictor: `a` and the cached constants `k` are the handle's
hipError_t ctk_launch_affine_rollout(hipStream_t st, int pred, const RolloutArgs& a, const EnvK& k, const float* samples,
                                     int rng_kind, const float* base, const float* scale, const float* wperm, bool log,
                                     hipEvent_t e0, hipEvent_t e1, const AffineBest* bst) {
    const dim3 grid(ctk_affine_rollout_blocks(pred, a.N));
    const size_t lds = ctk_affine_rollout_lds(a.H, pred);
    if (pred == CTK_PRED_ODE) launch_affine<CTK_ENV_CARTPOLE, CTK_PRED_ODE>(st, grid, lds, a, k, samples, rng_kind, base, scale, wperm, log, e0, e1, bst);
    else if (pred == CTK_PRED_MLP) launch_affine<CTK_ENV_CARTPOLE, CTK_PRED_MLP>(st, grid, lds, a, k, samples, rng_kind, base, scale, wperm, log, e0, e1, nullptr);
    else launch_affine<CTK_ENV_CARTPOLE, CTK_PRED_GRU>(st, grid, lds, a, k, samples, rng_kind, base, scale, wperm, log, e0, e1, nullptr);
    return hipGetLastError();
}

// The same 4-wave kernel for any environment's analytic predictor: a.H steps, a.C inputs (a.lo / a.hi per input); samples
// [N, H, C] or nullptr (Philox over the flat columns); base / scale [H*C]; bst as above with 2 + C words per workgroup.
hipError_t ctk_launch_affine_rollout_env(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a_in,
                                         const float* samples, int rng_kind, const float* base, const float* scale, bool log,
                                         hipEvent_t e0, hipEvent_t e1, const AffineBest* bst) {
    const dim3 grid(ctk_affine_rollout_blocks(CTK_PRED_ODE, a_in.N));
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        launch_affine<EV, CTK_PRED_ODE>(st, grid, ctk_affine_rollout_env_lds(EV, a_in.H), ctk_rollout_args(a_in, E::C, a_in.H * E::C),
                                        E::derive(params, dt, isteps), samples, rng_kind, base, scale, nullptr, log, e0, e1, bst);
    });
    return hipGetLastError();
}
// CEM-GMM, analytic predictor of any environment: sampling from the mixture inside the rollout (no plan pass, no extra launch)
const char* ctk_affine_rollout_mix_name(int env, bool log) { return ctk_kernel_name("ctk_affine_rollout_mix<%d, %4$s>", env, 0, 0, log ? "true" : "false"); }
size_t ctk_affine_rollout_mix_lds(int env, int H) {
    int C = 1;
    CTK_FOR_ENV(env, EV, { C = Env<EV>::C; });
    return (size_t)(affine_carve_floats(H * C, SAMP_TRAJ) + 2 * H * C) * sizeof(float);
}
hipError_t ctk_launch_affine_rollout_mix(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a_in,
                                         const float* normals, const float* uniforms, const float* mix, uint32_t ustream, bool log,
                                         hipEvent_t e0, hipEvent_t e1) {
    const dim3 grid(ctk_affine_rollout_blocks(CTK_PRED_ODE, a_in.N)), block(SAMP_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const RolloutArgs a = ctk_rollout_args(a_in, E::C, a_in.H * E::C);
        const typename E::K k = E::derive(params, dt, isteps);
        const size_t lds = ctk_affine_rollout_mix_lds(EV, a.H);
        ctk_with_bool(log, [&](auto log_c) {
            CTK_LAUNCH((ctk_affine_rollout_mix<EV, decltype(log_c)::value>), grid, block, lds, st, e0, e1, normals, mix, uniforms, ustream, a.N, a.H, a.P,
                       a.p_magic, a, k);
        });
    });
    return hipGetLastError();
}
size_t ctk_affine_rollout_env_lds(int env, int H) {
    int C = 1;
    CTK_FOR_ENV(env, EV, { C = Env<EV>::C; });
    return (size_t)affine_carve_floats(H * C, SAMP_TRAJ) * sizeof(float);
}

int ctk_affine_rollout_blocks(int pred, int N) { const int tr = affine_traj(pred); return (N + tr - 1) / tr; }

size_t ctk_affine_rollout_lds(int H, int pred) {
    return (size_t)(affine_carve_floats(H, affine_traj(pred)) + (pred == CTK_PRED_GRU ? GRU_EX_FLOATS : 0)) * sizeof(float);
}

hipError_t ctk_launch_select_topk(hipStream_t st, const float* J, int N, int K, int* idx_out, int ldj) {
    hipLaunchKernelGGL(ctk_select_topk, dim3((N + SEL_ROWS - 1) / SEL_ROWS), dim3(64 * SEL_WAVES), 0, st, J, ldj, N, K, idx_out);
    return hipGetLastError();
}

hipError_t ctk_launch_cem_refit(hipStream_t st, const float* Q, const int* idx, int K, int H, float* mu, float* sd, int ldq) {
    hipLaunchKernelGGL(ctk_cem_refit, dim3(H), dim3(256), 0, st, Q, ldq, idx, K, H, mu, sd);
    return hipGetLastError();
}

hipError_t ctk_launch_pack_candidates(hipStream_t st, const float* J, const float* Q, const int* idx, int K, int H, int global_offset,
                                      float* cand) {
    const int total = K * (2 + H);
    hipLaunchKernelGGL(ctk_pack_candidates, dim3((total + 255) / 256 > 64 ? 64 : (total + 255) / 256), dim3(256), 0, st, J, Q, idx, K, H,
                       global_offset, cand);
    return hipGetLastError();
}
