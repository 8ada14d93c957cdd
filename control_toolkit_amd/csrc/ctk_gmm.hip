// ctk_gmm.hip — CEM with a two-component Gaussian-mixture sampling distribution
// (Optimizers/optimizer_cem_gmm_tf.py).  Everything around these kernels is the CEM machinery of
// ctk_sampled.hip: the affine rollouts evaluate the plans, ctk_select_topk orders the elites.
//   ctk_gmm_sample_plans   Q[n] = clip(mu_k + z[n] * std_k), k = component of rollout n            (:59-60)
//   ctk_gmm_labels / ctk_gmm_refit   two clusters seeded by the best two elites, refit, clip          (:72-92)
//   ctk_gmm_finish         shift both tables one step, repeating the last row; u = elite[0,0,:]      (:109-120)
// The mixture's Categorical has a scalar batch shape, so MixtureSameFamily.sample([N]) draws ONE component index
// per rollout and the whole [H,C] plan comes from that component — not one index per element.
// Mixture state, one allocation: mu[2][HC] | std[2][HC] | probs[2] (component-major: each table is a contiguous [H,C]).
#include "ctk_device.h"
#include "ctk_launch.h"

// Q[n,h,c] = clip(mu_k[h,c] + z[n,h,c] * std_k[h,c]); k = 0 iff uniform[n] < probs[0].
// On-device draws: the normals as ctk_sample_plans draws them (stream = a.stream_id), the uniform of row n = word 0 of
// the Philox block (row, 0, call, ustream).
__global__ __launch_bounds__(256) void ctk_gmm_sample_plans(RolloutArgs a, const float* __restrict__ normals,
                                                            const float* __restrict__ uniforms, const float* __restrict__ mix,
                                                            uint32_t ustream, float* __restrict__ Q) {
    const int H = a.H * a.C;                  // flat (step, input) columns of a row, as in ctk_sample_plans
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= a.N * H) return;
    const int n = gid / H, h = gid - n * H;
    const int c = h % a.C;
    float e, u01;
    if (normals != nullptr) {
        e = normals[gid];
        u01 = uniforms[n];
    } else {
        float d4[4];
        draw4(a, (uint32_t)(a.global_row0 + n), (uint32_t)(h >> 2), 0, d4);
        e = d4[h & 3];
        u01 = u32_unit_halfopen(philox4x32_10(U4{(uint32_t)(a.global_row0 + n), 0u, a.call, ustream}, a.seed_lo, a.seed_hi).x);
    }
    const int k = u01 < mix[4 * H] ? 0 : 1;
    const float* mu = mix + k * H;
    const float* sd = mix + (2 + k) * H;
    Q[gid] = fminf(fmaxf(mu[h] + e * sd[h], a.lo[c]), a.hi[c]);
}

// label of an elite (one thread): 0 iff ||q - e0|| <= ||q - e1|| (2-norm over the HC columns, compared after the square root as
// the reference compares norms; tf.argmin gives a tie to elite 0's cluster).  One thread per elite with a serial sum: the HC loads of
// a row are independent and K rows are in flight at once (measured against a wave per elite in profiles/r06_cem_gmm.txt).
CTK_DEV float gmm_label(const float* __restrict__ q, const float* e0, const float* e1, int HC) {
    float d0 = 0.0f, d1 = 0.0f;
    for (int j = 0; j < HC; ++j) {
        const float v = q[j], a0 = v - e0[j], a1 = v - e1[j];
        d0 += a0 * a0;
        d1 += a1 * a1;
    }
    return sqrtf(d0) <= sqrtf(d1) ? 0.0f : 1.0f;
}

// the two-launch form's first launch (K labels do not fit the refit's LDS budget): labels to global memory
__global__ __launch_bounds__(256) void ctk_gmm_labels(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int K, int HC,
                                                      float* __restrict__ label) {
    const int kk = blockIdx.x * 256 + threadIdx.x;
    if (kk >= K) return;
    label[kk] = kk < 2 ? (float)kk : gmm_label(Q + (size_t)idx[kk] * ldq, Q + (size_t)idx[0] * ldq, Q + (size_t)idx[1] * ldq, HC);
}

// One block per column h.  LABELS_IN_LDS: every block first recomputes all K labels into LDS (the two seeds staged in LDS, K*HC
// loads out of L2: cheaper than a launch and a grid-wide wait), block 0 also writes them out; otherwise the labels come from
// ctk_gmm_labels.  LDS (floats): label[K] | seed 0 [HC] | seed 1 [HC].
// Then per cluster: count, mean, sum of squared deviations from that mean (mean first, as ctk_cem_refit), population std
// clipped to [std_min, std_max]; block 0 writes probs = (n0 / K, 1 - n0 / K).
template <bool LABELS_IN_LDS>
__global__ __launch_bounds__(256) void ctk_gmm_refit(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int K, int HC,
                                                     float* __restrict__ mix, float* __restrict__ label, float std_min, float std_max) {
    extern __shared__ float lab_s[];
    __shared__ float red[4][3];
    const int h = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const float* lab = label;
    if constexpr (LABELS_IN_LDS) {
        float* e_s = lab_s + K;
        const float* e0 = Q + (size_t)idx[0] * ldq;
        const float* e1 = Q + (size_t)idx[1] * ldq;
        for (int j = t; j < HC; j += 256) { e_s[j] = e0[j]; e_s[HC + j] = e1[j]; }
        __syncthreads();
        for (int kk = t; kk < K; kk += 256) {
            const float l = kk < 2 ? (float)kk : gmm_label(Q + (size_t)idx[kk] * ldq, e_s, e_s + HC, HC);
            lab_s[kk] = l;
            if (h == 0) label[kk] = l;
        }
        __syncthreads();
        lab = lab_s;
    }
    float s0 = 0.0f, s1 = 0.0f, c0 = 0.0f;
    for (int kk = t; kk < K; kk += 256) {
        const float q = Q[(size_t)idx[kk] * ldq + h];
        const bool first = lab[kk] == 0.0f;
        s0 += first ? q : 0.0f;
        s1 += first ? 0.0f : q;
        c0 += first ? 1.0f : 0.0f;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); c0 = wave_sum(c0);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = c0; }
    __syncthreads();
    const float n0 = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]), n1 = (float)K - n0;   // counts: exact in fp32
    const float mean0 = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) / n0;
    const float mean1 = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) / n1;
    __syncthreads();
    float v0 = 0.0f, v1 = 0.0f;
    for (int kk = t; kk < K; kk += 256) {
        const float q = Q[(size_t)idx[kk] * ldq + h];
        const bool first = lab[kk] == 0.0f;
        const float d = q - (first ? mean0 : mean1);
        v0 += first ? d * d : 0.0f;
        v1 += first ? 0.0f : d * d;
    }
    v0 = wave_sum(v0); v1 = wave_sum(v1);
    if (lane == 0) { red[wave][0] = v0; red[wave][1] = v1; }
    __syncthreads();
    if (t == 0) {
        mix[h] = mean0;
        mix[HC + h] = mean1;
        // tf.math.reduce_std: ddof = 0; the clip is part of every iteration here (:88-89)
        mix[2 * HC + h] = fminf(fmaxf(sqrtf((red[0][0] + red[1][0] + red[2][0] + red[3][0]) / n0), std_min), std_max);
        mix[3 * HC + h] = fminf(fmaxf(sqrtf((red[0][1] + red[1][1] + red[2][1] + red[3][1]) / n1), std_min), std_max);
        if (h == 0) {
            const float p = n0 / (float)K;
            mix[4 * HC] = p;
            mix[4 * HC + 1] = 1.0f - p;
        }
    }
}

// :109-120: mu and std of both components move one STEP (C floats) along the horizon and the last row is repeated
// (plain CEM refills the tail instead); probs stay.  u = first input of the best elite, published as ctk_g_cem_finish does.
__global__ __launch_bounds__(256) void ctk_gmm_finish(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int HC, int C,
                                                      float* __restrict__ mix, float* __restrict__ u_dev, float* __restrict__ u_host,
                                                      uint32_t seq) {
    extern __shared__ float old_s[];          // mu[2][HC] | std[2][HC]
    const int t = threadIdx.x;
    for (int i = t; i < 4 * HC; i += 256) old_s[i] = mix[i];
    __syncthreads();
    for (int i = t; i < 4 * HC; i += 256) {
        const int tab = i / HC, col = i - tab * HC;
        mix[i] = old_s[tab * HC + (col + C < HC ? col + C : col)];
    }
    if (t == 0) {
        float u[CTK_MAX_INPUTS];
        for (int c = 0; c < C; ++c) u[c] = Q[(size_t)idx[0] * ldq + c];
        publish_u_vec_launched(u_dev, u_host, u, C, seq);
    }
}

hipError_t ctk_launch_gmm_sample_plans(hipStream_t st, const RolloutArgs& a, const float* normals, const float* uniforms, const float* mix,
                                       uint32_t ustream, float* Q) {
    const int total = a.N * a.H * a.C;
    hipLaunchKernelGGL(ctk_gmm_sample_plans, dim3((total + 255) / 256), dim3(256), 0, st, a, normals, uniforms, mix, ustream, Q);
    return hipGetLastError();
}

bool ctk_gmm_refit_one_launch(int K, int HC) { return K + 2 * HC <= CTK_GMM_LDS_MAX_FLOATS; }

hipError_t ctk_launch_gmm_refit(hipStream_t st, const float* Q, const int* idx, int K, int HC, float* mix, float* label, float std_min,
                                float std_max, int ldq, bool two_launches) {
    if (ctk_gmm_refit_one_launch(K, HC) && !two_launches) {
        hipLaunchKernelGGL(ctk_gmm_refit<true>, dim3(HC), dim3(256), (size_t)(K + 2 * HC) * sizeof(float), st, Q, ldq, idx, K, HC, mix, label, std_min,
                           std_max);
    } else {
        hipLaunchKernelGGL(ctk_gmm_labels, dim3((K + 255) / 256), dim3(256), 0, st, Q, ldq, idx, K, HC, label);
        hipLaunchKernelGGL(ctk_gmm_refit<false>, dim3(HC), dim3(256), 0, st, Q, ldq, idx, K, HC, mix, label, std_min, std_max);
    }
    return hipGetLastError();
}

hipError_t ctk_launch_gmm_finish(hipStream_t st, const float* Q, const int* idx, int HC, int C, float* mix, float* u_dev, float* u_host,
                                 uint32_t seq, int ldq) {
    hipLaunchKernelGGL(ctk_gmm_finish, dim3(1), dim3(256), (size_t)4 * HC * sizeof(float), st, Q, ldq, idx, HC, C, mix, u_dev, u_host, seq);
    return hipGetLastError();
}
