// ctk_generic.hip — the environment-agnostic optimizer kernels: every template here is written against the
// Env<ID> interface of ctk_env.h only (S states, C control inputs, step / cost / adjoints), so the same code serves
// any plant the reference would select through predictor_specification / cost_function_specification
// (controller_mpc.py:67-82, cost_function_wrapper.py:59-66).  Shapes follow the reference: samples [N,P,C] / [N,H,C],
// plans Q [N,H,C], u_nom [H,C], trajectories [N,H+1,S]; a row of a [.,H,C] tensor is HC = H*C contiguous floats.
//
//   ctk_g_rollout<ENV, MODE, LOG>   one wave = 64 trajectories, one per lane, state in registers, the block's sample
//        tile staged in LDS by coalesced 16-B loads (or drawn by Philox), inputs formed inline:
//          MODE_MPPI    u = clip(shift(u_nom) + interp(stdev * noise))  + MPPI correction cost + block soft-min record
//                       {rho, a, b[P*C]}                                          (optimizer_mppi.py:154-193)
//          MODE_AFFINE  u = clip(base[h,c] + sample[n,h,c] * scale[h,c])           (CEM optimizer_cem_tf.py:64-66,
//                       random-action optimizer_random_action_tf.py:56-61, plain predict_core rollouts)
//   ctk_g_mppi_update<>             u_nom <- clip(shift(u_nom) + interp(b) / a) per input channel, u = u_nom[0,:]
//   ctk_g_cem_finish / ctk_g_pick_best_first   post-loop bookkeeping with C channels
//   ctk_g_rpgd_descent<ENV>         all Adam iterations of one MPC step in one launch: forward with a state tape,
//        reverse sweep through Env::step_vjp + cost gradients, per-plan clip_by_norm, Adam, clip, final cost pass
//        (optimizer_rpgd.py:306-338, :342)
//   ctk_g_rpgd_batch<ENV>           B independent RPGD problems of at most 64 plans, one workgroup each: the descent above (the same
//        text, ctk_g_rpgd_body.inc), then keep-k selection and warm start in the same launch (ctk_rpgd_warm.h)
//   ctk_g_rpgd_batch_pp<ENV>        the same with every problem's own derived constants, read from device memory behind the step records
// The block-record merge (ctk_mppi_merge<false>), the selection (ctk_select_topk), the refit (ctk_cem_refit) and the
// RPGD warm start are shared with the CartPole kernels: they only ever see P*C / H*C columns.
#include <type_traits>
#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_adam.h"
#include "ctk_rpgd_warm.h"
#include "ctk_launch.h"

// (G_TRAJ, trajectories per block, = CTK_G_TRAJ of ctk_launch.h)
constexpr int G_TRAJ = CTK_G_TRAJ;

// ---------------------------------------------------------------------------------------------------------------
// rollout + cost: the statements are ctk_g_rollout_body.inc, which ctk_batch_rollout.hip wraps a second time
// ---------------------------------------------------------------------------------------------------------------
template <int ENV, int MODE, bool LOG>
__global__ __launch_bounds__(G_TRAJ) void ctk_g_rollout(RolloutArgs a, typename Env<ENV>::K k, MppiK m, int cols_per_point,
                                                       const float* __restrict__ samples, const float* __restrict__ base,
                                                       const float* __restrict__ scale, int rng_kind, float* __restrict__ parts) {
#include "ctk_g_rollout_body.inc"
}

// u_nom <- clip(shift(u_nom) + interp(b) / a)  (optimizer_mppi.py:190), u = u_nom[0, :] (:191).
// parts: n_parts <= G_UPD_MAX_PARTS block (or shard) records {rho, a, b[P*C]}, merged here first — rho = min rho_r,
// a = sum a_r e^{-(rho_r - rho)/lambda}, b likewise (optimizer_mppi.py:163-168 re-associated, as ctk_mppi_merge) — so that the
// template path's MPPI step is two launches (rollout, this) instead of three.  LDS: w[n_parts] | b[P*C]
constexpr int G_UPD_MAX_PARTS = 1024;

template <int DUMMY>
__global__ __launch_bounds__(256) void ctk_g_mppi_update(const float* __restrict__ parts, int n_parts, float neg_inv_lbd, int P, int C, int H,
                                                        const InterpEntry* __restrict__ interp, const float* __restrict__ u_nom_in,
                                                        float* __restrict__ u_nom_out, RolloutArgs a, float* __restrict__ u_dev,
                                                        float* __restrict__ u_host, uint32_t seq) {
    extern __shared__ float lds[];
    __shared__ float u_s[CTK_MAX_INPUTS];
    __shared__ float red_s[4];
    const int PC = P * C, rs = 2 + PC, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    float* w_s = lds;                 // [n_parts]
    float* b_s = w_s + n_parts;       // [PC]
    float rho = INFINITY;
    for (int r = t; r < n_parts; r += 256) rho = fminf(rho, parts[(size_t)r * rs]);
    rho = wave_min(rho);
    if (lane == 0) red_s[wave] = rho;
    __syncthreads();
    rho = fminf(fminf(red_s[0], red_s[1]), fminf(red_s[2], red_s[3]));
    __syncthreads();
    float asum = 0.0f;
    for (int r = t; r < n_parts; r += 256) {
        const float w = expf(neg_inv_lbd * (parts[(size_t)r * rs] - rho));
        w_s[r] = w;
        asum += parts[(size_t)r * rs + 1] * w;
    }
    asum = wave_sum(asum);
    if (lane == 0) red_s[wave] = asum;
    __syncthreads();
    const float a_tot = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    for (int pc = t; pc < PC; pc += 256) {
        float acc = 0.0f;
        for (int r = 0; r < n_parts; ++r) acc += parts[(size_t)r * rs + 2 + pc] * w_s[r];
        b_s[pc] = acc;
    }
    __syncthreads();
    for (int hc = t; hc < H * C; hc += 256) {
        const int h = hc / C, c = hc - h * C;
        const InterpEntry e = interp[h];
        const int i1 = min(e.i0 + 1, P - 1);
        const float w = (b_s[e.i0 * C + c] * e.w0 + b_s[i1 * C + c] * e.w1) / a_tot;
        const float o = fminf(fmaxf(u_nom_in[min(h + 1, H - 1) * C + c] + w, a.lo[c]), a.hi[c]);
        u_nom_out[hc] = o;
        if (h == 0) u_s[c] = o;
    }
    __syncthreads();
    if (t == 0) publish_u_vec_launched(u_dev, u_host, u_s, C, seq);
}

// optimizer_cem_tf.py:99-102 with C channels: clip std, shift mean and std by one STEP (C floats), refill the tail with
// the mid-range / initial stdev; u = first input of the best elite (or of the mean: optimizer_cem_naive_grad_tf.py:103)
__global__ __launch_bounds__(256) void ctk_g_cem_finish(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int H, int C,
                                                       float* __restrict__ mu, float* __restrict__ sd, float std_min, float init_std,
                                                       RolloutArgs a, float* __restrict__ u_dev, float* __restrict__ u_host, uint32_t seq,
                                                       float std_max, int u_from_mu) {
    extern __shared__ float lds[];
    const int HC = H * C, t = threadIdx.x;
    float* m_s = lds;
    float* s_s = lds + HC;
    for (int i = t; i < HC; i += 256) {
        m_s[i] = mu[i];
        s_s[i] = fminf(fmaxf(sd[i], std_min), std_max);
    }
    __syncthreads();
    for (int i = t; i < HC; i += 256) {
        const int c = i % C;
        mu[i] = (i + C < HC) ? m_s[i + C] : (a.lo[c] + a.hi[c]) * 0.5f;
        sd[i] = (i + C < HC) ? s_s[i + C] : init_std;
    }
    if (t == 0) {
        float u[CTK_MAX_INPUTS];
        for (int c = 0; c < C; ++c) u[c] = u_from_mu ? m_s[c] : Q[(size_t)idx[0] * ldq + c];
        publish_u_vec_launched(u_dev, u_host, u, C, seq);
    }
}

__global__ void ctk_g_pick_best_first(const float* __restrict__ Q, int ldq, const int* __restrict__ idx, int C, float* __restrict__ u_dev,
                                      float* __restrict__ u_host, uint32_t seq) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float u[CTK_MAX_INPUTS];
        for (int c = 0; c < C; ++c) u[c] = Q[(size_t)idx[0] * ldq + c];
        publish_u_vec_launched(u_dev, u_host, u, C, seq);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// RPGD descent (optimizer_rpgd.py:306-338): a block keeps its 64 plans in LDS as [h*C+c][plan] (stride 65) across the
// iterations; wave 0 runs forward + reverse sweep (one plan per lane), all four waves do Adam with coalesced m/v traffic.
// Tape = the S state components entering every step ([h][i][lane], LDS when it fits, else global scratch); the reverse
// sweep recomputes a step's intermediates from them (Env::step_vjp).
// ---------------------------------------------------------------------------------------------------------------
constexpr int GR_WAVES = 4, GR_BLOCK = G_TRAJ * GR_WAVES, GR_LD = G_TRAJ + 1;

template <int ENV>
__global__ __launch_bounds__(GR_BLOCK) void ctk_g_rpgd_descent(RolloutArgs a, typename Env<ENV>::K k, AdamK ad, float* __restrict__ Q,
                                                              float* __restrict__ m, float* __restrict__ v,
                                                              const float* __restrict__ bc_table, int bc_len, int t0, int iters,
                                                              float* __restrict__ scratch, int tape_in_lds) {
    const RolloutArgs& lim = a;
#include "ctk_g_rpgd_body.inc"
}

// The batch form (include/ctk_hip.h: ctk_rpgd_batch_*): grid (1, problems of this launch), a problem's whole population in ONE workgroup
// (N <= 64, host-checked).  The prologue rebuilds ctk_g_rpgd_descent's arguments from the step record of blockIdx.y and the descriptor it
// names (both read-only, wave-uniform); the descent is the handle kernel's text; behind it comes what a template handle runs as two more
// launches, ctk_select_topk and ctk_rpgd_warmstart (rpgd_fused_tail: the fence and barrier make this launch's Q, m, v, J visible first).
// No workgroup waits for another.
static_assert(GR_BLOCK == RPGD_TAIL_BLOCK, "rpgd_fused_tail strides by the workgroup size");

template <int ENV>
__global__ __launch_bounds__(GR_BLOCK) void ctk_g_rpgd_batch(RolloutArgs a_tpl, typename Env<ENV>::K k, AdamK ad,
                                                            const float* __restrict__ bc_table, int bc_len, int tape_in_lds, FusedWarm fw_tpl,
                                                            const CtkRpgdBatchDesc* __restrict__ desc,
                                                            const CtkRpgdBatchStep* __restrict__ steps) {
#include "ctk_g_rpgd_batch_pro.inc"
#include "ctk_g_rpgd_body.inc"
#include "ctk_g_rpgd_batch_epi.inc"
}

// The PER-PROBLEM-PARAMETER form of the batch kernel (ctk_rpgd_problem_set_param): the same prologue, body and tail, but the derived
// constants `k` of the problem come from device memory instead of the by-value argument.  The host writes them BEHIND the step records, in
// the records' order (stride CtkBatchKStride<ENV>, derived with Env<ENV>::derive, as a handle's are), so they arrive with the records'
// transfer and element blockIdx.y of ksteps belongs to record blockIdx.y of steps — indexed by launch order, not by problem id.  The
// address depends on blockIdx.y alone: uniform, so the constants arrive by scalar loads like the record.  They are copied into a local K
// here, once, ahead of the body: the descent stores to Q / m / v through all its iterations, and nothing is left to be read again behind
// those stores.  No workgroup waits for another in this form either.
template <int ENV>
__global__ __launch_bounds__(GR_BLOCK) void ctk_g_rpgd_batch_pp(RolloutArgs a_tpl, const unsigned char* __restrict__ ksteps, AdamK ad,
                                                               const float* __restrict__ bc_table, int bc_len, int tape_in_lds, FusedWarm fw_tpl,
                                                               const CtkRpgdBatchDesc* __restrict__ desc,
                                                               const CtkRpgdBatchStep* __restrict__ steps) {
#include "ctk_g_rpgd_batch_pro.inc"
    const typename Env<ENV>::K k = *reinterpret_cast<const typename Env<ENV>::K*>(ksteps + (size_t)blockIdx.y * CtkBatchKStride<ENV>::value);
#include "ctk_g_rpgd_body.inc"
#include "ctk_g_rpgd_batch_epi.inc"
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------
size_t ctk_g_rollout_lds(int cols, int H, int C) {
    return (size_t)(G_TRAJ * tile_stride(cols) + G_TRAJ + 2 * H * C + 3 * H) * sizeof(float);
}

int ctk_g_rollout_blocks(int N) { return (N + G_TRAJ - 1) / G_TRAJ; }

const char* ctk_g_rollout_name(int env, int mode, bool log) {
    return ctk_kernel_name("ctk_g_rollout<%d, %d, %4$s>", env, mode == CTK_G_MODE_MPPI ? 0 : 1, 0, log ? "true" : "false");
}

hipError_t ctk_launch_g_rollout(hipStream_t st, int env, int mode, const RolloutArgs& a_in, const float* params, float dt, int isteps,
                                const MppiK& mk, const float* samples, const float* base, const float* scale, int rng_kind,
                                float* parts, bool log, hipEvent_t e0, hipEvent_t e1) {
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const int cols = (mode == CTK_G_MODE_MPPI ? a_in.P : a_in.H) * E::C;
        const RolloutArgs a = ctk_rollout_args(a_in, E::C, cols);
        const typename E::K k = E::derive(params, dt, isteps);
        const dim3 grid(ctk_g_rollout_blocks(a.N)), block(G_TRAJ);
        const size_t lds = ctk_g_rollout_lds(cols, a.H, E::C);
        ctk_with_bool(mode == CTK_G_MODE_MPPI, [&](auto mppi_c) {
            ctk_with_bool(log, [&](auto log_c) {
                constexpr int MODE = decltype(mppi_c)::value ? CTK_G_MODE_MPPI : CTK_G_MODE_AFFINE;
                CTK_LAUNCH((ctk_g_rollout<EV, MODE, decltype(log_c)::value>), grid, block, lds, st, e0, e1, a, k, mk, E::C, samples, base, scale,
                           rng_kind, parts);
            });
        });
    });
    return hipGetLastError();
}

int ctk_g_mppi_update_max_parts() { return G_UPD_MAX_PARTS; }

hipError_t ctk_launch_g_mppi_update(hipStream_t st, const float* parts, int n_parts, float neg_inv_lbd, int P, int C, int H,
                                    const InterpEntry* interp, const float* u_nom_in, float* u_nom_out, const RolloutArgs& a, float* u_dev,
                                    float* u_host, uint32_t seq) {
    hipLaunchKernelGGL(ctk_g_mppi_update<0>, dim3(1), dim3(256), (size_t)(n_parts + P * C) * sizeof(float), st, parts, n_parts, neg_inv_lbd, P, C, H,
                       interp, u_nom_in, u_nom_out, a, u_dev, u_host, seq);
    return hipGetLastError();
}

hipError_t ctk_launch_g_cem_finish(hipStream_t st, const float* Q, const int* idx, int H, int C, float* mu, float* sd, float std_min,
                                   float init_std, const RolloutArgs& a, float* u_dev, float* u_host, uint32_t seq, int ldq, float std_max,
                                   int u_from_mu) {
    hipLaunchKernelGGL(ctk_g_cem_finish, dim3(1), dim3(256), 2 * H * C * sizeof(float), st, Q, ldq, idx, H, C, mu, sd, std_min, init_std, a,
                       u_dev, u_host, seq, std_max, u_from_mu);
    return hipGetLastError();
}

hipError_t ctk_launch_g_pick_best_first(hipStream_t st, const float* Q, const int* idx, int C, float* u_dev, float* u_host, uint32_t seq,
                                        int ldq) {
    hipLaunchKernelGGL(ctk_g_pick_best_first, dim3(1), dim3(64), 0, st, Q, ldq, idx, C, u_dev, u_host, seq);
    return hipGetLastError();
}

static size_t g_rpgd_lds_base(int H, int C) { return (size_t)(2 * H * C * GR_LD + G_TRAJ) * sizeof(float); }

size_t ctk_g_rpgd_descent_lds(int env, int H, bool* tape_in_lds) {
    int NT = 0, C = 0;
    CTK_FOR_ENV(env, EV, { NT = Env<EV>::NT; C = Env<EV>::C; });
    const size_t base = g_rpgd_lds_base(H, C), tape = (size_t)H * NT * 64 * sizeof(float);
    const bool fits = base + tape <= 160 * 1024;
    if (tape_in_lds) *tape_in_lds = fits;
    return fits ? base + tape : base;
}

size_t ctk_g_rpgd_scratch_floats(int env, int N, int H) {
    int NT = 0;
    CTK_FOR_ENV(env, EV, { NT = Env<EV>::NT; });
    return (size_t)((N + G_TRAJ - 1) / G_TRAJ) * H * NT * 64;
}

static AdamK ctk_g_adam_k(float lr, float b1, float b2, float eps, float clip, int rule);   // below, with the _hp form's launcher
const char* ctk_g_rpgd_descent_name(int env) { return ctk_kernel_name("ctk_g_rpgd_descent<%d>", env); }

hipError_t ctk_launch_g_rpgd_descent(hipStream_t st, int env, const RolloutArgs& a_in, const float* params, float dt, int isteps, float lr,
                                     float b1, float b2, float eps, float clip, float* Q, float* m, float* v, const float* bc_table,
                                     int bc_len, int t0, int iters, float* scratch, hipEvent_t e0, hipEvent_t e1, int rule) {
    const AdamK ad = ctk_g_adam_k(lr, b1, b2, eps, clip, rule);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const RolloutArgs a = ctk_descent_args(a_in, E::C);
        const typename E::K k = E::derive(params, dt, isteps);
        bool tape_in_lds = false;
        const size_t lds = ctk_g_rpgd_descent_lds(env, a.H, &tape_in_lds);
        const dim3 grid((a.N + G_TRAJ - 1) / G_TRAJ), block(GR_BLOCK);
        CTK_LAUNCH((ctk_g_rpgd_descent<EV>), grid, block, lds, st, e0, e1, a, k, ad, Q, m, v, bc_table, bc_len, t0, iters, scratch,
                   tape_in_lds ? 1 : 0);
    });
    return hipGetLastError();
}


const char* ctk_g_rpgd_batch_name(int env, bool per_problem) {
    return ctk_kernel_name(per_problem ? "ctk_g_rpgd_batch_pp<%d>" : "ctk_g_rpgd_batch<%d>", env);
}

hipError_t ctk_launch_g_rpgd_batch(hipStream_t st, int env, const RolloutArgs& a_in, const float* params, float dt, int isteps, float lr,
                                   float b1, float b2, float eps, float clip, int rule, const float* bc_table, int bc_len,
                                   const RpgdFusedWarm& f, const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* steps_dev, int n_problems,
                                   const void* k_steps_dev) {
    const AdamK ad = ctk_g_adam_k(lr, b1, b2, eps, clip, rule);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const RolloutArgs a = ctk_descent_args(a_in, E::C);
        bool tape_in_lds = false;
        const size_t lds = ctk_g_rpgd_descent_lds(env, a.H, &tape_in_lds);
        FusedWarm fw{};
        fw.enabled = 1; fw.K = f.K;
        fw.w = WarmArgs{a.N, a.H, f.P, 0, 0, f.shift_previous, f.sampling_distribution, 0, f.sample_stdev, f.sample_mean, f.sample_min,
                        f.sample_max, f.whole_space, nullptr, 0, 0, 0};
        fw.p.interp = f.interp;
        const dim3 grid(1, n_problems), block(GR_BLOCK);
        if (k_steps_dev) {                             // per-problem constants: element j belongs to record j (ctk_mppi_batch_derive_k)
            hipLaunchKernelGGL((ctk_g_rpgd_batch_pp<EV>), grid, block, lds, st, a, static_cast<const unsigned char*>(k_steps_dev), ad, bc_table, bc_len,
                               tape_in_lds ? 1 : 0, fw, desc_dev, steps_dev);
        } else {
            const typename E::K k = E::derive(params, dt, isteps);
            hipLaunchKernelGGL((ctk_g_rpgd_batch<EV>), grid, block, lds, st, a, k, ad, bc_table, bc_len, tape_in_lds ? 1 : 0, fw, desc_dev, steps_dev);
        }
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The PER-PROBLEM-HYPER-PARAMETER form of the batched RPGD step (include/ctk_hip_family_hyper.h: ctk_rpgd_problem_set_hyper / _set_limits),
// defined LAST in this file with its launcher, so that every kernel that was here before keeps its text.  The prologue, body and tail
// of ctk_g_rpgd_batch_pp, statement for statement; ctk_g_rpgd_batch_hyp.inc takes, besides k, the problem's Adam constants, the address
// of the bias-correction table of its betas, its sampling constants and its limits from the SECOND part of the element behind the step
// records ([K | CtkRpgdBatchHyper], by record index as _pp's k).  No workgroup waits for another in this form either.
// ---------------------------------------------------------------------------------------------------------------
struct alignas(16) CtkRpgdBatchHyper {
    AdamK ad;                           // ctk_g_adam_k of the problem's learning_rate, betas, epsilon, clip and the batch's rule
    const float* bc_table;              // device table of the problem's (beta_1, beta_2): adam_bias_corrections, one per distinct pair
    uint64_t pad;
    float sample_stdev, sample_mean, sample_min, sample_max;
    float lo[CTK_MAX_INPUTS], hi[CTK_MAX_INPUTS];
};
static_assert(sizeof(AdamK) == 32 && sizeof(CtkRpgdBatchHyper) % 16 == 0, "the elements behind the step records stay 16-byte aligned");
template <int ENV>
struct CtkRpgdKhStride {
    static constexpr size_t value = CtkBatchKStride<ENV>::value + sizeof(CtkRpgdBatchHyper);
};

template <int ENV>
__global__ __launch_bounds__(GR_BLOCK) void ctk_g_rpgd_batch_hp(RolloutArgs a_tpl, const unsigned char* __restrict__ kh_steps, int bc_len, int tape_in_lds,
                                                               FusedWarm fw_tpl, const CtkRpgdBatchDesc* __restrict__ desc,
                                                               const CtkRpgdBatchStep* __restrict__ steps) {
#define CTK_RPGD_BATCH_HP
#include "ctk_g_rpgd_batch_pro.inc"
#include "ctk_g_rpgd_batch_hyp.inc"
#include "ctk_g_rpgd_body.inc"
#include "ctk_g_rpgd_batch_epi.inc"
#undef CTK_RPGD_BATCH_HP
}

// the Adam constants of every template launch (ctk_launch_g_rpgd_descent, ctk_launch_g_rpgd_batch) and of a problem's hyper block
static AdamK ctk_g_adam_k(float lr, float b1, float b2, float eps, float clip, int rule) {
    return AdamK{lr, b1, b2, (float)(1.0 - (double)b1), (float)(1.0 - (double)b2), eps, clip, rule};
}

size_t ctk_rpgd_batch_hyper_bytes() { return sizeof(CtkRpgdBatchHyper); }
size_t ctk_rpgd_batch_kh_stride(int env) {
    size_t stride = 0;
    CTK_FOR_ENV(env, EV, { stride = CtkRpgdKhStride<EV>::value; });
    return stride;
}
void ctk_rpgd_batch_fill_hyper(void* dst, float lr, float b1, float b2, float eps, float clip, int rule, const float* bc_table_dev,
                               float sample_stdev, float sample_mean, float sample_min, float sample_max, const float* lo, const float* hi, int C) {
    CtkRpgdBatchHyper e{};
    e.ad = ctk_g_adam_k(lr, b1, b2, eps, clip, rule);
    e.bc_table = bc_table_dev;
    e.sample_stdev = sample_stdev; e.sample_mean = sample_mean; e.sample_min = sample_min; e.sample_max = sample_max;
    for (int i = 0; i < C; ++i) { e.lo[i] = lo[i]; e.hi[i] = hi[i]; }
    __builtin_memcpy(dst, &e, sizeof(e));
}
const char* ctk_g_rpgd_batch_hp_name(int env) { return ctk_kernel_name("ctk_g_rpgd_batch_hp<%d>", env); }

hipError_t ctk_launch_g_rpgd_batch_hp(hipStream_t st, int env, const RolloutArgs& a_in, int bc_len, const RpgdFusedWarm& f,
                                      const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* steps_dev, int n_problems,
                                      const void* kh_steps_dev) {
    if (n_problems < 1 || !kh_steps_dev) return hipErrorInvalidValue;
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const RolloutArgs a = ctk_descent_args(a_in, E::C);
        bool tape_in_lds = false;
        const size_t lds = ctk_g_rpgd_descent_lds(env, a.H, &tape_in_lds);
        FusedWarm fw{};                                // as ctk_launch_g_rpgd_batch; the sampling constants come from the elements
        fw.enabled = 1; fw.K = f.K;
        fw.w = WarmArgs{a.N, a.H, f.P, 0, 0, f.shift_previous, f.sampling_distribution, 0, 0.0f, 0.0f, 0.0f, 0.0f, f.whole_space, nullptr, 0, 0, 0};
        fw.p.interp = f.interp;
        const dim3 grid(1, n_problems), block(GR_BLOCK);
        hipLaunchKernelGGL((ctk_g_rpgd_batch_hp<EV>), grid, block, lds, st, a, static_cast<const unsigned char*>(kh_steps_dev), bc_len,
                           tape_in_lds ? 1 : 0, fw, desc_dev, steps_dev);
    });
    return hipGetLastError();
}
