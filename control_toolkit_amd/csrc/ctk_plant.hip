// ctk_plant.hip — the plant of a batch's closed loop on the device (include/ctk_hip_run.h: ctk_batch_run / ctk_batch_plant_step; for
// the CEM and RPGD batches include/ctk_hip_loop.h: the same two bodies as ctk_cem_batch_plant[_noisy]<ENV> and
// ctk_rpgd_batch_plant[_noisy]<ENV>, over those families' descriptors and step records).
//
//   ctk_batch_plant<ENV>   one lane per step record: s' = Env<ENV>::step(k_plant[problem], s, u) — the one-step plant the rollout
//        kernels integrate (ctk_generic.hip: ctk_g_rollout calls the same function once per horizon step), with the checked sin / cos.
//        The state comes from the step record, the input from the problem's u_dev (what the controller launch ahead of this one
//        published) or from the caller's array, the constants from a per-problem array that the host derived with
//        ctk_mppi_batch_derive_k from the PLANT's parameter table and sub-step count — which may differ from the controller's.
//        The new state goes to the trace and, when the run has a next step, into that step's record, where the next controller
//        launch reads it as it reads a state the host wrote.
// Plain vector loads and stores; the launches of a run are ordered by their stream, so there is no flag and no wait in here.
#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_launch.h"

constexpr int PLANT_BLOCK = 64;

// the body of the plant kernels of every batch family: Desc / Rec are the family's descriptor and step record (ctk_launch.h), of which
// only id, s and u_dev are touched
template <int ENV, class Desc, class Rec>
__device__ __forceinline__ void plant_body(const Desc* __restrict__ desc, const Rec* __restrict__ cur, Rec* __restrict__ next,
                                           const unsigned char* __restrict__ kplant, const float* __restrict__ u_in,
                                           float* __restrict__ states_out, float* __restrict__ inputs_out, int n, size_t state_stride,
                                           size_t input_stride) {
    using E = Env<ENV>;
    constexpr int S = E::S, C = E::C;
    const int j = blockIdx.x * PLANT_BLOCK + threadIdx.x;
    if (j >= n) return;
    const Rec& q = cur[j];
    const int p = q.id;
    const typename E::K k = *reinterpret_cast<const typename E::K*>(kplant + (size_t)p * CtkBatchKStride<ENV>::value);
    const float* up = u_in ? u_in + (size_t)j * C : desc[p].u_dev;
    float s[S], u[C];
#pragma unroll
    for (int i = 0; i < S; ++i) s[i] = q.s[i];
#pragma unroll
    for (int c = 0; c < C; ++c) u[c] = up[c];
    E::step(k, s, u);
#pragma unroll
    for (int i = 0; i < S; ++i) states_out[(size_t)j * state_stride + i] = s[i];
    if (inputs_out) {
#pragma unroll
        for (int c = 0; c < C; ++c) inputs_out[(size_t)j * input_stride + c] = u[c];
    }
    if (next) {
#pragma unroll
        for (int i = 0; i < S; ++i) next[j].s[i] = s[i];
    }
}

#define CTK_PLANT_KERNEL(NAME, DESC, REC)                                                                                              \
    template <int ENV>                                                                                                                 \
    __global__ __launch_bounds__(PLANT_BLOCK) void NAME(const DESC* __restrict__ desc, const REC* __restrict__ cur, REC* __restrict__ next, \
                                                        const unsigned char* __restrict__ kplant, const float* __restrict__ u_in,      \
                                                        float* __restrict__ states_out, float* __restrict__ inputs_out, int n,         \
                                                        size_t state_stride, size_t input_stride) {                                    \
        plant_body<ENV>(desc, cur, next, kplant, u_in, states_out, inputs_out, n, state_stride, input_stride);                         \
    }
CTK_PLANT_KERNEL(ctk_batch_plant, CtkBatchDesc, CtkBatchStep)
CTK_PLANT_KERNEL(ctk_cem_batch_plant, CtkCemBatchDesc, CtkCemBatchStep)        // the CEM batch's closed loop (include/ctk_hip_loop.h)
CTK_PLANT_KERNEL(ctk_rpgd_batch_plant, CtkRpgdBatchDesc, CtkRpgdBatchStep)     // the RPGD batch's
#undef CTK_PLANT_KERNEL

const char* ctk_batch_plant_name(int env) { return ctk_kernel_name("ctk_batch_plant<%d>", env); }

#define CTK_PLANT_LAUNCHER(KERNEL, DESC, REC)                                                                                          \
    hipError_t ctk_launch_batch_plant(hipStream_t st, int env, const DESC* desc_dev, const REC* cur_dev, REC* next_dev, const void* kplant_dev, \
                                      const float* u_in_dev, float* states_out, float* inputs_out, int n_records, size_t state_stride, \
                                      size_t input_stride) {                                                                           \
        if (n_records < 1 || !desc_dev || !cur_dev || !kplant_dev || !states_out) return hipErrorInvalidValue;                         \
        const dim3 grid((n_records + PLANT_BLOCK - 1) / PLANT_BLOCK), block(PLANT_BLOCK);                                              \
        CTK_FOR_ENV(env, EV, {                                                                                                         \
            hipLaunchKernelGGL((KERNEL<EV>), grid, block, 0, st, desc_dev, cur_dev, next_dev, static_cast<const unsigned char*>(kplant_dev), \
                               u_in_dev, states_out, inputs_out, n_records, state_stride, input_stride);                               \
        });                                                                                                                            \
        return hipGetLastError();                                                                                                      \
    }
CTK_PLANT_LAUNCHER(ctk_batch_plant, CtkBatchDesc, CtkBatchStep)
CTK_PLANT_LAUNCHER(ctk_cem_batch_plant, CtkCemBatchDesc, CtkCemBatchStep)
CTK_PLANT_LAUNCHER(ctk_rpgd_batch_plant, CtkRpgdBatchDesc, CtkRpgdBatchStep)
#undef CTK_PLANT_LAUNCHER
const char* ctk_cem_batch_plant_name(int env) { return ctk_kernel_name("ctk_cem_batch_plant<%d>", env); }
const char* ctk_rpgd_batch_plant_name(int env) { return ctk_kernel_name("ctk_rpgd_batch_plant<%d>", env); }

// ---- the stochastic plant (include/ctk_hip_episode.h: ctk_batch_episodes / ctk_batch_plant_step_noisy) ----
//   ctk_batch_plant_noisy<ENV>   one lane per step record, beside ctk_batch_plant<ENV>:
//        n       = the normal draws [2 S] of (noise seed, stream CTK_PLANT_STREAM, call pos + t, row 0): draw4's arithmetic, column
//                  blocks 0 .. ceil(2 S / 4) - 1; columns [0, S) process noise, [S, 2 S) measurement noise
//        c_k     = Env<ENV>::stage_cost(k_plant, s_k, u_k, u_{k-1})           the realised cost, with the PLANT's constants
//        s_{k+1} = Env<ENV>::step(k_plant, s_k, u_k) + sigma_w * n[0:S]       the true state: to the state trace
//        y_{k+1} = s_{k+1} + sigma_v * n[S:2S]                                what the controller is given: to the observation trace
//                                                                             and into the next step's record
//        A component whose sigma is 0 is SELECTED, not added to (-0.0 survives); a record whose sigmas are all 0 draws nothing, and
//        its transition is then the one of ctk_batch_plant<ENV>.
//        Where the operands come from: the record's s holds y_k, not s_k, so the TRUE state is read from s_true (the state trace row
//        the previous transition wrote, or what the host put there for a segment's first step); u_k from the problem's u_dev (what
//        the controller launch ahead published) or the caller's array; u_{k-1} from u_last (the input trace row k - 1, or the host's
//        row for a segment's first step), because u_dev no longer holds it.  The noise record of lane j lies behind the step records
//        and travels with them; `t` is the step within the segment, added to the record's position.
// Plain vector loads and stores, no LDS, no scratch; ordered by the stream like ctk_batch_plant.
template <int ENV, class Desc, class Rec>
__device__ __forceinline__ void plant_noisy_body(const Desc* __restrict__ desc, const Rec* __restrict__ cur, Rec* __restrict__ next,
                                                 const unsigned char* __restrict__ kplant,
                                                 const CtkPlantNoise* __restrict__ noise, const float* __restrict__ u_in,
                                                 const float* __restrict__ s_true, const float* __restrict__ u_last,
                                                 float* __restrict__ states_out, float* __restrict__ obs_out, float* __restrict__ inputs_out,
                                                 float* __restrict__ costs_out, int n, uint32_t t, size_t s_true_stride, size_t u_last_stride,
                                                 size_t state_stride, size_t input_stride, size_t cost_stride) {
    using E = Env<ENV>;
    constexpr int S = E::S, C = E::C, NB = (2 * S + 3) / 4;
    const int j = blockIdx.x * PLANT_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int p = cur[j].id;
    const typename E::K k = *reinterpret_cast<const typename E::K*>(kplant + (size_t)p * CtkBatchKStride<ENV>::value);
    const CtkPlantNoise& nz = noise[j];
    const float* up = u_in ? u_in + (size_t)j * C : desc[p].u_dev;
    float s[S], s0[S], u[C], ul[C];
#pragma unroll
    for (int i = 0; i < S; ++i) s[i] = s0[i] = s_true[(size_t)j * s_true_stride + i];
#pragma unroll
    for (int c = 0; c < C; ++c) { u[c] = up[c]; ul[c] = u_last[(size_t)j * u_last_stride + c]; }
    const float cost = E::stage_cost(k, s0, u, ul);
    E::step(k, s, u);
    float y[S];
#pragma unroll
    for (int i = 0; i < S; ++i) y[i] = s[i];
    if (nz.any) {
        float z[NB * 4];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            // draw4 (ctk_device.h), kind 0, with the counter (row 0, column block, position, stream)
            const U4 r = philox4x32_10(U4{0u, (uint32_t)cb, nz.pos + t, CTK_PLANT_STREAM}, nz.seed_lo, nz.seed_hi);
            const float ra = sqrtf(-2.0f * logf(u32_unit_open(r.x)));
            const float rb = sqrtf(-2.0f * logf(u32_unit_open(r.z)));
            float sa, ca, sb, cb2;
            sincosf(6.28318530717958647692f * u32_unit_halfopen(r.y), &sa, &ca);
            sincosf(6.28318530717958647692f * u32_unit_halfopen(r.w), &sb, &cb2);
            z[4 * cb] = ra * ca; z[4 * cb + 1] = ra * sa; z[4 * cb + 2] = rb * cb2; z[4 * cb + 3] = rb * sb;
        }
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const float sw = nz.sigma_w[i], sv = nz.sigma_v[i];
            s[i] = sw != 0.0f ? s[i] + sw * z[i] : s[i];
            y[i] = sv != 0.0f ? s[i] + sv * z[S + i] : s[i];
        }
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        states_out[(size_t)j * state_stride + i] = s[i];
        obs_out[(size_t)j * state_stride + i] = y[i];
    }
    costs_out[(size_t)j * cost_stride] = cost;
    if (inputs_out) {
#pragma unroll
        for (int c = 0; c < C; ++c) inputs_out[(size_t)j * input_stride + c] = u[c];
    }
    if (next) {
#pragma unroll
        for (int i = 0; i < S; ++i) next[j].s[i] = y[i];
    }
}


#define CTK_PLANT_NOISY_KERNEL(NAME, DESC, REC)                                                                                        \
    template <int ENV>                                                                                                                 \
    __global__ __launch_bounds__(PLANT_BLOCK) void NAME(const DESC* __restrict__ desc, const REC* __restrict__ cur, REC* __restrict__ next, \
                                                        const unsigned char* __restrict__ kplant, const CtkPlantNoise* __restrict__ noise, \
                                                        const float* __restrict__ u_in, const float* __restrict__ s_true,              \
                                                        const float* __restrict__ u_last, float* __restrict__ states_out,              \
                                                        float* __restrict__ obs_out, float* __restrict__ inputs_out,                   \
                                                        float* __restrict__ costs_out, int n, uint32_t t, size_t s_true_stride,        \
                                                        size_t u_last_stride, size_t state_stride, size_t input_stride,                \
                                                        size_t cost_stride) {                                                          \
        plant_noisy_body<ENV>(desc, cur, next, kplant, noise, u_in, s_true, u_last, states_out, obs_out, inputs_out, costs_out, n, t,  \
                              s_true_stride, u_last_stride, state_stride, input_stride, cost_stride);                                  \
    }
CTK_PLANT_NOISY_KERNEL(ctk_batch_plant_noisy, CtkBatchDesc, CtkBatchStep)
CTK_PLANT_NOISY_KERNEL(ctk_cem_batch_plant_noisy, CtkCemBatchDesc, CtkCemBatchStep)      // the CEM batch's episodes (include/ctk_hip_loop.h)
CTK_PLANT_NOISY_KERNEL(ctk_rpgd_batch_plant_noisy, CtkRpgdBatchDesc, CtkRpgdBatchStep)   // the RPGD batch's
#undef CTK_PLANT_NOISY_KERNEL

const char* ctk_batch_plant_noisy_name(int env) { return ctk_kernel_name("ctk_batch_plant_noisy<%d>", env); }

#define CTK_PLANT_NOISY_LAUNCHER(KERNEL, DESC, REC)                                                                                    \
    hipError_t ctk_launch_batch_plant_noisy(hipStream_t st, int env, const DESC* desc_dev, const REC* cur_dev, REC* next_dev,          \
                                            const void* kplant_dev, const CtkPlantNoise* noise_dev, const float* u_in_dev,             \
                                            const float* s_true_dev, size_t s_true_stride, const float* u_last_dev, size_t u_last_stride, \
                                            uint32_t t, float* states_out, float* obs_out, float* inputs_out, float* costs_out,        \
                                            int n_records, size_t state_stride, size_t input_stride, size_t cost_stride) {             \
        if (n_records < 1 || !desc_dev || !cur_dev || !kplant_dev || !noise_dev || !s_true_dev || !u_last_dev || !states_out || !obs_out || \
            !costs_out)                                                                                                                \
            return hipErrorInvalidValue;                                                                                               \
        const dim3 grid((n_records + PLANT_BLOCK - 1) / PLANT_BLOCK), block(PLANT_BLOCK);                                              \
        CTK_FOR_ENV(env, EV, {                                                                                                         \
            hipLaunchKernelGGL((KERNEL<EV>), grid, block, 0, st, desc_dev, cur_dev, next_dev, static_cast<const unsigned char*>(kplant_dev), \
                               noise_dev, u_in_dev, s_true_dev, u_last_dev, states_out, obs_out, inputs_out, costs_out, n_records, t,  \
                               s_true_stride, u_last_stride, state_stride, input_stride, cost_stride);                                 \
        });                                                                                                                            \
        return hipGetLastError();                                                                                                      \
    }
CTK_PLANT_NOISY_LAUNCHER(ctk_batch_plant_noisy, CtkBatchDesc, CtkBatchStep)
CTK_PLANT_NOISY_LAUNCHER(ctk_cem_batch_plant_noisy, CtkCemBatchDesc, CtkCemBatchStep)
CTK_PLANT_NOISY_LAUNCHER(ctk_rpgd_batch_plant_noisy, CtkRpgdBatchDesc, CtkRpgdBatchStep)
#undef CTK_PLANT_NOISY_LAUNCHER
const char* ctk_cem_batch_plant_noisy_name(int env) { return ctk_kernel_name("ctk_cem_batch_plant_noisy<%d>", env); }
const char* ctk_rpgd_batch_plant_noisy_name(int env) { return ctk_kernel_name("ctk_rpgd_batch_plant_noisy<%d>", env); }
