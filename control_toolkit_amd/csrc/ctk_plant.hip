// ctk_plant.hip — the plant of a batch's closed loop on the device (include/ctk_hip_run.h: ctk_batch_run / ctk_batch_plant_step).
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

template <int ENV>
__global__ __launch_bounds__(PLANT_BLOCK) void ctk_batch_plant(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ cur,
                                                              CtkBatchStep* __restrict__ next, const unsigned char* __restrict__ kplant,
                                                              const float* __restrict__ u_in, float* __restrict__ states_out,
                                                              float* __restrict__ inputs_out, int n, size_t state_stride,
                                                              size_t input_stride) {
    using E = Env<ENV>;
    constexpr int S = E::S, C = E::C;
    const int j = blockIdx.x * PLANT_BLOCK + threadIdx.x;
    if (j >= n) return;
    const CtkBatchStep& q = cur[j];
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

const char* ctk_batch_plant_name(int env) { return ctk_kernel_name("ctk_batch_plant<%d>", env); }

hipError_t ctk_launch_batch_plant(hipStream_t st, int env, const CtkBatchDesc* desc_dev, const CtkBatchStep* cur_dev, CtkBatchStep* next_dev,
                                  const void* kplant_dev, const float* u_in_dev, float* states_out, float* inputs_out, int n_records,
                                  size_t state_stride, size_t input_stride) {
    if (n_records < 1 || !desc_dev || !cur_dev || !kplant_dev || !states_out) return hipErrorInvalidValue;
    const dim3 grid((n_records + PLANT_BLOCK - 1) / PLANT_BLOCK), block(PLANT_BLOCK);
    CTK_FOR_ENV(env, EV, {
        hipLaunchKernelGGL((ctk_batch_plant<EV>), grid, block, 0, st, desc_dev, cur_dev, next_dev, static_cast<const unsigned char*>(kplant_dev),
                           u_in_dev, states_out, inputs_out, n_records, state_stride, input_stride);
    });
    return hipGetLastError();
}
