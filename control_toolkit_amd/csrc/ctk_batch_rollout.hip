// ctk_batch_rollout.hip — the batch families' rollout of caller-supplied plans (include/ctk_hip_rollout.h: ctk_batch_rollout and its
// ctk_mlp_batch_ / ctk_gru_batch_ / ctk_cem_batch_ / ctk_rpgd_batch_ forms): predictor.predict_core(s, Q) + get_trajectory_cost for M
// plans of every listed problem in ONE launch, what B handles answer with B ctk_rollout calls.  One kernel family for all batch
// families: it needs no optimizer descriptor, only a rollout record per listed problem (ctk_launch.h: CtkBatchRolloutRec).
//   ctk_batch_rollout<ENV, PRED, WTRAJ>    wraps affine_rollout_body<ENV, PRED, WTRAJ, false> (ctk_affine_body.h), the body of
//        ctk_affine_rollout: what a CartPole handle with generic_kernels == 0 launches for its rollout (ODE, MLP, GRU); four waves, 64
//        trajectories per workgroup, 16 for the GRU
//   ctk_g_batch_rollout<ENV, WTRAJ>        wraps the affine mode of ctk_g_rollout (ctk_g_rollout_body.inc): every other handle's; one wave
// The two single-handle kernels do not sum the cost in the same order, so a batch takes the one its handles would launch.
// Grid (workgroups of M rows, records).  The prologue turns record blockIdx.y into the RolloutArgs, the constants k and the weight
// pointer the body expects — the pattern of ctk_mppi_batch_pro.inc: blockIdx.y is uniform, so record and constants arrive by scalar
// loads.  Base 0, scale 1 (zero_one: [2][H*C]) and infinite limits in the template: the plans are taken as given.  The body writes
// J, the trajectories and its copy of the plans through the record's pointers, which are the call's own scratch: nothing a step,
// a run or a read uses is written.  No flag, no wait, no atomics, no LDS beyond the body's carve; the launches are ordered by the
// batch's stream.
#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_mlp.h"
#include "ctk_gru.h"
#include "ctk_launch.h"
#include "ctk_affine_body.h"

// the prologue both kernels share.  Expects in scope: ENV; recs, kbase, a_tpl.  Leaves: q, a_in, k.
#define CTK_BATCH_ROLLOUT_PRO                                                                                              \
    const CtkBatchRolloutRec& q = recs[blockIdx.y];                                                                        \
    RolloutArgs a_in = a_tpl;                                                                                              \
    _Pragma("unroll") for (int i = 0; i < Env<ENV>::S; ++i) a_in.s0[i] = q.s[i];                                           \
    _Pragma("unroll") for (int c = 0; c < Env<ENV>::C; ++c) a_in.u_prev[c] = q.u_prev[c];                                  \
    a_in.u_prev_dev = nullptr;                                                                                             \
    a_in.J = q.J; a_in.Q_out = q.Q_out; a_in.traj_out = q.traj;                                                            \
    const typename Env<ENV>::K k = *reinterpret_cast<const typename Env<ENV>::K*>(kbase + (size_t)q.kidx * CtkBatchKStride<ENV>::value);

template <int ENV, int PRED, bool WTRAJ>
__global__ __launch_bounds__(SAMP_BLOCK) void ctk_batch_rollout(const CtkBatchRolloutRec* __restrict__ recs, const unsigned char* __restrict__ kbase,
                                                                const float* __restrict__ zero_one, const float* __restrict__ wbase,
                                                                uint32_t wstride, int H_, int P_, uint32_t pmagic_, RolloutArgs a_tpl) {
    CTK_BATCH_ROLLOUT_PRO
    const float* wperm = nullptr;
    if constexpr (PRED != CTK_PRED_ODE) wperm = wbase + (size_t)q.id * wstride;
    // a handle's per-call decision (ctk_api.hip: make_args), as the GRU batch's step forms it: the record's angle and the block's word
    if constexpr (PRED == CTK_PRED_GRU)
        a_in.fast_cos_ok = (fabsf(q.s[2]) <= CTK_SINCOS_FAST_LIMIT && reinterpret_cast<const uint32_t*>(wperm)[GRU_BATCH_WORD] != 0u) ? 1 : 0;
    const BestArgs none{nullptr, 0u, nullptr, nullptr, nullptr};
    affine_rollout_body<ENV, PRED, WTRAJ, false>(q.plans, zero_one, zero_one + P_, wperm, 0, q.m, H_, P_, pmagic_, a_in, k, none, nullptr, 0u);
}

template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(CTK_G_TRAJ) void ctk_g_batch_rollout(const CtkBatchRolloutRec* __restrict__ recs, const unsigned char* __restrict__ kbase,
                                                                 const float* __restrict__ zero_one, RolloutArgs a_tpl) {
    constexpr int MODE = CTK_G_MODE_AFFINE, G_TRAJ = CTK_G_TRAJ;
    constexpr bool LOG = WTRAJ;
    CTK_BATCH_ROLLOUT_PRO
    a_in.N = q.m;
    const RolloutArgs& a = a_in;
    const MppiK m{};                                   // (the affine mode reads none of it)
    const int cols_per_point = Env<ENV>::C, rng_kind = 0;
    const float* __restrict__ samples = q.plans;
    const float* __restrict__ base = zero_one;
    const float* __restrict__ scale = zero_one + a_tpl.P;
    float* __restrict__ parts = nullptr;
#include "ctk_g_rollout_body.inc"
}

// ---------------------------------------------------------------------------------------------
// template arguments <environment, (predictor,) materialise>
const char* ctk_batch_rollout_name(int env, bool generic, int pred, bool traj) {
    if (generic) return ctk_kernel_name("ctk_g_batch_rollout<%d, %4$s>", env, 0, 0, traj ? "true" : "false");
    return ctk_kernel_name("ctk_batch_rollout<%d, %d, %4$s>", env, pred, 0, traj ? "true" : "false");
}

int ctk_batch_rollout_blocks(bool generic, int pred, int M) { return generic ? ctk_g_rollout_blocks(M) : ctk_affine_rollout_blocks(pred, M); }

hipError_t ctk_launch_batch_rollout(hipStream_t st, int env, bool generic, int pred, const RolloutArgs& a_in, const CtkBatchRolloutRec* recs_dev,
                                    int n_records, int M, const void* k_dev, const float* zero_one_dev, const float* w_dev, size_t wstride,
                                    bool traj) {
    if (n_records < 1 || n_records > 65535 || M < 1 || !recs_dev || !k_dev || !zero_one_dev) return hipErrorInvalidValue;
    if (!generic && (env != CTK_ENV_CARTPOLE || (pred != CTK_PRED_ODE && !w_dev))) return hipErrorInvalidValue;
    if (generic && pred != CTK_PRED_ODE) return hipErrorInvalidValue;
    const unsigned char* kb = static_cast<const unsigned char*>(k_dev);
    const dim3 grid(ctk_batch_rollout_blocks(generic, pred, M), n_records);
    if (generic) {
        CTK_FOR_ENV(env, EV, {
            using E = Env<EV>;
            const RolloutArgs a = ctk_rollout_args(a_in, E::C, a_in.H * E::C);     // as ctk_launch_g_rollout forms a handle's
            const size_t lds = ctk_g_rollout_lds(a.P, a.H, E::C);
            ctk_with_bool(traj, [&](auto traj_c) {
                hipLaunchKernelGGL((ctk_g_batch_rollout<EV, decltype(traj_c)::value>), grid, dim3(CTK_G_TRAJ), lds, st, recs_dev, kb, zero_one_dev, a);
            });
        });
        return hipGetLastError();
    }
    // CartPole's tuned kernel: C = 1, a row of a plan is H columns (ctk_launch_affine_rollout of a handle's make_args)
    const RolloutArgs a = ctk_rollout_args(a_in, CTK_C, a_in.H);
    const size_t lds = ctk_affine_rollout_lds(a.H, pred);
    ctk_with_bool(traj, [&](auto traj_c) {
        constexpr bool T = decltype(traj_c)::value;
        constexpr int EV = CTK_ENV_CARTPOLE;
        if (pred == CTK_PRED_ODE)
            hipLaunchKernelGGL((ctk_batch_rollout<EV, CTK_PRED_ODE, T>), grid, dim3(SAMP_BLOCK), lds, st, recs_dev, kb, zero_one_dev, w_dev, (uint32_t)wstride, a.H, a.P, a.p_magic, a);
        else if (pred == CTK_PRED_MLP)
            hipLaunchKernelGGL((ctk_batch_rollout<EV, CTK_PRED_MLP, T>), grid, dim3(SAMP_BLOCK), lds, st, recs_dev, kb, zero_one_dev, w_dev, (uint32_t)wstride, a.H, a.P, a.p_magic, a);
        else
            hipLaunchKernelGGL((ctk_batch_rollout<EV, CTK_PRED_GRU, T>), grid, dim3(SAMP_BLOCK), lds, st, recs_dev, kb, zero_one_dev, w_dev, (uint32_t)wstride, a.H, a.P, a.p_magic, a);
    });
    return hipGetLastError();
}
