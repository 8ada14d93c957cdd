// ctk_cem_fused.hip — one CEM step (all outer iterations) in ONE launch, analytic predictor of any environment (ctk_env.h: C control
// inputs -> H*C columns per plan, below "H" where a column count is meant), <= CTK_CEM_FUSED_MAX_BLOCKS
// workgroups (all co-resident: one per CU).  Replaces, per outer iteration, the three launches rollout -> ctk_select_topk ->
// ctk_cem_refit and, after the loop, ctk_g_cem_finish (optimizer_cem_tf.py:61-80,83-111): SURVEY 8e's all-reduce form of the
// elite refit applied INSIDE one GPU, with the {value, tag} word hand-off of ctk_mppi.hip between workgroups.
//
// Per outer iteration, every workgroup (64 rollouts, 256 threads):
//   1. rollout    Q = clip(mu + eps * std) (:64-66), costs J of its 64 rows (anatomy of ctk_affine_rollout<ODE>; the NEXT
//                 iteration's sample tile is fetched by waves 1..3 while wave 0 runs the recurrence — it does not depend on mu/std);
//   2. hop 1      publishes its 64 costs as words {sortable key, tag}; polls all N words into LDS;
//   3. selection  finds the K-th smallest (key, index) of all N REDUNDANTLY (4-pass radix select on an LDS histogram; ties
//                 broken by index, the total order of ctk_select_topk / tf.argsort) -> which of ITS rows are elite (:73-75);
//   4. hop 2      publishes {n_b, m_b[H], M2_b[H]} of its elite rows: m_b = mean of d = q - mu (mu: the mean the samples were drawn around),
//                 M2_b = centred sum of squares — formed in one pass in double, published as floats; polls every workgroup's record;
//   5. refit      ONE pass over the records in a fixed order, in double: A = sum n_b m_b, B = sum (M2_b + n_b m_b^2) -> mean = mu + A/K,
//                 M2 = B - A^2/K (the 53 bits absorb the cancellation; the shift by mu keeps it small), identical bits in every
//                 workgroup -> mu, population std (:77-78) in LDS for the next iteration.  (First form: Chan's pairwise update in
//                 float — two passes, three barriers: 2.0 us per iteration against 1.0.  Raw sums as doubles, two words each: the
//                 records double and their gather eats the gain, 3.3 against 1.9 us.)
// After the loop: the workgroup that owns the cheapest row publishes u = elite[0,0] (:101); workgroup 0 clips the std, shifts
// both by one step and refills the tail (:99-102) into the handle's mu / std.
// Only the last iteration's plans, costs (and trajectories, WTRAJ) reach memory; BEST_IDX is materialised on demand by
// ctk_select_topk from those costs (ctk_api.hip: locate_buffer).
// Every wait is bounded by a wall clock; on expiry the error word behind {u, seq} is raised (ctk_api.hip:finish_step ->
// CTK_ERR_STATE) — never a silently wrong result.
// include/ctk_hip.h gives the batch's opaque C type the name ctk_cem_batch; in C++ a type and a template cannot share a name in one scope,
// and the kernel template below carries that name (it is what a kernel trace prints).  This translation unit never touches the C type, so
// the header's declarations see it under another name here.  (A different struct TAG in the header would not help: the typedef name itself is
// what collides.)  Whoever needs the C type in this file must move the code that does into ctk_batch.hip; the guard below keeps a second
// definition of the name, from any header added here later, from passing silently.
#ifdef ctk_cem_batch
#error "ctk_cem_batch is already a macro: the renaming below would hide it"
#endif
#define ctk_cem_batch ctk_cem_batch_opaque
#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_launch.h"
#undef ctk_cem_batch

#ifdef CTK_CEM_STAMPS   // diagnostic build (tools/diag_cem_fused.hip); never compiled into libctk_hip.so
#define CSTAMP(i)                                                                                  \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        if (threadIdx.x == 0 && a.stamps) a.stamps[(bx * 8 + it) * 16 + (i)] = wall_clock64(); \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    } while (0)
#else
#define CSTAMP(i)
#endif

// 64 rollouts per workgroup: wave 0 runs their recurrence (one per lane).  EIGHT waves per workgroup (CF_WAVES; launch_bounds(512)):
// everything between two recurrences (input preparation, hand-off polls, selection, moments, merge) is spread over 512 threads, two
// waves per SIMD — with four waves a SIMD holds ONE wave, every instruction of these phases issues at 4+ cycles and every LDS latency is exposed (measured: selection
// 4.0 us, merge 1.7 us per outer iteration at cfg3).
constexpr int CF_TRAJ = 64, CF_WAVES = 8, CF_BLOCK = CF_TRAJ * CF_WAVES;
constexpr int CF_CHUNK = 8;   // keys per thread and chunk of the counting loop
constexpr int CF_LLW = 8;   // hand-off words in flight per thread

struct CemFusedK {
    int its, K, nblk;
    unsigned long long per_it;      // samples per outer iteration (N * H)
    unsigned long long* llJ;        // [N]              {sortable key of J_n, tag}
    unsigned long long* llS;        // [nblk][1 + 2H]   {n_b | m_b[H] | M2_b[H], tag}
    uint32_t tag0;                  // tag of iteration it = tag0 + it (host: consecutive across launches, never 0)
    float std_min, std_max, init_std;
    float mid[CTK_MAX_INPUTS];      // per input: the tail refill of the mean (:99-102)
    float* mu; float* sd;           // [H*C] device, in / out
    float* u_dev; float* u_host; int* idx_out; uint32_t seq;
    unsigned long long timeout_ticks;   // wall_clock64 ticks (100 MHz) per hop
};

// LDS carve (4-byte words)
struct CemCarve {
    int tile0, tile1, ubuf, cin, mu, sd, keys, recs, part, hist, misc, total;
};
__host__ __device__ inline CemCarve cem_carve(int N, int H, int nblk) {
    const int ts = tile_stride(H), us = (H + 1) | 1, rs = 1 + 2 * H;
    CemCarve c;
    int o = 0;
    c.tile0 = o; o += CF_TRAJ * ts;
    c.tile1 = o; o += CF_TRAJ * ts;
    c.ubuf = o; o += CF_TRAJ * us;
    c.cin = o; o += CF_BLOCK;
    c.mu = o; o += H;
    c.sd = o; o += H;
    c.keys = o; o += (N + CF_BLOCK * CF_CHUNK - 1) / (CF_BLOCK * CF_CHUNK) * (CF_BLOCK * CF_CHUNK);   // padded: the counting loop reads whole chunks
    c.recs = o; o += nblk * rs;
    o = (o + 1) & ~1;
    c.part = o; o += 4 * CF_BLOCK;          // [SEG][H] {S1, S2} doubles of the segmented refit (SEG * H <= CF_BLOCK)
    c.hist = o; o += 256;
    c.misc = o; o += 80 + 2 * CF_WAVES;   // [0..7] selection scalars | [8] n_b | [16..79] elite rows | [80..) two per-wave reduction rows
    c.total = (o + 3) & ~3;
    return c;
}

CTK_DEV unsigned long long ll_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
CTK_DEV void ll_st(unsigned long long* p, uint32_t payload, uint32_t tag) {
    __hip_atomic_store(p, ((unsigned long long)tag << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Polls words [0, n) of `src` (thread t takes t, t + nthreads, ...) until each carries `tag`; sink(i, payload).
// All of a thread's pending words are re-polled TOGETHER (one memory round trip per round, not one per word: the words of a
// batch come from CF_LLW different workgroups, and a stale first read of each would otherwise cost its own round trip).
template <class Sink>
CTK_DEV bool ll_gather(const unsigned long long* src, int n, uint32_t tag, int t, int nthreads, unsigned long long ticks, Sink&& sink) {
    bool expired = false;
    const unsigned long long t0 = wall_clock64();
    for (int i0 = t; i0 < n; i0 += nthreads * CF_LLW) {
        unsigned long long w[CF_LLW];
#pragma unroll
        for (int j = 0; j < CF_LLW; ++j) {
            const int i = i0 + j * nthreads;
            w[j] = i < n ? ll_ld(src + i) : ((unsigned long long)tag << 32);
        }
        for (;;) {
            bool pending = false;
#pragma unroll
            for (int j = 0; j < CF_LLW; ++j) pending |= (uint32_t)(w[j] >> 32) != tag;
            if (!pending) break;
            if (wall_clock64() - t0 > ticks) { expired = true; break; }
            __builtin_amdgcn_s_sleep(1);
#pragma unroll
            for (int j = 0; j < CF_LLW; ++j) {
                const int i = i0 + j * nthreads;
                if ((uint32_t)(w[j] >> 32) != tag) w[j] = ll_ld(src + i);
            }
        }
#pragma unroll
        for (int j = 0; j < CF_LLW; ++j) {
            const int i = i0 + j * nthreads;
            if (i < n) sink(i, (uint32_t)w[j]);
        }
    }
    return expired;
}

// sample tile of one iteration into LDS by the threads tsub in [0, nsub) (a subset of the workgroup): tile[r*ts + c] = eps[row0+r][c];
// rows beyond N and the pad columns read as zeros.  No barrier inside.
CTK_DEV void cem_fetch_tile(float* tile, const float* __restrict__ samples, const RolloutArgs& a, int row0, int tsub, int nsub) {
    const int P = a.P, ts = tile_stride(P);
    const int rows = max(0, min(CF_TRAJ, a.N - row0));
    if (rows < CF_TRAJ) {
        for (int i = tsub + rows * ts; i < CF_TRAJ * ts; i += nsub) tile[i] = 0.0f;
    }
    for (int r = tsub; r < rows; r += nsub)
        for (int c = P; c < ts; ++c) tile[r * ts + c] = 0.0f;
    if (samples != nullptr) {
        const float* src = samples + (size_t)row0 * P;
        const int total = rows * P;
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4* src4 = reinterpret_cast<const float4*>(src);
            const int n4 = total >> 2;
            for (int b0 = 0; b0 < n4; b0 += 4 * nsub) {
                float4 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i4 = b0 + j * nsub + tsub;
                    if (i4 < n4) v[j] = src4[i4];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i4 = b0 + j * nsub + tsub;
                    if (i4 < n4) {
                        const int flat = i4 << 2;
                        int r = P >= 2 ? (int)__umulhi((uint32_t)flat, a.p_magic) : flat, c = flat - r * P;
                        const float e4[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            tile[r * ts + c] = e4[q];
                            if (++c == P) { c = 0; ++r; }
                        }
                    }
                }
            }
            done = n4 << 2;
        }
        for (int i = done + tsub; i < total; i += nsub) {
            const int r = P >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i;
            tile[r * ts + (i - r * P)] = src[i];
        }
    } else {
        // on-device Philox, addressed by (global row, column block, call, stream = iteration): the draws of ctk_affine_rollout
        const int tpr = nsub / CF_TRAJ;              // threads per row (nsub is a multiple of 64)
        const int r = tsub % CF_TRAJ, cb0 = tsub / CF_TRAJ;
        if (r < rows) {
            const uint32_t grow = (uint32_t)(a.global_row0 + row0 + r);
            for (int cb = cb0; cb * 4 < P; cb += tpr) {
                float d[4];
                draw4(a, grow, (uint32_t)cb, 0, d);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cb * 4 + j < P) tile[r * ts + cb * 4 + j] = d[j];
            }
        }
    }
}

template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(CF_BLOCK) void ctk_cem_fused(const float* __restrict__ samples, RolloutArgs a_in, typename Env<ENV>::K k, CemFusedK cf) {
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    extern __shared__ float lds[];
    RolloutArgs a = a_in;
    const float* mid = cf.mid;
    const uint32_t bx = blockIdx.x;                // unsigned, as blockIdx.x is: the body's index arithmetic keeps its types
#include "ctk_cem_body.inc"
}

// ---------------------------------------------------------------------------------------------
// The BATCH form (include/ctk_hip.h: ctk_cem_batch_*): B independent CEM problems of one configuration in ONE launch — the same statements
// (ctk_cem_body.inc) around per-problem operands.  Grid (workgroups per problem, problems of this launch): blockIdx.y picks the step
// record, the record's id the problem's descriptor (ctk_launch.h: CtkCemBatchStep / CtkCemBatchDesc, both in device memory; blockIdx.y is
// uniform, so both are read with scalar loads, as a launched kernel reads its kernarg segment).  The prologue rebuilds from them what
// ctk_cem_fused takes as arguments (samples, a, cf); what the problems share stays by value (a_tpl, k, cf_tpl).  The leading arguments are
// the dwords the first loads depend on (the two tables, then the sizes the LDS carve and the tile fetch need): they are the preloaded ones.
//
// PROGRESS.  Every workgroup of a problem waits, twice per outer iteration, for ALL workgroups of that problem (ll_gather over llJ / llS),
// and for no workgroup of another problem: each problem has its own hand-off words and its own tags.  A problem therefore makes progress
// exactly when its nblk workgroups are resident at the same time.  ctk_cem_fused guarantees that by nblk <= CTK_CEM_FUSED_MAX_BLOCKS <=
// CUs and LDS <= 128 KiB: a CU without a workgroup of this kernel admits one, so while a workgroup is still pending fewer than nblk are
// resident, some CU holds none, and the pending one is placed.  The host keeps the same guarantee for a launch of this kernel
// (ctk_batch.hip: ctk_cem_batch_create): problems * nblk <= CUs.  While any workgroup of the launch is pending fewer than CUs workgroups are
// resident, so some CU holds none and admits it — whatever the dispatch order or placement, all workgroups of the launch become
// co-resident, and with them all workgroups of every problem.  Problems of one launch may loop a different number of times (its is per
// record): a problem that finishes early only frees CUs.  Like the single kernel's, the argument assumes that the CUs are this launch's
// to take while it is placed: a kernel of another process on a shared card, or of this process on another stream (a ctk_select_topk of a
// BEST_IDX read runs on the batch's own stream, behind the step), can hold CUs and delay a workgroup.  That case is not excluded, it is
// covered: every wait stays bounded by the wall clock (ll_gather), and one that runs out raises the error word of ITS problem's pinned
// slot (CTK_ERR_STATE naming the problem) — never a hang, never a silently wrong result.
// ---------------------------------------------------------------------------------------------
template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(CF_BLOCK) void ctk_cem_batch(const CtkCemBatchDesc* __restrict__ desc, const CtkCemBatchStep* __restrict__ steps,
                                                          int N_, int H_, int P_, uint32_t pmagic_, int nblk_, int K_, RolloutArgs a_tpl,
                                                          typename Env<ENV>::K k, CemFusedK cf_tpl) {
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    extern __shared__ float lds[];
#include "ctk_cem_batch_pro.inc"
#include "ctk_cem_body.inc"
}

// The PER-PROBLEM-PARAMETER form of the batch kernel (ctk_cem_problem_set_param): the same prologue and the same body, but the derived
// constants `k` of the problem come from device memory instead of the by-value argument.  The host writes them BEHIND the step records, in
// the records' order (stride CtkBatchKStride<ENV>, derived with Env<ENV>::derive, as a handle's are), so they arrive with the records'
// transfer and element blockIdx.y of ksteps belongs to record blockIdx.y of steps — indexed by launch order, not by problem id.  The
// address depends on blockIdx.y alone: uniform, so the constants arrive by scalar loads like the record; they are copied into a local K
// here, ahead of the body's first global store, and stay in SGPRs as the kernarg copy does.  ksteps stands among the leading (preloaded)
// arguments: the load depends on it.
template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(CF_BLOCK) void ctk_cem_batch_pp(const CtkCemBatchDesc* __restrict__ desc, const CtkCemBatchStep* __restrict__ steps,
                                                             int N_, int H_, int P_, uint32_t pmagic_, int nblk_, int K_,
                                                             const unsigned char* __restrict__ ksteps, RolloutArgs a_tpl, CemFusedK cf_tpl) {
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    extern __shared__ float lds[];
#include "ctk_cem_batch_pro.inc"
    const typename E::K k = *reinterpret_cast<const typename E::K*>(ksteps + (size_t)blockIdx.y * CtkBatchKStride<ENV>::value);
#include "ctk_cem_body.inc"
}

// ---------------------------------------------------------------------------------------------
// H below: flat columns of a plan (mpc_horizon * control inputs)
int ctk_cem_fused_blocks(int N) { return (N + CF_TRAJ - 1) / CF_TRAJ; }
size_t ctk_cem_fused_ll_words(int N, int H) { return (size_t)N + (size_t)ctk_cem_fused_blocks(N) * (1 + 2 * H); }
size_t ctk_cem_fused_lds(int N, int H) { return (size_t)cem_carve(N, H, ctk_cem_fused_blocks(N)).total * sizeof(float); }
bool ctk_cem_fusable(int pred, int N, int H) {
    return pred == CTK_PRED_ODE && ctk_cem_fused_blocks(N) <= CTK_CEM_FUSED_MAX_BLOCKS && ctk_cem_fused_lds(N, H) <= 128 * 1024;
}
const char* ctk_cem_fused_name(int env, bool log) {
    return ctk_kernel_name("ctk_cem_fused<%d, %4$s>", env, 0, 0, log ? "true" : "false");
}

// a_in.H steps, a_in.C inputs (limits per input); the kernel constants are derived from the environment's parameter table
hipError_t ctk_launch_cem_fused(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a_in, const float* samples,
                                const CemFusedLaunch& c, bool log, hipEvent_t e0, hipEvent_t e1) {
    const int nblk = ctk_cem_fused_blocks(a_in.N);
    const dim3 grid(nblk), block(CF_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const int HC = a_in.H * E::C;
        const RolloutArgs a = ctk_rollout_args(a_in, E::C, HC);
        const typename E::K k = E::derive(params, dt, isteps);
        CemFusedK cf{};
        cf.its = c.its; cf.K = c.K; cf.nblk = nblk; cf.per_it = (unsigned long long)a.N * HC;
        cf.llJ = c.ll; cf.llS = c.ll + a.N; cf.tag0 = c.tag0;
        cf.std_min = c.std_min; cf.std_max = c.std_max; cf.init_std = c.init_std;
        for (int i = 0; i < E::C; ++i) cf.mid[i] = 0.5f * (a.lo[i] + a.hi[i]);
        cf.mu = c.mu; cf.sd = c.sd; cf.u_dev = c.u_dev; cf.u_host = c.u_host; cf.idx_out = c.idx_out; cf.seq = c.seq;
        cf.timeout_ticks = (unsigned long long)(c.timeout_s * 1.0e8);
        const size_t lds = ctk_cem_fused_lds(a.N, HC);
        ctk_with_bool(log, [&](auto log_c) { CTK_LAUNCH((ctk_cem_fused<EV, decltype(log_c)::value>), grid, block, lds, st, e0, e1, samples, a, k, cf); });
    });
    return hipGetLastError();
}

const char* ctk_cem_batch_name(int env, bool log, bool per_problem) {
    return ctk_kernel_name(per_problem ? "ctk_cem_batch_pp<%d, %4$s>" : "ctk_cem_batch<%d, %4$s>", env, 0, 0, log ? "true" : "false");
}

// n_problems step records from steps_dev on, as ONE launch of grid (workgroups per problem, n_problems); the caller keeps
// n_problems * workgroups per problem within the device's CU count (the progress argument above the kernel)
hipError_t ctk_launch_cem_batch(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a_in, const CemFusedLaunch& c,
                                const CtkCemBatchDesc* desc_dev, const CtkCemBatchStep* steps_dev, int n_problems, bool log, const void* k_steps_dev) {
    const int nblk = ctk_cem_fused_blocks(a_in.N);
    if (n_problems < 1 || nblk > CTK_CEM_FUSED_MAX_BLOCKS) return hipErrorInvalidValue;
    const dim3 grid(nblk, n_problems), block(CF_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const int HC = a_in.H * E::C;
        const RolloutArgs a = ctk_rollout_args(a_in, E::C, HC);
        CemFusedK cf{};                                // its, tag0, seq and every pointer come from the records and descriptors
        cf.K = c.K; cf.nblk = nblk; cf.per_it = (unsigned long long)a.N * HC;
        cf.std_min = c.std_min; cf.std_max = c.std_max; cf.init_std = c.init_std;
        for (int i = 0; i < E::C; ++i) cf.mid[i] = 0.5f * (a.lo[i] + a.hi[i]);
        cf.timeout_ticks = (unsigned long long)(c.timeout_s * 1.0e8);
        const size_t lds = ctk_cem_fused_lds(a.N, HC);
        if (lds > 128 * 1024) return hipErrorInvalidValue;
        if (k_steps_dev) {                             // per-problem constants: element j belongs to record j (ctk_mppi_batch_derive_k)
            ctk_with_bool(log, [&](auto log_c) {
                hipLaunchKernelGGL((ctk_cem_batch_pp<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.N, a.H, a.P, a.p_magic,
                                   nblk, c.K, static_cast<const unsigned char*>(k_steps_dev), a, cf);
            });
        } else {
            const typename E::K k = E::derive(params, dt, isteps);
            ctk_with_bool(log, [&](auto log_c) {
                hipLaunchKernelGGL((ctk_cem_batch<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.N, a.H, a.P, a.p_magic, nblk,
                                   c.K, a, k, cf);
            });
        }
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The PER-PROBLEM-HYPER-PARAMETER form of the batch kernel (include/ctk_hip_family_hyper.h: ctk_cem_problem_set_hyper / _set_limits),
// defined LAST in this file with its launcher, so that every kernel that was here before keeps its text.  The prologue and the body of
// ctk_cem_batch_pp, statement for statement; ctk_cem_batch_hyp.inc takes, besides k, the problem's cem_best_k, cem_stdev_min,
// cem_initial_action_stdev, the middle of its limits and the limits from the SECOND part of the element behind the step records
// ([K | CtkCemBatchHyper], by record index as _pp's k: blockIdx.y alone, uniform, scalar loads).  All workgroups of a problem read
// the same element, so each selects the same K rows and refits with the same 1 / K: the progress argument above ctk_cem_batch stands
// as written — this form adds no wait, atomic or hand-off.
// ---------------------------------------------------------------------------------------------
struct alignas(16) CtkCemBatchHyper {
    int32_t K;                          // cem_best_k
    float std_min, init_std;            // cem_stdev_min, cem_initial_action_stdev
    uint32_t pad;
    float mid[CTK_MAX_INPUTS];          // 0.5f * (lo + hi), the launcher's expression, formed on the host
    float lo[CTK_MAX_INPUTS], hi[CTK_MAX_INPUTS];
};
static_assert(sizeof(CtkCemBatchHyper) % 16 == 0, "the elements behind the step records stay 16-byte aligned");
template <int ENV>
struct CtkCemKhStride {
    static constexpr size_t value = CtkBatchKStride<ENV>::value + sizeof(CtkCemBatchHyper);
};

template <int ENV, bool WTRAJ>
__global__ __launch_bounds__(CF_BLOCK) void ctk_cem_batch_hp(const CtkCemBatchDesc* __restrict__ desc, const CtkCemBatchStep* __restrict__ steps,
                                                             int N_, int H_, int P_, uint32_t pmagic_, int nblk_,
                                                             const unsigned char* __restrict__ kh_steps, RolloutArgs a_tpl, CemFusedK cf_tpl) {
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    extern __shared__ float lds[];
#define CTK_CEM_BATCH_HP
#include "ctk_cem_batch_pro.inc"
#undef CTK_CEM_BATCH_HP
#include "ctk_cem_batch_hyp.inc"
#include "ctk_cem_body.inc"
}

size_t ctk_cem_batch_hyper_bytes() { return sizeof(CtkCemBatchHyper); }
size_t ctk_cem_batch_kh_stride(int env) {
    size_t stride = 0;
    CTK_FOR_ENV(env, EV, { stride = CtkCemKhStride<EV>::value; });
    return stride;
}
void ctk_cem_batch_fill_hyper(void* dst, int K, float std_min, float init_std, const float* lo, const float* hi, int C) {
    CtkCemBatchHyper e{};
    e.K = K; e.std_min = std_min; e.init_std = init_std;
    for (int i = 0; i < C; ++i) { e.lo[i] = lo[i]; e.hi[i] = hi[i]; e.mid[i] = 0.5f * (lo[i] + hi[i]); }   // ctk_launch_cem_batch's expression
    __builtin_memcpy(dst, &e, sizeof(e));
}
const char* ctk_cem_batch_hp_name(int env, bool log) { return ctk_kernel_name("ctk_cem_batch_hp<%d, %4$s>", env, 0, 0, log ? "true" : "false"); }

hipError_t ctk_launch_cem_batch_hp(hipStream_t st, int env, const RolloutArgs& a_in, const CemFusedLaunch& c, const CtkCemBatchDesc* desc_dev,
                                   const CtkCemBatchStep* steps_dev, int n_problems, bool log, const void* kh_steps_dev) {
    const int nblk = ctk_cem_fused_blocks(a_in.N);
    if (n_problems < 1 || nblk > CTK_CEM_FUSED_MAX_BLOCKS || !kh_steps_dev) return hipErrorInvalidValue;
    const dim3 grid(nblk, n_problems), block(CF_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const int HC = a_in.H * E::C;
        const RolloutArgs a = ctk_rollout_args(a_in, E::C, HC);
        CemFusedK cf{};                                // K, std_min, init_std and mid[] come from the elements; std_max is a handle's
        cf.nblk = nblk; cf.per_it = (unsigned long long)a.N * HC;
        cf.std_max = c.std_max;
        cf.timeout_ticks = (unsigned long long)(c.timeout_s * 1.0e8);
        const size_t lds = ctk_cem_fused_lds(a.N, HC);
        if (lds > 128 * 1024) return hipErrorInvalidValue;
        ctk_with_bool(log, [&](auto log_c) {
            hipLaunchKernelGGL((ctk_cem_batch_hp<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.N, a.H, a.P, a.p_magic, nblk,
                               static_cast<const unsigned char*>(kh_steps_dev), a, cf);
        });
    });
    return hipGetLastError();
}
