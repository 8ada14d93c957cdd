// ctk_mppi.hip — MPPI on gfx950 (replaces reference Optimizers/optimizer_mppi.py:181-193).
//
//   ctk_mppi_rollout_ode   64 trajectories per 256-thread block.  All four waves do the parts
//        that do not depend on the state (coalesced HBM read of the block's [64,P] perturbation
//        tile into LDS, interpolation + nominal + clip + MPPI correction for all H steps into an
//        LDS input buffer); then ONE wave runs the H-step recurrence, one trajectory per lane,
//        state in registers, inputs prefetched from LDS {stage cost, Euler step}; then all four
//        waves form the block-local soft-min partial (rho_b, a_b, b_b[P]) by wave shuffles + LDS
//        column sums (sum_n e_n * delta_u_n is linear in the inducing points, so the reduction
//        runs over P values per trajectory instead of H).
//   ctk_mppi_merge         merges partial records {rho, a, b[P]} (blocks of one GPU, or the
//        all-gathered records of several GPUs — SURVEY.md 8e) and either emits one record or
//        applies the update u_nom <- clip(shift(u_nom) + interp(b)/a)   (:163-168,:184,:190).
#ifdef CTK_STAMPS   // diagnostic build (tools/diag_mppi_stamps.hip); never compiled into libctk_hip.so
#define STAMP(i)                                                                                   \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        unsigned long long _t;                                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                 \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        if (threadIdx.x == 0 && a.stamps) a.stamps[blockIdx.x * 16 + (i)] = _t;                     \
    } while (0)
#else
#define STAMP(i)
#endif

#include "ctk_rollout.h"
#include "ctk_env.h"
#include "ctk_mlp.h"
#include "ctk_gru.h"
#include "ctk_launch.h"
#include "ctk_mppi_merge.h"
#include <cstring>
#include <type_traits>

constexpr int MPPI_TRAJ = 64;     // trajectories per block: one wave runs the recurrence
constexpr int MPPI_WAVES = 4;     // waves per block: the prologue / epilogue are spread over all four
constexpr int MPPI_BLOCK = MPPI_TRAJ * MPPI_WAVES;

// LDS carve (floats): tile[64][ts] | ubuf[64][us] | corr[4][64] | e[64] | colsum[4][P] | w0,w1,un,i0 [H] each
__host__ __device__ inline int ubuf_stride(int H) { return (H + 1) | 1; }

// ---------------------------------------------------------------------------------------------
// Multi-GPU exchange without a collective library call (xGMI is point-to-point): every rank owns an
// uncached, IPC-exported exchange buffer  recs[2 parities][W][2+P] | flags[2][W]  that all peers have mapped.
// One 256-thread block per rank and step: store my shard record into slot [parity][rank] of EVERY rank's
// buffer (system-scope stores over xGMI), fence, raise flag [parity][rank] = seq there; wait until all W
// flags in MY buffer carry seq; merge the W records and apply the MPPI update — every rank arrives at the
// identical u_nom.  Parity double-buffering: a peer can run at most one step ahead (it needs my flag of step
// seq+1 to finish that step), so it never overwrites a slot I am still reading.  The wait is bounded by a
// wall-clock timeout; on expiry the step publishes NaN and an error word the host turns into CTK_ERR_STATE.
// ---------------------------------------------------------------------------------------------
struct P2PArgs {
    float* bufs[CTK_P2P_MAX_WORLD];   // exchange buffer of every rank (bufs[rank] is local memory)
    int rank, world, rs;              // rs = 2 + P floats per record
    uint32_t seq;
    uint32_t* err_host;               // pinned, device-visible error word
    unsigned long long timeout_ticks; // wall_clock64 ticks (100 MHz)
};

// the exchange, by one 256-thread block (its own launch, or the tail of the rollout launch's block 0); `bad` is a
// workgroup-shared word
CTK_DEV void p2p_exchange_and_update(float* lds, int* bad, const P2PArgs& x, int P, float neg_inv_lbd, const MppiUpdateArgs& up,
                                     int stage_ok) {
    const int t = threadIdx.x, W = x.world, rs = x.rs, par = (int)(x.seq & 1u);
    float* mine = x.bufs[x.rank];
    const size_t slot = (size_t)(par * W + x.rank) * rs, flags0 = (size_t)2 * W * rs;
    if (t == 0) *bad = 0;
    for (int w = 0; w < W; ++w) {
        if (w == x.rank) continue;
        float* dst = x.bufs[w] + slot;
        for (int i = t; i < rs; i += MERGE_BLOCK)
            __hip_atomic_store(dst + i, ld_rec<2>(mine + slot + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __threadfence_system();
    __syncthreads();
    if (t < W) {
        uint32_t* f = reinterpret_cast<uint32_t*>(x.bufs[t] + flags0) + par * W + x.rank;
        __hip_atomic_store(f, x.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (t < W) {
        const uint32_t* f = reinterpret_cast<const uint32_t*>(mine + flags0) + par * W + t;
        const unsigned long long t0 = wall_clock64();
        while ((int32_t)(__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - x.seq) < 0) {
            if (wall_clock64() - t0 > x.timeout_ticks) { atomicExch(bad, 1); break; }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    __syncthreads();
    if (*bad) {
        if (t == 0) {
            __hip_atomic_store(x.err_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            publish_u(up.u_dev, up.u_host, __builtin_nanf(""), up.seq);
        }
        return;
    }
    mppi_merge_block<true, 2, 1, true, true, true>(lds, mine + (size_t)par * W * rs, W, P, neg_inv_lbd, nullptr, up, stage_ok != 0 ? 1 : 0);
}

__global__ __launch_bounds__(MERGE_BLOCK) void ctk_mppi_p2p_exchange(P2PArgs x, int P, float neg_inv_lbd, MppiUpdateArgs up, int stage_ok) {
    extern __shared__ float lds[];
    __shared__ int bad;
    p2p_exchange_and_update(lds, &bad, x, P, neg_inv_lbd, up, stage_ok);
}

// grid.x blocks; block b merges records [b*per_block, ...)
template <bool FINAL>
__global__ __launch_bounds__(MERGE_BLOCK) void ctk_mppi_merge(const float* __restrict__ parts, int n_parts, int per_block,
                                                             int P, float neg_inv_lbd, float* __restrict__ out_rec,
                                                             MppiUpdateArgs up, int stage_ok) {
    extern __shared__ float lds[];
    const int first = blockIdx.x * per_block;
    const int cnt = min(per_block, n_parts - first);
    mppi_merge_block<FINAL, false>(lds, parts + (size_t)first * (2 + P), cnt, P, neg_inv_lbd,
                                   out_rec ? out_rec + (size_t)blockIdx.x * (2 + P) : nullptr, up, stage_ok != 0 ? 1 : 0);
}

// floats of the rollout carve (everything but the GRU exchange slots), rounded up so that what follows is
// 16-byte aligned.
// traj = trajectories per workgroup: 64 (ODE: one wave runs them, one per lane; MLP: 16 per wave) or
// GRU_TRAJ = 16 (GRU: the four waves share one 16-trajectory MFMA column block, ctk_gru.h)
// PC = P*C sample columns, HC = H*C inputs per trajectory (C control inputs; CartPole: C = 1)
__host__ __device__ inline int mppi_carve_floats(int PC, int HC, int traj, int H) {
    const int f = traj * tile_stride(PC) + traj * ubuf_stride(HC) + MPPI_BLOCK + traj + MPPI_WAVES * PC + 3 * H + HC;
    return (f + 3) & ~3;
}
__host__ __device__ inline int mppi_carve_floats(int P, int H, int traj) { return mppi_carve_floats(P, H, traj, H); }
constexpr int MPPI_PAIR_TRAJ = 32;   // MLP pair form: two tiles per workgroup, two waves per tile
__host__ __device__ inline int mppi_traj(int pred) { return pred == CTK_PRED_GRU ? GRU_TRAJ : pred == CTK_PRED_MLP_PAIR ? MPPI_PAIR_TRAJ : MPPI_TRAJ; }

// In-launch tail of the rollout kernel (single-GPU, <= 256 blocks): the block whose ticket is last
// merges all block records and applies the update, saving the second launch and its boundary.
struct FuseArgs {
    int mode;             // 0: records only; 1: last block merges + updates u_nom/u; 2: last block emits ONE merged record
    int stage_ok;         // the launch's LDS holds all records staged (merge_lds with staging)
    const P2PArgs* p2p;   // mode 3: device-resident exchange description (ctk_p2p_connect); block 0 goes on to exchange + update
    uint32_t p2p_seq;     // mode 3: this step's exchange sequence number (parity = buffer half)
    unsigned long long* ll;   // {value, seq} words [blocks][2+P] for the low-latency hand-off (needs stage_ok); nullptr: ticket path
    unsigned* counter;    // zero before the launch; the last block resets it
    float* out_rec;       // mode 2
    MppiUpdateArgs up;    // mode 1
};

// Argument order: the 14 dwords the first global loads depend on come first — with
// -amdgpu-kernarg-preload-count=14 (Makefile) the command processor delivers them in SGPRs at wave launch, so the
// sample loads do not wait for a cold scalar-cache miss on the kernel-argument segment (MI355X: gfx940+ feature).
// N_/H_/P_/pmagic_ duplicate fields of `a` for that reason.
// P2P: the instantiations whose merging block goes on to exchange records with peer GPUs (fuse mode 3, ctk_p2p_step);
// kept apart because that tail costs the network-predictor kernels registers they need in the recurrence (measured:
// GRU 83 -> 109 us per launch when every instantiation carried it).
// ENV: the environment (ctk_env.h).  The analytic-predictor instantiation (PRED = ODE) is written against Env<ENV> only — C
// control inputs (sample columns P*C, inputs H*C per trajectory, per-channel interpolation / clip / correction / update), the
// recurrence through Env::cost_step, the input-only cost terms through Env::input_cost; CartPole is Env<0>, C = 1.  The network
// predictors' instantiations are CartPole's (other environments: ctk_generic_net.hip).
// P_ = inducing points; pmagic_ = magic of the P_*C sample columns of a row.
// FORM (ctk_launch.h: CTK_MPPI_FORM_*): the four-argument kernel is FORM 0 — the tail of at most CTK_MPPI_FUSE_MAX_BLOCKS_LL records and
// CTK_MPPI_LL_NARROW_WORDS words (one 8-deep poll batch, one thread per column in the merge), the pipelined recurrence; the launcher
// takes the five-argument overload for the other forms (many records; the previous recurrence and the late publish of u, diagnostic
// switches).  One body text.  FORM 0 publishes u AHEAD of the plan update (part 5: EARLY_U) in a merge + update launch of the analytic
// predictor with one control input; every other launch, and the resident and batch kernels, publish it from the final update.
#define CTK_BODY_EARLY_U   // the launched kernel: u ahead of the plan update where the form allows it (ctk_launch.h: ctk_mppi_early_u_ok)
template <int ENV, int PRED, bool LOG, bool P2P = false>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_rollout(const float* __restrict__ samples,
                                                               const float* __restrict__ u_nom,
                                                               const InterpEntry* __restrict__ interp,
                                                               const float* __restrict__ wperm,
                                                               float* __restrict__ parts, int N_, int H_, int P_,
                                                               uint32_t pmagic_, RolloutArgs a_in, typename Env<ENV>::K k, MppiK m, FuseArgs fz) {
    constexpr int FORM = 0;
    extern __shared__ float lds[];
#include "ctk_mppi_body.inc"
}
template <int ENV, int PRED, bool LOG, bool P2P, int FORM>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_rollout(const float* __restrict__ samples,
                                                               const float* __restrict__ u_nom,
                                                               const InterpEntry* __restrict__ interp,
                                                               const float* __restrict__ wperm,
                                                               float* __restrict__ parts, int N_, int H_, int P_,
                                                               uint32_t pmagic_, RolloutArgs a_in, typename Env<ENV>::K k, MppiK m, FuseArgs fz) {
    static_assert(FORM != 0, "FORM 0 is the four-argument kernel");
    extern __shared__ float lds[];
#include "ctk_mppi_body.inc"
}
#undef CTK_BODY_EARLY_U

// ---------------------------------------------------------------------------------------------
// The RESIDENT form (opt-in: ctk_resident_enable): the same step — the same statements, ctk_mppi_body.inc — served
// by a kernel that stays on the device and takes its per-step inputs (state, previous input, sample pointer, sequence number, Philox
// position, which u_nom buffer is current) from a MAILBOX instead of a launch: what a launch-per-step loop pays per step in the runtime
// and the command processor is paid once.
//   * the mailbox lives in fine-grained DEVICE memory that the host stores into through the PCIe BAR (posted writes): every workgroup
//     polls local memory, and no PCIe READ is left on the request path (a read round trip is 1.4 - 5 us depending on the box,
//     tools/diag_mailbox_vram.hip).  Where the host cannot reach device memory (ctk_api.hip probes it) the mailbox is pinned host memory:
//     block 0 polls it — ONE poller: sixteen queue on the read path — fetches the request in one coalesced access and relays it through
//     device memory.  Everything a step leaves for the next one (u_nom, u) is published by the step's closing fence and acquired with
//     the next request;
//   * every wait is bounded by the wall clock: no request for `idle_ticks` -> the kernel leaves (the next ctk_step launches it again);
//     the other workgroups follow block 0 (its "left" flag) or give up after 4 x that.  It therefore never holds the device longer than
//     idle_ticks beyond its last step — a device-wide synchronize of anybody else waits at most that long; ctk_resident_stop / every
//     other API call on the handle ends it at once (cmd = EXIT);
//   * leaving is announced (state = LEAVING, fence, re-read the request number; then LEFT as the kernel's last store).  A request that
//     crosses the announcement in flight is either seen by the re-read and served, or lost with the kernel — the host sees LEFT while it
//     waits for the result and launches the kernel again with that request as its first.
// ---------------------------------------------------------------------------------------------
CTK_DEV uint32_t box_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM); }
CTK_DEV void box_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }

// what a launch passes as kernel arguments, in DEVICE memory here: as by-value kernel arguments these ~120 dwords stay live in SGPRs across
// the request loop (218 spilled, read back lane by lane inside the recurrence: block 0's step 14.8 us); behind a pointer they are
// scalar-loaded where a step needs them, as a launched kernel loads its kernarg segment
template <class K>
struct ResidentArgs {
    const InterpEntry* interp;
    float* parts;
    int N, H, P;
    uint32_t pmagic;
    float* unom0;
    float* unom1;
    RolloutArgs base;
    K k;
    MppiK m;
    FuseArgs fz0;
};

template <int ENV, int FORM>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_resident(const ResidentArgs<typename Env<ENV>::K>* __restrict__ ra,
                                                                const CtkResidentBox* box, int box_local, CtkResidentStat* stat, CtkResidentBox* relay,
                                                                unsigned long long idle_ticks, uint32_t first_req) {
    extern __shared__ float lds[];
    __shared__ CtkResidentBox req_s;
    __shared__ float uown_s[CTK_MAX_INPUTS];          // the optimizer's own last output, as the prepared inputs assumed it
    __shared__ int upd_ok_s;
    // ---- the names the body's parts expect; what changes per step is assigned before the part that reads it
    constexpr int PRED = CTK_PRED_ODE;
    constexpr bool LOG = false, P2P = false;
    const InterpEntry* interp = ra->interp;
    float* parts = ra->parts;
    const int N_ = ra->N, H_ = ra->H, P_ = ra->P;
    const uint32_t pmagic_ = ra->pmagic;
    float* const unom0 = ra->unom0; float* const unom1 = ra->unom1;
    const typename Env<ENV>::K& k = ra->k;
    const MppiK& m = ra->m;
    const float* samples = nullptr;
    const float* u_nom = unom0;
    const float* wperm = nullptr;
    const RolloutArgs& a_in = ra->base;
    FuseArgs fz = ra->fz0;
    const float* const d_u = ra->base.u_prev_dev;     // where the step publishes its own output
#ifdef CTK_RES_STAMPS                                   // diagnostic build only: where block 0's step goes (shader cycles since the request was fetched)
    unsigned long long c_req = 0;
#pragma push_macro("STAMP")
#undef STAMP
#define STAMP(i) do { if ((blockIdx.x == 0 || blockIdx.x == 5) && threadIdx.x == 0 && (i) >= 3) __hip_atomic_store(&stat->stamps[(blockIdx.x ? 6 : 0) + (i) - 2], (uint32_t)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); } while (0)
#endif
#define CTK_BODY_RESIDENT                             // the kernel goes on behind the publish: its release stays (part 1: PUB_REL)
#define CTK_BODY_S1 16                                // as the launched kernel: the same split of the steps over the waves = the same sums, bit for bit
#include "ctk_mppi_body_1_decl.inc"
#include "ctk_mppi_body_3_defs.inc"
#undef CTK_BODY_S1
    // inputs of a whole step (sample tile, tables, clipped inputs, input-only costs) from `samples` / `a.call` / `u_nom` / `a.u_prev*`
    auto do_pre = [&]() {
#include "ctk_mppi_body_2_pro1.inc"
#include "ctk_mppi_body_4_phase_a.inc"
        // phase B too (part 5 runs it under the first S1 steps of the recurrence; it is idempotent, so running it here as well only means
        // that the recurrence finds every input ready): waves 1..3, their thirds of [S1, H)
        if (wave != 0) {
            const int Hb = (H - S1 + MPPI_WAVES - 2) / (MPPI_WAVES - 1);
            prologue2(lane, min(H, S1 + (wave - 1) * Hb), min(H, S1 + (wave - 1) * Hb + Hb), wave, corr_keep);
        }
        __syncthreads();
    };
    // recurrence from `a.s0`, costs, block record, hand-off; block 0: merge, update, publish {u, seq}
    auto do_post = [&]() {
#include "ctk_mppi_body_5_post.inc"
    };
#ifdef CTK_RES_STAMPS
#pragma pop_macro("STAMP")
#endif
#undef CTK_BODY_RESIDENT
    uint32_t served = first_req - 1u;                 // request number of the last step this workgroup has taken
    unsigned long long t_seen = 0, t_relayed = 0;
    bool pre_ok = false;                              // the inputs of the NEXT step are already in LDS, formed for ...
    const float* pre_samples = nullptr;               // ... these draws (nullptr: the in-kernel sampler at position pre_call)
    uint32_t pre_call = 0, pre_cur = 0;
    for (;;) {
        // ---- the next request.  Wave 0: lane 0 polls ONE word; then the request is moved as a whole — its dwords by as many lanes in one
        //      coalesced access (a dword at a time over PCIe is a round trip each: 24 us measured).  box_local: every workgroup reads the
        //      box itself (device memory); else block 0 reads it (host memory) and relays it.  The relay's cmd word is also the "block 0 has
        //      left" flag the other workgroups watch.
        if (threadIdx.x < 64) {
            constexpr int BOXW = (int)(sizeof(CtkResidentBox) / sizeof(uint32_t));
            static_assert(BOXW <= 64 && offsetof(CtkResidentBox, req) == 0 && offsetof(CtkResidentBox, cmd) == 4 &&
                          offsetof(CtkResidentBox, upd) == sizeof(CtkResidentBox) - 4, "request layout");
            const int lane = threadIdx.x;
            const unsigned long long t0 = wall_clock64();
            int leave = 0, from_relay = 0;
            uint32_t w = 0;
            constexpr int TAILW = (int)(offsetof(CtkResidentBox, tail) / sizeof(uint32_t));
            // box_local: the whole box in ONE pass per poll (its dwords by as many lanes); req == tail != served: a complete new request
            auto poll_box = [&]() {
                const uint32_t x = lane < BOXW ? __hip_atomic_load(reinterpret_cast<const uint32_t*>(box) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
                const uint32_t head = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), tl = (uint32_t)__builtin_amdgcn_readlane((int)x, TAILW);
                w = x;
                return head != served && tl == head;
            };
            if (blockIdx.x == 0) {
                bool have = false;                                       // w already holds the request (box_local)
                for (;;) {
                    if (box_local) { if (poll_box()) { have = true; break; } }
                    else if (__builtin_amdgcn_readfirstlane((int)(lane == 0 ? __hip_atomic_load(&box->req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u)) != (int)served) break;
                    if (wall_clock64() - t0 > idle_ticks) {              // nothing to do: leave, unless a request slips in right now
                        if (lane == 0) { box_store(&stat->state, CTK_RES_LEAVING); __threadfence_system(); }
                        const int slipped = __builtin_amdgcn_readfirstlane((int)(lane == 0 ? (box_load(&box->req) != served ? 1u : 0u) : 0u));
                        if (slipped) { if (lane == 0) box_store(&stat->state, CTK_RES_RUNNING); continue; }   // (its tail may still be in flight: poll on)
                        leave = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                t_seen = wall_clock64();
                if (!leave) {
                    if (!have && lane < BOXW) w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(box) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    w = lane == 0 ? served + 1u : (lane == 1 ? (uint32_t)CTK_RES_CMD_EXIT : 0u);
                }
                if (lane < BOXW) reinterpret_cast<uint32_t*>(&req_s)[lane] = w;
                if (!box_local || leave) {
                    // hand it to the other workgroups; the release also publishes what the last step left (u_nom, u)
                    if (lane != 0 && lane < BOXW - 1)     // (not the last word: relay->upd is block 0's "update published" flag)
                        __hip_atomic_store(reinterpret_cast<uint32_t*>(relay) + lane, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    if (lane == 0) __hip_atomic_store(&relay->req, w, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
                t_relayed = wall_clock64();
            } else {
                leave = 1;
                for (;;) {                                               // (wave-uniform: every lane takes every turn)
                    if (box_local && poll_box()) { leave = 0; break; }
                    const uint32_t rc = lane == 0 ? __hip_atomic_load(&relay->cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                    if (__builtin_amdgcn_readfirstlane((int)rc) == CTK_RES_CMD_EXIT) break;                      // block 0 has left
                    if (!box_local) {
                        const uint32_t rr = lane == 0 ? __hip_atomic_load(&relay->req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : served;
                        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)rr) != served) { leave = 0; from_relay = 1; break; }
                    }
                    if (wall_clock64() - t0 > 4 * idle_ticks + 100000ull) break;       // never wait for ever
                    __builtin_amdgcn_s_sleep(1);
                }
                if (leave) w = lane == 1 ? (uint32_t)CTK_RES_CMD_EXIT : 0u;
                else if (from_relay && lane < BOXW) w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(relay) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane < BOXW) reinterpret_cast<uint32_t*>(&req_s)[lane] = w;
            }
        }
        __syncthreads();
        if (req_s.cmd != CTK_RES_CMD_STEP) break;        // workgroup-uniform
        served = req_s.req;
        // ---- are the prepared inputs those of THIS request?  (workgroup-uniform: every thread evaluates the same LDS words)
        bool hit = pre_ok && req_s.samples == pre_samples && (req_s.samples != nullptr || req_s.call == pre_call) && req_s.cur == pre_cur;
        if (hit && !req_s.dev_uprev) {
#pragma unroll
            for (int c = 0; c < C; ++c) hit = hit && __builtin_bit_cast(uint32_t, req_s.u_prev[c]) == __builtin_bit_cast(uint32_t, uown_s[c]);
        }
#pragma unroll
        for (int i = 0; i < S; ++i) a.s0[i] = req_s.s[i];
        fz.up.seq = req_s.seq;
        fz.up.u_nom_in = req_s.cur ? unom1 : unom0; fz.up.u_nom_out = req_s.cur ? unom0 : unom1;
        fz.up.w0_l = nullptr; fz.up.w1_l = nullptr; fz.up.un_l = nullptr; fz.up.i0_l = nullptr;
        // (no acquire fence on the way here: the request was read with uncached atomics, in program order behind the poll that saw its
        //  number; what the prepared inputs were formed from was acquired when they were formed.  An acquire HERE would empty the L2 that
        //  the inputs' preparation has just warmed for the merge tail: + 2 us measured.)
        if (!hit) {                                       // first step, an unexpected sample buffer / previous input: form them now
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");       // draws written by the host or by another kernel; u_nom / u of the last step
            samples = req_s.samples; u_nom = fz.up.u_nom_in; a.call = req_s.call;
#pragma unroll
            for (int c = 0; c < C; ++c) a.u_prev[c] = req_s.u_prev[c];
            a.u_prev_dev = req_s.dev_uprev ? d_u : nullptr;
            do_pre();
        }
        const unsigned long long c_post0 = clock64();
#ifdef CTK_RES_STAMPS
        c_req = c_post0;
        if ((blockIdx.x == 0 || blockIdx.x == 5) && threadIdx.x == 0) __hip_atomic_store(&stat->stamps[blockIdx.x ? 6 : 0], (uint32_t)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
        do_post();
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            __hip_atomic_store(&stat->c_body, (uint32_t)(clock64() - c_post0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&stat->t_relay, (uint32_t)(t_relayed - t_seen) | (hit ? 0x80000000u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&stat->t_body, (uint32_t)(wall_clock64() - t_relayed), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        // ---- while the host works on the result: the NEXT step's inputs.  They need this step's update (u_nom, u), which block 0
        //      publishes behind its merge: fence, then the request number in relay->upd (agent scope); the others wait for it — bounded
        __threadfence();
        __syncthreads();                                  // req_s is stable until the next wait; the LDS carve is free again
        if (blockIdx.x == 0) {
            if (threadIdx.x == 0) { __hip_atomic_store(&relay->upd, req_s.req, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); upd_ok_s = 1; }
        } else if (threadIdx.x == 0) {
            const unsigned long long t0 = wall_clock64();
            int ok = 1;
            while (__hip_atomic_load(&relay->upd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != req_s.req) {
                if (wall_clock64() - t0 > 20000ull) { ok = 0; break; }          // 200 us: then this workgroup forms its inputs at the next request
                __builtin_amdgcn_s_sleep(1);
            }
            upd_ok_s = ok;
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        pre_ok = false;
        if (upd_ok_s && req_s.next_known) {
            if (threadIdx.x < C) uown_s[threadIdx.x] = __hip_atomic_load(d_u + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pre_samples = req_s.next_samples; pre_call = req_s.call + 1u; pre_cur = req_s.cur ^ 1u;
            samples = pre_samples; u_nom = pre_cur ? unom1 : unom0; a.call = pre_call; a.u_prev_dev = d_u;
            do_pre();                                     // ends with a workgroup barrier: uown_s is visible too
            pre_ok = true;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        box_store(&stat->served, served);
        box_store(&stat->state, CTK_RES_LEFT);
    }
}

// ---------------------------------------------------------------------------------------------
// The BATCH form (include/ctk_hip.h: ctk_batch_*): B independent problems of one configuration in ONE launch — the same step, the same
// statements (ctk_mppi_body.inc, unchanged, FORM 0), around per-problem inputs.  Grid (workgroups per problem, problems of this launch):
// blockIdx.y picks the step record, the record's id the problem's descriptor (ctk_launch.h: CtkBatchStep / CtkBatchDesc, both in device
// memory; blockIdx.y is uniform, so both are read with scalar loads, as a launched kernel reads its kernarg segment).  The prologue
// rebuilds from them what ctk_mppi_rollout takes as arguments (a_in, fz, samples, u_nom, parts); everything the problems share stays by
// value.  The body addresses its problem through blockIdx.x / gridDim.x and those names only, so workgroup x of problem y computes what
// workgroup x of a single handle's launch computes, and block 0 of a problem polls the {value, seq} words of ITS problem only.
// Argument order as ctk_mppi_rollout's (five pointers, then N / H / P / magic: the preloaded dwords), so that the body's kernarg prefetch
// touches the same span; wperm is the body's (unused: analytic predictor), spare pads the fifth pointer.
// ---------------------------------------------------------------------------------------------
template <int ENV, bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                             const InterpEntry* __restrict__ interp, const float* __restrict__ wperm,
                                                             const void* spare, int N_, int H_, int P_, uint32_t pmagic_, RolloutArgs a_tpl,
                                                             typename Env<ENV>::K k, MppiK m, FuseArgs fz_tpl) {
    constexpr int PRED = CTK_PRED_ODE, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    (void)spare;
#include "ctk_mppi_body.inc"
}

// The PER-PROBLEM-PARAMETER form of the batch kernel (ctk_problem_set_param): the same prologue and the same body, but the derived
// constants `k` of the problem come from the array kdev [B] (stride CtkBatchKStride<ENV>, written by the host with Env<ENV>::derive, as a
// handle's are) instead of the by-value argument; kdev takes the place of `spare`, so the preloaded dwords are where they were.  q.id is
// uniform, so the constants arrive by scalar loads like the descriptor; they are copied into a local K here, ahead of the body's first
// global store, and stay in SGPRs through the recurrence.
template <int ENV, bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_pp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                const InterpEntry* __restrict__ interp, const float* __restrict__ wperm,
                                                                const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                RolloutArgs a_tpl, MppiK m, FuseArgs fz_tpl) {
    constexpr int PRED = CTK_PRED_ODE, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    const typename Env<ENV>::K k = *reinterpret_cast<const typename Env<ENV>::K*>(kdev + (size_t)q.id * CtkBatchKStride<ENV>::value);
#include "ctk_mppi_body.inc"
}

// The MLP forms of the batch kernel (include/ctk_hip.h: ctk_mlp_batch_*): the same prologue around the body of
// ctk_mppi_rollout<0, CTK_PRED_MLP_PAIR, LOG, false> — 32 trajectories per workgroup, two waves per 16-trajectory tile, grid
// (ceil(N / 32), problems of this launch).  The network is the plant here, so it is per problem: wbase is the base of the per-problem
// weight tables ([B][wstride] floats, each table in the per-lane layout of a handle's d_wperm), wstride rides behind the preloaded
// dwords.  q.id is uniform, so the table's address is scalar arithmetic; the weights themselves are fetched per lane by the body's
// mlp_load_fwd_thin(wperm), as in a handle's launch.  The descriptor is read where the body reads fz / a (the tail's d.ll and u slots
// are scalar loads the compiler places; the instantiations carry no scratch: DESIGN 2.1d).
template <bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_mlp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                 const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                 const void* spare, int N_, int H_, int P_, uint32_t pmagic_, uint32_t wstride,
                                                                 RolloutArgs a_tpl, EnvK k, MppiK m, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_MLP_PAIR, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    (void)spare;
    const float* wperm = wbase + (size_t)q.id * wstride;
#include "ctk_mppi_body.inc"
}

// ... with per-problem cost constants (ctk_mlp_problem_set_param): k from kdev [B], exactly as ctk_mppi_batch_pp takes it
template <bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_mlp_pp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                    const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                    const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                    uint32_t wstride, RolloutArgs a_tpl, MppiK m, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_MLP_PAIR, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    const EnvK k = *reinterpret_cast<const EnvK*>(kdev + (size_t)q.id * CtkBatchKStride<CTK_ENV_CARTPOLE>::value);
    const float* wperm = wbase + (size_t)q.id * wstride;
#include "ctk_mppi_body.inc"
}

// The GRU forms of the batch kernel (include/ctk_hip.h: ctk_gru_batch_*): the same prologue around the body of
// ctk_mppi_rollout<0, CTK_PRED_GRU, LOG, false[, FORM]> — 16 trajectories per workgroup shared by its four waves (ctk_gru.h), grid
// (ceil(N / 16), problems of this launch).  FORM is the launch's, as for a handle: 0 or CTK_MPPI_FORM_WIDE_TAIL (64 records of cfg2's
// 52 words are more than the narrow tail's one poll batch); the tail addresses its problem through blockIdx.x, gridDim.x and fz alone
// in either form.  wbase is the base of the per-problem blocks ([B][wstride] floats: table | carried hidden state | fast-cosine word |
// pad, ctk_gru.h: GRU_BATCH_*): the body reads the table at wperm and the hidden state at wperm + GRU_TABLE_FLOATS, as in a handle's
// launch; nothing here writes the block (the hidden state advances in ctk_gru_advance_batch, ctk_sampled.hip, behind the launch).
// a.fast_cos_ok is a handle's per-step decision (ctk_api.hip: make_args): |s[2]| inside the unchecked cosine's range — the record's
// state, which in a run the plant kernel wrote — and the block's word, the half of it the host keeps.  q.id is uniform: scalar work.
template <bool LOG, int FORM>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_gru(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                 const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                 const void* spare, int N_, int H_, int P_, uint32_t pmagic_, uint32_t wstride,
                                                                 RolloutArgs a_tpl, EnvK k, MppiK m, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_GRU;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    (void)spare;
    const float* wperm = wbase + (size_t)q.id * wstride;
    a_in.fast_cos_ok = (fabsf(q.s[2]) <= CTK_SINCOS_FAST_LIMIT && reinterpret_cast<const uint32_t*>(wperm)[GRU_BATCH_WORD] != 0u) ? 1 : 0;
#include "ctk_mppi_body.inc"
}

// ... with per-problem cost constants (ctk_gru_problem_set_param): k from kdev [B], exactly as ctk_mppi_batch_pp takes it
template <bool LOG, int FORM>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_gru_pp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                    const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                    const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                    uint32_t wstride, RolloutArgs a_tpl, MppiK m, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_GRU;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
    const EnvK k = *reinterpret_cast<const EnvK*>(kdev + (size_t)q.id * CtkBatchKStride<CTK_ENV_CARTPOLE>::value);
    const float* wperm = wbase + (size_t)q.id * wstride;
    a_in.fast_cos_ok = (fabsf(q.s[2]) <= CTK_SINCOS_FAST_LIMIT && reinterpret_cast<const uint32_t*>(wperm)[GRU_BATCH_WORD] != 0u) ? 1 : 0;
#include "ctk_mppi_body.inc"
}

// The PER-PROBLEM-HYPER-PARAMETER forms (include/ctk_hip_hyper.h: *_problem_set_hyper / *_problem_set_limits): the _pp forms with the
// optimizer's own constants per problem as well.  The array in kdev's slot has, for these forms, elements of two parts — the problem's
// derived constants K (CtkBatchKStride<ENV> bytes, as in _pp) and right behind them its CtkBatchHyper (ctk_launch.h: MppiK written by the
// host with mppi_constants, as a handle's is, and the input limits), stride CtkBatchKhStride<ENV> — so `k`, `m` and the limits all hang
// on the preloaded pointer and the record's id alone and are fetched in ONE scalar round trip, the one that fetches k in _pp
// (ctk_mppi_batch_hyp.inc).  The by-value `m` is gone; the preloaded dwords are where they were.
template <int ENV>
struct CtkBatchKhStride {
    static constexpr size_t value = CtkBatchKStride<ENV>::value + sizeof(CtkBatchHyper);
};
template <int ENV, bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_hp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                const InterpEntry* __restrict__ interp, const float* __restrict__ wperm,
                                                                const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                RolloutArgs a_tpl, FuseArgs fz_tpl) {
    constexpr int PRED = CTK_PRED_ODE, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
#include "ctk_mppi_batch_hyp.inc"
#include "ctk_mppi_body.inc"
}

template <bool LOG>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_mlp_hp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                    const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                    const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                    uint32_t wstride, RolloutArgs a_tpl, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_MLP_PAIR, FORM = 0;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
#include "ctk_mppi_batch_hyp.inc"
    const float* wperm = wbase + (size_t)q.id * wstride;
#include "ctk_mppi_body.inc"
}

template <bool LOG, int FORM>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_batch_gru_hp(const CtkBatchDesc* __restrict__ desc, const CtkBatchStep* __restrict__ steps,
                                                                    const InterpEntry* __restrict__ interp, const float* __restrict__ wbase,
                                                                    const unsigned char* __restrict__ kdev, int N_, int H_, int P_, uint32_t pmagic_,
                                                                    uint32_t wstride, RolloutArgs a_tpl, FuseArgs fz_tpl) {
    constexpr int ENV = CTK_ENV_CARTPOLE, PRED = CTK_PRED_GRU;
    constexpr bool P2P = false;
    extern __shared__ float lds[];
#include "ctk_mppi_batch_pro.inc"
#include "ctk_mppi_batch_hyp.inc"
    const float* wperm = wbase + (size_t)q.id * wstride;
    a_in.fast_cos_ok = (fabsf(q.s[2]) <= CTK_SINCOS_FAST_LIMIT && reinterpret_cast<const uint32_t*>(wperm)[GRU_BATCH_WORD] != 0u) ? 1 : 0;
#include "ctk_mppi_body.inc"
}

// ---------------------------------------------------------------------------------------------
// Throughput variant (ODE, N >= CTK_MPPI_THROUGHPUT_MIN_N): one wave per block, 64 trajectories, the
// inputs formed inline in the recurrence instead of through an LDS input buffer.  LDS per block is the
// sample tile only (13.5 KiB at P = 50 instead of 27 KiB), so ~11 recurrence waves are resident per CU
// instead of 5 and the VALU issue slots of every SIMD are covered by several waves.  Same arithmetic in
// the same order as the 4-wave kernel's prologue 2 + recurrence; block records merged by separate launches.
// ---------------------------------------------------------------------------------------------
template <bool LOG>
__global__ __launch_bounds__(64) void ctk_mppi_rollout_tp(RolloutArgs a, EnvK k, MppiK m, const float* __restrict__ samples,
                                                          const float* __restrict__ u_nom,
                                                          const InterpEntry* __restrict__ interp, float* __restrict__ parts) {
    extern __shared__ float lds[];
    const int P = a.P, H = a.H, ts = tile_stride(P);
    float* tile = lds;                 // [64][ts]
    float* e_s = tile + 64 * ts;       // [64]
    float* w0_s = e_s + 64;            // per-step tables [H] x 4
    float* w1_s = w0_s + H;
    float* un_s = w1_s + H;
    int* i0_s = reinterpret_cast<int*>(un_s + H);
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * 64;
    const int n = row0 + lane;
    const bool valid = n < a.N;

    load_tile_early<64, 64>(tile, samples, a, row0, m.stdev, 0, [&] {
        for (int h = lane; h < H; h += 64) {
            const InterpEntry e = interp[h];
            i0_s[h] = e.i0; w0_s[h] = e.w0; w1_s[h] = e.w1;
            un_s[h] = u_nom[min(h + 1, H - 1)];
        }
    });
    __syncthreads();

    const float* my = tile + lane * ts;
    const bool ident = a.identity_interp != 0;
    // The input-only cost terms are quadratic forms of (du, u, u - u_prev): four running sums in the recurrence,
    //   correction (:154-155)  cc * (k_dd S(du^2) + R S(u du) + k_uu S(u^2)),   stage cost  ccR S(u^2) + ccrc S((u - u_prev)^2),
    // scaled once after the loop — 5 instructions per step instead of 13 (this kernel is VALU-bound: profiles/r01_mppi_largeN_pmc.txt).
    float s_dd = 0.0f, s_ud = 0.0f, s_uu = 0.0f, s_rc = 0.0f;
    float uprev = uniform_u_prev0(a);
    float amax = 0.0f;
    auto F_at = [&](int h) {
        float du;
        if (ident) du = my[h];
        else { const int i0 = i0_s[h]; du = my[i0] * w0_s[h] + my[i0 + 1] * w1_s[h]; }
        const float u = fminf(fmaxf(un_s[h] + du, a.lo[0]), a.hi[0]);
        const float dr = u - uprev;
        s_dd = fmaf(du, du, s_dd); s_ud = fmaf(u, du, s_ud); s_uu = fmaf(u, u, s_uu); s_rc = fmaf(dr, dr, s_rc);
        uprev = u;
        if constexpr (LOG) {
            if (valid) a.Q_out[(size_t)n * H + h] = u;
        }
        return k.u_max * u;
    };
    float J;
    if (k.intermediate_steps == 1) J = recur_ode_state_cost<LOG, false, true>(a, k, n, valid, F_at, &amax);
    else J = recur_ode_state_cost<LOG, true, false>(a, k, n, valid, F_at, &amax);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(amax <= CTK_SINCOS_FAST_LIMIT)) != 0, 0)) {
        s_dd = 0.0f; s_ud = 0.0f; s_uu = 0.0f; s_rc = 0.0f; uprev = uniform_u_prev0(a);
        J = recur_ode_state_cost<LOG, true, false>(a, k, n, valid, F_at, &amax);
    }
    const float corr = m.cc * (m.k_dd * s_dd + m.R * s_ud + m.k_uu * s_uu);
    const float cin = k.ccR * s_uu + k.ccrc_weight * s_rc;
    J = (J + cin) * a.inv_Hp1 + corr;
    if (valid) a.J[n] = J;

    const float rho = wave_min(valid ? J : INFINITY);
    const float e = valid ? expf(m.neg_inv_lbd * (J - rho)) : 0.0f;
    const float asum = wave_sum(e);
    e_s[lane] = e;
    __syncthreads();
    float* rec = parts + (size_t)blockIdx.x * (2 + P);
    if (lane == 0) { rec[0] = rho; rec[1] = asum; }
    for (int p = lane; p < P; p += 64) {
        float acc = 0.0f;
#pragma unroll 8
        for (int r = 0; r < 64; ++r) acc += e_s[r] * tile[r * ts + p];
        rec[2 + p] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Throughput variant that STREAMS the samples (identity interpolation, samples in a buffer).  With P = H the whole-horizon LDS
// tile is what limits residency (13.5 KiB per wave -> ~8 waves per CU, profiles/r01_mppi_largeN_pmc.txt), and at ~2 waves per
// SIMD the recurrence is bound by its own dependent-issue latency, not by VALU throughput (a wave64 VALU op issues in 2 cycles
// when enough waves share the SIMD; measured: tools/diag_pk_rate.hip).  Here the wave moves TPS_CK = 16 steps at a time:
// 64 rows x 16 steps are read as 64-byte row segments (16 lanes per row: every fetched line is used once), transposed through
// a 4.3 KiB wave-private LDS patch into 16 registers per lane, and the next chunk's loads are in flight while the current
// 16 steps run.  The epilogue's weighted column sums re-read the block's rows (row-coalesced; they are still in L2 / MALL).
// (Reading each lane's row directly, a dword per step, was tried first: 16x amplification of the L2->L1 traffic, no gain.)
// ---------------------------------------------------------------------------------------------
constexpr int TPS_CK = 16, TPS_LD = TPS_CK + 1;

// RES (round 3, opt-in — measured slower, see tps_resident): the patch becomes the wave's WHOLE [64][H+1] tile, filled chunk by chunk as
// the stream arrives, so the epilogue's weighted column sums read LDS instead of re-reading the block's rows.
template <bool LOG, bool RES = false>
__global__ __launch_bounds__(64) void ctk_mppi_rollout_tps(RolloutArgs a, EnvK k, MppiK m, const float* __restrict__ samples,
                                                           const float* __restrict__ u_nom, float* __restrict__ parts) {
    extern __shared__ float lds[];
    const int P = a.P, H = a.H;               // P == H (identity interpolation)
    const int LD = RES ? (H | 1) : TPS_LD;    // RES: an odd row stride >= H (conflict-free row walk)
    float* xs = lds;                          // [64][LD]: transposition patch, or (RES) the whole tile
    float* e_s = xs + 64 * LD;                // [64]
    float* un_s = e_s + 64;                   // [H] shifted nominal input
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * 64;
    const int n = row0 + lane;
    const bool valid = n < a.N;
    const int last = a.N - 1 - row0;          // last valid row of the block (rows beyond N re-read it; their weight is 0)
    // element e = lane + 64 i of a chunk: row e / 16, column e % 16 -> lanes 16j .. 16j+15 read one 64-byte row segment
    const int crow = lane >> 4, ccol = lane & 15;
    const float* cbase = samples + (size_t)row0 * P;
    float nxt[TPS_CK], cur[TPS_CK];
    auto fetch = [&](int h0) {
        const int c = min(h0 + ccol, H - 1);
#pragma unroll
        for (int i = 0; i < TPS_CK; ++i) nxt[i] = cbase[(size_t)min(crow + 4 * i, last) * P + c];
    };
    auto transpose = [&](int h0) {            // nxt (chunk layout) -> cur (this lane's 16 steps); the patch / tile is the wave's own
        if constexpr (RES) {
            if (h0 + ccol < H) {
#pragma unroll
                for (int i = 0; i < TPS_CK; ++i) xs[(crow + 4 * i) * LD + h0 + ccol] = nxt[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
            for (int i = 0; i < TPS_CK; ++i) cur[i] = xs[lane * LD + min(h0 + i, H - 1)];
        } else {
#pragma unroll
            for (int i = 0; i < TPS_CK; ++i) xs[(crow + 4 * i) * TPS_LD + ccol] = nxt[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
            for (int i = 0; i < TPS_CK; ++i) cur[i] = xs[lane * TPS_LD + i];
        }
    };
    fetch(0);
    for (int h = lane; h < H; h += 64) un_s[h] = u_nom[min(h + 1, H - 1)];   // optimizer_mppi.py:184 (shift)
    __syncthreads();

    const float up0 = uniform_u_prev0(a);
    float s_dd = 0.0f, s_ud = 0.0f, s_uu = 0.0f, s_rc = 0.0f, uprev = up0;   // quadratic-form sums, as in ctk_mppi_rollout_tp
    float J;
    bool redo = k.intermediate_steps != 1;
    if (!redo) {
        State4 s{a.s0[0], a.s0[1], a.s0[2], a.s0[3]};
        float csum = 0.0f, am = 0.0f, e_dd = 0.0f, e_ud = 0.0f;
        float4* traj = nullptr;
        if constexpr (LOG) {
            if (a.traj_out) traj = reinterpret_cast<float4*>(a.traj_out) + (size_t)n * (H + 1);
        }
        for (int h0 = 0; h0 < H; h0 += TPS_CK) {
            transpose(h0);
            if (h0 + TPS_CK < H) fetch(h0 + TPS_CK);
#pragma unroll
            for (int i = 0; i < TPS_CK; ++i) {
                const int h = h0 + i;
                if (h < H) {
                    // u = clip(u_nom + stdev * eps) as one fma + one median; the sums over the RAW draw (scaled once after the loop)
                    const float eps = cur[i];
                    const float u = __builtin_amdgcn_fmed3f(fmaf(eps, m.stdev, un_s[h]), a.lo[0], a.hi[0]);
                    const float dr = u - uprev;
                    e_dd = fmaf(eps, eps, e_dd); e_ud = fmaf(u, eps, e_ud); s_uu = fmaf(u, u, s_uu); s_rc = fmaf(dr, dr, s_rc);
                    uprev = u;
                    float sn, cs;
                    ctk_sincosf_fast(s.th, &sn, &cs);
                    am = fmaxf(am, fabsf(s.th));
                    if constexpr (LOG) {
                        if (valid) a.Q_out[(size_t)n * H + h] = u;
                        if (valid && traj) traj[h] = make_float4(s.x, s.v, s.th, s.om);
                    }
                    ode_cost_substep(k, s, k.u_max * u, sn, cs, csum);
                }
            }
        }
        if constexpr (LOG) {
            if (valid && traj) traj[H] = make_float4(s.x, s.v, s.th, s.om);
        }
        s_dd = m.stdev * m.stdev * e_dd; s_ud = m.stdev * e_ud;
        J = csum + terminal_cost(k, s);
        redo = __builtin_amdgcn_ballot_w64(!(am <= CTK_SINCOS_FAST_LIMIT)) != 0;
    }
    if (__builtin_expect(redo, 0)) {   // Euler sub-steps, or an angle beyond the fast sincos range somewhere in the wave: checked recurrence
        s_dd = 0.0f; s_ud = 0.0f; s_uu = 0.0f; s_rc = 0.0f; uprev = up0;
        const float* my = samples + (size_t)min(n, a.N - 1) * P;
        float amax;
        auto F_at = [&](int h) {
            const float du = my[h] * m.stdev;
            const float u = fminf(fmaxf(un_s[h] + du, a.lo[0]), a.hi[0]);
            const float dr = u - uprev;
            s_dd = fmaf(du, du, s_dd); s_ud = fmaf(u, du, s_ud); s_uu = fmaf(u, u, s_uu); s_rc = fmaf(dr, dr, s_rc);
            uprev = u;
            if constexpr (LOG) {
                if (valid) a.Q_out[(size_t)n * H + h] = u;
            }
            return k.u_max * u;
        };
        J = recur_ode_state_cost<LOG, true, false>(a, k, n, valid, F_at, &amax);
    }
    J = (J + k.ccR * s_uu + k.ccrc_weight * s_rc) * a.inv_Hp1 + m.cc * (m.k_dd * s_dd + m.R * s_ud + m.k_uu * s_uu);
    if (valid) a.J[n] = J;

    const float rho = wave_min(valid ? J : INFINITY);
    const float e = valid ? expf(m.neg_inv_lbd * (J - rho)) : 0.0f;
    const float asum = wave_sum(e);
    e_s[lane] = e;
    __syncthreads();
    float* rec = parts + (size_t)blockIdx.x * (2 + P);
    if (lane == 0) { rec[0] = rho; rec[1] = asum; }
    // b[p] = sum_r e_r eps[r][p] over the block's 64 rows, in the CHUNK layout of the main loop: lane (row group crow, column ccol)
    // holds rows crow, crow+4, ... of column h0 + ccol — 16 row-segment loads all in flight, 16 FMAs against the rows' weights (LDS
    // broadcast), two cross-group adds; every lane busy.  (Each lane walking one column over 64 rows: 16 of the kernel's 113 us at
    // N = 2^20 — 50 of 64 lanes active, 8 loads in flight.)  The rows are still in L2 / MALL.  Rows beyond N carry weight 0.
    auto fetch_into = [&](float (&dst)[TPS_CK], int h0) {
        const int c = min(h0 + ccol, H - 1);
#pragma unroll
        for (int i = 0; i < TPS_CK; ++i) dst[i] = cbase[(size_t)min(crow + 4 * i, last) * P + c];
    };
    auto column_sums = [&](const float (&v)[TPS_CK], int h0) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < TPS_CK; ++i) acc = fmaf(e_s[crow + 4 * i], v[i], acc);
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        if (lane < TPS_CK && h0 + lane < H) rec[2 + h0 + lane] = acc * m.stdev;
    };
    if constexpr (RES) {                                  // the tile is resident: no second pass through memory
        for (int h0 = 0; h0 < H; h0 += TPS_CK) {
            const int c = min(h0 + ccol, H - 1);
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < TPS_CK; ++i) acc = fmaf(e_s[crow + 4 * i], xs[(crow + 4 * i) * LD + c], acc);
            acc += __shfl_xor(acc, 16, 64);
            acc += __shfl_xor(acc, 32, 64);
            if (lane < TPS_CK && h0 + lane < H) rec[2 + h0 + lane] = acc * m.stdev;
        }
        return;
    }
    fetch_into(nxt, 0);                                   // two chunks in flight: one being summed, the next one landing
    for (int h0 = 0; h0 < H; h0 += 2 * TPS_CK) {
        if (h0 + TPS_CK < H) fetch_into(cur, h0 + TPS_CK);
        column_sums(nxt, h0);
        if (h0 + 2 * TPS_CK < H) fetch_into(nxt, h0 + 2 * TPS_CK);
        if (h0 + TPS_CK < H) column_sums(cur, h0 + TPS_CK);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
bool ctk_mppi_uses_throughput_kernel(int pred, int N) { return pred == CTK_PRED_ODE && N >= CTK_MPPI_THROUGHPUT_MIN_N; }

// MLP at sizes that leave SIMDs idle -> the pair form
static int kernel_pred(int pred, int N) {
    static const bool off = getenv("CTK_MPPI_NO_PAIR") != nullptr;   // diagnostic switch: A/B the two forms
    return (pred == CTK_PRED_MLP && N <= CTK_MPPI_PAIR_MAX_N && !off) ? CTK_PRED_MLP_PAIR : pred;
}

// which throughput form a launch takes: 2 = streaming (ctk_mppi_rollout_tps: sample buffer + identity interpolation), 1 = whole-horizon
// tile (ctk_mppi_rollout_tp: in-kernel sampler, or P < H), 0 = not a throughput launch.  ONE predicate for the launcher and the name.
static int throughput_form(int pred, int N, bool have_samples, bool identity_interp) {
    if (!ctk_mppi_uses_throughput_kernel(pred, N)) return 0;
    static const bool no_direct = getenv("CTK_MPPI_TP_TILE") != nullptr;   // diagnostic switch: A/B the two throughput forms
    return (have_samples && identity_interp && !no_direct) ? 2 : 1;
}

// the streaming kernel's resident-tile form (RES) is opt-in: measured SLOWER than the patch + re-read form (N = 2^20: 112.4 vs 105.4 us) —
// the re-read hits L2 / MALL, and 13 KiB of LDS per wave costs a twelfth of the residency.  CTK_MPPI_TPS_RESIDENT: diagnostic switch (A/B)
static bool tps_resident(int H) {
    static const bool on = getenv("CTK_MPPI_TPS_RESIDENT") != nullptr;
    return on && (size_t)64 * (H | 1) * sizeof(float) <= 16 * 1024;
}

// the previous recurrence (ctk_launch.h: CTK_MPPI_FORM_OLD_RECUR) — diagnostic switch: A/B and the bit-identity test
static bool mppi_old_recur() {
    static const bool on = getenv("CTK_MPPI_OLD_RECUR") != nullptr;
    return on;
}
// the late publish of u (ctk_launch.h: CTK_MPPI_FORM_LATE_U) — diagnostic switch: A/B and the bit-identity test
static bool mppi_late_u() {
    static const bool on = getenv("CTK_MPPI_LATE_U") != nullptr;
    return on;
}
// the form of a 4-wave launch of `blocks` records of `cols` columns (fz.ll: the {value, seq} tail); the old recurrence is the
// analytic predictor's only
static int mppi_form(int kp, int blocks, int cols, bool ll) {
    return (ll && ctk_ll_tail_wide(blocks, cols) ? CTK_MPPI_FORM_WIDE_TAIL : 0) | (kp == CTK_PRED_ODE && mppi_old_recur() ? CTK_MPPI_FORM_OLD_RECUR : 0);
}
// ... of an environment's analytic-predictor launch (one recurrence unless env_pipelined)
template <int ENV>
static int mppi_env_form(int blocks, int cols, bool ll) {
    return mppi_form(CTK_PRED_ODE, blocks, cols, ll) & (env_pipelined<ENV>::value ? ~0 : ~CTK_MPPI_FORM_OLD_RECUR);
}

// name of the kernel ctk_launch_mppi_rollout runs for these arguments (identity_interp as RolloutArgs carries it: period 1 AND P == H;
// form: the launch's CTK_MPPI_FORM_* bits, known to the launcher)
const char* ctk_mppi_rollout_name(int pred, bool log, int N, bool identity_interp, bool have_samples, bool p2p, int H, int form) {
    const int tf = throughput_form(pred, N, have_samples, identity_interp);
    if (tf == 2) return ctk_kernel_name("ctk_mppi_rollout_tps<%4$s, %5$s>", 0, 0, 0, log ? "true" : "false", (H > 0 && tps_resident(H)) ? "true" : "false");
    if (tf == 1) return log ? "ctk_mppi_rollout_tp<true>" : "ctk_mppi_rollout_tp<false>";
    // template arguments <environment, predictor form, materialise, peer-to-peer tail[, form]>: what rocprofv3's kernel trace shows
    const int kp = pred == CTK_PRED_ODE ? CTK_PRED_ODE : pred == CTK_PRED_GRU ? CTK_PRED_GRU : kernel_pred(pred, N);
    if (form != 0) return ctk_kernel_name("ctk_mppi_rollout<0, %1$d, %4$s, %5$s, %2$d>", kp, form, 0, log ? "true" : "false", p2p ? "true" : "false");
    return ctk_kernel_name("ctk_mppi_rollout<0, %d, %4$s, %5$s>", kp, 0, 0, log ? "true" : "false", p2p ? "true" : "false");
}

int ctk_mppi_num_blocks(int N, int pred) {
    const int tr = mppi_traj(kernel_pred(pred, N));
    return (N + tr - 1) / tr;
}


// C control inputs (CartPole kernels: 1): P*C sample columns, H*C inputs per trajectory
size_t ctk_mppi_rollout_lds(int P, int H, int pred, int N, int C) {
    const int kp = kernel_pred(pred, N);
    const size_t roll = (size_t)(mppi_carve_floats(P * C, H * C, mppi_traj(kp), H) + (kp == CTK_PRED_GRU ? GRU_EX_FLOATS : kp == CTK_PRED_MLP_PAIR ? 2 * MLP_PAIR_EX : 0)) * sizeof(float);
    const size_t tail = merge_lds(P * C, CTK_MPPI_FUSE_MAX_BLOCKS);
    return roll > tail ? roll : tail;
}

// LDS of one launch: the rollout carve, or the fused tail's (staged) merge scratch if larger
static size_t rollout_launch_lds(int P, int H, int pred, int N, int blocks, int* stage_ok, int C = 1) {
    size_t lds = ctk_mppi_rollout_lds(P, H, pred, N, C);
    *stage_ok = 0;
    P *= C;
    if (ctk_ll_records_ok(blocks, P) && merge_can_stage(P, blocks)) {
        const size_t st = merge_lds_staged(P, blocks);
        if (st > lds) lds = st;
        *stage_ok = 1;
    }
    return lds;
}

// the kernel-side fuse argument of a 4-wave launch (rollout or resident) of an environment with C inputs; stage_ok: rollout_launch_lds
static FuseArgs mppi_fuse_args(const MppiFuse& fuse, int stage_ok, const RolloutArgs& a, int C, const float* u_nom_in, float* u_nom_out) {
    FuseArgs fz{};
    fz.mode = fuse.mode; fz.stage_ok = stage_ok; fz.counter = fuse.counter; fz.out_rec = fuse.out_rec;
    fz.ll = (fuse.mode != 0 && stage_ok) ? fuse.ll : nullptr;
    fz.p2p = static_cast<const P2PArgs*>(fuse.p2p); fz.p2p_seq = fuse.p2p_seq;
    fz.up = mppi_update_args(a, C, u_nom_in, u_nom_out, fuse.u_dev, fuse.u_host, fuse.seq);
    return fz;
}

// a launch's CTK_MPPI_FORM_* bits as a constant: f(integral_constant<int, form>).  OLD: the instantiations with the previous recurrence
// exist (the analytic predictor of a pipelined environment: mppi_form / mppi_env_form raise that bit nowhere else).  LATE: those with the
// late publish of u exist (launch_mppi_4wave raises that bit, never together with WIDE_TAIL)
template <bool OLD, bool LATE = false, class F>
static void with_mppi_form(int form, F&& f) {
    using std::integral_constant;
    constexpr int W = CTK_MPPI_FORM_WIDE_TAIL, O = CTK_MPPI_FORM_OLD_RECUR, L = CTK_MPPI_FORM_LATE_U;
    if (form == 0) f(integral_constant<int, 0>{});
    else if (form == W) f(integral_constant<int, W>{});
    else if (LATE && form == L) { if constexpr (LATE) f(integral_constant<int, L>{}); }
    else if constexpr (OLD) {
        if (form == O) f(integral_constant<int, O>{});
        else if (LATE && form == (L | O)) { if constexpr (LATE) f(integral_constant<int, L | O>{}); }
        else f(integral_constant<int, W | O>{});
    }
}

// One launch of the 4-wave kernel ctk_mppi_rollout<ENV, PRED, log, p2p[, form]>: a.P inducing points of ENV's C inputs, `k` the
// caller's constants (CartPole: the handle's cached ones), PRED the kernel variant (kernel_pred; the network predictors are CartPole's).
// Returns the form it launched.
template <int ENV, int PRED>
static int launch_mppi_4wave(hipStream_t st, const RolloutArgs& a, const typename Env<ENV>::K& k, const MppiK& m, const float* samples,
                             const float* u_nom, const float* wperm, float* parts, bool log, const MppiFuse& fuse, hipEvent_t e0, hipEvent_t e1) {
    constexpr int C = Env<ENV>::C;
    constexpr bool ODE = PRED == CTK_PRED_ODE;
    static_assert(ODE || ENV == CTK_ENV_CARTPOLE, "network predictors: CartPole instantiations only");
    const int PC = a.P * C;
    const dim3 grid((a.N + mppi_traj(PRED) - 1) / mppi_traj(PRED)), block(MPPI_BLOCK);
    int stage_ok;
    size_t lds = rollout_launch_lds(a.P, a.H, PRED, a.N, (int)grid.x, &stage_ok, C);
    const bool p2p = ENV == CTK_ENV_CARTPOLE && fuse.mode == 3;      // (the peer-to-peer tail is CartPole's)
    if (p2p) lds = std::max(lds, merge_lds_staged(a.P, fuse.p2p_world));   // the tail also stages the `world` records of the exchange
    const FuseArgs fz = mppi_fuse_args(fuse, stage_ok, a, C, u_nom, fuse.u_nom_out);
    const uint32_t pmagic = ctk_magic_of(PC);
    int form;
    if constexpr (ODE) form = mppi_env_form<ENV>((int)grid.x, PC, fz.ll != nullptr);
    else form = mppi_form(PRED, (int)grid.x, PC, fz.ll != nullptr);
    // the late publish of u, on request: only where FORM 0 would publish early, so that the switch changes no other launch
    constexpr bool LATE = ctk_mppi_early_u_ok(0, PRED, C, false);
    if (LATE && mppi_late_u() && fz.mode == 1 && fz.ll != nullptr && ctk_mppi_early_u_ok(form, PRED, C, p2p)) form |= CTK_MPPI_FORM_LATE_U;
    auto go = [&](auto kernel) { CTK_LAUNCH(kernel, grid, block, lds, st, e0, e1, samples, u_nom, a.interp, wperm, parts, a.N, a.H, a.P, pmagic, a, k, m, fz); };
    with_mppi_form<ODE && env_pipelined<ENV>::value, LATE>(form, [&](auto form_c) {
        ctk_with_bool(log, [&](auto log_c) {
            ctk_with_bool(p2p, [&](auto p2p_c) {
                constexpr int FV = decltype(form_c)::value;
                constexpr bool LV = decltype(log_c)::value, XV = ENV == CTK_ENV_CARTPOLE && decltype(p2p_c)::value;
                if constexpr (FV == 0) go(ctk_mppi_rollout<ENV, PRED, LV, XV>);      // (FORM 0 is the four-argument kernel)
                else if constexpr ((FV & CTK_MPPI_FORM_LATE_U) != 0 && XV) (void)0;   // (never launched: LATE_U is raised without the peer-to-peer tail only)
                else go(ctk_mppi_rollout<ENV, PRED, LV, XV, FV>);
            });
        });
    });
    return form;
}

hipError_t ctk_launch_mppi_rollout(hipStream_t st, int pred, const RolloutArgs& a, const EnvK& k, const MppiK& m,
                                   const float* samples, const float* u_nom, const float* wperm, float* parts, bool log,
                                   const MppiFuse& fuse, hipEvent_t e0, hipEvent_t e1, const char** ran) {
    if (const int tf = throughput_form(pred, a.N, samples != nullptr, a.identity_interp != 0)) {
        const dim3 grid(ctk_mppi_num_blocks(a.N, pred));
        if (ran) *ran = ctk_mppi_rollout_name(pred, log, a.N, a.identity_interp != 0, samples != nullptr, false, a.H);
        if (tf == 2) {
            const bool res = tps_resident(a.H);
            const size_t lds_s = (size_t)(64 * (res ? (a.H | 1) : TPS_LD) + 64 + a.H) * sizeof(float);
            ctk_with_bool(log, [&](auto log_c) {
                ctk_with_bool(res, [&](auto res_c) {
                    CTK_LAUNCH((ctk_mppi_rollout_tps<decltype(log_c)::value, decltype(res_c)::value>), grid, dim3(64), lds_s, st, e0, e1, a, k, m, samples,
                               u_nom, parts);
                });
            });
            return hipGetLastError();
        }
        const size_t lds_tp = (size_t)(64 * tile_stride(a.P) + 64 + 4 * a.H) * sizeof(float);
        ctk_with_bool(log, [&](auto log_c) {
            CTK_LAUNCH((ctk_mppi_rollout_tp<decltype(log_c)::value>), grid, dim3(64), lds_tp, st, e0, e1, a, k, m, samples, u_nom, a.interp, parts);
        });
        return hipGetLastError();
    }
    const int kp = kernel_pred(pred, a.N);
    int form;
    if (kp == CTK_PRED_ODE) form = launch_mppi_4wave<CTK_ENV_CARTPOLE, CTK_PRED_ODE>(st, a, k, m, samples, u_nom, wperm, parts, log, fuse, e0, e1);
    else if (kp == CTK_PRED_MLP_PAIR) form = launch_mppi_4wave<CTK_ENV_CARTPOLE, CTK_PRED_MLP_PAIR>(st, a, k, m, samples, u_nom, wperm, parts, log, fuse, e0, e1);
    else if (kp == CTK_PRED_MLP) form = launch_mppi_4wave<CTK_ENV_CARTPOLE, CTK_PRED_MLP>(st, a, k, m, samples, u_nom, wperm, parts, log, fuse, e0, e1);
    else form = launch_mppi_4wave<CTK_ENV_CARTPOLE, CTK_PRED_GRU>(st, a, k, m, samples, u_nom, wperm, parts, log, fuse, e0, e1);
    if (ran) *ran = ctk_mppi_rollout_name(pred, log, a.N, a.identity_interp != 0, samples != nullptr, fuse.mode == 3, a.H, form);
    return hipGetLastError();
}

// The same 4-wave kernel for any environment's analytic predictor (ctk_env.h): a.P = inducing points, a.C = control inputs,
// a.lo / a.hi per input; the kernel constants are derived here from the environment's parameter table.  fuse as above
// (modes 0, 1, 2; the peer-to-peer tail is CartPole's).
hipError_t ctk_launch_mppi_rollout_env(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                       const float* samples, const float* u_nom, float* parts, bool log, const MppiFuse& fuse,
                                       hipEvent_t e0, hipEvent_t e1) {
    CTK_FOR_ENV(env, EV, {
        launch_mppi_4wave<EV, CTK_PRED_ODE>(st, a, Env<EV>::derive(params, dt, isteps), m, samples, u_nom, nullptr, parts, log, fuse, e0, e1);
    });
    return hipGetLastError();
}
hipError_t ctk_launch_mppi_resident(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                    float* u_nom0, float* u_nom1, float* parts, const MppiFuse& fuse, const CtkResidentBox* box_dev, int box_local,
                                    CtkResidentStat* stat_dev, CtkResidentBox* relay, double idle_us, uint32_t first_req, void* args_dev, void* args_host) {
    const dim3 grid(ctk_mppi_num_blocks(a.N, CTK_PRED_ODE)), block(MPPI_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        const int PC = a.P * E::C;
        const typename E::K k = E::derive(params, dt, isteps);
        int stage_ok;
        const size_t lds = rollout_launch_lds(a.P, a.H, CTK_PRED_ODE, a.N, (int)grid.x, &stage_ok, E::C);
        if (!stage_ok || fuse.ll == nullptr) return hipErrorInvalidValue;          // the resident form is the {value, seq} hand-off only
        MppiFuse f1 = fuse;                                                            // ... of a merge + update step; the request carries the sequence number
        f1.mode = 1; f1.seq = 0u;
        const FuseArgs fz = mppi_fuse_args(f1, stage_ok, a, E::C, u_nom0, u_nom1);
        const unsigned long long ticks = (unsigned long long)(idle_us * 100.0);        // wall_clock64: 100 MHz
        using RA = ResidentArgs<typename E::K>;
        static_assert(sizeof(RA) <= CTK_RES_ARGS_BYTES, "resident argument block");
        RA* hostra = static_cast<RA*>(args_host);               // staging that outlives the asynchronous copy (the handle's)
        *hostra = RA{a.interp, parts, a.N, a.H, a.P, ctk_magic_of(PC), u_nom0, u_nom1, a, k, m, fz};
        const hipError_t ce = hipMemcpyAsync(args_dev, hostra, sizeof(RA), hipMemcpyHostToDevice, st);
        if (ce != hipSuccess) return ce;
        // (every environment has the resident kernel in all four forms, though only a pipelined one's launch can carry OLD_RECUR)
        with_mppi_form<true>(mppi_env_form<EV>((int)grid.x, PC, true), [&](auto form_c) {
            hipLaunchKernelGGL((ctk_mppi_resident<EV, decltype(form_c)::value>), grid, block, lds, st, static_cast<const RA*>(args_dev), box_dev, box_local,
                               stat_dev, relay, ticks, first_req);
        });
    });
    return hipGetLastError();
}
// (the form of a resident launch: ctk_launch_mppi_resident; the handle names the kernel before it knows the launch)
const char* ctk_mppi_resident_name(int env, int N, int P) {
    int form = 0;
    CTK_FOR_ENV(env, EV, { form = mppi_env_form<EV>((N + MPPI_TRAJ - 1) / MPPI_TRAJ, P * Env<EV>::C, true); });
    return ctk_kernel_name("ctk_mppi_resident<%d, %d>", env, form);
}

size_t ctk_mppi_rollout_env_lds(int env, int P, int H, int N) {
    int C = 1;
    CTK_FOR_ENV(env, EV, { C = Env<EV>::C; });
    int stage_ok;
    return rollout_launch_lds(P, H, CTK_PRED_ODE, N, (N + MPPI_TRAJ - 1) / MPPI_TRAJ, &stage_ok, C);
}
const char* ctk_mppi_rollout_env_name(int env, bool log) {
    return ctk_kernel_name("ctk_mppi_rollout<%d, 0, %4$s, false>", env, 0, 0, log ? "true" : "false");
}

// the launches of the _hp forms (per-problem optimizer constants and limits).  LAYOUT STEERING, on purpose: these are plain functions
// defined at the END of the file only so that their kernels are instantiated last and laid out in the code object behind every kernel
// that was there before them — the existing kernels then keep their text to the byte, pc-relative displacements included (the check
// that accompanied their introduction compared the disassembly of every existing symbol).  launch_batch_hp dispatches on the
// environment a second time for the same reason.  Do not fold them back into the launchers above.
static void launch_batch_hp(hipStream_t st, int env, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev,
                            const unsigned char* k_dev, uint32_t pmagic, const RolloutArgs& a, const FuseArgs& fz, bool log);
static void launch_batch_mlp_hp(hipStream_t st, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, const float* w_dev,
                                const unsigned char* k_dev, uint32_t pmagic, uint32_t wstride, const RolloutArgs& a,
                                const FuseArgs& fz, bool log);
static void launch_batch_gru_hp(hipStream_t st, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, const float* w_dev,
                                const unsigned char* k_dev, uint32_t pmagic, uint32_t wstride, const RolloutArgs& a,
                                const FuseArgs& fz, bool log, int form);

// ---- the batch form (ctk_mppi_batch): FORM 0 of the 4-wave kernel with the {value, seq} tail, nothing else
int ctk_mppi_batch_fit(int env, int N, int H, int P, size_t* lds_out, int* blocks_out) {
    int C = 1;
    CTK_FOR_ENV(env, EV, { C = Env<EV>::C; });
    const int blocks = (N + MPPI_TRAJ - 1) / MPPI_TRAJ, PC = P * C;
    if (blocks_out) *blocks_out = blocks;
    if (ctk_mppi_uses_throughput_kernel(CTK_PRED_ODE, N)) return 1;
    if (!ctk_ll_records_ok(blocks, PC) || ctk_ll_tail_wide(blocks, PC)) return 2;
    int stage_ok;
    const size_t lds = rollout_launch_lds(P, H, CTK_PRED_ODE, N, blocks, &stage_ok, C);
    if (lds_out) *lds_out = lds;
    if (!stage_ok) return 3;
    if (lds > 160 * 1024) return 4;
    return 0;
}
const char* ctk_mppi_batch_name(int env, bool log, bool per_problem, bool hyper) {
    return ctk_kernel_name(hyper ? "ctk_mppi_batch_hp<%d, %4$s>" : per_problem ? "ctk_mppi_batch_pp<%d, %4$s>" : "ctk_mppi_batch<%d, %4$s>", env, 0, 0,
                           log ? "true" : "false");
}
size_t ctk_mppi_batch_kh_stride(int env) {
    size_t stride = 0;
    CTK_FOR_ENV(env, EV, { stride = CtkBatchKhStride<EV>::value; });
    return stride;
}
size_t ctk_mppi_batch_k_stride(int env) {
    size_t stride = 0;
    CTK_FOR_ENV(env, EV, { stride = CtkBatchKStride<EV>::value; });
    return stride;
}
void ctk_mppi_batch_derive_k(int env, const float* params, float dt, int isteps, void* dst) {
    CTK_FOR_ENV(env, EV, {
        const typename Env<EV>::K k = Env<EV>::derive(params, dt, isteps);
        std::memcpy(dst, &k, sizeof(k));
    });
}

hipError_t ctk_launch_mppi_batch(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                 const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log, const void* k_dev,
                                 bool hyper) {
    size_t lds;
    int blocks;
    if (n_problems < 1 || (hyper && !k_dev) || ctk_mppi_batch_fit(env, a.N, a.H, a.P, &lds, &blocks) != 0) return hipErrorInvalidValue;
    const dim3 grid(blocks, n_problems), block(MPPI_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        FuseArgs fz{};                                 // merge + update by block 0 of every problem over the staged {value, seq} words;
        fz.mode = 1; fz.stage_ok = 1;                  // the pointers and the sequence number are the descriptors' / the step records'
        fz.up = mppi_update_args(a, E::C, nullptr, nullptr, nullptr, nullptr, 0u);
        const uint32_t pmagic = ctk_magic_of(a.P * E::C);
        if (hyper) {                                   // ... with each problem's optimizer constants and limits behind them (ctk_mppi_batch_kh_stride)
            launch_batch_hp(st, EV, grid, block, lds, desc_dev, steps_dev, static_cast<const unsigned char*>(k_dev), pmagic, a, fz, log);
        } else if (k_dev) {                            // per-problem constants: the array the host derived (ctk_mppi_batch_derive_k)
            ctk_with_bool(log, [&](auto log_c) {
                hipLaunchKernelGGL((ctk_mppi_batch_pp<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp,
                                   static_cast<const float*>(nullptr), static_cast<const unsigned char*>(k_dev), a.N, a.H, a.P, pmagic, a, m, fz);
            });
        } else {
            const typename E::K k = E::derive(params, dt, isteps);
            ctk_with_bool(log, [&](auto log_c) {
                hipLaunchKernelGGL((ctk_mppi_batch<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp,
                                   static_cast<const float*>(nullptr), static_cast<const void*>(nullptr), a.N, a.H, a.P, pmagic, a, k, m, fz);
            });
        }
    });
    return hipGetLastError();
}

// ---- the MLP batch form (ctk_mppi_batch_mlp): the pair form of the 4-wave kernel with the narrow {value, seq} tail, nothing else.  The
// blocks, the LDS and the form come from the functions a handle's launch takes them from, so the two can never disagree.
int ctk_mppi_batch_mlp_fit(int N, int H, int P, size_t* lds_out, int* blocks_out) {
    const int blocks = ctk_mppi_num_blocks(N, CTK_PRED_MLP);
    if (blocks_out) *blocks_out = blocks;
    if (kernel_pred(CTK_PRED_MLP, N) != CTK_PRED_MLP_PAIR) return 1;
    if (!ctk_ll_records_ok(blocks, P) || ctk_ll_tail_wide(blocks, P)) return 2;
    int stage_ok;
    const size_t lds = rollout_launch_lds(P, H, CTK_PRED_MLP, N, blocks, &stage_ok);
    if (lds_out) *lds_out = lds;
    if (!stage_ok) return 3;
    if (lds > 160 * 1024) return 4;
    return 0;
}
const char* ctk_mppi_batch_mlp_name(bool log, bool per_problem, bool hyper) {
    return hyper ? (log ? "ctk_mppi_batch_mlp_hp<true>" : "ctk_mppi_batch_mlp_hp<false>") : per_problem ? (log ? "ctk_mppi_batch_mlp_pp<true>" : "ctk_mppi_batch_mlp_pp<false>") : (log ? "ctk_mppi_batch_mlp<true>" : "ctk_mppi_batch_mlp<false>");
}
size_t ctk_mppi_batch_mlp_table_floats() { return (size_t)64 * (MLP_FWD_PER_LANE + MLP_BWD_PER_LANE); }

hipError_t ctk_launch_mppi_batch_mlp(hipStream_t st, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                     const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log,
                                     const float* w_dev, const void* k_dev, bool hyper) {
    size_t lds;
    int blocks;
    if (n_problems < 1 || w_dev == nullptr || (hyper && !k_dev) || ctk_mppi_batch_mlp_fit(a.N, a.H, a.P, &lds, &blocks) != 0) return hipErrorInvalidValue;
    const dim3 grid(blocks, n_problems), block(MPPI_BLOCK);
    FuseArgs fz{};                                     // as ctk_launch_mppi_batch: merge + update by block 0 of every problem
    fz.mode = 1; fz.stage_ok = 1;
    fz.up = mppi_update_args(a, CTK_C, nullptr, nullptr, nullptr, nullptr, 0u);
    const uint32_t pmagic = ctk_magic_of(a.P), wstride = (uint32_t)ctk_mppi_batch_mlp_table_floats();
    if (hyper) {
        launch_batch_mlp_hp(st, grid, block, lds, desc_dev, steps_dev, w_dev, static_cast<const unsigned char*>(k_dev), pmagic, wstride, a, fz, log);
    } else if (k_dev) {
        ctk_with_bool(log, [&](auto log_c) {
            hipLaunchKernelGGL((ctk_mppi_batch_mlp_pp<decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp, w_dev,
                               static_cast<const unsigned char*>(k_dev), a.N, a.H, a.P, pmagic, wstride, a, m, fz);
        });
    } else {
        const EnvK k = Env<CTK_ENV_CARTPOLE>::derive(params, dt, isteps);
        ctk_with_bool(log, [&](auto log_c) {
            hipLaunchKernelGGL((ctk_mppi_batch_mlp<decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp, w_dev,
                               static_cast<const void*>(nullptr), a.N, a.H, a.P, pmagic, wstride, a, k, m, fz);
        });
    }
    return hipGetLastError();
}

// ---- the GRU batch form (ctk_mppi_batch_gru): the GRU form of the 4-wave kernel with the {value, seq} tail in the FORM a handle's launch
// of these sizes takes.  Blocks, LDS, the staging test and the form come from the functions launch_mppi_4wave takes them from.
int ctk_mppi_batch_gru_fit(int N, int H, int P, size_t* lds_out, int* blocks_out, int* form_out) {
    const int blocks = ctk_mppi_num_blocks(N, CTK_PRED_GRU);
    if (blocks_out) *blocks_out = blocks;
    if (form_out) *form_out = 0;
    if (!ctk_ll_records_ok(blocks, P)) return 2;
    int stage_ok;
    const size_t lds = rollout_launch_lds(P, H, CTK_PRED_GRU, N, blocks, &stage_ok);
    if (lds_out) *lds_out = lds;
    if (!stage_ok) return 3;
    if (lds > 160 * 1024) return 4;
    if (form_out) *form_out = mppi_form(CTK_PRED_GRU, blocks, P, true);
    return 0;
}
const char* ctk_mppi_batch_gru_name(bool log, int form, bool per_problem, bool hyper) {
    return ctk_kernel_name(hyper ? "ctk_mppi_batch_gru_hp<%4$s, %1$d>" : per_problem ? "ctk_mppi_batch_gru_pp<%4$s, %1$d>" : "ctk_mppi_batch_gru<%4$s, %1$d>", form, 0, 0, log ? "true" : "false");
}
size_t ctk_mppi_batch_gru_table_floats() { return (size_t)GRU_TABLE_FLOATS; }
size_t ctk_mppi_batch_gru_hidden_floats() { return (size_t)GRU_HIDDEN_FLOATS; }
size_t ctk_mppi_batch_gru_block_floats() { return (size_t)GRU_BATCH_BLOCK_FLOATS; }

hipError_t ctk_launch_mppi_batch_gru(hipStream_t st, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                     const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log, int form,
                                     const float* w_dev, const void* k_dev, bool hyper) {
    size_t lds;
    int blocks, fit_form;
    if (n_problems < 1 || w_dev == nullptr || (hyper && !k_dev) || ctk_mppi_batch_gru_fit(a.N, a.H, a.P, &lds, &blocks, &fit_form) != 0 || form != fit_form) return hipErrorInvalidValue;
    const dim3 grid(blocks, n_problems), block(MPPI_BLOCK);
    FuseArgs fz{};                                     // as ctk_launch_mppi_batch: merge + update by block 0 of every problem
    fz.mode = 1; fz.stage_ok = 1;
    fz.up = mppi_update_args(a, CTK_C, nullptr, nullptr, nullptr, nullptr, 0u);
    const uint32_t pmagic = ctk_magic_of(a.P), wstride = (uint32_t)GRU_BATCH_BLOCK_FLOATS;
    if (hyper) {
        launch_batch_gru_hp(st, grid, block, lds, desc_dev, steps_dev, w_dev, static_cast<const unsigned char*>(k_dev), pmagic, wstride, a, fz, log, form);
        return hipGetLastError();
    }
    with_mppi_form<false>(form, [&](auto form_c) {
        ctk_with_bool(log, [&](auto log_c) {
            constexpr int FV = decltype(form_c)::value;
            constexpr bool LV = decltype(log_c)::value;
            if (k_dev) {
                hipLaunchKernelGGL((ctk_mppi_batch_gru_pp<LV, FV>), grid, block, lds, st, desc_dev, steps_dev, a.interp, w_dev,
                                   static_cast<const unsigned char*>(k_dev), a.N, a.H, a.P, pmagic, wstride, a, m, fz);
            } else {
                const EnvK k = Env<CTK_ENV_CARTPOLE>::derive(params, dt, isteps);
                hipLaunchKernelGGL((ctk_mppi_batch_gru<LV, FV>), grid, block, lds, st, desc_dev, steps_dev, a.interp, w_dev,
                                   static_cast<const void*>(nullptr), a.N, a.H, a.P, pmagic, wstride, a, k, m, fz);
            }
        });
    });
    return hipGetLastError();
}

hipError_t ctk_launch_mppi_merge_partial(hipStream_t st, const float* parts, int n_parts, int per_block, int P,
                                         float neg_inv_lbd, float* out_rec) {
    const int blocks = (n_parts + per_block - 1) / per_block;
    const bool stage = merge_can_stage(P, per_block);
    hipLaunchKernelGGL(ctk_mppi_merge<false>, dim3(blocks), dim3(MERGE_BLOCK), stage ? merge_lds_staged(P, per_block) : merge_lds(P, per_block),
                       st, parts, n_parts, per_block, P, neg_inv_lbd, out_rec, MppiUpdateArgs{}, stage ? 1 : 0);
    return hipGetLastError();
}

size_t ctk_p2p_buffer_floats(int world, int P) { return (size_t)2 * world * (2 + P) + (size_t)2 * world; }
size_t ctk_p2p_args_bytes() { return sizeof(P2PArgs); }
void ctk_p2p_fill_args(void* dst, float* const* bufs, int rank, int world, int P, uint32_t* err_host, double timeout_s) {
    P2PArgs x{};
    for (int w = 0; w < world; ++w) x.bufs[w] = bufs[w];
    x.rank = rank; x.world = world; x.rs = 2 + P; x.seq = 0; x.err_host = err_host;
    x.timeout_ticks = (unsigned long long)(timeout_s * 1.0e8);
    std::memcpy(dst, &x, sizeof(x));
}
bool ctk_mppi_fusable(int P, int blocks, bool have_ll) {
    if (blocks <= CTK_MPPI_FUSE_MAX_BLOCKS) return true;
    return have_ll && ctk_ll_records_ok(blocks, P) && merge_can_stage(P, blocks);
}
bool ctk_p2p_can_fuse(int P, int world, int blocks) {
    return ctk_ll_records_ok(blocks, P) && merge_can_stage(P, blocks) && merge_can_stage(P, world);
}

hipError_t ctk_launch_mppi_p2p_exchange(hipStream_t st, float* const* bufs, int rank, int world, int P, uint32_t p2p_seq,
                                        uint32_t* err_host, double timeout_s, float neg_inv_lbd, int H, const InterpEntry* interp,
                                        const float* u_nom_in, float* u_nom_out, float lo, float hi, float* u_dev, float* u_host,
                                        uint32_t seq) {
    P2PArgs x{};
    for (int w = 0; w < world; ++w) x.bufs[w] = bufs[w];
    x.rank = rank; x.world = world; x.rs = 2 + P; x.seq = p2p_seq; x.err_host = err_host;
    x.timeout_ticks = (unsigned long long)(timeout_s * 1.0e8);
    const bool stage = merge_can_stage(P, world);
    hipLaunchKernelGGL(ctk_mppi_p2p_exchange, dim3(1), dim3(MERGE_BLOCK), stage ? merge_lds_staged(P, world) : merge_lds(P, world), st,
                       x, P, neg_inv_lbd,
                       MppiUpdateArgs{nullptr, nullptr, nullptr, nullptr, H, interp, u_nom_in, u_nom_out, lo, hi, u_dev, u_host, seq},
                       stage ? 1 : 0);
    return hipGetLastError();
}

hipError_t ctk_launch_mppi_update(hipStream_t st, const float* parts, int n_parts, int P, float neg_inv_lbd, int H,
                                  const InterpEntry* interp, const float* u_nom_in, float* u_nom_out, float lo, float hi,
                                  float* u_dev, float* u_host, uint32_t seq) {
    const bool stage = merge_can_stage(P, n_parts);
    hipLaunchKernelGGL(ctk_mppi_merge<true>, dim3(1), dim3(MERGE_BLOCK), stage ? merge_lds_staged(P, n_parts) : merge_lds(P, n_parts), st,
                       parts, n_parts, n_parts, P, neg_inv_lbd, (float*)nullptr,
                       MppiUpdateArgs{nullptr, nullptr, nullptr, nullptr, H, interp, u_nom_in, u_nom_out, lo, hi, u_dev, u_host, seq}, stage ? 1 : 0);
    return hipGetLastError();
}

// ---- the launches of the _hp forms of the batch kernels (declared above ctk_mppi_batch_fit): the _pp launches without `m` (k_dev: the array of two-part elements)
static void launch_batch_hp(hipStream_t st, int env, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev,
                            const unsigned char* k_dev, uint32_t pmagic, const RolloutArgs& a, const FuseArgs& fz, bool log) {
    CTK_FOR_ENV(env, EV, {
        ctk_with_bool(log, [&](auto log_c) {
            hipLaunchKernelGGL((ctk_mppi_batch_hp<EV, decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp,
                               static_cast<const float*>(nullptr), k_dev, a.N, a.H, a.P, pmagic, a, fz);
        });
    });
}
static void launch_batch_mlp_hp(hipStream_t st, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, const float* w_dev,
                                const unsigned char* k_dev, uint32_t pmagic, uint32_t wstride, const RolloutArgs& a,
                                const FuseArgs& fz, bool log) {
    ctk_with_bool(log, [&](auto log_c) {
        hipLaunchKernelGGL((ctk_mppi_batch_mlp_hp<decltype(log_c)::value>), grid, block, lds, st, desc_dev, steps_dev, a.interp, w_dev, k_dev, a.N, a.H,
                           a.P, pmagic, wstride, a, fz);
    });
}
static void launch_batch_gru_hp(hipStream_t st, dim3 grid, dim3 block, size_t lds, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, const float* w_dev,
                                const unsigned char* k_dev, uint32_t pmagic, uint32_t wstride, const RolloutArgs& a,
                                const FuseArgs& fz, bool log, int form) {
    with_mppi_form<false>(form, [&](auto form_c) {
        ctk_with_bool(log, [&](auto log_c) {
            hipLaunchKernelGGL((ctk_mppi_batch_gru_hp<decltype(log_c)::value, decltype(form_c)::value>), grid, block, lds, st, desc_dev, steps_dev,
                               a.interp, w_dev, k_dev, a.N, a.H, a.P, pmagic, wstride, a, fz);
        });
    });
}

// ---------------------------------------------------------------------------------------------
// The LAUNCHED-AHEAD form (ctk_launch.h: CtkAheadBox / CtkAheadGate; include/ctk_hip_ahead.h): ctk_mppi_rollout<ENV, 0,
// false, false> — the same body text, FORM 0, the early order of u where FORM 0 takes it — behind a GATE.  The launch is issued while
// the previous step's kernel still runs, so it carries what was known then; at its entry every workgroup waits for the request that
// brings the rest (state, previous input, sample pointer), and only then touches anything: nothing is read ahead, so a sample buffer
// refilled in place is read as the request finds it (the system-scope acquire behind the gate drops what the caches held of it).
//   * wave 0 of every workgroup reads the mailbox in ONE pass per look (its dwords by as many lanes, uncached): req == the launch's
//     number and tail == req is a complete request (the host writes payload + tail, sfence, req);
//   * workgroup 0 decides.  Its wait is bounded by the wall-clock fuse: LEAVING, fence, one more look — a request that slipped in is
//     served — else it stores the launch's number into the relay word, LEFT as its last store, and the kernel has written nothing else.
//     The host takes LEFT for "not served", consumes a sequence number and launches the step as ever;
//   * the other workgroups take the request from the mailbox themselves (no relay hop on the path) and leave when the relay word or
//     cmd = EXIT says so, or after 4 x the fuse + 1 ms.  A request that lands between workgroup 0's last look and their next one is
//     rolled out by them for nothing: their record words carry a sequence number the host has consumed, only workgroup 0 ever merges,
//     updates and publishes, and the stream orders the next launch behind them.
// Defined LAST in this file, like the _hp launches above and for their reason: every kernel that was here before keeps its text.
// ---------------------------------------------------------------------------------------------
#define CTK_BODY_EARLY_U
template <int ENV>
__global__ __launch_bounds__(MPPI_BLOCK) void ctk_mppi_ahead(const CtkAheadBox* box, const float* __restrict__ u_nom,
                                                             const InterpEntry* __restrict__ interp, const float* __restrict__ wperm,
                                                             float* __restrict__ parts, int N_, int H_, int P_, uint32_t pmagic_,
                                                             RolloutArgs a_tpl, typename Env<ENV>::K k, MppiK m, FuseArgs fz, CtkAheadGate g) {
    constexpr int PRED = CTK_PRED_ODE, FORM = 0;
    constexpr bool LOG = false, P2P = false;
    constexpr int BOXW = CTK_AHEAD_BOX_WORDS, TAILW = BOXW - 1;
    static_assert(offsetof(CtkAheadBox, req) == 0 && offsetof(CtkAheadBox, cmd) == 4 && offsetof(CtkAheadBox, tail) == 4 * TAILW && BOXW <= 64 &&
                  sizeof(CtkAheadBox) == 128, "request layout");
    extern __shared__ float lds[];
    __shared__ uint32_t req_s[BOXW];
    __shared__ int leave_s;
    if (threadIdx.x < 64) {                                      // wave 0 (wave-uniform below: every lane takes every turn)
        const int gl = threadIdx.x;
        const unsigned long long t0 = wall_clock64();
        uint32_t w = 0;
        auto look = [&]() {
            const uint32_t x = gl < BOXW ? __hip_atomic_load(reinterpret_cast<const uint32_t*>(box) + gl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
            w = x;
            return (uint32_t)__builtin_amdgcn_readlane((int)x, 0) == g.req && (uint32_t)__builtin_amdgcn_readlane((int)x, TAILW) == g.req;
        };
        // (relaxed: the state word orders nothing — a release here would write the L2 back on the request's path)
        auto state_store = [&](uint32_t v) { __hip_atomic_store(g.state, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
        int leave = 0;
        if (blockIdx.x == 0) {
            for (;;) {
                if (look()) break;
                if (wall_clock64() - t0 > g.fuse_ticks) {
                    if (gl == 0) { state_store(ctk_ahead_state(g.req, CTK_RES_LEAVING)); __threadfence_system(); }
                    if (!look()) leave = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (!leave && (uint32_t)__builtin_amdgcn_readlane((int)w, 1) != (uint32_t)CTK_RES_CMD_STEP) leave = 1;   // cancelled
            if (gl == 0) {
                if (leave) {
                    __hip_atomic_store(g.relay, g.req, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    state_store(ctk_ahead_state(g.req, CTK_RES_LEFT));
                } else {
                    state_store(ctk_ahead_state(g.req, CTK_RES_RUNNING));
                }
            }
        } else {
            leave = 1;
            for (;;) {
                if (look()) { leave = (uint32_t)__builtin_amdgcn_readlane((int)w, 1) != (uint32_t)CTK_RES_CMD_STEP ? 1 : 0; break; }
                const uint32_t rr = gl == 0 ? __hip_atomic_load(g.relay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                if ((uint32_t)__builtin_amdgcn_readfirstlane((int)rr) == g.req) break;            // workgroup 0 has left
                if (wall_clock64() - t0 > 4 * g.fuse_ticks + 100000ull) break;                    // never wait for ever
                __builtin_amdgcn_s_sleep(1);
            }
        }
        if (gl < BOXW) req_s[gl] = w;
        if (gl == 0) leave_s = leave;
    }
    __syncthreads();
    if (leave_s) return;                                         // workgroup-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");                // draws written by the host or by a kernel of another stream since this launch began
    // ---- what ctk_mppi_rollout takes as arguments, from the template and the request (uniform: into scalar registers)
    auto rq = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)req_s[i]); };
    RolloutArgs a_in = a_tpl;
#pragma unroll
    for (int i = 0; i < Env<ENV>::S; ++i) a_in.s0[i] = __builtin_bit_cast(float, rq(6 + i));
#pragma unroll
    for (int c = 0; c < Env<ENV>::C; ++c) a_in.u_prev[c] = __builtin_bit_cast(float, rq(14 + c));
    if (rq(2) == 0u) a_in.u_prev_dev = nullptr;
    const float* samples = reinterpret_cast<const float*>((unsigned long long)rq(4) | ((unsigned long long)rq(5) << 32));
#include "ctk_mppi_body.inc"
}
#undef CTK_BODY_EARLY_U

bool ctk_mppi_ahead_ok(int env, int N, int H, int P) {
    if (N < 1 || ctk_mppi_uses_throughput_kernel(CTK_PRED_ODE, N) || mppi_late_u()) return false;
    bool ok = false;
    CTK_FOR_ENV(env, EV, {
        const int blocks = (N + MPPI_TRAJ - 1) / MPPI_TRAJ;
        int stage_ok;
        const size_t lds = rollout_launch_lds(P, H, CTK_PRED_ODE, N, blocks, &stage_ok, Env<EV>::C);
        ok = stage_ok != 0 && mppi_env_form<EV>(blocks, P * Env<EV>::C, true) == 0 && lds + 256 <= 160 * 1024;   // (+ the gate's static words)
    });
    return ok;
}
const char* ctk_mppi_ahead_name(int env) { return ctk_kernel_name("ctk_mppi_ahead<%d>", env); }

hipError_t ctk_launch_mppi_ahead(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                 const float* u_nom, float* parts, const MppiFuse& fuse, const CtkAheadGate& gate) {
    const dim3 grid((a.N + MPPI_TRAJ - 1) / MPPI_TRAJ), block(MPPI_BLOCK);
    CTK_FOR_ENV(env, EV, {
        using E = Env<EV>;
        int stage_ok;
        const size_t lds = rollout_launch_lds(a.P, a.H, CTK_PRED_ODE, a.N, (int)grid.x, &stage_ok, E::C);
        if (!stage_ok || fuse.ll == nullptr || fuse.mode != 1) return hipErrorInvalidValue;   // the merge + update step with the {value, seq} tail only
        const FuseArgs fz = mppi_fuse_args(fuse, stage_ok, a, E::C, u_nom, fuse.u_nom_out);
        hipLaunchKernelGGL((ctk_mppi_ahead<EV>), grid, block, lds, st, gate.box, u_nom, a.interp, static_cast<const float*>(nullptr), parts, a.N, a.H, a.P,
                           ctk_magic_of(a.P * E::C), a, E::derive(params, dt, isteps), m, fz, gate);
    });
    return hipGetLastError();
}
