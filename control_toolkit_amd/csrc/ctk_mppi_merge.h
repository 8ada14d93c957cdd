// ctk_mppi_merge.h — the soft-min merge of MPPI partial records {rho, a, b[P]} (optimizer_mppi.py:163-168 re-associated) and the
// MPPI update, as device functions of ONE 256-thread workgroup: shared by ctk_mppi.hip (the merge kernels, the fused tail of
// ctk_mppi_rollout) and by the network template kernels (ctk_generic_net.hip, ctk_gru4.hip), whose MPPI launches end in the same
// low-latency hand-off (mppi_ll_tail below).
#pragma once
#include "ctk_device.h"
#include "ctk_common.h"

// ---------------------------------------------------------------------------------------------
// merge of partial records {rho, a, b[P]} by one 256-thread block.
// FINAL=false: writes one merged record to `out_rec`.
// FINAL=true : applies the MPPI update and publishes u.
// SC1: the records were handed over inside ONE launch (fused tail below): every load of them is an
//      agent-scope relaxed atomic load (global_load ... sc1), cdna_hip_programming.md G16.
// ---------------------------------------------------------------------------------------------
constexpr int MERGE_BLOCK = 256;
constexpr int MERGE_CHUNK = 1024;

// LD: 0 plain loads (records written by an earlier launch); 1 agent-scope (handed over inside ONE launch);
//     2 system-scope (records stored by peer GPUs into this GPU's uncached exchange buffer, ctk_mppi_p2p_exchange)
template <int LD>
CTK_DEV float ld_rec(const float* p) {
    if constexpr (LD == 1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (LD == 2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else return *p;
}
CTK_DEV void st_rec(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct MppiUpdateArgs {
    // per-step tables already resident in this block's LDS (fused tail) — nullptr: read them from memory
    // (un_l: the shifted nominal plan [H*C])
    const float* w0_l = nullptr; const float* w1_l = nullptr; const float* un_l = nullptr; const int* i0_l = nullptr;
    int H;
    const InterpEntry* interp;
    const float* u_nom_in;
    float* u_nom_out;
    float lo, hi;          // C == 1
    float* u_dev;
    float* u_host;
    uint32_t seq;
    int C = 1;             // control inputs: records carry b[P*C], the update runs per channel
    float lo_c[CTK_MAX_INPUTS] = {}, hi_c[CTK_MAX_INPUTS] = {};   // C > 1
};
// ... of an in-launch tail (host side): tables from memory, the limits of `a`'s C inputs
inline MppiUpdateArgs mppi_update_args(const RolloutArgs& a, int C, const float* u_nom_in, float* u_nom_out, float* u_dev, float* u_host, uint32_t seq) {
    MppiUpdateArgs up{nullptr, nullptr, nullptr, nullptr, a.H, a.interp, u_nom_in, u_nom_out, a.lo[0], a.hi[0], u_dev, u_host, seq};
    up.C = C;
    for (int c = 0; c < C; ++c) { up.lo_c[c] = a.lo[c]; up.hi_c[c] = a.hi[c]; }
    return up;
}

// entry h of the MPPI update, C == 1: u_nom[h] <- clip(shift(u_nom)[h] + interp(b)[h] / a) (optimizer_mppi.py:184, :190).  ONE function
// for the final update and for the early form of entry 0 (mppi_early_u), so that both are the same operations
CTK_DEV float mppi_update_entry(float b0, float b1, float w0, float w1, float a_tot, float un, float lo, float hi) {
    const float w = (b0 * w0 + b1 * w1) / a_tot;
    return fminf(fmaxf(un + w, lo), hi);   // optimizer_mppi.py:190
}

// rows w*RPW .. w*RPW+RPW-1 of column p of a block record's numerator, b_b[p] = sum_r e_r * tile[r][p]: ONE function for the epilogue's
// full pass and for the two columns that wave 0 forms ahead of it, so that both sum in the same order with the same contraction
// (mppi_col_sum: the arithmetic — acc = e_r * tile_r + acc from zero over r = 0 .. RPW-1 — whatever the operands come from)
template <int RPW, class FE, class FT>
CTK_DEV float mppi_col_sum(FE e_at, FT tile_at) {
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < RPW; ++r) acc += e_at(r) * tile_at(r);
    return acc;
}
template <int RPW>
CTK_DEV float mppi_col_partial(const float* e_s, const float* tile, int ts, int w, int p) {
    return mppi_col_sum<RPW>([&](int r) { return e_s[w * RPW + r]; }, [&](int r) { return tile[(w * RPW + r) * ts + p]; });
}
// ... the early form's operands: the column's RPW tile values are in registers already (read under the soft-min partial, they do not
// depend on J), the row group's RPW weights come out of e_s in 16-byte reads (contiguous, 64-byte aligned: ONE wait in front of the sum)
template <int RPW>
CTK_DEV void mppi_col_tile_regs(float (&tv)[RPW], const float* tile, int ts, int w, int p) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) tv[r] = tile[(w * RPW + r) * ts + p];
}
template <int RPW>
CTK_DEV float mppi_col_partial_regs(const float* e_s, const float (&tv)[RPW], int w) {
    static_assert(RPW % 4 == 0, "the weights of a row group are read as float4");
    float ev[RPW];
#pragma unroll
    for (int q = 0; q < RPW / 4; ++q) {
        const float4 e4 = reinterpret_cast<const float4*>(e_s + w * RPW)[q];
        ev[4 * q] = e4.x; ev[4 * q + 1] = e4.y; ev[4 * q + 2] = e4.z; ev[4 * q + 3] = e4.w;
    }
    return mppi_col_sum<RPW>([&](int r) { return ev[r]; }, [&](int r) { return tv[r]; });
}

// scratch: >= 8 + (P + 1) + min(cnt, MERGE_CHUNK) floats of LDS, plus cnt*(2+P) more when `stage`
// (all records fetched into LDS by ONE wide pass: one memory round trip instead of one per record).
// CH: control inputs of the FINAL update (compile time: the C == 1 instantiations are CartPole's statement sequence, unchanged)
// MANY: the sliced column sums of many narrow records are compiled in (a caller that never merges more than 128 records leaves them out)
// PUB: the FINAL update publishes u (false: entry 0 went out ahead of the plan update, mppi_early_u; C == 1 only)
// REL: ... with publish_u's system-scope release — the callers whose kernel does NOT end behind the publish (the resident kernel, the
//      peer-to-peer exchange); every launched form takes the relaxed publish (ctk_device.h: publish_u_launched)
template <bool FINAL, int SC1, int CH = 1, bool MANY = true, bool PUB = true, bool REL = false>
CTK_DEV void mppi_merge_block(float* scratch, const float* base, int cnt, int P, float neg_inv_lbd, float* out_rec,
                              const MppiUpdateArgs& up, int stage) {
    float* red = scratch;             // [4] cross-wave scratch
    float* b_s = scratch + 8;         // [P + 1] merged numerator
    float* sc_s = b_s + P + 1;        // [chunk] per-record rescale factors
    float* st_s = sc_s + (cnt < MERGE_CHUNK ? cnt : MERGE_CHUNK);   // [cnt][2+P] staged records
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int rs = 2 + P;
    if (stage == 1) {
        const int tot = cnt * rs;
        for (int i0 = 0; i0 < tot; i0 += 4 * MERGE_BLOCK) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j * MERGE_BLOCK + t;
                if (i < tot) v[j] = ld_rec<SC1>(base + i);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j * MERGE_BLOCK + t;
                if (i < tot) st_s[i] = v[j];
            }
        }
        __syncthreads();
    }
    auto rec_at = [&](int i, int f) -> float { return stage != 0 ? st_s[i * rs + f] : ld_rec<SC1>(base + (size_t)i * rs + f); };

    float r = INFINITY;
    for (int i = t; i < cnt; i += MERGE_BLOCK) r = fminf(r, rec_at(i, 0));
    r = wave_min(r);
    if (lane == 0) red[wave] = r;
    __syncthreads();
    const float rho = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    __syncthreads();

    float a_acc = 0.0f;
    float b_acc[4] = {0.f, 0.f, 0.f, 0.f};   // thread t owns columns t, t+256, ... (P <= 1024)
    for (int c0 = 0; c0 < cnt; c0 += MERGE_CHUNK) {
        const int cn = min(MERGE_CHUNK, cnt - c0);
        for (int i = t; i < cn; i += MERGE_BLOCK) {
            const float sc = expf(neg_inv_lbd * (rec_at(c0 + i, 0) - rho));   // e^{-(rho_r - rho)/lambda}
            sc_s[i] = sc;
            a_acc += rec_at(c0 + i, 1) * sc;
        }
        __syncthreads();
        if (MANY && stage != 0 && cnt > 128 && cnt <= MERGE_CHUNK && 2 * P <= MERGE_BLOCK) {
            // many narrow records (a shard of configs[4]: 256 records of 11 columns): one thread per column would walk all of them with
            // 245 threads idle.  Thread (slice, column) sums every slices-th record; the slices meet through LDS in slice order.
            // (cnt > 128 with staged records did not exist before round 4: no earlier result changes its association)
            const int slices = MERGE_BLOCK / P, sl = t / P, p = t - sl * P;
            float* part_s = st_s + (size_t)cnt * rs;           // [slices][P], behind the staged records (merge_lds_staged reserves it)
            if (sl < slices) {
                float acc = 0.0f;
                for (int i = sl; i < cn; i += slices) acc += rec_at(i, 2 + p) * sc_s[i];
                part_s[sl * P + p] = acc;
            }
            __syncthreads();
            if (t < P) {
                float acc = 0.0f;
                for (int q = 0; q < slices; ++q) acc += part_s[q * P + t];
                b_acc[0] = acc;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = t + j * MERGE_BLOCK;
                if (p < P) {
                    float acc = b_acc[j];
                    for (int i = 0; i < cn; ++i) acc += rec_at(c0 + i, 2 + p) * sc_s[i];
                    b_acc[j] = acc;
                }
            }
        }
        __syncthreads();
    }
    a_acc = wave_sum(a_acc);
    if (lane == 0) red[wave] = a_acc;
    __syncthreads();
    const float a_tot = red[0] + red[1] + red[2] + red[3];

    if constexpr (!FINAL) {
        if (t == 0) { out_rec[0] = rho; out_rec[1] = a_tot; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = t + j * MERGE_BLOCK;
            if (p < P) out_rec[2 + p] = b_acc[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = t + j * MERGE_BLOCK;
            if (p < P) b_s[p] = b_acc[j];
        }
        if (t == 0) b_s[P] = 0.0f;   // pad read by i0+1 when P == 1
        __syncthreads();
        if constexpr (CH == 1) {
            for (int h = t; h < up.H; h += MERGE_BLOCK) {
                InterpEntry e; float un;
                if (up.w0_l) { e = InterpEntry{up.i0_l[h], up.w0_l[h], up.w1_l[h]}; un = up.un_l[h]; }
                else { e = up.interp[h]; un = up.u_nom_in[min(h + 1, up.H - 1)]; }
                const float o = mppi_update_entry(b_s[e.i0], b_s[e.i0 + 1], e.w0, e.w1, a_tot, un, up.lo, up.hi);
                up.u_nom_out[h] = o;
                if constexpr (PUB) {
                    if (h == 0) {                            // :191 u = u_nom[0,0,:]
                        if constexpr (REL) publish_u(up.u_dev, up.u_host, o, up.seq);
                        else publish_u_launched(up.u_dev, up.u_host, o, up.seq);
                    }
                }
            }
        } else {
            static_assert(PUB, "the early form of entry 0 is the C == 1 update's");
            // P here = P*C record columns; inducing point i of channel c is column i*C + c
            constexpr int C = CH;
            const int Pp = P / C;
            float* u_s = scratch;             // red[] is dead: the C outputs of step 0
            for (int hc = t; hc < up.H * C; hc += MERGE_BLOCK) {
                const int h = hc / C, c = hc - h * C;
                InterpEntry e; float un;
                if (up.w0_l) { e = InterpEntry{up.i0_l[h], up.w0_l[h], up.w1_l[h]}; un = up.un_l[hc]; }
                else { e = up.interp[h]; un = up.u_nom_in[min(h + 1, up.H - 1) * C + c]; }
                const int i1 = min(e.i0 + 1, Pp - 1);
                const float w = (b_s[e.i0 * C + c] * e.w0 + b_s[i1 * C + c] * e.w1) / a_tot;
                const float o = fminf(fmaxf(un + w, up.lo_c[c]), up.hi_c[c]);   // optimizer_mppi.py:190
                up.u_nom_out[hc] = o;
                if (h == 0) u_s[c] = o;
            }
            __syncthreads();
            if (t == 0) {                                    // :191 u = u_nom[0,0,:]
                if constexpr (REL) publish_u_vec(up.u_dev, up.u_host, u_s, C, up.seq);
                else publish_u_vec_launched(up.u_dev, up.u_host, u_s, C, up.seq);
            }
        }
    }
}


// start of the staged records inside the merge scratch (see mppi_merge_block)
CTK_DEV float* merge_stage_ptr(float* scratch, int cnt, int P) { return scratch + 8 + (P + 1) + (cnt < MERGE_CHUNK ? cnt : MERGE_CHUNK); }

// Low-latency hand-off of a record word: value and the launch's sequence number travel in ONE 8-byte store, so
// the reader polls the data itself — no "drain my stores, then signal" step and no ticket (cf. RCCL's LL protocol).
CTK_DEV void ll_store(unsigned long long* p, float v, uint32_t seq) {
    __hip_atomic_store(p, ((unsigned long long)seq << 32) | (unsigned long long)__builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// One batch of a thread's {value, seq} words, i0 + j*STRIDE < tot (j < LLW), polled until each carries `seq`, then staged as floats in
// st[]: ONE bounded loop whose every pass (re)loads the words that have not arrived — the first pass is one pipelined batch of LLW loads —
// checks them and sleeps once.  Returns true when the bound ran out with a word missing (staged as NaN).
constexpr int LL_POLL_SPINS = 1 << 22;
template <int LLW, int STRIDE>
CTK_DEV bool ll_poll_stage(const unsigned long long* ll, float* st, int i0, int tot, uint32_t seq) {
    unsigned long long w[LLW];
    unsigned pend = 0;
#pragma unroll
    for (int j = 0; j < LLW; ++j) pend |= (i0 + j * STRIDE < tot ? 1u : 0u) << j;
    for (int spin = 0;; ++spin) {
#pragma unroll
        for (int j = 0; j < LLW; ++j)
            if ((pend >> j) & 1u) w[j] = __hip_atomic_load(ll + i0 + j * STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int j = 0; j < LLW; ++j)
            if (((pend >> j) & 1u) && (uint32_t)(w[j] >> 32) == seq) pend &= ~(1u << j);
        if (pend == 0 || spin >= LL_POLL_SPINS) break;
        __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int j = 0; j < LLW; ++j) {
        const int i = i0 + j * STRIDE;
        if (i < tot) st[i] = ((pend >> j) & 1u) ? __builtin_nanf("") : __builtin_bit_cast(float, (uint32_t)w[j]);
    }
    return pend != 0;
}
// ... as a function of its own, for the 4-wave rollout kernel (ctk_mppi_body_5_post.inc).  Only block 0 runs the poll, once, at the very
// end of the launch, but inlined its divergent loop takes part in the scheduling and register allocation of the whole kernel: with it
// the cold (checked sin / cos) recurrence loop of ctk_mppi_rollout<0, 0, false, false> came out in another block layout and four more
// SGPRs were spilled.  One call (no stack: the callee keeps to registers) costs the tail nothing that can be measured.
template <int LLW, int STRIDE>
__device__ __attribute__((noinline)) bool ll_poll_stage_call(const unsigned long long* ll, float* st, int i0, int tot, uint32_t seq) {
    return ll_poll_stage<LLW, STRIDE>(ll, st, i0, tot, seq);
}

// Entry 0 of the MPPI update AHEAD of the plan update (C == 1, at most 64*NB block records): ONE wave (all 64 lanes) of the merging
// workgroup polls, of every block's record, only the four words that entry needs — rho_b, a_b and the columns c0 = i0(0) and c0 + 1
// (c0 + 1 == P: the zero pad, no word) — and merges them in registers: lane i % 64 holds block i.  No LDS, no barrier.  The association
// is mppi_merge_block's for cnt <= 128 (thread t = record t there): rho the min over all blocks, sc_i = expf(neg_inv_lbd*(rho_i - rho)),
// a_tot = red[0] + red[1] + red[2] + red[3] with red[k] the wave_sum of lanes' a_i*sc_i of batch k (zero for an absent batch), the two
// columns as acc += rec_i * sc_i over i = 0 .. nb-1 from zero; then mppi_update_entry.  The value is therefore bit for bit the
// u_nom_out[0] that the final update stores later.  *expired: the bounded poll ran out (the missing words enter as NaN, as in the tail).
//
// The poll is a software pipeline of LL_EARLY_DEPTH passes: a ring of LL_EARLY_DEPTH x NB x 4 words in registers, statically unrolled.
// A pass loads every lane's eight words into its slot; while it is outstanding the next pass goes out into the next slot, one sleep
// behind it, and the OLDEST pass is checked behind a partial wait (loads return in order: vmcnt(loads of the younger passes)).  A word
// seen keeps the value of the pass that saw it (v[][]); a slot whose pass missed a word is issued again.  The loop ends on the first
// pass after which every word is there; a younger pass still in flight is not used and not waited for (its registers are dead).  A
// single-pass poll pays one full memory round trip per look, so a block that lags block 0 by a few hundred cycles costs u a second
// round trip; here the second look follows the first by the sleep.  The slots start with a sequence number that cannot match, so
// the first LL_EARLY_DEPTH - 1 checks are of nothing and the loop needs no prologue of loads (the kernel body keeps to 4 x NB x
// LL_EARLY_DEPTH polling loads: tests/test_mppi_recurrence_isa.py).  Bound: LL_POLL_SPINS passes, as before.
// stamps (diagnostic builds, tools/diag_mppi_stamps.hip): [12] first pass issued, [13] the pass that completed returned, [14] passes issued.
#ifdef CTK_STAMPS
CTK_DEV unsigned long long ll_stamp_time() {          // (kept in a register: a store inside the poll would join its loads' counter)
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#endif
constexpr int LL_EARLY_DEPTH = 2;
#ifndef CTK_EARLY_POLL_SLEEP
#define CTK_EARLY_POLL_SLEEP 1          // s_sleep argument between two issues (0: none)
#endif
template <int NB, int D = LL_EARLY_DEPTH>
CTK_DEV float mppi_early_u(const unsigned long long* ll, int nb, int P, int c0, float w0, float w1, float un, float neg_inv_lbd,
                           float lo, float hi, uint32_t seq, bool* expired, [[maybe_unused]] unsigned long long* stamps = nullptr) {
    const int lane = threadIdx.x & 63, rs = 2 + P;
    const bool has1 = c0 + 1 < P;
    unsigned long long w[D][NB][4];
    float v[NB][4];
    unsigned pend = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        if (k * 64 + lane < nb) pend |= (has1 ? 0xFu : 0x7u) << (4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[k][j] = __builtin_nanf("");
#pragma unroll
            for (int d = 0; d < D; ++d) w[d][k][j] = (unsigned long long)~seq << 32;
        }
    }
    int spin = 0;                             // passes issued
#ifdef CTK_STAMPS
    unsigned long long t_first = 0;
#endif
    // Every lane loads its eight words in every pass, from addresses that are in bounds for every lane (an absent block: the last
    // one; the absent fourth word: the third again), and the loop's exit is the wave's: there is NO branch around a load, which is
    // what lets the compiler count the younger pass (behind a branch it waits vmcnt(0) at the join).  What a pass may TAKE is still
    // only a word not yet seen: `pend` guards the check.
    const unsigned long long* rl[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) rl[k] = ll + (size_t)min(k * 64 + lane, nb - 1) * rs;
    const int o2 = c0 + 2, o3 = has1 ? c0 + 3 : c0 + 2;
    auto issue = [&](int d) {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[d][k][j] = __hip_atomic_load(rl[k] + (j < 2 ? j : j == 2 ? o2 : o3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        ++spin;
    };
    auto check = [&](int d) {
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((pend >> (4 * k + j)) & 1u) && (uint32_t)(w[d][k][j] >> 32) == seq) {
                    v[k][j] = __builtin_bit_cast(float, (uint32_t)w[d][k][j]);
                    pend &= ~(1u << (4 * k + j));
                }
    };
    [&] {
#pragma nounroll
        for (;;) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                issue((d + D - 1) % D);       // the youngest pass goes out ...
#ifdef CTK_STAMPS
                if (spin == 1) t_first = ll_stamp_time();
#endif
                check(d);                     // ... and the oldest is looked at: D - 1 passes stay in flight
                if (__builtin_amdgcn_ballot_w64(pend != 0) == 0 || spin >= LL_POLL_SPINS + D - 1) return;
                if constexpr (CTK_EARLY_POLL_SLEEP > 0) __builtin_amdgcn_s_sleep(CTK_EARLY_POLL_SLEEP);
            }
        }
    }();
#ifdef CTK_STAMPS
    const unsigned long long t_done = ll_stamp_time();
    if (threadIdx.x == 0 && stamps) { stamps[12] = t_first; stamps[13] = t_done; stamps[14] = (unsigned long long)spin; }   // block 0's row
#endif
    *expired = __builtin_amdgcn_ballot_w64(pend != 0) != 0;
    auto val = [&](int k, int j) { return v[k][j]; };      // (a word never seen: NaN)

    float red[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
#pragma unroll
    for (int k = 0; k < NB; ++k) red[k] = wave_min(k * 64 + lane < nb ? val(k, 0) : INFINITY);
    const float rho = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));

    float sc[NB];
    float asum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        float a_acc = 0.0f;
        sc[k] = 0.0f;
        if (k * 64 + lane < nb) {
            sc[k] = expf(neg_inv_lbd * (val(k, 0) - rho));   // e^{-(rho_r - rho)/lambda}
            a_acc += val(k, 1) * sc[k];
        }
        asum[k] = wave_sum(a_acc);
    }
    const float a_tot = asum[0] + asum[1] + asum[2] + asum[3];

    float b0 = 0.0f, b1 = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int v0 = __builtin_bit_cast(int, val(k, 2)), v1 = __builtin_bit_cast(int, has1 ? val(k, 3) : 0.0f), vs = __builtin_bit_cast(int, sc[k]);
        const int cn = max(0, min(64, nb - k * 64));   // (an absent batch: none)
        auto add = [&](int i) {               // record k*64 + i: i ascending from zero, the same two accumulators
            const float s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vs, i));
            b0 += __builtin_bit_cast(float, __builtin_amdgcn_readlane(v0, i)) * s;
            b1 += __builtin_bit_cast(float, __builtin_amdgcn_readlane(v1, i)) * s;
        };
        // whole chunks of 16 records with constant lane numbers (straight-line: no compare and branch per record; 16 blocks = one
        // chunk), then a rolled remainder
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (cn >= 16 * (q + 1)) {
#pragma unroll
                for (int j = 0; j < 16; ++j) add(16 * q + j);
            }
        }
        for (int i = cn & ~15; i < cn; ++i) add(i);
    }
    return mppi_update_entry(b0, b1, w0, w1, a_tot, un, lo, hi);
}

// The fused tail of an MPPI rollout launch of 256-thread workgroups whose blocks have published their records as {value, seq} words
// (ll_store): called by block 0 (all threads, after a barrier that retires its own use of `lds`), which polls every word until it
// carries this launch's sequence number — the words ARE the data — stages them in LDS, merges, and either applies the update and
// publishes u (mode 1) or writes the shard's ONE record (mode 2).  lds: merge_lds_staged(P, nb) bytes.  A bounded poll that runs out
// raises the error word behind {u, seq}: ctk_api.hip:finish_step returns CTK_ERR_STATE.
template <int CH>
CTK_DEV void mppi_ll_tail(float* lds, const unsigned long long* ll, int nb, int P, float neg_inv_lbd, int mode, float* out_rec,
                          const MppiUpdateArgs& up) {
    const int t = threadIdx.x, tot = nb * (2 + P);
    float* st = merge_stage_ptr(lds, nb, P);
    bool expired = false;
    for (int i0 = t; i0 < tot; i0 += MERGE_BLOCK * 8) expired |= ll_poll_stage<8, MERGE_BLOCK>(ll, st, i0, tot, up.seq);   // 8 words in flight per thread
    if (expired && up.u_host) host_word_store(up.u_host, 2, 2u);   // (drained ahead of the barrier: the merge's publish cannot overtake it)
    __syncthreads();
    if (mode == 1) mppi_merge_block<true, 0, CH>(lds, nullptr, nb, P, neg_inv_lbd, nullptr, up, 2);
    else mppi_merge_block<false, 0, CH>(lds, nullptr, nb, P, neg_inv_lbd, out_rec, up, 2);
}

// kernel argument of the network template kernels' MPPI launches (ctk_generic_net.hip, ctk_gru4.hip): mode 0 = block records only
struct NetFuse {
    int mode = 0;                       // 1 merge + update + publish u; 2 merge into ONE record (sharded step_begin)
    unsigned long long* ll = nullptr;   // [blocks][2 + P*C] {value, seq} words
    float* out_rec = nullptr;           // mode 2
    MppiUpdateArgs up{};
};

// LDS of a merge by one workgroup (bytes); with all records staged in LDS (used when it stays <= 64 KiB)
inline size_t merge_lds(int P, int cnt) { return (size_t)(8 + P + 1 + (cnt < MERGE_CHUNK ? cnt : MERGE_CHUNK)) * sizeof(float); }
inline size_t merge_lds_staged(int P, int cnt) { return merge_lds(P, cnt) + ((size_t)cnt * (2 + P) + MERGE_BLOCK) * sizeof(float); }   // (+ the column slices' partial sums)
inline bool merge_can_stage(int P, int cnt) { return merge_lds_staged(P, cnt) <= 64 * 1024; }
