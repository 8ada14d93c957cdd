// ctk_affine_body.h — the body of the 4-wave affine rollout kernels, u[n,h] = clip(base[h] + sample[n,h] * scale[h]), with its workgroup
// anatomy and LDS carve.  Translation units that wrap it: ctk_sampled.hip (ctk_affine_rollout, ctk_affine_rollout_mix: a handle's CEM,
// random-action and plain rollouts) and ctk_batch_rollout.hip (ctk_batch_rollout: the batch families' rollouts of caller-supplied plans).
// The text is what stood in ctk_sampled.hip; include it behind ctk_rollout.h, ctk_env.h, ctk_mlp.h, ctk_gru.h and ctk_launch.h.
#pragma once

constexpr int SAMP_TRAJ = 64;                 // trajectories per block
constexpr int SAMP_WAVES = 4;
constexpr int SAMP_BLOCK = SAMP_TRAJ * SAMP_WAVES;

// Same anatomy as ctk_mppi_rollout (ctk_mppi.hip): 4-wave prologues (coalesced sample tile -> LDS; inputs
// of all H steps, input-only cost terms, coalesced write of the plans Q), then the recurrence on one
// wave (ODE, one trajectory per lane) or on all four (MLP, 16 trajectories per wave on MFMA).
// GRU: the four waves share ONE 16-trajectory column block (ctk_gru.h), so a workgroup owns 16 trajectories.
// LDS carve (floats): tile[TRAJ][ts] | ubuf[TRAJ][us] | cin[256/TRAJ][TRAJ] | base[H] | scale[H] | (GRU) exchange slots
// H here = H*C flat (step, input) columns of a plan (C control inputs; CartPole: C = 1)
__host__ __device__ inline int affine_carve_floats(int H, int traj) {
    const int f = traj * tile_stride(H) + traj * ((H + 1) | 1) + SAMP_BLOCK + 2 * H;
    return (f + 3) & ~3;
}
__host__ __device__ inline int affine_traj(int pred) { return pred == CTK_PRED_GRU ? GRU_TRAJ : SAMP_TRAJ; }

// Optional in-launch arg-min tail (random-action, optimizer_random_action_tf.py:62-68: u = first input of the cheapest
// plan): every block hands {key(J), index, first input} of its cheapest rollout to block 0 as {payload, sequence number}
// words (the hand-off form of ctk_mppi.hip), block 0 picks the global minimum under the total order (J, index) — what
// ctk_select_topk(K = 1) + ctk_g_pick_best_first do in two more launches — and publishes u.
struct BestArgs {
    unsigned long long* ll;   // [blocks][2 + C] words {key, index, first input[C]}; nullptr: no tail
    uint32_t seq;
    float* u_dev;
    float* u_host;
    int* idx_out;
};
CTK_DEV void ll_put(unsigned long long* p, uint32_t payload, uint32_t seq) {
    __hip_atomic_store(p, ((unsigned long long)seq << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// *expired is raised when the bounded poll runs out (the payload is then stale: the caller reports it, see below)
CTK_DEV uint32_t ll_get(const unsigned long long* p, uint32_t seq, bool* expired) {
    unsigned long long w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int spin = 0; (uint32_t)(w >> 32) != seq && spin < (1 << 22); ++spin) {
        __builtin_amdgcn_s_sleep(1);
        w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if ((uint32_t)(w >> 32) != seq) *expired = true;
    return (uint32_t)w;
}

// ENV: the environment (ctk_env.h); the analytic-predictor instantiation is written against Env<ENV> only (C control inputs:
// H*C sample columns and inputs per trajectory, per-channel base / scale / clip; recurrence through Env::cost_step); the network
// predictors' instantiations are CartPole's.  P_ = H*C sample columns of a row, pmagic_ its magic.
// MIX (CEM-GMM, optimizer_cem_gmm_tf.py:59-60; analytic predictor only): the population is drawn from a mixture of TWO diagonal
// Gaussians, one component per ROW.  base / scale point at component 0's tables inside the mixture state mu[2][HC] | std[2][HC] | probs[2]
// (base = mu, scale = std: component 1's tables lie HC floats further, probs[0] at base[4*HC]); both components are staged in LDS
// (component 1 behind the carve, where the GRU's exchange slots would be) and input_at picks by the row's component:
// 0 iff uniform[n] < probs[0], uniform[n] from `uniforms` or word 0 of the Philox block (row, 0, call, ustream).
template <int ENV, int PRED, bool WTRAJ, bool MIX>
CTK_DEV void affine_rollout_body(const float* __restrict__ samples, const float* __restrict__ base, const float* __restrict__ scale,
                                 const float* __restrict__ wperm, int rng_kind, int N_, int H_, int P_, uint32_t pmagic_,
                                 const RolloutArgs& a_in, const typename Env<ENV>::K& k, const BestArgs& best,
                                 const float* __restrict__ uniforms, uint32_t ustream) {
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    static_assert(PRED == CTK_PRED_ODE || ENV == CTK_ENV_CARTPOLE, "network predictors: CartPole instantiations only");
    static_assert(!MIX || PRED == CTK_PRED_ODE, "mixture sampling: analytic predictor only");
    extern __shared__ float lds[];
    RolloutArgs a = a_in;
    a.N = N_; a.H = H_; a.P = P_; a.p_magic = pmagic_;
    constexpr int TRAJ = (PRED == CTK_PRED_GRU) ? GRU_TRAJ : SAMP_TRAJ;
    constexpr int CHUNKS = SAMP_BLOCK / TRAJ;
    const int H = a.H, HC = H * C, ts = tile_stride(a.P), us = (HC + 1) | 1;   // a.P == H*C here: one sample per step and input
    float* tile = lds;
    float* ubuf = tile + TRAJ * ts;
    float* cin_s = ubuf + TRAJ * us;
    float* base_s = cin_s + SAMP_BLOCK;
    float* scale_s = base_s + HC;
    float* gru_ex = lds + affine_carve_floats(HC, TRAJ);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * TRAJ;
    const int n = row0 + lane;
    const bool valid = lane < TRAJ && n < a.N;

    load_tile_early<TRAJ, SAMP_BLOCK>(tile, samples, a, row0, 1.0f, rng_kind, [&] {
        for (int h = t; h < HC; h += SAMP_BLOCK) {
            base_s[h] = base[h]; scale_s[h] = scale[h];
            if constexpr (MIX) { gru_ex[h] = base[HC + h]; gru_ex[HC + h] = scale[HC + h]; }
        }
    });
    __syncthreads();
    const float* mbase = base_s;       // the tables this thread's trajectory (ODE: trajectory = lane) is drawn from
    const float* mscale = scale_s;
    if constexpr (MIX) {
        float u01 = 0.0f;
        if (uniforms != nullptr) { if (n < a.N) u01 = uniforms[n]; }
        else u01 = u32_unit_halfopen(philox4x32_10(U4{(uint32_t)(a.global_row0 + n), 0u, a.call, ustream}, a.seed_lo, a.seed_hi).x);
        if (!(u01 < base[4 * HC])) { mbase = gru_ex; mscale = gru_ex + HC; }
    }

    // inputs of the steps [hbeg, hend) of trajectory ptraj into ubuf + their input-only stage-cost terms (returned)
    auto prepare = [&](int ptraj, int hbeg, int hend) {
        const float* my = tile + ptraj * ts;
        auto input_at = [&](int h, int c) { return fminf(fmaxf(mbase[h * C + c] + my[h * C + c] * mscale[h * C + c], a.lo[c]), a.hi[c]); };
        float cin = 0.0f;
        float uprev[C];
#pragma unroll
        for (int c = 0; c < C; ++c)
            uprev[c] = (hbeg == 0 || hbeg >= H) ? (a.u_prev_dev ? a.u_prev_dev[c] : a.u_prev[c]) : input_at(hbeg - 1, c);
#pragma unroll 2
        for (int h = hbeg; h < hend; ++h) {
            float u[C];
#pragma unroll
            for (int c = 0; c < C; ++c) u[c] = input_at(h, c);
            cin += E::input_cost(k, u, uprev);
#pragma unroll
            for (int c = 0; c < C; ++c) { uprev[c] = u[c]; ubuf[ptraj * us + h * C + c] = u[c]; }
        }
        return cin;
    };
    // the plans, coalesced: Q[row0*H + i] for the block's contiguous span (elite refit / logging read it)
    auto write_plans = [&](int first, int stride) {
        const int total = min(TRAJ, a.N - row0) * HC;
        float* dst = a.Q_out + (size_t)row0 * HC;
        for (int i = first; i < total; i += stride) {
            const int r = HC >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i;
            dst[i] = ubuf[r * us + (i - r * HC)];
        }
    };

    if constexpr (PRED == CTK_PRED_ODE) {
        // Two phases, as in ctk_mppi_rollout: all four waves prepare the first S1 steps; then wave 0 runs the recurrence
        // over them while waves 1..3 prepare the rest; they meet when wave 0 reaches step S1, after which waves 1..3
        // write the plans out while wave 0 finishes the horizon.  Per-wave sums of the input-only terms: a wave's
        // phase-A part is carried into its phase-B sum (slot = wave).
        const int S1 = min(H, 16), Ha = (S1 + SAMP_WAVES - 1) / SAMP_WAVES;
        const float cin_a = prepare(lane, min(S1, wave * Ha), min(S1, wave * Ha + Ha));
        if (wave == 0) cin_s[lane] = cin_a;
        __syncthreads();
        const float* myu = ubuf + lane * us;
        float sx[S];
#pragma unroll
        for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
        float csum = 0.0f, amax = 0.0f;
        float* traj = nullptr;
        if constexpr (WTRAJ) {
            if (a.traj_out) traj = a.traj_out + (size_t)n * (H + 1) * S;
        }
        const bool single = E::fast_ok(k);
        if (wave == 0) {
            if (single) recur_env_range<ENV, WTRAJ, true, true>(k, traj, valid, myu, 0, S1, sx, csum, amax);
        } else {
            const int Hb = (H - S1 + SAMP_WAVES - 2) / (SAMP_WAVES - 1);
            cin_s[wave * SAMP_TRAJ + lane] = cin_a + prepare(lane, min(H, S1 + (wave - 1) * Hb), min(H, S1 + (wave - 1) * Hb + Hb));
        }
        __syncthreads();
        if (wave == 0) {
            float J = 0.0f;
            if (single) {
                recur_env_range<ENV, WTRAJ, true, true>(k, traj, valid, myu, S1, H, sx, csum, amax);
                if constexpr (WTRAJ) {
                    if (valid && traj) store_state<S>(traj + (size_t)H * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
            if (!single || __builtin_expect(__builtin_amdgcn_ballot_w64(E::out_of_range(amax)) != 0, 0)) {
#pragma unroll
                for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
                csum = 0.0f;
                recur_env_range<ENV, WTRAJ, false, true>(k, traj, valid, myu, 0, H, sx, csum, amax);
                if constexpr (WTRAJ) {
                    if (valid && traj) store_state<S>(traj + (size_t)H * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
            J += (cin_s[lane] + cin_s[SAMP_TRAJ + lane]) + (cin_s[2 * SAMP_TRAJ + lane] + cin_s[3 * SAMP_TRAJ + lane]);
            J *= a.inv_Hp1;
            if (valid) a.J[n] = J;
            if (best.ll) {
                const uint32_t key = valid ? f32_sortable(J) : 0xFFFFFFFFu;
                const uint32_t kmin = wave_min_u32(key);
                const uint32_t imin = wave_min_u32(key == kmin && valid ? (uint32_t)n : 0x7FFFFFFFu);   // ties: smallest index
                constexpr int BW = 2 + C;           // words per workgroup: key, index, the plan's first input [C]
                if (lane == 0) {
                    unsigned long long* r = best.ll + (size_t)blockIdx.x * BW;
                    ll_put(r, kmin, best.seq);
                    ll_put(r + 1, imin, best.seq);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        ll_put(r + 2 + c, imin < (uint32_t)a.N ? __builtin_bit_cast(uint32_t, ubuf[(imin - (uint32_t)row0) * us + c]) : 0u, best.seq);
                }
                if (blockIdx.x == 0) {              // every block finishes unconditionally: the polls terminate (and are bounded)
                    uint32_t bk = 0xFFFFFFFFu, bi = 0x7FFFFFFFu, bu[C] = {};
                    bool expired = false;
                    for (int b = lane; b < (int)gridDim.x; b += 64) {
                        const uint32_t kb = ll_get(best.ll + (size_t)b * BW, best.seq, &expired), ib = ll_get(best.ll + (size_t)b * BW + 1, best.seq, &expired);
                        uint32_t ub[C];
#pragma unroll
                        for (int c = 0; c < C; ++c) ub[c] = ll_get(best.ll + (size_t)b * BW + 2 + c, best.seq, &expired);
                        if (kb < bk || (kb == bk && ib < bi)) {
                            bk = kb; bi = ib;
#pragma unroll
                            for (int c = 0; c < C; ++c) bu[c] = ub[c];
                        }
                    }
                    // a stale record may have won or lost wrongly: tell the host (ctk_api.hip:finish_step -> CTK_ERR_STATE)
                    if (expired) host_word_store(best.u_host, 2, 2u);   // (drained by this wave, whose winner lane stores the flag below)
                    const uint32_t gk = wave_min_u32(bk);
                    const uint32_t gi = wave_min_u32(bk == gk ? bi : 0x7FFFFFFFu);
                    if (bk == gk && bi == gi) {     // exactly one lane holds the winner
                        best.idx_out[0] = (int)gi;
                        if constexpr (C == 1) publish_u_launched(best.u_dev, best.u_host, __builtin_bit_cast(float, bu[0]), best.seq);
                        else {
                            float uo[C];
#pragma unroll
                            for (int c = 0; c < C; ++c) uo[c] = __builtin_bit_cast(float, bu[c]);
                            publish_u_vec_launched(best.u_dev, best.u_host, uo, C, best.seq);
                        }
                    }
                }
            }
        } else {
            write_plans(t - 64, SAMP_BLOCK - 64);
        }
        return;
    }

    {   // network predictors: inputs of all H steps first; thread (trajectory t % TRAJ, chunk t / TRAJ)
        const int ptraj = t % TRAJ, chunk = t / TRAJ;
        const int Hc = (H + CHUNKS - 1) / CHUNKS;
        cin_s[chunk * TRAJ + ptraj] = prepare(ptraj, min(H, chunk * Hc), min(H, chunk * Hc + Hc));
    }
    __syncthreads();
    write_plans(t, SAMP_BLOCK);

    if constexpr (PRED == CTK_PRED_MLP) {
        const int tr = wave * CTK_MLP_TRAJ_PER_WAVE + (lane & 15);
        const float* myu = ubuf + tr * us;
        const MlpFwdT w = mlp_load_fwd_thin(wperm);
        float J = rollout_mlp<false, WTRAJ, false>(a, k, w, row0 + wave * CTK_MLP_TRAJ_PER_WAVE, [&](int h) { return myu[h]; });
        J += ((cin_s[tr] + cin_s[SAMP_TRAJ + tr]) + (cin_s[2 * SAMP_TRAJ + tr] + cin_s[3 * SAMP_TRAJ + tr])) * a.inv_Hp1;
        if (lane < 16 && row0 + tr < a.N) a.J[row0 + tr] = J;
    } else if constexpr (PRED == CTK_PRED_GRU) {
        // the four waves share the workgroup's 16 trajectories; wave 0 ends with J (lane = trajectory for lanes 0..15)
        const float* myu = ubuf + (lane & 15) * us;
        float J = rollout_gru<WTRAJ, false>(a, k, wperm, wperm + GRU_TABLE_FLOATS, gru_ex, row0, [&](int h) { return myu[h]; });
        if (wave == 0 && valid) {
            float cs = 0.0f;
#pragma unroll
            for (int cnk = 0; cnk < CHUNKS; ++cnk) cs += cin_s[cnk * TRAJ + lane];
            a.J[n] = J + cs * a.inv_Hp1;
        }
    }
}
