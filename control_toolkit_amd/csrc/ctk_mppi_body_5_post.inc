// ctk_mppi_body_5_post.inc — part 5 of 5 of the body of ctk_mppi_rollout<ENV, PRED, LOG, P2P> (ctk_mppi.hip: the kernel's header comment and DESIGN.md 2.1 describe
// it), kept as TEXT so that the resident form (ctk_mppi_resident) compiles the SAME statements around other per-step inputs and in another
// order in time.  The launched kernel includes the five parts back to back (its ISA is what it was before the split).
//   1 decl    step-invariant definitions: the LDS carve, indices           4 phase_a  inputs of the first S1 steps (all four waves)
//   2 pro1    per-step tables + the sample tile into LDS                   5 post     recurrence (+ phase B), epilogue, record hand-off, merge tail
//   3 defs    S1, corr_keep, the prologue2 lambda
// Expects in scope: ENV, PRED, LOG, P2P; samples, u_nom, interp, wperm, parts, N_, H_, P_, pmagic_, a_in, k, m, fz; `extern __shared__ float lds[]`.

    // ---- the recurrence --------------------------------------------------------------------------
    float J = 0.0f;
    if constexpr (PRED == CTK_PRED_ODE) {
        // wave 0 only: one trajectory per lane, state in registers, through the environment's cost_step
        const float* myF = ubuf + lane * us;
        float sx[S];
#pragma unroll
        for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
        float csum = 0.0f, amax = 0.0f;
        float* traj = nullptr;
        if constexpr (LOG) {
            if (a.traj_out) traj = a.traj_out + (size_t)n * (H + 1) * S;
        }
        const bool single = E::fast_ok(k);
        if (wave == 0) {                           // steps [0, S1) while the others prepare [S1, H)
            if (single) recur_env_range<ENV, LOG, true, false, PIPE>(k, traj, valid, myF, 0, S1, sx, csum, amax);
        } else {
            const int Hb = (H - S1 + MPPI_WAVES - 2) / (MPPI_WAVES - 1);        // phase B: wave w takes its third of [S1, H)
            prologue2(lane, min(H, S1 + (wave - 1) * Hb), min(H, S1 + (wave - 1) * Hb + Hb), wave, corr_keep);
        }
        __syncthreads();                           // waves 1..3 have been waiting here since ~step 4 of wave 0
        if (wave == 0) {
            if (single) {
                recur_env_range<ENV, LOG, true, false, PIPE>(k, traj, valid, myF, S1, H, sx, csum, amax);
                if constexpr (LOG) {
                    if (valid && traj) store_state<S>(traj + (size_t)H * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
#ifndef CTK_DIAG_NO_COLD
            // Euler sub-steps (intermediate_steps > 1), or an angle beyond the fast sincos range somewhere in the
            // wave (~never): the whole horizon with the checked sincos, all inputs being ready by now
            if (!single || __builtin_expect(__builtin_amdgcn_ballot_w64(E::out_of_range(amax)) != 0, 0)) {
#pragma unroll
                for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
                csum = 0.0f;
                recur_env_range<ENV, LOG, false>(k, traj, valid, myF, 0, H, sx, csum, amax);
                if constexpr (LOG) {
                    if (valid && traj) store_state<S>(traj + (size_t)H * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
#endif
            J *= a.inv_Hp1;
        }
    } else if constexpr (PRED == CTK_PRED_MLP) {
        // all four waves: 16 trajectories each on the fp32 matrix cores (ctk_mlp.h)
        const int tr = wave * CTK_MLP_TRAJ_PER_WAVE + (lane & 15);
        const float* myu = ubuf + tr * us;
        const MlpFwdT w = mlp_load_fwd_thin(wperm);
        const float Jw = rollout_mlp<false, LOG, false>(a, k, w, row0 + wave * CTK_MLP_TRAJ_PER_WAVE, [&](int h) { return myu[h]; });
        if (lane < 16) e_s[tr] = Jw;          // hand the 64 costs to wave 0 (e_s doubles as J scratch)
        __syncthreads();
        if (wave == 0) J = e_s[lane];
        __syncthreads();
    } else if constexpr (PRED == CTK_PRED_MLP_PAIR) {
        // waves (2p, 2p+1) share tile p of the workgroup's two (ctk_mlp.h: mlp_step_pair)
        const int pair = wave >> 1, half = wave & 1;
        const int tr = pair * CTK_MLP_TRAJ_PER_WAVE + (lane & 15);
        const float* myu = ubuf + tr * us;
        const MlpFwdHalf w = mlp_half_of(mlp_load_fwd_thin(wperm), half);
        float* ex = gru_ex + pair * MLP_PAIR_EX;           // the exchange slots follow the rollout carve
        float amax;
        float Jw = rollout_mlp_pair_impl<false, LOG, false, false>(a, k, w, row0 + pair * CTK_MLP_TRAJ_PER_WAVE, half, ex, [&](int h) { return myu[h]; }, &amax);
        // an angle beyond the unchecked cos's range anywhere in the WORKGROUP (never in practice): all waves redo, checked
        if (__builtin_expect(__syncthreads_or(!(amax <= CTK_SINCOS_FAST_LIMIT)), 0))
            Jw = rollout_mlp_pair_impl<false, LOG, false, true>(a, k, w, row0 + pair * CTK_MLP_TRAJ_PER_WAVE, half, ex, [&](int h) { return myu[h]; }, &amax);
        if (half == 0 && lane < 16) e_s[tr] = Jw;
        __syncthreads();
        if (wave == 0) J = e_s[lane & (TRAJ - 1)];
        __syncthreads();
    } else {
        // the four waves share the workgroup's 16 trajectories (ctk_gru.h); wave 0 ends with J of trajectory
        // lane & 15 in every lane, i.e. lane = trajectory for lanes 0..15
        const float* myu = ubuf + (lane & 15) * us;
        J = rollout_gru<LOG, false>(a, k, wperm, wperm + GRU_TABLE_FLOATS, gru_ex, row0, [&](int h) { return myu[h]; });
    }
    if (wave == 0) {
        // EARLY_U, off the chain between J and the publish: what the early form reads that does not depend on J.  Entry 0 of the tables
        // (c0 = i0(0), w0, w1, un) is read here, beside the correction partials below (one wait for both); the 16 tile values of the column
        // partial of lanes 0..7 follow, behind J and ahead of wave_min, and arrive under the soft-min partial.  (The grid size and the
        // limits stay where they are used: scalar loads share the LDS counter, and fetched here they put a full wait for the table
        // reads in front of the correction partials in EVERY block.)
        [[maybe_unused]] int eu_c0 = 0;
        [[maybe_unused]] float eu_w0 = 0.0f, eu_w1 = 0.0f, eu_un = 0.0f;
        [[maybe_unused]] float eu_tile[RPW];
        [[maybe_unused]] bool eu_on = false;
        if constexpr (TRAJ == MPPI_TRAJ) {
            const float cr0 = corr_s[lane], cr1 = corr_s[TRAJ + lane], cr2 = corr_s[2 * TRAJ + lane], cr3 = corr_s[3 * TRAJ + lane];
            if constexpr (EARLY_U) {
                eu_on = fz.mode == 1 && use_ll;
                if (eu_on) { eu_c0 = i0_s[0]; eu_w0 = w0_s[0]; eu_w1 = w1_s[0]; eu_un = un_s[0]; }   // (behind the partials' reads: one wait)
            }
            J += (cr0 + cr1) + (cr2 + cr3);
        } else {
            float cs = 0.0f;
#pragma unroll
            for (int cnk = 0; cnk < CHUNKS; ++cnk) cs += corr_s[cnk * TRAJ + (lane & (TRAJ - 1))];
            J += cs;
        }
        if constexpr (EARLY_U) {
            asm volatile("" : "+v"(J));       // J is formed HERE, ahead of the tile reads' issue (they are waited for behind the soft-min)
            if (eu_on && lane < 8) mppi_col_tile_regs<RPW>(eu_tile, tile, ts, lane & 3, eu_c0 + (lane >> 2));   // (column P: the tile's zero pad)
        }
        STAMP(3);
        if (valid) a.J[n] = J;
        // block-local soft-min partial (optimizer_mppi.py:163-168 restricted to this block)
        const float rho = wave_min(valid ? J : INFINITY);
        const float e = valid ? expf(m.neg_inv_lbd * (J - rho)) : 0.0f;
        const float asum = wave_sum(e);
        if (lane < TRAJ) e_s[lane] = e;
        if (lane == 0) {
            if (use_ll) {
                unsigned long long* rl = fz.ll + (size_t)blockIdx.x * (2 + P);
                ll_store(rl, rho, fz.up.seq); ll_store(rl + 1, asum, fz.up.seq);
            } else {
                float* rec = parts + (size_t)blockIdx.x * (2 + P);
                st_rec(rec, rho); st_rec(rec + 1, asum);
            }
        }
        // ---- u ahead of the plan update (EARLY_U, ctk_mppi_body_1_decl.inc): the caller waits for u = u_nom_new[0] alone, and entry 0
        //      of the update reads, of every block's record, only rho_b, a_b and the columns c0 = i0(0) and c0 + 1.  Wave 0 of every block
        //      forms those two column sums here, ahead of the workgroup's barrier and full pass, and publishes them in their slots of the
        //      block's record (the full pass stores the same values under the same sequence number again); wave 0 of block 0 then polls
        //      the four words of every block, merges them in registers and publishes {u, seq}.  Everything below — the barrier, the full
        //      column sums, the full poll, the merge, the update of all H entries — is as in the late order, minus the publish.
        if constexpr (EARLY_U) {
            if (eu_on) {
                const int c0 = eu_c0;
                float cs = 0.0f;
                if (lane < 8) cs = mppi_col_partial_regs<RPW>(e_s, eu_tile, lane & 3);   // mppi_col_partial's sum, its operands fetched above
                cs += dpp_mov<DPP_QUAD_XOR1>(cs);                     // lanes 4c .. 4c+3: (s0 + s1) + (s2 + s3), the full pass's order
                cs += dpp_mov<DPP_QUAD_XOR2>(cs);
                if ((lane == 0 || lane == 4) && c0 + (lane >> 2) < P)
                    ll_store(fz.ll + (size_t)blockIdx.x * (2 + P) + 2 + c0 + (lane >> 2), cs, fz.up.seq);
                if (blockIdx.x == 0) {
                    bool late = false;                // the bounded poll ran out: error word 2, as in the tail
                    const float o = mppi_early_u<CTK_MPPI_FUSE_MAX_BLOCKS_LL / 64>(fz.ll, (int)gridDim.x, P, c0, eu_w0, eu_w1, eu_un, m.neg_inv_lbd,
                                                                                  fz.up.lo, fz.up.hi, fz.up.seq, &late
#ifdef CTK_STAMPS
                                                                                  , a.stamps
#endif
                                                                                  );
                    STAMP(11);                        // u formed (stamp 7 below: published)
                    if (lane == 0) {
                        // ctk_api.hip:finish_step turns a non-zero error word (the dword behind {u, seq}) into CTK_ERR_STATE
                        if (late && fz.up.u_host) host_word_store(fz.up.u_host, 2, 2u);   // (drained here only: the flag must not overtake it)
                        publish_u_launched(fz.up.u_dev, fz.up.u_host, o, fz.up.seq);   // optimizer_mppi.py:191 u = u_nom[0,0,:]  (EARLY_U: a launched form)
                    }
                    STAMP(7);
                }
            }
        }
    }
    __syncthreads();
    STAMP(4);

    // ---- epilogue (256 threads): b_b[p] = sum_r e_r * tile[r][p]; wave w sums rows RPW*w..RPW*w+RPW-1 ----
    for (int p = lane; p < P; p += 64) col_s[wave * P + p] = mppi_col_partial<RPW>(e_s, tile, ts, wave, p);
    __syncthreads();
    float* rec = parts + (size_t)blockIdx.x * (2 + P);
    for (int p = t; p < P; p += MPPI_BLOCK) {
        const float v = (col_s[p] + col_s[P + p]) + (col_s[2 * P + p] + col_s[3 * P + p]);
        if (use_ll) ll_store(fz.ll + (size_t)blockIdx.x * (2 + P) + 2 + p, v, fz.up.seq);
        else st_rec(rec + 2 + p, v);
    }
    STAMP(5);

    // ---- fused tail, low-latency form: block 0 polls every record word until it carries this launch's sequence
    //      number (the words ARE the data), staging them in LDS, then merges.  One memory round trip after the
    //      slowest block's stores instead of three (drain stores / ticket / fetch).  The other blocks are done.
    //      Every block of the grid finishes unconditionally, so the wait terminates; it is bounded anyway.
    if (use_ll) {
        if (blockIdx.x == 0) {
            __syncthreads();                      // col_s / tile are dead: the merge scratch may overwrite them
            const int nb = (int)gridDim.x, tot = nb * (2 + P);
            float* st = merge_stage_ptr(lds, nb, P);
            bool expired = false;                 // a bounded poll ran out: surfaced to the host through the error word
            // LLW words in flight per thread: the first pass over a thread's words is one pipelined batch of loads, not LLW round trips
            // (ctk_mppi_merge.h: ll_poll_stage; every later pass re-reads what has not arrived, then sleeps once).
            // A SECOND batch starts only when the first has arrived, i.e. after the slowest workgroup's record — a whole extra round trip
            // (~2 us) behind the launch's critical path: up to 16 words per thread go out as ONE batch (a configs[4] shard: 13 per thread).
            // Only the WIDE_TAIL form carries the 16-deep batch: the launcher takes it exactly when the records exceed one 8-deep batch.
            auto poll = [&](auto llw_tag) {
                constexpr int LLW = decltype(llw_tag)::value;
                for (int i0 = t; i0 < tot; i0 += MPPI_BLOCK * LLW) expired |= ll_poll_stage_call<LLW, MPPI_BLOCK>(fz.ll, st, i0, tot, fz.up.seq);
            };
            if constexpr (WIDE_TAIL) {
                if (tot > MPPI_BLOCK * 8 && tot <= MPPI_BLOCK * 16) poll(std::integral_constant<int, 16>{});
                else poll(std::integral_constant<int, 8>{});
            } else {
                poll(std::integral_constant<int, 8>{});
            }
            // ctk_api.hip:finish_step turns a non-zero error word (the dword behind {u, seq}) into CTK_ERR_STATE
            if (expired && fz.up.u_host) host_word_store(fz.up.u_host, 2, 2u);   // (drained ahead of the barrier: the merge's publish cannot overtake it)
            __syncthreads();
            const size_t scratch_floats = 8 + P + 1 + min(nb, MERGE_CHUNK) + (size_t)tot + MERGE_BLOCK;   // (+ the column slices of many narrow records)
            if (scratch_floats <= (size_t)(w0_s - lds)) { fz.up.w0_l = w0_s; fz.up.w1_l = w1_s; fz.up.un_l = un_s; fz.up.i0_l = i0_s; }
            if (fz.mode == 1) mppi_merge_block<true, 0, C, WIDE_TAIL, !EARLY_U, PUB_REL>(lds, nullptr, nb, P, m.neg_inv_lbd, nullptr, fz.up, 2);   // (EARLY_U: u is out already)
            else mppi_merge_block<false, 0, C, WIDE_TAIL>(lds, nullptr, nb, P, m.neg_inv_lbd, fz.out_rec, fz.up, 2);
            if constexpr (P2P) {
                // sharded step over peer-to-peer stores, all in this launch: the shard's record (just written to
                // fz.out_rec = this rank's slot of its own exchange buffer by this block) goes to every peer, their
                // records arrive, merge, update (ctk_mppi_p2p_exchange's body)
                __shared__ int bad;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the record's stores have landed
                __syncthreads();
                P2PArgs x = *fz.p2p;
                x.seq = fz.p2p_seq;
                const size_t scratch_w = 8 + P + 1 + min(x.world, MERGE_CHUNK) + (size_t)x.world * (2 + P);
                if (scratch_w > (size_t)(w0_s - lds)) { fz.up.w0_l = nullptr; fz.up.w1_l = nullptr; fz.up.un_l = nullptr; fz.up.i0_l = nullptr; }
                p2p_exchange_and_update(lds, &bad, x, P, m.neg_inv_lbd, fz.up, 1);
            }
        }
        STAMP(6);
        kernarg_prefetch_sink(ka_sink, parts);
        return;
    }

    // ---- fused tail: hand-off of the block records inside the launch (cdna_hip_programming.md G16,
    //      sc1 form: every record store above is a write-through agent-scope store, every storing wave
    //      drains its stores, the workgroup meets, ONE lane takes a ticket; the block that drew the last
    //      ticket reads every record with sc1 loads).  Placement-independent.
    if (fz.mode != 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* last_s = reinterpret_cast<int*>(lds);
        if (t == 0) {
            const unsigned ticket = __hip_atomic_fetch_add(fz.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *last_s = (ticket == gridDim.x - 1) ? 1 : 0;
        }
        __syncthreads();
        const bool last = *last_s != 0;
        __syncthreads();
        if (last) {
            // the merge scratch grows from lds[0]; the per-step tables at the end of the carve stay intact
            // whenever the scratch ends below them
            const size_t scratch_floats = 8 + P + 1 + min((int)gridDim.x, MERGE_CHUNK) + (fz.stage_ok ? (size_t)gridDim.x * (2 + P) + MERGE_BLOCK : 0);
            if (scratch_floats <= (size_t)(w0_s - lds)) { fz.up.w0_l = w0_s; fz.up.w1_l = w1_s; fz.up.un_l = un_s; fz.up.i0_l = i0_s; }
            if (fz.mode == 1) mppi_merge_block<true, 1, C, WIDE_TAIL, true, PUB_REL>(lds, parts, (int)gridDim.x, P, m.neg_inv_lbd, nullptr, fz.up, fz.stage_ok != 0 ? 1 : 0);
            else mppi_merge_block<false, 1, C, WIDE_TAIL>(lds, parts, (int)gridDim.x, P, m.neg_inv_lbd, fz.out_rec, fz.up, fz.stage_ok != 0 ? 1 : 0);
            if (t == 0) __hip_atomic_store(fz.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    STAMP(6);
    kernarg_prefetch_sink(ka_sink, parts);
