// ctk_cem_body.inc — the one-launch CEM step's statements, included once by ctk_cem_fused and once by ctk_cem_batch (ctk_cem_fused.hip).
// Expects in scope: ENV, WTRAJ, E = Env<ENV>, C, S, lds; samples (this step's draws or nullptr), a (RolloutArgs, a local copy: stream_id is
// written), k (Env<ENV>::K), cf (CemFusedK), mid (cf.mid of the KERNEL ARGUMENT: the one array the body indexes dynamically — through a
// local copy of the struct that index would put the whole copy into scratch), bx (this workgroup's index within ITS problem: rows bx * 64 .., record bx; workgroup 0 of a
// problem writes the problem's mu / sd).  cf.nblk is the workgroup count of the problem.  The body names no other coordinate, so workgroup
// x of a batch's problem runs the statements of workgroup x of a single handle's launch on the same operands.
    // Hs steps; H = Hs*C flat (step, input) columns of a plan = sample columns of a row (a.P): one sample per step and input
    const int N = a.N, Hs = a.H, H = Hs * C, ts = tile_stride(a.P), us = (H + 1) | 1, rs = 1 + 2 * H;
    const CemCarve cv = cem_carve(N, H, cf.nblk);
    float* tiles[2] = {lds + cv.tile0, lds + cv.tile1};
    float* ubuf = lds + cv.ubuf;
    float* cin_s = lds + cv.cin;
    float* mu_s = lds + cv.mu;
    float* sd_s = lds + cv.sd;
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds + cv.keys);
    float* recs = lds + cv.recs;
    double* part = reinterpret_cast<double*>(lds + cv.part);
    int* hist = reinterpret_cast<int*>(lds + cv.hist);
    int* sel = reinterpret_cast<int*>(lds + cv.misc);            // [0] prefix (as bits) [1] want
    int* nb_s = reinterpret_cast<int*>(lds + cv.misc) + 8;
    int* erow = reinterpret_cast<int*>(lds + cv.misc) + 16;       // [64] this workgroup's elite rows, ascending
    uint32_t* red = reinterpret_cast<uint32_t*>(lds + cv.misc) + 80;   // [2][CF_WAVES]
    auto red_min = [&](int row) { uint32_t v = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 0; w < CF_WAVES; ++w) v = min(v, red[row * CF_WAVES + w]);
        return v; };
    auto red_sum = [&](int row) { uint32_t v = 0u;
#pragma unroll
        for (int w = 0; w < CF_WAVES; ++w) v += red[row * CF_WAVES + w];
        return v; };
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = bx * CF_TRAJ;
    const int n = row0 + lane;
    const bool valid = n < N;                                     // wave 0: lane = row of the workgroup
    float up0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) up0[c] = a.u_prev_dev ? a.u_prev_dev[c] : a.u_prev[c];
    bool expired = false;

    for (int h = t; h < H; h += CF_BLOCK) { mu_s[h] = cf.mu[h]; sd_s[h] = cf.sd[h]; }
    a.stream_id = 0;
    cem_fetch_tile(tiles[0], samples, a, row0, t, CF_BLOCK);
    __syncthreads();

    for (int it = 0; it < cf.its; ++it) {
        const bool last_it = it + 1 == cf.its;
        const uint32_t tag = cf.tag0 + (uint32_t)it;
        float* tile = tiles[it & 1];
        CSTAMP(0);
        // ---- 1. rollout ---------------------------------------------------------------------------------------------
        auto prepare = [&](int ptraj, int hbeg, int hend) {
            const float* my = tile + ptraj * ts;
            auto input_at = [&](int h, int c) { return fminf(fmaxf(mu_s[h * C + c] + my[h * C + c] * sd_s[h * C + c], a.lo[c]), a.hi[c]); };   // :64-66
            float cin = 0.0f;
            float uprev[C];
#pragma unroll
            for (int c = 0; c < C; ++c) uprev[c] = (hbeg == 0 || hbeg >= Hs) ? up0[c] : input_at(hbeg - 1, c);
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
        const int S1 = min(Hs, 16), Ha = (S1 + CF_WAVES - 1) / CF_WAVES;
        const float cin_a = prepare(lane, min(S1, wave * Ha), min(S1, wave * Ha + Ha));
        if (wave == 0) cin_s[lane] = cin_a;
        __syncthreads();
        CSTAMP(1);
        const float* myu = ubuf + lane * us;
        float sx[S];
#pragma unroll
        for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
        float csum = 0.0f, amax = 0.0f;
        float* traj = nullptr;
        if constexpr (WTRAJ) {
            if (a.traj_out && last_it) traj = a.traj_out + (size_t)n * (Hs + 1) * S;
        }
        const bool single = E::fast_ok(k);
        if (wave == 0) {
            if (single) recur_env_range<ENV, WTRAJ, true, true>(k, traj, valid, myu, 0, S1, sx, csum, amax);
        } else {
            const int Hb = (Hs - S1 + CF_WAVES - 2) / (CF_WAVES - 1);
            cin_s[wave * CF_TRAJ + lane] = cin_a + prepare(lane, min(Hs, S1 + (wave - 1) * Hb), min(Hs, S1 + (wave - 1) * Hb + Hb));
        }
        __syncthreads();
        if (wave == 0) {
            float J = 0.0f;
            if (single) {
                recur_env_range<ENV, WTRAJ, true, true>(k, traj, valid, myu, S1, Hs, sx, csum, amax);
                if constexpr (WTRAJ) {
                    if (valid && traj) store_state<S>(traj + (size_t)Hs * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
            if (!single || __builtin_expect(__builtin_amdgcn_ballot_w64(E::out_of_range(amax)) != 0, 0)) {
#pragma unroll
                for (int i = 0; i < S; ++i) sx[i] = a.s0[i];
                csum = 0.0f;
                recur_env_range<ENV, WTRAJ, false, true>(k, traj, valid, myu, 0, Hs, sx, csum, amax);
                if constexpr (WTRAJ) {
                    if (valid && traj) store_state<S>(traj + (size_t)Hs * S, sx);
                }
                J = csum + E::terminal_cost(k, sx);
            }
            float cin = 0.0f;
#pragma unroll
            for (int w = 0; w < CF_WAVES; ++w) cin += cin_s[w * CF_TRAJ + lane];
            J += cin;
            J *= a.inv_Hp1;
            CSTAMP(2);
            if (valid) {
                ll_st(cf.llJ + n, f32_sortable(J), tag);          // ---- 2. hop 1: publish
                if (last_it) a.J[n] = J;
            }
        } else {
            const int tsub = t - 64, nsub = CF_BLOCK - 64;
            if (last_it && a.Q_out) {                             // the plans, coalesced (ctk_read / logging)
                const int total = max(0, min(CF_TRAJ, N - row0)) * H;
                float* dst = a.Q_out + (size_t)row0 * H;
                for (int i = tsub; i < total; i += nsub) {
                    const int r = H >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i;
                    dst[i] = ubuf[r * us + (i - r * H)];
                }
            }
            if (!last_it) {                                       // next iteration's samples: independent of mu / std
                RolloutArgs an = a;
                an.stream_id = (uint32_t)(it + 1);
                cem_fetch_tile(tiles[(it + 1) & 1], samples ? samples + (size_t)cf.per_it * (it + 1) : nullptr, an, row0, tsub, nsub);
            }
        }
        // all N costs into LDS (waves 1..3 start polling while wave 0 still runs the recurrence); their range on the way
        uint32_t kmin_t = 0xFFFFFFFFu, kmax_t = 0u;
        expired |= ll_gather(cf.llJ, N, tag, t, CF_BLOCK, cf.timeout_ticks, [&](int i, uint32_t v) {
            keys[i] = v; kmin_t = min(kmin_t, v); kmax_t = max(kmax_t, v);
        });
        CSTAMP(3);
        kmin_t = wave_min_u32(kmin_t);
        kmax_t = ~wave_min_u32(~kmax_t);
        if (lane == 0) { red[wave] = kmin_t; red[CF_WAVES + wave] = ~kmax_t; }
        __syncthreads();
        const uint32_t kbase = red_min(0);
        const uint32_t krange = ~red_min(1) - kbase;
        if (t == 0) { sel[0] = 0; sel[1] = cf.K; }

        // ---- 3. K-th smallest key: MSB-first radix select over d = key - kbase, 8 bits per pass.  Only the bits the range
        //      needs are walked, and the first digit buckets the costs LINEARLY over [min, max] (the raw top bits of a float are
        //      nearly constant over a population's costs: every key in one bin serialises the LDS atomics).  (Compacting the first
        //      pass's bucket and ranking its keys by brute force instead of the later passes was measured: slower, 4.0 vs 3.0 us.)
        const int nbits = 32 - __builtin_clz(krange | 1u);
        const int passes = (nbits + 7) >> 3;
        for (int pass = 0; pass < passes; ++pass) {
            const int hi = nbits - 8 * pass, lo = max(hi - 8, 0);   // this pass's digit = bits [lo, hi) of d: the first one is full
            const uint32_t dmask = (1u << (hi - lo)) - 1u;
            if (t < 256) hist[t] = 0;
            __syncthreads();
            const uint32_t prefix = (uint32_t)sel[0];
            const int want = sel[1];
            for (int j0 = t; j0 < N; j0 += CF_BLOCK * CF_CHUNK) { // unconditional LDS reads in flight (keys[] is padded), then the counting
                uint32_t dj[CF_CHUNK];
#pragma unroll
                for (int u = 0; u < CF_CHUNK; ++u) dj[u] = keys[j0 + u * CF_BLOCK] - kbase;
#pragma unroll
                for (int u = 0; u < CF_CHUNK; ++u) {
                    const bool act = (j0 + u * CF_BLOCK < N) & (pass == 0 || (dj[u] >> hi) == prefix);
                    if (act) atomicAdd(&hist[(dj[u] >> lo) & dmask], 1);
                }
            }
            __syncthreads();
            if (pass == 0) CSTAMP(9);
            if (wave == 0) {
                const int b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
                const int c = b0 + b1 + b2 + b3;
                // inclusive prefix over the 64 lanes: DPP row shifts inside each row of 16, then the three row totals
                int inc = c;
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, true);   // row_shr:1, zero fill
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, true);   // row_shr:2
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, true);   // row_shr:4
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xF, 0xF, true);   // row_shr:8
                const int r0 = __builtin_amdgcn_readlane(inc, 15), r1 = __builtin_amdgcn_readlane(inc, 31), r2 = __builtin_amdgcn_readlane(inc, 47);
                inc += lane >= 48 ? r0 + r1 + r2 : (lane >= 32 ? r0 + r1 : (lane >= 16 ? r0 : 0));
                const unsigned long long hit = __builtin_amdgcn_ballot_w64(inc >= want);
                const int first = hit ? __builtin_ctzll(hit) : 64;   // hit != 0: the histogram holds >= want keys
                if (lane == first) {
                    int below = inc - c, dgt = 4 * lane, bsel = b0;
                    if (below + b0 >= want) { dgt += 0; }
                    else if (below + b0 + b1 >= want) { below += b0; dgt += 1; bsel = b1; }
                    else if (below + b0 + b1 + b2 >= want) { below += b0 + b1; dgt += 2; bsel = b2; }
                    else { below += b0 + b1 + b2; dgt += 3; bsel = b3; }
                    sel[0] = (int)((prefix << (hi - lo)) | (uint32_t)dgt);
                    sel[1] = want - below;
                    sel[2] = bsel;                                // keys in the chosen bin (last pass: keys == the K-th smallest)
                }
            }
            __syncthreads();
            if (pass == 0) CSTAMP(10);
            if (pass == 1) CSTAMP(11);
        }
        CSTAMP(4);
        const uint32_t T32 = kbase + (uint32_t)sel[0];            // the K-th smallest key
        const int r_ties = sel[1];                                // of the keys == T32, the first r_ties in index order are elite
        // ties in front of this workgroup's rows — only when the cut falls INSIDE a group of equal keys (workgroup-uniform)
        const bool cut_in_tie = sel[2] != r_ties;
        __syncthreads();                                          // red[] (the range) and sel[] have been read by everyone
        if (cut_in_tie) {
            int tb = 0;
            for (int j = t; j < min(row0, N); j += CF_BLOCK) tb += keys[j] == T32;
            tb = (int)wave_sum((float)tb);                        // exact: < 2^24
            if (lane == 0) red[wave] = (uint32_t)tb;
        } else if (lane == 0) red[wave] = 0u;
        __syncthreads();
        const int ties_before = (int)red_sum(0);
        if (wave == 0) {
            const uint32_t ki = valid ? keys[n] : 0xFFFFFFFFu;
            const bool tie = valid && ki == T32;
            const unsigned long long tm = __builtin_amdgcn_ballot_w64(tie);
            const int my_tie_rank = ties_before + __builtin_popcountll(tm & ((1ull << lane) - 1ull));
            const bool elite = valid && (ki < T32 || (tie && my_tie_rank < r_ties));
            const unsigned long long em = __builtin_amdgcn_ballot_w64(elite);
            if (elite) erow[__builtin_popcountll(em & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0) nb_s[0] = __builtin_popcountll(em);
        }
        __syncthreads();

        CSTAMP(5);
        // ---- 4. local moments of the elite rows, hop 2 --------------------------------------------------------------
        const int nb = nb_s[0];
        unsigned long long* myrec = cf.llS + (size_t)bx * rs;
        if (t == 0) ll_st(myrec, (uint32_t)nb, tag);
        for (int h = t; h < H; h += CF_BLOCK) {
            const double mu0 = (double)mu_s[h];
            double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
            for (int e = 0; e < nb; ++e) { const double d = (double)ubuf[erow[e] * us + h] - mu0; s1 += d; s2 = fma(d, d, s2); }
            const double mb = nb > 0 ? s1 / (double)nb : 0.0;
            const double m2 = fma(-mb, s1, s2);                   // sum (d - m_b)^2 = s2 - s1^2 / n_b
            ll_st(myrec + 1 + h, __builtin_bit_cast(uint32_t, (float)mb), tag);
            ll_st(myrec + 1 + H + h, __builtin_bit_cast(uint32_t, (float)(m2 > 0.0 ? m2 : 0.0)), tag);
        }
        CSTAMP(6);
        expired |= ll_gather(cf.llS, cf.nblk * rs, tag, t, CF_BLOCK, cf.timeout_ticks,
                             [&](int i, uint32_t v) { reinterpret_cast<uint32_t*>(recs)[i] = v; });
        __syncthreads();

        CSTAMP(7);
        // ---- 5. refit (:77-78; population std): A = sum n_b m_b, B = sum (M2_b + n_b m_b^2) in double, in a fixed order (segments of the
        //      workgroup range, then the segments): every workgroup arrives at the same bits.  One pass, one barrier.
        //      (One thread per column walking all workgroups: 4.4 us at cfg3.)
        {
            constexpr int SEGMAX = 16;
            const double invK = 1.0 / (double)cf.K;               // == 1 / sum_b n_b: the elite set has exactly K rows
            const int* nrec = reinterpret_cast<const int*>(recs);
            auto add_rec = [&](int bq, int h, double& A, double& B) {
                const double nbq = (double)nrec[bq * rs], mb = (double)recs[bq * rs + 1 + h];
                A = fma(nbq, mb, A);
                B += (double)recs[bq * rs + 1 + H + h] + nbq * mb * mb;
            };
            auto finish = [&](int h, double A, double B) {
                const double mshift = A * invK;
                const double var = fma(-mshift, mshift, B * invK);
                mu_s[h] = (float)((double)mu_s[h] + mshift);
                sd_s[h] = (float)sqrt(var > 0.0 ? var : 0.0);     // tf.math.reduce_std: ddof = 0
            };
            const bool multi = H <= CF_BLOCK && cf.nblk > 8;      // few workgroups: the plain walk is shorter than the barrier
            const int SEG = multi ? min(SEGMAX, CF_BLOCK / H) : 1, per = (cf.nblk + SEG - 1) / SEG;
            if (multi) {
                const int hcol = t % H, sg = t / H;
                if (sg < SEG) {
                    double A = 0.0, B = 0.0;
                    const int bb = sg * per, be = min(cf.nblk, bb + per);
                    for (int bq = bb; bq < be; ++bq) add_rec(bq, hcol, A, B);
                    part[(sg * H + hcol) * 2] = A; part[(sg * H + hcol) * 2 + 1] = B;
                }
                __syncthreads();
                if (t < H) {
                    double A = 0.0, B = 0.0;
                    for (int q = 0; q < SEG; ++q) { A += part[(q * H + t) * 2]; B += part[(q * H + t) * 2 + 1]; }
                    finish(t, A, B);
                }
            } else {
                for (int h = t; h < H; h += CF_BLOCK) {
                    double A = 0.0, B = 0.0;
                    for (int bq = 0; bq < cf.nblk; ++bq) add_rec(bq, h, A, B);
                    finish(h, A, B);
                }
            }
        }
        __syncthreads();
        CSTAMP(8);

        if (last_it) {
            // u = elite[0,0,:] (:101): first input of the cheapest row under (J, index), published by its owner
            const uint32_t gk = kbase;                            // the cheapest cost's key (this iteration's range, above)
            int best = 0x7FFFFFFF;
            for (int j = t; j < N; j += CF_BLOCK)
                if (keys[j] == gk) { best = j; break; }           // j ascending per thread: its smallest match
            best = (int)wave_min_u32((uint32_t)best);
            __syncthreads();                                      // red[] is read above by everyone
            if (lane == 0) red[wave] = (uint32_t)best;
            __syncthreads();
            const int gbest = (int)red_min(0);
            if (t == 0 && gbest >= row0 && gbest < row0 + CF_TRAJ) {
                cf.idx_out[0] = gbest;
                if (expired) host_word_store(cf.u_host, 2, 2u);    // (drained: the flag below must not overtake it)
                if constexpr (C == 1) publish_u_launched(cf.u_dev, cf.u_host, ubuf[(gbest - row0) * us], cf.seq);
                else publish_u_vec_launched(cf.u_dev, cf.u_host, ubuf + (gbest - row0) * us, C, cf.seq);
            }
            // :99-102 clip the std, shift both by one step, refill the tail — the handle's distribution for the next MPC step
            if (bx == 0) {
                for (int h = t; h < H; h += CF_BLOCK) {
                    cf.mu[h] = (h + C < H) ? mu_s[h + C] : mid[h - (H - C)];      // shift by one STEP = C columns
                    cf.sd[h] = (h + C < H) ? fminf(fmaxf(sd_s[h + C], cf.std_min), cf.std_max) : cf.init_std;
                }
            }
        }
    }
    // a wait that ran out in a workgroup that does not own the best row still has to reach the host
    if (expired && t == 0) __hip_atomic_store(reinterpret_cast<uint32_t*>(cf.u_host) + 2, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
