// ctk_g_rollout_body.inc — the statements of the one-wave template rollout kernel ctk_g_rollout<ENV, MODE, LOG> (ctk_generic.hip), included by
// that kernel and by the batch families' rollout of caller-supplied plans (ctk_batch_rollout.hip: ctk_g_batch_rollout), the way ctk_mppi_body.inc
// and ctk_g_rpgd_body.inc serve their kernels.  An include file and not a device function: with the body behind a function call the
// compiler lays ctk_g_rollout out differently, and that kernel keeps its instruction text.
// Expects in scope: ENV, MODE, LOG; a (RolloutArgs), k (Env<ENV>::K), m (MppiK), cols_per_point, samples, base, scale, rng_kind, parts.
// rollout + cost.  a.P = number of sample columns per row (P*C for MPPI, H*C for the affine modes), a.p_magic its magic.
// LDS (floats): tile[64][ts] | e[64] | base[HC] | scale[HC] | w0[H] w1[H] i0[H]
    using E = Env<ENV>;
    constexpr int S = E::S, C = E::C;
    extern __shared__ float lds[];
    const int H = a.H, HC = H * C, cols = a.P, ts = tile_stride(cols);
    float* tile = lds;
    float* e_s = tile + G_TRAJ * ts;
    float* base_s = e_s + G_TRAJ;             // MPPI: shifted nominal plan; affine: base
    float* scale_s = base_s + HC;             // affine only
    float* w0_s = scale_s + HC;               // MPPI only: interpolation table
    float* w1_s = w0_s + H;
    int* i0_s = reinterpret_cast<int*>(w1_s + H);
    const int lane = threadIdx.x;
    const int row0 = blockIdx.x * G_TRAJ;
    const int n = row0 + lane;
    const bool valid = n < a.N;
    (void)cols_per_point;

    load_tile_early<G_TRAJ, G_TRAJ>(tile, samples, a, row0, MODE == CTK_G_MODE_MPPI ? m.stdev : 1.0f, rng_kind, [&] {
        if constexpr (MODE == CTK_G_MODE_MPPI) {
            for (int h = lane; h < H; h += G_TRAJ) {
                const InterpEntry e = a.interp[h];
                i0_s[h] = e.i0; w0_s[h] = e.w0; w1_s[h] = e.w1;
            }
            for (int hc = lane; hc < HC; hc += G_TRAJ) {
                const int h = hc / C, c = hc - h * C;
                base_s[hc] = base[min(h + 1, H - 1) * C + c];                         // optimizer_mppi.py:184 (shift, repeat last)
            }
        } else {
            for (int hc = lane; hc < HC; hc += G_TRAJ) { base_s[hc] = base[hc]; scale_s[hc] = scale[hc]; }
        }
    });
    __syncthreads();

    const float* my = tile + lane * ts;
    float s[S], up[C];
#pragma unroll
    for (int i = 0; i < S; ++i) s[i] = a.s0[i];
#pragma unroll
    for (int c = 0; c < C; ++c) up[c] = a.u_prev_dev ? a.u_prev_dev[c] : a.u_prev[c];
    float csum = 0.0f, corr = 0.0f;
    const int Pm1 = cols / C - 1;             // MPPI: last inducing point
    for (int h = 0; h < H; ++h) {
        float u[C];
        if constexpr (MODE == CTK_G_MODE_MPPI) {
            const int i0 = i0_s[h], i1 = min(i0 + 1, Pm1);
            const float w0 = w0_s[h], w1 = w1_s[h];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float du = my[i0 * C + c] * w0 + my[i1 * C + c] * w1;          // Interpolator.py:97-106, per input channel
                u[c] = fminf(fmaxf(base_s[h * C + c] + du, a.lo[c]), a.hi[c]);        // optimizer_mppi.py:186-187
                corr += m.cc * (m.k_dd * (du * du) + m.R * u[c] * du + m.k_uu * (u[c] * u[c]));   // :154-155, summed over h and c
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                u[c] = fminf(fmaxf(base_s[h * C + c] + my[h * C + c] * scale_s[h * C + c], a.lo[c]), a.hi[c]);
        }
        if constexpr (LOG || MODE == CTK_G_MODE_AFFINE) {
            if (valid && a.Q_out) {
#pragma unroll
                for (int c = 0; c < C; ++c) a.Q_out[(size_t)n * HC + h * C + c] = u[c];
            }
        }
        csum += E::stage_cost(k, s, u, up);
        if constexpr (LOG) {
            if (valid && a.traj_out) {
#pragma unroll
                for (int i = 0; i < S; ++i) a.traj_out[((size_t)n * (H + 1) + h) * S + i] = s[i];
            }
        }
        E::step(k, s, u);
#pragma unroll
        for (int c = 0; c < C; ++c) up[c] = u[c];
    }
    if constexpr (LOG) {
        if (valid && a.traj_out) {
#pragma unroll
            for (int i = 0; i < S; ++i) a.traj_out[((size_t)n * (H + 1) + H) * S + i] = s[i];
        }
    }
    // mean over [H stage costs | terminal] (Cost_Functions/__init__.py:90-93); the MPPI correction is added unscaled
    const float J = (csum + E::terminal_cost(k, s)) * a.inv_Hp1 + corr;
    if (valid) a.J[n] = J;

    if constexpr (MODE == CTK_G_MODE_MPPI) {
        // block-local soft-min record (optimizer_mppi.py:163-168 restricted to this block; merged by ctk_mppi_merge)
        const float rho = wave_min(valid ? J : INFINITY);
        const float e = valid ? expf(m.neg_inv_lbd * (J - rho)) : 0.0f;
        const float asum = wave_sum(e);
        e_s[lane] = e;
        __syncthreads();
        float* rec = parts + (size_t)blockIdx.x * (2 + cols);
        if (lane == 0) { rec[0] = rho; rec[1] = asum; }
        for (int p = lane; p < cols; p += G_TRAJ) {
            float acc = 0.0f;
#pragma unroll 8
            for (int r = 0; r < G_TRAJ; ++r) acc += e_s[r] * tile[r * ts + p];
            rec[2 + p] = acc;
        }
    }
