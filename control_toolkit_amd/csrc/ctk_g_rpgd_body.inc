// ctk_g_rpgd_body.inc — the body of the template RPGD descent (ctk_generic.hip): all Adam iterations of one MPC step and get_action's cost
// pass for the 64 plans of workgroup blockIdx.x.  Included by ctk_g_rpgd_descent<ENV> (whose arguments these names are) and by the batch
// form ctk_g_rpgd_batch<ENV> (whose prologue rebuilds them from a step record), so both compile the same text.
// Expects ENV, a, k, ad, Q, m, v, bc_table, bc_len, t0, iters, scratch, tape_in_lds in scope, and lim: the RolloutArgs whose limits lo / hi are
// indexed with a run-time channel (the kernel argument itself: a per-problem copy indexed like that would have to live in private memory).
// Leaves g_s, t, HC (and the rest) behind it.
    using E = Env<ENV>;
    constexpr int S = E::S, C = E::C;
    extern __shared__ float lds[];
    const int H = a.H, HC = H * C;
    float* q_s = lds;                        // [HC][65]
    float* g_s = q_s + HC * GR_LD;           // [HC][65]
    float* sc_s = g_s + HC * GR_LD;          // [64]
    float* tape_l = sc_s + G_TRAJ;           // [H][NT][64]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * G_TRAJ;
    const int rows = min(G_TRAJ, a.N - row0);
    const int total = rows * HC;
    const size_t gbase = (size_t)row0 * HC;
    constexpr int NT = E::NT;                // taped values per step (Env::fwd_tape / bwd_tape: the sweep recomputes nothing)
    float* tape = tape_in_lds ? tape_l : scratch + (size_t)blockIdx.x * H * NT * 64;

    for (int i = t; i < G_TRAJ * HC; i += GR_BLOCK) {      // a.p_magic = ceil(2^32 / HC)
        const int r = HC >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i, hc = i - r * HC;
        q_s[hc * GR_LD + r] = i < total ? Q[gbase + i] : 0.0f;
    }
    __syncthreads();

    float up0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) up0[c] = a.u_prev_dev ? a.u_prev_dev[c] : a.u_prev[c];
    const float inv = a.inv_Hp1;

    // forward pass of a gradient iteration: no cost, NT taped values per step; the final state in sF
    auto forward_tape = [&](float (&sF)[S]) {
        float s[S];
#pragma unroll
        for (int i = 0; i < S; ++i) s[i] = a.s0[i];
        float un[C];
#pragma unroll
        for (int c = 0; c < C; ++c) un[c] = q_s[c * GR_LD + lane];
        for (int h = 0; h < H; ++h) {
            float u[C], tp[NT];
#pragma unroll
            for (int c = 0; c < C; ++c) u[c] = un[c];
            if (h + 1 < H) {
#pragma unroll
                for (int c = 0; c < C; ++c) un[c] = q_s[((h + 1) * C + c) * GR_LD + lane];
            }
            E::fwd_tape(k, s, u, tp);
#pragma unroll
            for (int i = 0; i < NT; ++i) tape[((size_t)h * NT + i) * 64 + lane] = tp[i];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) sF[i] = s[i];
    };
    // get_action's cost pass (:342): the recurrence of the sampling kernels (Env::cost_step, checked fallback) + the input-only terms
    auto final_cost = [&]() {
        float u[C], up[C], cin = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) up[c] = up0[c];
        for (int h = 0; h < H; ++h) {
#pragma unroll
            for (int c = 0; c < C; ++c) u[c] = q_s[(h * C + c) * GR_LD + lane];
            cin += E::input_cost(k, u, up);
#pragma unroll
            for (int c = 0; c < C; ++c) up[c] = u[c];
        }
        auto run = [&](auto fast) {
            constexpr bool FAST = decltype(fast)::value;
            float s[S], csum = 0.0f, amax = 0.0f;
#pragma unroll
            for (int i = 0; i < S; ++i) s[i] = a.s0[i];
            float un[C];
#pragma unroll
            for (int c = 0; c < C; ++c) un[c] = q_s[c * GR_LD + lane];
            for (int h = 0; h < H; ++h) {
                float f[C];
#pragma unroll
                for (int c = 0; c < C; ++c) f[c] = E::prep_input(k, un[c], c);
                if (h + 1 < H) {
#pragma unroll
                    for (int c = 0; c < C; ++c) un[c] = q_s[((h + 1) * C + c) * GR_LD + lane];
                }
                E::template cost_step<FAST>(k, s, f, csum, amax);
            }
            const float J = csum + E::terminal_cost(k, s);
            return __builtin_amdgcn_ballot_w64(FAST && E::out_of_range(amax)) != 0 ? __builtin_nanf("") : J;
        };
        float J = E::fast_ok(k) ? run(std::true_type{}) : __builtin_nanf("");
        if (__builtin_amdgcn_ballot_w64(J != J) != 0) J = run(std::false_type{});   // wave-uniform: Euler sub-steps or an angle out of range
        return (J + cin) * inv;
    };

    for (int it = 0; it < iters; ++it) {
        if (wave == 0) {
            float sH[S], lam[S];
            forward_tape(sH);
            E::terminal_grad(k, sH, lam);
#pragma unroll
            for (int i = 0; i < S; ++i) lam[i] *= inv;
            float nrm2 = 0.0f;
            float gp_next[C];                 // d stage_{h+1} / d u_h (through u_prev of the next step)
#pragma unroll
            for (int c = 0; c < C; ++c) gp_next[c] = 0.0f;
            for (int h = H - 1; h >= 0; --h) {
                float tp[NT], u[C], upv[C];
#pragma unroll
                for (int i = 0; i < NT; ++i) tp[i] = tape[((size_t)h * NT + i) * 64 + lane];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    u[c] = q_s[(h * C + c) * GR_LD + lane];
                    upv[c] = h > 0 ? q_s[((h - 1) * C + c) * GR_LD + lane] : up0[c];
                }
                float du[C], gu[C], gp[C];
                E::bwd_tape(k, tp, u, lam, du, inv);
                E::input_grad(k, u, upv, gu, gp);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float g = (gu[c] + gp_next[c]) * inv + du[c];
                    g_s[(h * C + c) * GR_LD + lane] = g;
                    nrm2 += g * g;
                    gp_next[c] = gp[c];
                }
            }
            sc_s[lane] = ad.clip / fmaxf(sqrtf(nrm2), ad.clip);       // clip_by_norm over [H,C] (:315,:334)
        }
        __syncthreads();
        const int ti = t0 + it + 1;
        const float bc1 = ti <= bc_len ? bc_table[2 * (ti - 1)] : 1.0f;
        const float bc2 = ti <= bc_len ? bc_table[2 * (ti - 1) + 1] : 1.0f;
        for (int i = t; i < total; i += GR_BLOCK) {
            const int r = HC >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i, hc = i - r * HC, c = hc % C;
            float mm = 0.0f, vv = 0.0f;
            if (ad.rule != 2) { mm = m[gbase + i]; vv = v[gbase + i]; }
            const float g = g_s[hc * GR_LD + r] * sc_s[r];
            q_s[hc * GR_LD + r] = adam_update(ad, q_s[hc * GR_LD + r], g, mm, vv, bc1, bc2, lim.lo[c], lim.hi[c]);
            if (ad.rule != 2) { m[gbase + i] = mm; v[gbase + i] = vv; }
        }
        __syncthreads();
    }
    if (wave == 0) {                          // get_action's forward pass (:342)
        const float J = final_cost();
        if (row0 + lane < a.N) a.J[row0 + lane] = J;
    }
    __syncthreads();
    for (int i = t; i < total; i += GR_BLOCK) {
        const int r = HC >= 2 ? (int)__umulhi((uint32_t)i, a.p_magic) : i, hc = i - r * HC;
        Q[gbase + i] = q_s[hc * GR_LD + r];
    }
