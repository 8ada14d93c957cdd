// ctk_mppi_body_1_decl.inc — part 1 of 5 of the body of ctk_mppi_rollout<ENV, PRED, LOG, P2P> (ctk_mppi.hip: the kernel's header comment and DESIGN.md 2.1 describe
// it), kept as TEXT so that the resident form (ctk_mppi_resident) compiles the SAME statements around other per-step inputs and in another
// order in time.  The launched kernel includes the five parts back to back (its ISA is what it was before the split).
//   1 decl    step-invariant definitions: the LDS carve, indices           4 phase_a  inputs of the first S1 steps (all four waves)
//   2 pro1    per-step tables + the sample tile into LDS                   5 post     recurrence (+ phase B), epilogue, record hand-off, merge tail
//   3 defs    S1, corr_keep, the prologue2 lambda
// Expects in scope: ENV, PRED, LOG, P2P, FORM (ctk_launch.h: CTK_MPPI_FORM_*); samples, u_nom, interp, wperm, parts, N_, H_, P_, pmagic_, a_in, k, m, fz; `extern __shared__ float lds[]`.
    using E = Env<ENV>;
    constexpr int C = E::C, S = E::S;
    static_assert(PRED == CTK_PRED_ODE || ENV == CTK_ENV_CARTPOLE, "network predictors: CartPole instantiations only");
    RolloutArgs a = a_in;
    a.N = N_; a.H = H_; a.P = P_ * C; a.p_magic = pmagic_;      // a.P: sample COLUMNS of a row (what the tile loader walks)
    constexpr int TRAJ = (PRED == CTK_PRED_GRU) ? GRU_TRAJ : (PRED == CTK_PRED_MLP_PAIR) ? MPPI_PAIR_TRAJ : MPPI_TRAJ;   // trajectories of this workgroup
    constexpr int CHUNKS = MPPI_BLOCK / TRAJ;                             // horizon chunks of prologue 2 (4 / 16)
    constexpr int RPW = TRAJ / MPPI_WAVES;                                // tile rows per wave in the epilogue
    const int Pp = P_, P = Pp * C, H = a.H, HC = H * C, ts = tile_stride(P), us = ubuf_stride(HC);   // Pp points, P columns
    float* tile = lds;                         // [TRAJ][ts]  stdev * noise at the inducing points (point i, channel c: column i*C + c)
    float* ubuf = tile + TRAJ * ts;            // [TRAJ][us]  clipped inputs u_run [H*C]
    float* corr_s = ubuf + TRAJ * us;          // [CHUNKS][TRAJ] per-chunk partial MPPI correction costs
    float* e_s = corr_s + MPPI_BLOCK;          // [TRAJ]
    float* col_s = e_s + TRAJ;                 // [4][P]    per-wave partial column sums
    float* w0_s = col_s + MPPI_WAVES * P;      // [H] [H] [H*C] [H]  per-step tables
    float* w1_s = w0_s + H;
    float* un_s = w1_s + H;
    int* i0_s = reinterpret_cast<int*>(un_s + HC);
    float* gru_ex = lds + mppi_carve_floats(P, HC, TRAJ, H);   // GRU only: exchange slots of the four waves (ctk_gru.h)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * TRAJ;
    const int n = row0 + lane;                 // wave 0's view: lane = trajectory of the workgroup
    const bool valid = lane < TRAJ && n < a.N;
    const bool use_ll = fz.mode != 0 && fz.ll != nullptr;   // kernel-argument uniform
    constexpr bool WIDE_TAIL = (FORM & CTK_MPPI_FORM_WIDE_TAIL) != 0;   // the 16-deep poll and the sliced merge of many narrow records
    constexpr bool PIPE = (FORM & CTK_MPPI_FORM_OLD_RECUR) == 0 && env_pipelined<ENV>::value;   // recurrence: sin / cos one step ahead
    // u ahead of the plan update (part 5): the launched kernel's order unless LATE_U; the resident and batch forms keep the late order
#ifdef CTK_BODY_EARLY_U
    constexpr bool EARLY_U = ctk_mppi_early_u_ok(FORM, PRED, C, P2P);
#else
    constexpr bool EARLY_U = false;
#endif
    // the publish of u: a launched kernel's end orders everything the step leaves, so {u, seq} goes out relaxed (ctk_device.h:
    // publish_u_launched); the resident kernel stays on the device and keeps publish_u's release
#ifdef CTK_BODY_RESIDENT
    constexpr bool PUB_REL = true;
#else
    constexpr bool PUB_REL = false;
#endif

    const uint32_t ka_sink = kernarg_prefetch<sizeof(RolloutArgs) + sizeof(typename E::K) + sizeof(MppiK) + 5 * sizeof(void*) + 16 + sizeof(FuseArgs)>();
