// ctk_cem_batch_pro.inc — the prologue of the batch forms of the one-launch CEM step (ctk_cem_fused.hip: ctk_cem_batch, ctk_cem_batch_pp,
// ctk_cem_batch_hp): from the step record of blockIdx.y and the descriptor it names, what ctk_cem_fused takes as arguments (samples, a,
// cf, mid, bx).  Expects desc, steps, N_, H_, P_, pmagic_, nblk_, K_, a_tpl, cf_tpl and the constants S, C in scope.
// CTK_CEM_BATCH_HP (defined around the include by ctk_cem_batch_hp alone): K_ is not expected, cf.K is left to ctk_cem_batch_hyp.inc, and
// mid is left to it too, where it names the problem's array in device memory; the other two forms see the text they always saw.
    const CtkCemBatchStep& q = steps[blockIdx.y];
    const CtkCemBatchDesc& d = desc[q.id];
    RolloutArgs a = a_tpl;                         // limits, inv_Hp1, global_row0 (launcher)
    a.N = N_; a.H = H_; a.P = P_; a.p_magic = pmagic_;
#pragma unroll
    for (int i = 0; i < S; ++i) a.s0[i] = q.s[i];
#pragma unroll
    for (int c = 0; c < C; ++c) a.u_prev[c] = q.u_prev[c];
    a.u_prev_dev = q.dev_uprev ? d.u_dev : nullptr;
    a.J = d.J; a.Q_out = d.Q_out; a.traj_out = d.traj_out;
    a.seed_lo = d.seed_lo; a.seed_hi = d.seed_hi; a.call = q.call;
    const float* samples = q.samples;
    CemFusedK cf = cf_tpl;                         // per_it, std_min / std_max / init_std, mid[], timeout_ticks (launcher)
#ifdef CTK_CEM_BATCH_HP
    cf.nblk = nblk_;
#else
    cf.nblk = nblk_; cf.K = K_;
#endif
    cf.its = q.its; cf.tag0 = q.tag0; cf.seq = q.seq;
    cf.llJ = d.ll; cf.llS = d.ll + N_;
    cf.mu = d.mu; cf.sd = d.sd; cf.u_dev = d.u_dev; cf.u_host = d.u_host; cf.idx_out = d.idx_out;
#ifndef CTK_CEM_BATCH_HP
    const float* mid = cf_tpl.mid;                 // shared by value: read where the kernel argument lies
#endif
    const uint32_t bx = blockIdx.x;                // unsigned, as blockIdx.x is: the body's index arithmetic keeps its types
