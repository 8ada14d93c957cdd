// ctk_g_rpgd_batch_epi.inc — what follows ctk_g_rpgd_body.inc in both forms of the batched RPGD step (ctk_generic.hip: ctk_g_rpgd_batch,
// ctk_g_rpgd_batch_pp): the keep-k selection and the warm start of the problem (ctk_rpgd_warm.h: rpgd_fused_tail), described by the step
// record and the descriptor.  Expects what ctk_g_rpgd_batch_pro.inc and the body leave, and fw_tpl; under CTK_RPGD_BATCH_HP also hy
// (ctk_g_rpgd_batch_hyp.inc), whose sampling constants replace the launcher's.
    FusedWarm fw = fw_tpl;                         // K, P, shift_previous, the sampling constants, interp (launcher)
#ifdef CTK_RPGD_BATCH_HP
    fw.w.sample_stdev = hy.sample_stdev; fw.w.sample_mean = hy.sample_mean; fw.w.sample_min = hy.sample_min; fw.w.sample_max = hy.sample_max;
#endif
    fw.idx_out = d.idx;
    fw.w.n_new = rec.resample ? a.N - fw.K : 0;
    fw.w.gather = rec.resample ? 1 : 0;
    fw.p.draws = rec.draws;
    fw.p.Q_old = Q; fw.p.m_old = m; fw.p.v_old = v; fw.p.ages_old = d.ages[cur];
    fw.p.Q_new = d.pop[cur ^ 1u]; fw.p.m_new = d.m[cur ^ 1u]; fw.p.v_new = d.v[cur ^ 1u]; fw.p.ages_new = d.ages[cur ^ 1u];
    fw.p.u_nom = d.u_nom; fw.p.u_dev = d.u_dev; fw.p.u_host = d.u_host; fw.p.seq = rec.seq;
    rpgd_fused_tail(a, lim, fw, g_s, t, HC);
