// ctk_g_rpgd_batch_pro.inc — the prologue the forms of the batched RPGD step share (ctk_generic.hip: ctk_g_rpgd_batch, ctk_g_rpgd_batch_pp,
// ctk_g_rpgd_batch_hp): from the step record of blockIdx.y and the descriptor it names, what ctk_g_rpgd_body.inc expects of
// ctk_g_rpgd_descent's arguments.  Expects in scope: ENV; desc, steps, a_tpl.  Leaves: rec, d, lim, a, cur, Q, m, v, t0, iters, scratch.
// CTK_RPGD_BATCH_HP (defined around the include by ctk_g_rpgd_batch_hp alone): lim is left to ctk_g_rpgd_batch_hyp.inc, where it names the
// problem's limits in device memory; the other two forms see the text they always saw.
    const CtkRpgdBatchStep& rec = steps[blockIdx.y];
    const CtkRpgdBatchDesc& d = desc[rec.id];
#ifndef CTK_RPGD_BATCH_HP
    const RolloutArgs& lim = a_tpl;                // the limits are read where the kernel argument lies (ctk_g_rpgd_body.inc)
#endif
    RolloutArgs a = a_tpl;                         // sizes, p_magic, inv_Hp1, global_row0 (launcher)
#pragma unroll
    for (int i = 0; i < Env<ENV>::S; ++i) a.s0[i] = rec.s[i];
#pragma unroll
    for (int c = 0; c < Env<ENV>::C; ++c) a.u_prev[c] = rec.u_prev[c];
    a.u_prev_dev = rec.dev_uprev ? d.u_dev : nullptr;
    a.J = d.J;
    a.seed_lo = d.seed_lo; a.seed_hi = d.seed_hi; a.call = rec.call;
    const uint32_t cur = rec.cur & 1u;
    float* __restrict__ Q = d.pop[cur];
    float* __restrict__ m = d.m[cur];
    float* __restrict__ v = d.v[cur];
    const int t0 = rec.t0, iters = rec.iters;
    float* __restrict__ scratch = d.scratch;       // blockIdx.x == 0: the problem's own slice
