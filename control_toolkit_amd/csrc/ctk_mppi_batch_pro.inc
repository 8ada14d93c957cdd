// ctk_mppi_batch_pro.inc — the prologue both forms of the batch kernel share (ctk_mppi.hip: ctk_mppi_batch / ctk_mppi_batch_pp): from the
// step record of blockIdx.y and the descriptor of its problem to what ctk_mppi_body.inc expects of ctk_mppi_rollout's arguments.
// Expects in scope: ENV; desc, steps, a_tpl, fz_tpl.  Leaves: q, d, a_in, samples, u_nom, parts, fz.
    const CtkBatchStep& q = steps[blockIdx.y];
    const CtkBatchDesc& d = desc[q.id];
    RolloutArgs a_in = a_tpl;
#pragma unroll
    for (int i = 0; i < Env<ENV>::S; ++i) a_in.s0[i] = q.s[i];
#pragma unroll
    for (int c = 0; c < Env<ENV>::C; ++c) a_in.u_prev[c] = q.u_prev[c];
    a_in.u_prev_dev = q.dev_uprev ? d.u_dev : nullptr;
    a_in.J = d.J; a_in.Q_out = d.Q_out; a_in.traj_out = d.traj_out;
    a_in.seed_lo = d.seed_lo; a_in.seed_hi = d.seed_hi; a_in.call = q.call;
    const float* samples = q.samples;
    const float* u_nom = q.cur ? d.unom[1] : d.unom[0];
    float* parts = d.parts;
    FuseArgs fz = fz_tpl;                      // mode 1, stage_ok, the shared update constants (launcher)
    fz.ll = d.ll;
    fz.up.seq = q.seq;
    fz.up.u_nom_in = u_nom; fz.up.u_nom_out = q.cur ? d.unom[0] : d.unom[1];
    fz.up.u_dev = d.u_dev; fz.up.u_host = d.u_host;
