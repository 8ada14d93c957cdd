// ctk_g_rpgd_batch_hyp.inc — what ctk_g_rpgd_batch_hp (ctk_generic.hip) puts behind the shared prologue in place of ctk_g_rpgd_batch_pp's
// load of k: element blockIdx.y of the array behind the step records is [K | CtkRpgdBatchHyper] (stride CtkRpgdKhStride<ENV>).  k as in
// _pp; the problem's Adam constants and the address of its bias-correction table under the names the body reads (ad, bc_table); `lim`
// names its limits WHERE THEY LIE in the element (RpgdLimits: the body and the tail index them by a lane's input, and a local copy
// indexed so would live in scratch, which the other two forms do not have); its sampling constants are taken from hy by
// ctk_g_rpgd_batch_epi.inc.  The element's address needs the kernel argument and blockIdx.y only: scalar loads, in the round trip
// that fetches the record and, in _pp, k.
// Expects in scope: ENV; kh_steps.  Leaves: k, hy, ad, bc_table, lim.
    const unsigned char* kh = kh_steps + (size_t)blockIdx.y * CtkRpgdKhStride<ENV>::value;
    const typename Env<ENV>::K k = *reinterpret_cast<const typename Env<ENV>::K*>(kh);
    const CtkRpgdBatchHyper& hy = *reinterpret_cast<const CtkRpgdBatchHyper*>(kh + CtkBatchKStride<ENV>::value);
    const AdamK ad = hy.ad;
    const float* __restrict__ bc_table = hy.bc_table;
    const RpgdLimits lim{hy.lo, hy.hi};
