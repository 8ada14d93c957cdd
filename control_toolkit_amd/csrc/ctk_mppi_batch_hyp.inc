// ctk_mppi_batch_hyp.inc — what the _hp forms of the batch kernel (ctk_mppi.hip: ctk_mppi_batch_hp / _mlp_hp / _gru_hp) put behind the
// shared prologue in place of the _pp forms' load of k: the problem's element of the array in kdev's slot is [K | CtkBatchHyper]
// (ctk_launch.h; stride CtkBatchKhStride<ENV>).  k as in _pp; the optimizer constants and input limits into what ctk_mppi_body.inc reads
// them from — a local MppiK m, a_in.lo / hi, and the update's fz.up.lo / hi / lo_c / hi_c (mppi_update_args).  The element's address
// needs the preloaded pointer and the uniform q.id only, so all of it arrives by scalar loads in the round trip that fetches the
// descriptor and, in _pp, k: no dependent load is added ahead of the sample-tile loads.  The values stay in SGPRs through the
// recurrence as k does in the _pp forms.
// Expects in scope: ENV; kdev, q, a_in, fz.  Leaves: k, m.
    const unsigned char* kh = kdev + (size_t)q.id * CtkBatchKhStride<ENV>::value;
    const typename Env<ENV>::K k = *reinterpret_cast<const typename Env<ENV>::K*>(kh);
    const CtkBatchHyper& hy = *reinterpret_cast<const CtkBatchHyper*>(kh + CtkBatchKStride<ENV>::value);
    const MppiK m = hy.m;
#pragma unroll
    for (int c = 0; c < Env<ENV>::C; ++c) {
        a_in.lo[c] = hy.lo[c]; a_in.hi[c] = hy.hi[c];
        fz.up.lo_c[c] = hy.lo[c]; fz.up.hi_c[c] = hy.hi[c];
    }
    fz.up.lo = hy.lo[0]; fz.up.hi = hy.hi[0];
