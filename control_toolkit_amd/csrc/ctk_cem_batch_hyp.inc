// ctk_cem_batch_hyp.inc — what ctk_cem_batch_hp (ctk_cem_fused.hip) puts behind the shared prologue in place of ctk_cem_batch_pp's load of
// k: element blockIdx.y of the array behind the step records is [K | CtkCemBatchHyper] (stride CtkCemKhStride<ENV>).  k as in _pp; the
// problem's cem_best_k, deviations and limits into what ctk_cem_body.inc reads them from — cf.K, cf.std_min, cf.init_std and a.lo /
// a.hi; `mid`, the one array the body indexes dynamically, names the problem's middles WHERE THEY LIE in the element (a local copy
// indexed so would put cf in scratch, which the other two forms do not have: they read the kernel-argument segment).  The element's address needs the preloaded
// pointer and blockIdx.y only, so all of it arrives by scalar loads in the round trip that fetches the record and, in _pp, k: no load
// the first tile or the state depends on waits for one more.  Every workgroup of a problem reads the same element.
// Expects in scope: ENV, E, C; kh_steps, a, cf.  Leaves: k, mid.
    const unsigned char* kh = kh_steps + (size_t)blockIdx.y * CtkCemKhStride<ENV>::value;
    const typename E::K k = *reinterpret_cast<const typename E::K*>(kh);
    const CtkCemBatchHyper& hy = *reinterpret_cast<const CtkCemBatchHyper*>(kh + CtkBatchKStride<ENV>::value);
    cf.K = hy.K; cf.std_min = hy.std_min; cf.init_std = hy.init_std;
#pragma unroll
    for (int c = 0; c < C; ++c) { a.lo[c] = hy.lo[c]; a.hi[c] = hy.hi[c]; }
    const float* mid = hy.mid;
