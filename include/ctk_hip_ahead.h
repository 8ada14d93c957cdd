/* ctk_hip_ahead.h — the launched-ahead form of the MPPI step: part of the C ABI of libctk_hip.so, included by ctk_hip.h (include that;
 * this file holds the declarations so that the lists of entry points in the other headers stay what they are).  Added without an ABI
 * bump, as the batch families and the other headers were: ctk_abi_version() stays 6. */
#ifndef CTK_HIP_AHEAD_H
#define CTK_HIP_AHEAD_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A caller that steps in a tight loop (Controllers/controller_mpc.py:104 called back to back, a benchmark, a simulation) pays the
 * launch call and the dispatch latency in front of every step, while the device stands idle.  Once such a loop is recognised, ctk_step
 * for step k also LAUNCHES the kernel of step k+1 (kernel ctk_mppi_ahead<ENV>): it is queued on the handle's stream behind step k's
 * kernel, starts when that ends, and waits at its entry for a request — state, previous input, sample pointer — which the next
 * ctk_step stores into a mailbox in device memory.  One launch per step and the same arithmetic: results are bit for bit those of the
 * launched step.  Nothing is read before the request is seen.
 *
 *  - the wait is bounded by a wall-clock FUSE (fuse_us).  A kernel whose request does not come leaves without having written
 *    anything; the next ctk_step finds that out, consumes a sequence number and launches the step as ever.  After ctk_step returns,
 *    ONE such bounded kernel of the handle may therefore be queued: a device-wide synchronize issued by anybody waits at most fuse_us
 *    for it.  Every other call on the handle that touches device state (read, get/set_state, set_param, reset, rollout, set_stream,
 *    sharded and peer-to-peer steps, resident_enable, destroy) first cancels it (the kernel leaves at once) and waits for that;
 *  - ARMING.  A step is eligible when it is an MPPI step of the analytic predictor in the one-launch regime with the narrow
 *    {value, seq} tail, on the handle's OWN stream, with device samples or the in-kernel sampler, without step log, per-launch timing,
 *    a pending sharded step or the resident form.  The form arms once the last CTK_AHEAD_ARM_AFTER steps were eligible and each
 *    arrived within fuse_us of the previous step's result; it disarms on a step that is not eligible and after
 *    CTK_AHEAD_DISARM_AFTER consecutive launches that were not taken, and re-arms by the same rule.  A slow caller never sees it;
 *  - it needs a mailbox in fine-grained device memory that the host can store into through the PCIe BAR (probed once); where that is
 *    not to be had the form stays off;
 *  - ctk_dominant_kernel keeps naming the launched kernel of the handle's configuration (the kernel a timed launch runs; the same body
 *    text); ctk_ahead_kernel names ctk_mppi_ahead<ENV>, as a kernel trace prints it, once a step was served by it ("" until then).
 *
 * ctk_ahead_rule_step is the arming rule itself, a pure function of its arguments (no device): `r` is the rule's state (zero it to
 * start), eligible / gap_us describe the arriving step (gap_us: since the previous step's result; < 0: there was none), outcome the
 * fate of the launch the PREVIOUS step issued (CTK_AHEAD_NONE: it issued none).  Returns 1 if the arriving step may launch ahead. */
#define CTK_AHEAD_ARM_AFTER 8
#define CTK_AHEAD_DISARM_AFTER 2
enum ctk_ahead_outcome { CTK_AHEAD_NONE = 0, CTK_AHEAD_TAKEN = 1, CTK_AHEAD_UNTAKEN = 2 };
typedef struct ctk_ahead_rule {
    int32_t streak;    /* consecutive eligible steps that arrived within the fuse */
    int32_t armed;
    int32_t untaken;   /* consecutive launches that were not taken */
    int32_t arms;      /* times the rule went from not armed to armed */
} ctk_ahead_rule;
int ctk_ahead_rule_step(ctk_ahead_rule* r, int eligible, double gap_us, double fuse_us, int outcome);

typedef struct ctk_ahead_counters {
    uint64_t launched;    /* kernels launched ahead */
    uint64_t taken;       /* ... that served their step */
    uint64_t untaken;     /* ... that left on their fuse (the step was then launched as ever) */
    uint64_t cancelled;   /* ... that another call on the handle ended */
    uint64_t arms;        /* times the form armed */
    int32_t armed;        /* is it armed now */
    int32_t pending;      /* is a kernel queued now */
    int32_t available;    /* 1: the handle can use the form (sizes, mailbox); 0: it never will */
    int32_t on;           /* the switch (ctk_ahead_enable; CTK_MPPI_NO_AHEAD in the environment sets it to 0 for the process) */
} ctk_ahead_counters;

/* on: 0 off (a queued kernel is cancelled first) | 1 on (the default for every handle).  fuse_us: within [1, 1e4]; <= 0 keeps the
 * current value (default CTK_AHEAD_DEFAULT_FUSE_US). */
#define CTK_AHEAD_DEFAULT_FUSE_US 20.0
int ctk_ahead_enable(ctk_handle* h, int on, double fuse_us);
int ctk_ahead_stats(const ctk_handle* h, ctk_ahead_counters* out, double* fuse_us);
const char* ctk_ahead_kernel(const ctk_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_AHEAD_H */
