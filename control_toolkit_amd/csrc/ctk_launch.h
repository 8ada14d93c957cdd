// ctk_launch.h — host-callable launchers implemented in the kernel translation units.
#pragma once
#include <hip/hip_ext.h>
#include "ctk_common.h"

// Launch with the dispatch's own begin/end timestamps attached to (ev_start, ev_stop) when given
// (hipExtLaunchKernelGGL): the measured interval is the kernel, not the queue around it.
#define CTK_LAUNCH(kernel, grid, block, lds, st, e0, e1, ...)                                         \
    do {                                                                                              \
        if (e0) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, e0, e1, 0, __VA_ARGS__);          \
        else hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                           \
    } while (0)

// a runtime flag as a compile-time constant: f(std::true_type{}) or f(std::false_type{}), so that a launch whose template takes the
// flag writes its argument list once (f is a generic lambda, called in place: nothing is stored)
#include <type_traits>
template <class F>
inline void ctk_with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// RolloutArgs as an environment's template kernels take them: C inputs, `cols` flat sample columns per row (P*C or H*C) and their divisor
inline RolloutArgs ctk_rollout_args(const RolloutArgs& a_in, int C, int cols) {
    RolloutArgs a = a_in;
    a.C = C; a.P = cols; a.p_magic = ctk_magic_of(cols);
    return a;
}
// ... and their descent kernels: the rows are the H*C columns of a plan, a.P stays the caller's
inline RolloutArgs ctk_descent_args(const RolloutArgs& a_in, int C) {
    RolloutArgs a = a_in;
    a.C = C; a.p_magic = ctk_magic_of(a.H * C);
    return a;
}

// kernel names as rocprofv3's trace prints them, formatted once per (template, arguments) and kept for the process's lifetime
// (ctk_dominant_kernel returns the pointer); any number of environments
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
inline const char* ctk_kernel_name(const char* fmt, int a = 0, int b = 0, int c = 0, const char* s0 = "", const char* s1 = "") {
    static std::map<std::string, std::string> names;
    static std::mutex mu;
    char buf[160];
    std::snprintf(buf, sizeof buf, fmt, a, b, c, s0, s1);
    std::lock_guard<std::mutex> lock(mu);
    return names.emplace(buf, buf).first->second.c_str();
}

// ---- ctk_mppi.hip ---------------------------------------------------------------------------
const char* ctk_mppi_rollout_name(int pred, bool log, int N, bool identity_interp = false, bool have_samples = true, bool p2p = false, int H = 0,
                                  int form = 0);
int ctk_mppi_num_blocks(int N, int pred);   // workgroups = block records of one rollout launch (64 trajectories each; GRU: 16)
bool ctk_mppi_uses_throughput_kernel(int pred, int N);
size_t ctk_mppi_rollout_lds(int P, int H, int pred = 0, int N = 1 << 30, int C = 1);
// MLP, N <= CTK_MPPI_PAIR_MAX_N: workgroups of 32 trajectories with a tile's network step shared by two waves (ctk_mlp.h:
// mlp_step_pair) — at these sizes 16 trajectories per wave leave half of the chip's SIMDs idle.
constexpr int CTK_MPPI_PAIR_MAX_N = 8192;
constexpr int CTK_PRED_MLP_PAIR = 3;   // kernel-variant id (internal to the launchers, not a ctk_predictor value)
// wperm: per-lane permuted MLP weights (ctk_api.hip: permute_mlp_weights), nullptr for the ODE predictor
// In-launch merge by the last block to finish (<= CTK_MPPI_FUSE_MAX_BLOCKS blocks).
constexpr int CTK_MPPI_FUSE_MAX_BLOCKS = 64;     // ticket form: beyond this the last block's serial record fetch costs more than a launch
constexpr int CTK_MPPI_FUSE_MAX_BLOCKS_LL = 128; // {value, seq} form (records staged in LDS): measured 26.7 vs 29.5 us at 128 blocks, 30.8 vs 29.1 at 256
// ... of FULL-width records (cfg2: 2 + 50 words).  What the tail block pays for is WORDS polled and staged, not records: a shard of
// BASELINE configs[4] (N 8 192, period 10: 256 records of 2 + 11 words = 3 328 words, half of cfg2's 128 x 52) hands over in-launch as
// well (round 4: ctk_mppi_step_begin at that size was rollout + merge<false> + merge<true>, three launches)
constexpr int CTK_MPPI_FUSE_MAX_BLOCKS_LL_NARROW = 512, CTK_MPPI_FUSE_MAX_WORDS_LL_NARROW = 4096;
inline bool ctk_ll_records_ok(int blocks, int cols) {
    return blocks <= CTK_MPPI_FUSE_MAX_BLOCKS_LL ||
           (blocks <= CTK_MPPI_FUSE_MAX_BLOCKS_LL_NARROW && blocks * (2 + cols) <= CTK_MPPI_FUSE_MAX_WORDS_LL_NARROW);
}
// Forms of the 4-wave rollout kernel (ctk_mppi.hip: ctk_mppi_rollout / ctk_mppi_resident), chosen per launch.  Bits:
//   WIDE_TAIL  the {value, seq} tail of more than CTK_MPPI_FUSE_MAX_BLOCKS_LL records or CTK_MPPI_LL_NARROW_WORDS words: the 16-deep
//              poll batch and the sliced merge of many narrow records (a configs[4] shard).  Without it the tail has only the 8-deep
//              batch and one thread per column — what a launch within those sizes runs in either form, so the results do not depend on it
//   OLD_RECUR  the recurrence without sin / cos one step ahead (ctk_env.h: recur_env_range): diagnostic switch CTK_MPPI_OLD_RECUR,
//              bit for bit the same results (tests/test_gpu_mppi_pipelined.py)
//   LATE_U     u = u_nom_new[0] is published by the final update, behind the plan update of all H entries — the order before FORM 0
//              published it ahead of them (ctk_mppi_body_5_post.inc: EARLY_U): diagnostic switch CTK_MPPI_LATE_U, bit for bit the same
//              results (tests/test_gpu_mppi_early_u.py).  Raised only where FORM 0 would take the early order: the late order is
//              what every other launch runs anyway (ctk_mppi_early_u_ok), under the name it had
constexpr int CTK_MPPI_FORM_WIDE_TAIL = 1, CTK_MPPI_FORM_OLD_RECUR = 2, CTK_MPPI_FORM_LATE_U = 4;
// does a launched 4-wave kernel of this form compile the early order?  (pred: the kernel variant, 0 = the analytic predictor; C control
// inputs; at run time it also takes a merge + update launch with the {value, seq} tail: fuse mode 1)
constexpr bool ctk_mppi_early_u_ok(int form, int pred, int C, bool p2p) {
    return (form & (CTK_MPPI_FORM_LATE_U | CTK_MPPI_FORM_WIDE_TAIL)) == 0 && pred == 0 && C == 1 && !p2p;
}
constexpr int CTK_MPPI_LL_NARROW_WORDS = 8 * 256;   // one 8-deep poll batch of the 256-thread merging workgroup
inline bool ctk_ll_tail_wide(int blocks, int cols) {
    return blocks > CTK_MPPI_FUSE_MAX_BLOCKS_LL || blocks * (2 + cols) > CTK_MPPI_LL_NARROW_WORDS;
}
// can a rollout launch of `blocks` workgroups merge and update in-launch?  (have_ll: the handle owns the LL word buffer)
bool ctk_mppi_fusable(int P, int blocks, bool have_ll);
// From this many rollouts on (ODE predictor) the latency-oriented 4-wave block gives way to the
// throughput-oriented single-wave block (half the LDS, 2x the resident recurrence waves per CU).
constexpr int CTK_MPPI_THROUGHPUT_MIN_N = 32768;
// The resident form's mailbox: one request per MPPI step, written by the HOST only — the payload first, then `req`.  Where it lives:
// in fine-grained DEVICE memory that the host stores into through the PCIe BAR (posted writes + sfence; every workgroup then polls LOCAL
// memory: no PCIe read on the request path), or — where the host cannot reach device memory — in pinned host memory, polled by ONE
// workgroup that relays it to the others through device memory (`relay`).  What the DEVICE reports goes to CtkResidentStat in pinned host
// memory.  ctk_mppi.hip: ctk_mppi_resident.
enum { CTK_RES_CMD_STEP = 0, CTK_RES_CMD_EXIT = 1 };
enum { CTK_RES_IDLE = 0, CTK_RES_RUNNING = 1, CTK_RES_LEAVING = 2, CTK_RES_LEFT = 3 };
struct CtkResidentBox {
    uint32_t req;                       // request number (monotonic within a handle); written LAST
    uint32_t cmd;                       // CTK_RES_CMD_*
    uint32_t seq;                       // the step's sequence number: tag of its record words and of {u, seq}
    uint32_t call;                      // Philox position of the step (in-kernel sampler)
    uint32_t cur;                       // which u_nom buffer holds the current plan
    uint32_t dev_uprev;                 // 1: the previous input is the optimizer's own last output on the device (u_prev == NULL at the API)
    const float* samples;               // this step's draws (device pointer), or nullptr
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
    const float* next_samples;          // the host's guess at the NEXT step's draws (nullptr with next_known: the in-kernel sampler): the kernel forms
    uint32_t next_known;                // that step's inputs while the host works on this one; a wrong guess costs nothing but that work
    uint32_t tail;                      // == req, written with the payload BEFORE req: a reader that finds req == tail in ONE pass over the box has a
    uint32_t pad;                       //    consistent request (writes arrive in order), and needs no second round trip for the payload
    uint32_t upd;                       // relay only: request number whose update (u_nom, u) block 0 has published
};
struct CtkResidentStat {                // device -> host
    uint32_t state;                     // CTK_RES_*
    uint32_t served;                    // last request taken, written when the kernel leaves
    uint32_t t_relay, t_body;           // diagnostics: wall-clock ticks (10 ns) block 0 spent fetching / relaying the last request, and in its step
    uint32_t c_body;                    // ... and that step in shader-clock cycles (clock64)
    uint32_t stamps[12];                // diagnostic builds (-DCTK_RES_STAMPS): the body's STAMP(i) points, shader cycles since the request
};

struct MppiFuse {
    int mode = 0;              // 0 records only, 1 merge + update u_nom/u, 2 merge into ONE record (sharded step_begin),
                               // 3 = 2 + peer-to-peer exchange + update in the same launch (ctk_p2p_step)
    unsigned* counter = nullptr;
    float* out_rec = nullptr;  // mode 2
    unsigned long long* ll = nullptr;   // [blocks][2+P] {value, seq} words: low-latency hand-off (else ticket + fetch)
    const void* p2p = nullptr;          // mode 3 (needs ll): device-resident P2PArgs; block 0 exchanges with the peers and updates
    uint32_t p2p_seq = 0;
    int p2p_world = 0;
    float* u_nom_out = nullptr, *u_dev = nullptr, *u_host = nullptr;   // mode 1
    uint32_t seq = 0;          // sequence number published with u (mode 1)
};
hipError_t ctk_launch_mppi_rollout(hipStream_t st, int pred, const RolloutArgs& a, const EnvK& k, const MppiK& m,
                                   const float* samples, const float* u_nom, const float* wperm, float* parts, bool log,
                                   const MppiFuse& fuse, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                                   const char** ran = nullptr);   // *ran: name of the kernel this call launched
// the 4-wave kernel for any environment's analytic predictor (a.P inducing points, a.C inputs; constants derived from `params`)
hipError_t ctk_launch_mppi_rollout_env(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                       const float* samples, const float* u_nom, float* parts, bool log, const MppiFuse& fuse,
                                       hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
size_t ctk_mppi_rollout_env_lds(int env, int P, int H, int N);
// the resident form of the same kernel (fuse mode 1 with the {value, seq} hand-off only): launched once, serves requests from `box`
hipError_t ctk_launch_mppi_resident(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                    float* u_nom0, float* u_nom1, float* parts, const MppiFuse& fuse, const CtkResidentBox* box_dev, int box_local,
                                    CtkResidentStat* stat_dev, CtkResidentBox* relay, double idle_us, uint32_t first_req, void* args_dev, void* args_host);
constexpr size_t CTK_RES_ARGS_BYTES = 1024;   // device + host staging block for the resident kernel's argument struct
const char* ctk_mppi_resident_name(int env, int N, int P);   // N rollouts, P inducing points (per control input)
const char* ctk_mppi_rollout_env_name(int env, bool log);
// The LAUNCHED-AHEAD form of the same kernel (ctk_mppi.hip: ctk_mppi_ahead<ENV>; include/ctk_hip_ahead.h): still one launch per step, but
// the launch of step k+1 is issued while the device works on step k.  What is known at that time travels as kernel arguments (the
// buffers, the next sequence number, Philox position and plan buffer); what only the step's caller knows — state, previous input, sample
// pointer — arrives in a MAILBOX the kernel waits for at its entry: fine-grained device memory the host stores into through the PCIe
// BAR (payload + tail, sfence, request number, as CtkResidentBox).  The wait is bounded by a wall-clock fuse; a kernel that saw no
// request leaves having written nothing but its state word.
struct alignas(128) CtkAheadBox {        // one 128-byte line: a reader's single pass over it sees the host's stores in their order
    uint32_t req;                       // request number (monotonic within a handle; each launch waits for exactly ONE number); written LAST
    uint32_t cmd;                       // CTK_RES_CMD_STEP | CTK_RES_CMD_EXIT (cancel: the kernel leaves at once)
    uint32_t dev_uprev;                 // 1: the previous input is the optimizer's own last output on the device (u_prev == NULL at the API)
    uint32_t pad;
    const float* samples;               // this step's draws (device pointer), or nullptr: the in-kernel sampler
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
    uint32_t tail;                      // == req, written with the payload BEFORE req (CtkResidentBox::tail)
};
constexpr int CTK_AHEAD_BOX_WORDS = 19;  // dwords of CtkAheadBox up to and including tail
// the state word (pinned host memory, written by workgroup 0 only): (request number << 2) | CTK_RES_RUNNING (the request was taken) /
// CTK_RES_LEAVING (the fuse ran out; the request is looked for once more) / CTK_RES_LEFT (left without a step: the kernel's last store)
constexpr uint32_t ctk_ahead_state(uint32_t req, uint32_t code) { return (req << 2) | code; }
struct CtkAheadGate {
    const CtkAheadBox* box;             // device address of the mailbox
    uint32_t* state;                    // device address of the state word (pinned host memory)
    uint32_t* relay;                    // device memory: workgroup 0 stores `req` here when it leaves, the other workgroups follow
    uint32_t req;                       // the request number this launch waits for
    uint32_t pad;
    unsigned long long fuse_ticks;      // wall_clock64 ticks (100 MHz)
};
// may a handle of these sizes step through ctk_mppi_ahead?  (the one-launch step with the narrow {value, seq} tail, FORM 0)
bool ctk_mppi_ahead_ok(int env, int N, int H, int P);
const char* ctk_mppi_ahead_name(int env);
// a: make_args of a zero state with u_prev == NULL (u_prev_dev = the handle's d_u) and the NEXT step's Philox position; fuse: mode 1
// with the next step's sequence number and plan buffers, as mppi_rollout would fill it for that step
hipError_t ctk_launch_mppi_ahead(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                 const float* u_nom, float* parts, const MppiFuse& fuse, const CtkAheadGate& gate);
// the BATCH form of the same kernel (ctk_mppi.hip: ctk_mppi_batch<ENV, LOG>; include/ctk_hip.h: ctk_batch_*): B independent problems of ONE
// configuration, grid (workgroups per problem, problems of this launch).  What differs per problem reaches the kernel through two arrays in
// device memory: the descriptor [B] (where the problem's buffers are; written once, at creation) and the step records [problems of this
// step] (which problem, its state / previous input / sample pointer / Philox position / sequence number / current plan buffer; written by
// the host into pinned memory and copied with ONE transfer ahead of the launch).  blockIdx.y picks the step record, its id the descriptor.
struct CtkBatchDesc {
    float* parts;                       // [blocks][2 + P*C] block records (the ticket path's; unused by the {value, seq} tail)
    unsigned long long* ll;             // [blocks][2 + P*C] {value, seq} record words
    float* J;                           // [N]
    float* Q_out;                       // [N,H,C]
    float* traj_out;                    // [N,H+1,S] or nullptr
    float* unom[2];                     // [H,C] nominal plan, ping-pong
    float* u_dev;                       // [C] the problem's own last output
    float* u_host;                      // pinned {u, seq} slot (16 floats) with the error words behind it
    uint32_t seed_lo, seed_hi;          // Philox key
};
struct CtkBatchStep {
    int32_t id;                         // problem index = descriptor index
    uint32_t seq;                       // tag of this step's record words and of {u, seq}
    uint32_t call;                      // Philox position
    uint32_t cur;                       // which unom buffer holds the current plan (the step writes the other one)
    uint32_t dev_uprev;                 // 1: the previous input is the problem's own last output (u_prev == NULL at the API)
    uint32_t pad;
    const float* samples;               // this problem's draws [N,P,C] (device pointer) or nullptr: the in-kernel sampler
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
};
// One problem's optimizer constants and input limits (include/ctk_hip_hyper.h: *_problem_set_hyper / *_problem_set_limits; kernels
// ctk_mppi_batch_hp<ENV, LOG>, ctk_mppi_batch_mlp_hp<LOG>, ctk_mppi_batch_gru_hp<LOG, FORM>).  m is mppi_constants of the problem's
// values, the function behind a handle's; lo / hi are what a handle's launch carries in RolloutArgs and in the update's arguments.  For
// the _hp forms the per-problem array has elements of two parts, [K (ctk_mppi_batch_k_stride bytes) | CtkBatchHyper], at stride
// ctk_mppi_batch_kh_stride(env): both parts are read by scalar loads on the record's id off ONE pointer, in one round trip.
struct alignas(16) CtkBatchHyper {
    MppiK m;
    float lo[CTK_MAX_INPUTS], hi[CTK_MAX_INPUTS];
};
static_assert(sizeof(CtkBatchHyper) % 16 == 0, "the elements of the per-problem array stay 16-byte aligned");
size_t ctk_mppi_batch_kh_stride(int env);
// 0: a problem of these sizes runs in the batch kernel; else why not (1 throughput sizes, 2 more records / words than the FORM 0 tail takes,
// 3 the records do not fit the tail's LDS staging, 4 LDS over 160 KiB); *lds_out: dynamic LDS of a launch, *blocks_out: workgroups per problem
int ctk_mppi_batch_fit(int env, int N, int H, int P, size_t* lds_out, int* blocks_out);
// per_problem: the form whose constants come from an array in device memory (ctk_mppi_batch_pp<ENV, LOG>), one element per problem
// hyper: the form that also takes the optimizer constants and limits per problem (ctk_mppi_batch_hp<ENV, LOG>, CtkBatchHyper)
const char* ctk_mppi_batch_name(int env, bool log, bool per_problem = false, bool hyper = false);
// that array: element p at byte p * ctk_mppi_batch_k_stride(env) (sizeof(Env<env>::K) rounded up to 16), filled by
// ctk_mppi_batch_derive_k = Env<env>::derive(params, dt, isteps), the function behind a handle's constants (double -> fp32 once)
size_t ctk_mppi_batch_k_stride(int env);
void ctk_mppi_batch_derive_k(int env, const float* params, float dt, int isteps, void* dst);
// n_problems step records from `steps_dev` on, as ONE launch; a: the shared template (limits, sizes, interpolation table; s0 / u_prev / the
// output pointers / seed / call come from the records and descriptors).  k_dev == nullptr: ctk_mppi_batch, every problem with the
// constants of `params`; else ctk_mppi_batch_pp, problem p with element p of k_dev (`params` unused).  hyper (needs k_dev):
// ctk_mppi_batch_hp, k_dev has the two-part elements [K | CtkBatchHyper], whose second part stands in place of `m` and of a's limits
hipError_t ctk_launch_mppi_batch(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                 const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log,
                                 const void* k_dev = nullptr, bool hyper = false);
// the MLP forms of the batch kernel (ctk_mppi.hip: ctk_mppi_batch_mlp<LOG> / ctk_mppi_batch_mlp_pp<LOG>; include/ctk_hip.h: ctk_mlp_batch_*):
// CartPole's MLP predictor in the pair form (32 trajectories per workgroup), the same descriptors and step records, plus per-problem
// weight tables w_dev [B][ctk_mppi_batch_mlp_table_floats()] in the per-lane layout of a handle's launch (ctk_api.hip: permute_mlp_weights).
// fit: 0, or why not — 1 a handle of this N does not run the pair form (N > CTK_MPPI_PAIR_MAX_N, or the diagnostic switch
// CTK_MPPI_NO_PAIR), 2 / 3 / 4 as ctk_mppi_batch_fit
int ctk_mppi_batch_mlp_fit(int N, int H, int P, size_t* lds_out, int* blocks_out);
const char* ctk_mppi_batch_mlp_name(bool log, bool per_problem = false, bool hyper = false);
size_t ctk_mppi_batch_mlp_table_floats();
hipError_t ctk_launch_mppi_batch_mlp(hipStream_t st, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                     const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log,
                                     const float* w_dev, const void* k_dev = nullptr, bool hyper = false);
// the GRU forms of the batch kernel (ctk_mppi.hip: ctk_mppi_batch_gru<LOG, FORM> / ctk_mppi_batch_gru_pp<LOG, FORM>; include/ctk_hip.h:
// ctk_gru_batch_*): CartPole's GRU predictor, 16 trajectories per workgroup, the same descriptors and step records, in the FORM a handle
// of the configuration launches (0 or CTK_MPPI_FORM_WIDE_TAIL: mppi_form over the {value, seq} tail).  Problem p's block of w_dev, at
// p * ctk_mppi_batch_gru_block_floats(), is
//   [ per-lane table, ctk_mppi_batch_gru_table_floats() | carried hidden state h1[32] h2[32] | fast-cosine word | pad to 16 bytes ]
// — table | hidden as in a handle's d_wperm (ctk_api.hip: permute_gru_weights), so the body reads both where it reads a handle's.  The word
// is 1 where the network's outputs stay inside the unchecked cosine's range whatever the state (the host's net_out_bound * hidden_scale
// <= CTK_SINCOS_FAST_LIMIT); the kernel forms a.fast_cos_ok from it and |s[2]| of the step record, a handle's per-step decision.
// fit: 0 for exactly the sizes at which a handle hands its block records over in-launch through the {value, seq} words, else why not —
// 2 the records are too many for that tail (ctk_ll_records_ok), 3 they do not fit its LDS staging, 4 LDS over 160 KiB; *form_out: the FORM
int ctk_mppi_batch_gru_fit(int N, int H, int P, size_t* lds_out, int* blocks_out, int* form_out);
const char* ctk_mppi_batch_gru_name(bool log, int form, bool per_problem = false, bool hyper = false);
size_t ctk_mppi_batch_gru_table_floats();
size_t ctk_mppi_batch_gru_hidden_floats();
size_t ctk_mppi_batch_gru_block_floats();
hipError_t ctk_launch_mppi_batch_gru(hipStream_t st, const float* params, float dt, int isteps, const RolloutArgs& a, const MppiK& m,
                                     const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_problems, bool log, int form,
                                     const float* w_dev, const void* k_dev = nullptr, bool hyper = false);
// ctk_sampled.hip: ctk_gru_advance_batch, the hidden-state advance behind a step of the GRU batch — one workgroup per step record, the
// record's problem advanced by (the record's state, the problem's own last output desc[id].u_dev), in place in its block of w_dev
hipError_t ctk_launch_gru_advance_batch(hipStream_t st, const CtkBatchDesc* desc_dev, const CtkBatchStep* steps_dev, int n_records, float* w_dev);
// ---- ctk_plant.hip : the plant of a batch's closed loop (include/ctk_hip_run.h: ctk_batch_run / ctk_batch_plant_step) ----
// ONE launch of ctk_batch_plant<env>, one lane per record: record j of cur_dev (its id = the problem, its s = the state) advanced by
// Env<env>::step with element id of kplant_dev (stride ctk_mppi_batch_k_stride(env), filled by ctk_mppi_batch_derive_k from the PLANT's
// table and sub-step count) and the input u_in_dev [n][C], or, where that is NULL, the problem's own last output (its descriptor's
// u_dev).  The new state goes to states_out + j * state_stride, the input to inputs_out + j * input_stride (NULL: not kept) and, where
// next_dev is given, into next_dev[j].s — the record the next controller launch reads.
const char* ctk_batch_plant_name(int env);
hipError_t ctk_launch_batch_plant(hipStream_t st, int env, const CtkBatchDesc* desc_dev, const CtkBatchStep* cur_dev, CtkBatchStep* next_dev,
                                  const void* kplant_dev, const float* u_in_dev, float* states_out, float* inputs_out, int n_records,
                                  size_t state_stride, size_t input_stride);
// ---- ctk_plant.hip : the stochastic plant (include/ctk_hip_episode.h: ctk_batch_episodes / ctk_batch_plant_step_noisy) ----
// The Philox stream of the plants' noise: far from the optimizers' stream ids, which are small iteration numbers ("PLNT").
constexpr uint32_t CTK_PLANT_STREAM = 0x504C4E54u;
// One per step record of a segment's FIRST step, behind the records and travelling with them: the problem's noise at the segment start.
struct CtkPlantNoise {
    float sigma_w[CTK_MAX_STATES];      // process noise, per-step standard deviation per state (0: none)
    float sigma_v[CTK_MAX_STATES];      // measurement noise
    uint32_t seed_lo, seed_hi;          // Philox key of the noise
    uint32_t pos;                       // noise position at the segment start (the launch of step t draws at pos + t)
    uint32_t any;                       // some sigma is not 0 (else the record draws nothing)
};
// ONE launch of ctk_batch_plant_noisy<env>, one lane per record: record j's problem advanced from its TRUE state
// s_true_dev + j * s_true_stride with the input u_in_dev [n][C] (NULL: the problem's own last output) — the realised stage cost of
// (true state, input, u_last_dev + j * u_last_stride) to costs_out + j * cost_stride, the new true state to states_out + j * state_stride,
// the observation to obs_out + j * state_stride and, where next_dev is given, into next_dev[j].s; the input to inputs_out + j *
// input_stride (NULL: not kept).  noise_dev [n]; t: this launch's step within the segment.
const char* ctk_batch_plant_noisy_name(int env);
hipError_t ctk_launch_batch_plant_noisy(hipStream_t st, int env, const CtkBatchDesc* desc_dev, const CtkBatchStep* cur_dev, CtkBatchStep* next_dev,
                                        const void* kplant_dev, const CtkPlantNoise* noise_dev, const float* u_in_dev, const float* s_true_dev,
                                        size_t s_true_stride, const float* u_last_dev, size_t u_last_stride, uint32_t t, float* states_out,
                                        float* obs_out, float* inputs_out, float* costs_out, int n_records, size_t state_stride,
                                        size_t input_stride, size_t cost_stride);
// ---- ctk_plant.hip : the same two plants for the CEM and RPGD batches (include/ctk_hip_loop.h: ctk_cem_batch_run / ctk_rpgd_batch_run ...) ----
// Kernels ctk_cem_batch_plant<env> / ctk_cem_batch_plant_noisy<env> and ctk_rpgd_batch_plant<env> / ctk_rpgd_batch_plant_noisy<env>: the
// bodies of ctk_batch_plant / ctk_batch_plant_noisy over the family's descriptor and step record (id, s and u_dev are all they touch),
// so the launchers are overloads of the two above with the same arguments and meaning.
struct CtkCemBatchDesc; struct CtkCemBatchStep; struct CtkRpgdBatchDesc; struct CtkRpgdBatchStep;
const char* ctk_cem_batch_plant_name(int env);
const char* ctk_cem_batch_plant_noisy_name(int env);
const char* ctk_rpgd_batch_plant_name(int env);
const char* ctk_rpgd_batch_plant_noisy_name(int env);
hipError_t ctk_launch_batch_plant(hipStream_t st, int env, const CtkCemBatchDesc* desc_dev, const CtkCemBatchStep* cur_dev, CtkCemBatchStep* next_dev,
                                  const void* kplant_dev, const float* u_in_dev, float* states_out, float* inputs_out, int n_records,
                                  size_t state_stride, size_t input_stride);
hipError_t ctk_launch_batch_plant(hipStream_t st, int env, const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* cur_dev, CtkRpgdBatchStep* next_dev,
                                  const void* kplant_dev, const float* u_in_dev, float* states_out, float* inputs_out, int n_records,
                                  size_t state_stride, size_t input_stride);
hipError_t ctk_launch_batch_plant_noisy(hipStream_t st, int env, const CtkCemBatchDesc* desc_dev, const CtkCemBatchStep* cur_dev, CtkCemBatchStep* next_dev,
                                        const void* kplant_dev, const CtkPlantNoise* noise_dev, const float* u_in_dev, const float* s_true_dev,
                                        size_t s_true_stride, const float* u_last_dev, size_t u_last_stride, uint32_t t, float* states_out,
                                        float* obs_out, float* inputs_out, float* costs_out, int n_records, size_t state_stride,
                                        size_t input_stride, size_t cost_stride);
hipError_t ctk_launch_batch_plant_noisy(hipStream_t st, int env, const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* cur_dev, CtkRpgdBatchStep* next_dev,
                                        const void* kplant_dev, const CtkPlantNoise* noise_dev, const float* u_in_dev, const float* s_true_dev,
                                        size_t s_true_stride, const float* u_last_dev, size_t u_last_stride, uint32_t t, float* states_out,
                                        float* obs_out, float* inputs_out, float* costs_out, int n_records, size_t state_stride,
                                        size_t input_stride, size_t cost_stride);
hipError_t ctk_launch_mppi_merge_partial(hipStream_t st, const float* parts, int n_parts, int per_block, int P,
                                         float neg_inv_lbd, float* out_rec);
// direct peer-to-peer record exchange + merge + update (ctk_mppi.hip: ctk_mppi_p2p_exchange)
constexpr int CTK_P2P_MAX_WORLD = 16;
size_t ctk_p2p_buffer_floats(int world, int P);
size_t ctk_p2p_args_bytes();   // sizeof the device-resident exchange description
// fills `dst` (host memory, ctk_p2p_args_bytes()) for upload
void ctk_p2p_fill_args(void* dst, float* const* bufs, int rank, int world, int P, uint32_t* err_host, double timeout_s);
bool ctk_p2p_can_fuse(int P, int world, int blocks);   // the rollout launch's LDS can stage `world` records too
hipError_t ctk_launch_mppi_p2p_exchange(hipStream_t st, float* const* bufs, int rank, int world, int P, uint32_t p2p_seq,
                                        uint32_t* err_host, double timeout_s, float neg_inv_lbd, int H, const InterpEntry* interp,
                                        const float* u_nom_in, float* u_nom_out, float lo, float hi, float* u_dev, float* u_host,
                                        uint32_t seq);
hipError_t ctk_launch_mppi_update(hipStream_t st, const float* parts, int n_parts, int P, float neg_inv_lbd, int H,
                                  const InterpEntry* interp, const float* u_nom_in, float* u_nom_out, float lo, float hi,
                                  float* u_dev, float* u_host, uint32_t seq);

// up to four device-to-device copies in ONE launch (the step log, ctk_api.hip:log_step); n_i floats each, n_i == 0 skips
struct CopyJob { const float* src; float* dst; unsigned n; };
hipError_t ctk_launch_copy4(hipStream_t st, const CopyJob (&jobs)[4]);

// ---- ctk_sampled.hip : u[n,h] = clip(base[h] + sample[n,h] * scale[h]) rollouts, selection ----
const char* ctk_affine_rollout_name(int pred, bool log);
size_t ctk_affine_rollout_lds(int H, int pred = 0);
// GRU: hidden <- cell(hidden, [s, u]) for the carried state behind the weight table (ctk_gru.h); u_dev NULL: u_val
hipError_t ctk_launch_gru_advance(hipStream_t st, const float* s, const float* u_dev, float u_val, float* wperm);
// samples [N,H] (device) or nullptr (Philox, rng_kind 0 normal / 1 uniform); base/scale [H] device.
// bst (ODE predictor only, <= CTK_AFFINE_BEST_MAX_BLOCKS workgroups): in-launch arg-min — block 0 picks the cheapest
// rollout under (J, index), writes its index to idx_out[0] and publishes its first input {u, seq}
struct AffineBest { unsigned long long* ll; uint32_t seq; float* u_dev; float* u_host; int* idx_out; };
constexpr int CTK_AFFINE_BEST_MAX_BLOCKS = 128;
int ctk_affine_rollout_blocks(int pred, int N);
hipError_t ctk_launch_affine_rollout(hipStream_t st, int pred, const RolloutArgs& a, const EnvK& k, const float* samples,
                                     int rng_kind, const float* base, const float* scale, const float* wperm, bool log,
                                     hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const AffineBest* bst = nullptr);
// the 4-wave kernel for any environment's analytic predictor (constants derived from `params`; bst: 2 + C words per workgroup)
hipError_t ctk_launch_affine_rollout_env(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a,
                                         const float* samples, int rng_kind, const float* base, const float* scale, bool log,
                                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const AffineBest* bst = nullptr);
size_t ctk_affine_rollout_env_lds(int env, int H);
const char* ctk_affine_rollout_env_name(int env, bool log);
// Smallest-K selection under the total order (J, index) and CEM refit
// (optimizer_cem_tf.py:73-78): idx_out[K] ascending, mu/std [H] from Q[idx].
hipError_t ctk_launch_select_topk(hipStream_t st, const float* J, int N, int K, int* idx_out, int ldj = 1);
hipError_t ctk_launch_cem_refit(hipStream_t st, const float* Q, const int* idx, int K, int H, float* mu, float* sd, int ldq);
// plans of one CEM-with-gradient iteration: Q[n,h] = clip(mu[h] + eps[n,h] * std[h]) (optimizer_cem_naive_grad_tf.py:60-62)
hipError_t ctk_launch_sample_plans(hipStream_t st, const RolloutArgs& a, const float* samples, const float* mu, const float* sd, float* Q);
hipError_t ctk_launch_cem_build_population(hipStream_t st, const RolloutArgs& a, int K, int first, const float* Q_prev, const int* idx,
                                           const float* eps_elite, const float* eps_rest, const float* mu, const float* sd, float* Q);
// this shard's best-K records {J, global index, Q[H]} for the sharded selection
hipError_t ctk_launch_pack_candidates(hipStream_t st, const float* J, const float* Q, const int* idx, int K, int H, int global_offset,
                                      float* cand);
// ---- ctk_gmm.hip: CEM with a two-component mixture (optimizer_cem_gmm_tf.py) -------------------
// mix = mu[2][HC] | std[2][HC] | probs[2] (one allocation); label [K] fp32 0/1 (entries 0 and 1 are the seeds)
// plans Q[n] = clip(mu_k + z[n] * std_k), k = 0 iff uniform[n] < probs[0]; normals == nullptr: Philox (normals on a.stream_id,
// the uniform of row n = word 0 of block (row, 0, call, ustream))
constexpr uint32_t CTK_GMM_UNIFORM_STREAM = 0x40000000u;   // + outer iteration
hipError_t ctk_launch_gmm_sample_plans(hipStream_t st, const RolloutArgs& a, const float* normals, const float* uniforms, const float* mix,
                                       uint32_t ustream, float* Q);
// sampling INSIDE the rollout (ctk_sampled.hip: ctk_affine_rollout_mix<ENV, TRAJ>, analytic predictor of any environment): both components'
// tables staged in LDS, picked per row — no plan pass and no extra launch; same draws and the same arithmetic as the pair above
const char* ctk_affine_rollout_mix_name(int env, bool log);
size_t ctk_affine_rollout_mix_lds(int env, int H);
hipError_t ctk_launch_affine_rollout_mix(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a,
                                         const float* normals, const float* uniforms, const float* mix, uint32_t ustream, bool log,
                                         hipEvent_t e0, hipEvent_t e1);
// labels + per-cluster mean / clipped population std + probs: ONE launch while the K labels and the two seed plans fit the refit's
// LDS budget (every workgroup recomputes the labels), a label launch + a refit launch beyond
constexpr int CTK_GMM_LDS_MAX_FLOATS = 12 * 1024;   // K + 2*HC floats of dynamic LDS (48 KiB) beside the kernel's static words
bool ctk_gmm_refit_one_launch(int K, int HC);
// two_launches: take the label launch + refit launch form whatever K is (diagnostic switch CTK_GMM_TWO_LAUNCH, bit for bit the same results)
hipError_t ctk_launch_gmm_refit(hipStream_t st, const float* Q, const int* idx, int K, int HC, float* mix, float* label, float std_min,
                                float std_max, int ldq, bool two_launches = false);
// shift mu / std one step repeating the last row; u = Q[idx[0]][0, :]
hipError_t ctk_launch_gmm_finish(hipStream_t st, const float* Q, const int* idx, int HC, int C, float* mix, float* u_dev, float* u_host,
                                 uint32_t seq, int ldq);

// ---- ctk_cem_fused.hip : one CEM step (all outer iterations) in ONE launch, CartPole ODE ---------
constexpr int CTK_CEM_FUSED_MAX_BLOCKS = 128;     // workgroups of 64 rollouts, all co-resident (one per CU)
struct CemFusedLaunch {
    int its, K;                   // outer iterations of this step (optimizer_cem_tf.py:92), cem_best_k
    unsigned long long* ll;       // ctk_cem_fused_ll_words(N, H) hand-off words, zero at allocation
    uint32_t tag0;                // tags tag0 .. tag0 + its - 1: consecutive across launches
    float std_min, std_max, init_std;
    float* mu; float* sd;         // [H*C] the handle's distribution, in / out
    float* u_dev; float* u_host; int* idx_out; uint32_t seq;
    double timeout_s;             // wall-clock bound of every in-launch wait
};
// H: flat columns of a plan (mpc_horizon * control inputs)
bool ctk_cem_fusable(int pred, int N, int H);
size_t ctk_cem_fused_ll_words(int N, int H);
const char* ctk_cem_fused_name(int env, bool log);
// a.H steps, a.C inputs with their limits; constants derived from the environment's parameter table `params`
hipError_t ctk_launch_cem_fused(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const float* samples,
                                const CemFusedLaunch& c, bool log, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// the BATCH form of the same step (ctk_cem_fused.hip: ctk_cem_batch<ENV, TRAJ>; include/ctk_hip.h: ctk_cem_batch_*): B independent problems of
// ONE configuration, grid (workgroups per problem, problems of this launch).  As for ctk_mppi_batch, what differs per problem reaches the
// kernel through two arrays in device memory: the descriptor [B] (the problem's buffers; written once, at creation) and the step records
// [problems of this step] (written by the host into pinned memory, ONE transfer ahead of the launches).
struct CtkCemBatchDesc {
    unsigned long long* ll;             // ctk_cem_fused_ll_words(N, H*C) hand-off words of THIS problem, zero at allocation
    float* mu; float* sd;               // [H*C] the problem's distribution, in / out
    float* J;                           // [N]
    float* Q_out;                       // [N,H,C]
    float* traj_out;                    // [N,H+1,S] or nullptr
    float* u_dev;                       // [C] the problem's own last output
    float* u_host;                      // pinned {u, seq} slot (16 floats) with the error words behind it
    int* idx_out;                       // [N] idx_out[0] = the cheapest row (BEST_IDX is materialised on demand)
    uint32_t seed_lo, seed_hi;          // Philox key
};
struct CtkCemBatchStep {
    int32_t id;                         // problem index = descriptor index
    uint32_t seq;                       // published with u
    uint32_t call;                      // Philox position
    uint32_t tag0;                      // hand-off tags tag0 .. tag0 + its - 1 (per problem: consecutive across its steps, never 0)
    int32_t its;                        // outer iterations of THIS problem's step (warm-up or cem_outer_it)
    uint32_t dev_uprev;                 // 1: the previous input is the problem's own last output (u_prev == NULL at the API)
    const float* samples;               // this problem's draws [its,N,H,C] (device pointer) or nullptr: the in-kernel sampler
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
};
static_assert(sizeof(CtkCemBatchStep) % 16 == 0, "the per-problem constants lie behind the step records, 16-aligned");
// per_problem: the form whose constants come from device memory (ctk_cem_batch_pp<ENV, TRAJ>), one element per step record
const char* ctk_cem_batch_name(int env, bool log, bool per_problem = false);
// c: K, the std constants and timeout_s only (its / tag0 / seq and the pointers are the records' and descriptors'); a: the shared template.
// k_steps_dev == nullptr: ctk_cem_batch, every problem with the constants of `params`; else ctk_cem_batch_pp, record j of steps_dev with
// element j of k_steps_dev (stride ctk_mppi_batch_k_stride(env), filled by ctk_mppi_batch_derive_k; `params` unused)
hipError_t ctk_launch_cem_batch(hipStream_t st, int env, const float* params, float dt, int isteps, const RolloutArgs& a, const CemFusedLaunch& c,
                                const CtkCemBatchDesc* desc_dev, const CtkCemBatchStep* steps_dev, int n_problems, bool log,
                                const void* k_steps_dev = nullptr);
// The form with per-problem hyper-parameters and limits (include/ctk_hip_family_hyper.h; ctk_cem_batch_hp<ENV, TRAJ>).  Behind the step
// records lies one two-part element per record, in record order, [K (ctk_mppi_batch_k_stride bytes) | hyper block] at stride
// ctk_cem_batch_kh_stride(env): the block (cem_best_k, the two deviations, the middle and the limits of every input) stands in place
// of c.K, c.std_min, c.init_std and a's limits.  ctk_cem_batch_fill_hyper writes a block; the middle is the launcher's 0.5f * (lo + hi).
size_t ctk_cem_batch_hyper_bytes();
size_t ctk_cem_batch_kh_stride(int env);
void ctk_cem_batch_fill_hyper(void* dst, int K, float std_min, float init_std, const float* lo, const float* hi, int C);
const char* ctk_cem_batch_hp_name(int env, bool log);
// c: timeout_s only; kh_steps_dev: element j belongs to record j of steps_dev
hipError_t ctk_launch_cem_batch_hp(hipStream_t st, int env, const RolloutArgs& a, const CemFusedLaunch& c, const CtkCemBatchDesc* desc_dev,
                                   const CtkCemBatchStep* steps_dev, int n_problems, bool log, const void* kh_steps_dev);
int ctk_cem_fused_blocks(int N);        // workgroups of a problem (64 rollouts each)
size_t ctk_cem_fused_lds(int N, int H); // dynamic LDS of a launch, bytes

// ---- ctk_rpgd.hip ---------------------------------------------------------------------------
const char* ctk_rpgd_descent_name(int pred, int N, int H = 0);
bool ctk_rpgd_uses_persistent(int pred, int N, int H);   // the whole descent as one launch: producers + resident Jacobian workers
// host-side state of the persistent form, per handle (the launcher advances both): sequence numbers of the in-launch hand-off
// (64 per launch) and the base of the workers' ticket counter, which lives in the handle's scratch and only ever counts up
struct RpgdPersist { uint32_t seq0, ticket_base; uint32_t* err_word; };
constexpr int CTK_RPGD_WIDE_MAX_N = 4096;
bool ctk_rpgd_uses_wide(int pred, int N);
int ctk_rpgd_fused_max_n(int pred, int N);   // one-launch step (keep-k / warm start as the descent's tail) up to this population   // MLP, small populations: phase launches + grid-wide step Jacobians (ctk_rpgd.hip)
size_t ctk_rpgd_descent_lds(int pred, int H, bool* tape_in_lds);
size_t ctk_rpgd_scratch_floats(int pred, int N, int H);
// All `iters` clipped-gradient Adam iterations + the final cost pass; bc_table[2*(t-1)] = 1-b1^t, [..+1] = 1-b2^t
// Single-workgroup step (N <= 64): keep-k selection + warm start as the tail of the descent launch (ctk_rpgd.hip: FusedWarm).
// Q/m/v of the descent are the old population; the rest describes the new one (arguments of ctk_launch_rpgd_warmstart).
struct RpgdFusedWarm {
    int K; int* idx_out;
    int P, n_new, gather, shift_previous, sampling_distribution, fresh_tail;
    int whole_space;      // sample_whole_control_space: uniform draws span the per-input limits (optimizer_rpgd.py:200-203)
    float sample_stdev, sample_mean, sample_min, sample_max;
    const float* draws; const float* ages_old;
    float* Q_new; float* m_new; float* v_new; float* ages_new;
    const InterpEntry* interp; float* u_nom; float* u_dev; float* u_host; uint32_t seq;
};
constexpr int CTK_RPGD_FUSED_MAX_N = 64;
hipError_t ctk_launch_rpgd_descent(hipStream_t st, int pred, const RolloutArgs& a, const EnvK& k, float lr, float b1, float b2,
                                   float eps, float clip, float* Q, float* m, float* v, const float* bc_table, int bc_len,
                                   int t0, int iters, const float* wperm, float* scratch, hipEvent_t ev_start = nullptr,
                                   hipEvent_t ev_stop = nullptr, int rule = 0, const RpgdFusedWarm* fused = nullptr,
                                   RpgdPersist* pers = nullptr);
// a.C control inputs, a.lo / a.hi the per-input limits; whole_space: uniform samples span [lo[c], hi[c]] (sample_whole_control_space)
hipError_t ctk_launch_rpgd_warmstart(hipStream_t st, const RolloutArgs& a, int N, int H, int P, int n_new, int gather, int shift_previous,
                                     int sampling_distribution, int reset, int whole_space, float sample_stdev,
                                     float sample_mean, float sample_min, float sample_max, const float* draws, const int* idx,
                                     const float* Q_old, const float* m_old, const float* v_old, const float* ages_old,
                                     float* Q_new, float* m_new, float* v_new, float* ages_new, const InterpEntry* interp,
                                     float* u_nom, float* u_dev, float* u_host, uint32_t seq, const float* recs = nullptr,
                                     int rs = 0, int keeper_base = 0, int fresh_tail = 0);
// the BATCH form of the RPGD step (ctk_generic.hip: ctk_g_rpgd_batch<ENV>; include/ctk_hip.h: ctk_rpgd_batch_*): B independent problems of ONE
// configuration with at most CTK_RPGD_FUSED_MAX_N plans each, one workgroup per problem, grid (1, problems of this launch).  As for
// ctk_mppi_batch and ctk_cem_batch, what differs per problem reaches the kernel through two arrays in device memory, both read-only to
// it: the descriptor [B] (the problem's buffers; written once, at creation) and the step records [problems of this step] (written by
// the host into pinned memory, ONE transfer ahead of the launches).  blockIdx.y picks the step record, its id the descriptor.
struct CtkRpgdBatchDesc {
    float* pop[2]; float* m[2]; float* v[2];   // [N,H,C] population and Adam moments, ping-pong
    float* ages[2];                     // [N]
    float* J;                           // [N]
    int* idx;                           // [N] idx[0 .. keep_k) = the keepers, ascending cost (BEST_IDX)
    float* u_nom;                       // [H,C] the best plan before the warm start
    float* u_dev;                       // [C] the problem's own last output
    float* u_host;                      // pinned {u, seq} slot (16 floats)
    float* scratch;                     // [H * NT * 64] the state tape when it does not fit in LDS
    uint32_t seed_lo, seed_hi;          // Philox key
};
struct CtkRpgdBatchStep {
    int32_t id;                         // problem index = descriptor index
    uint32_t seq;                       // published with u
    uint32_t call;                      // Philox position
    uint32_t cur;                       // which buffer holds the current population (the warm start writes the other one; a reset this one)
    int32_t iters;                      // Adam iterations of THIS problem's step (warm-up or outer_its)
    int32_t t0;                         // Adam steps the problem has taken (bias correction)
    int32_t resample;                   // 1: keep the best keep_k plans and draw N - keep_k fresh ones (count % resamp_per == 0)
    uint32_t dev_uprev;                 // 1: the previous input is the problem's own last output (u_prev == NULL at the API)
    const float* draws;                 // this problem's draws [N - keep_k, P, C] (reset: [N, P, C]; device pointer) or nullptr: Philox
    uint64_t pad;
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
};
static_assert(sizeof(CtkRpgdBatchStep) % 16 == 0, "step records are copied and indexed as an array; the per-problem constants lie behind them, 16-aligned");
// ctk_rpgd.hip: the warm start with reset = 1 (sample_actions of every plan, moments and ages 0) of n_problems records in ONE launch,
// grid (blocks, problems); f: P, the sampling constants and interp only; the records' id / call / cur / draws are read
hipError_t ctk_launch_rpgd_batch_reset(hipStream_t st, const RolloutArgs& a, const RpgdFusedWarm& f, const CtkRpgdBatchDesc* desc_dev,
                                       const CtkRpgdBatchStep* steps_dev, int n_problems);
hipError_t ctk_launch_rpgd_pack_keepers(hipStream_t st, const float* J, const float* Q, const float* m, const float* v,
                                        const float* ages, const int* idx, int K, int H, int global_offset, float* out);

// ---- ctk_generic.hip : environment-agnostic template kernels (ctk_env.h) ------------------------------------
constexpr int CTK_G_MODE_MPPI = 0, CTK_G_MODE_AFFINE = 1;
size_t ctk_g_rollout_lds(int cols, int H, int C);
int ctk_g_rollout_blocks(int N);                 // 64 trajectories per workgroup = block records of one MPPI launch
const char* ctk_g_rollout_name(int env, int mode, bool log);
// a.P = inducing points (MPPI) — the launcher turns it into sample columns per row (P*C or H*C); params = the handle's
// primary parameters of `env` (derived constants are formed per launch on the host, double -> fp32 once)
hipError_t ctk_launch_g_rollout(hipStream_t st, int env, int mode, const RolloutArgs& a, const float* params, float dt, int isteps,
                                const MppiK& mk, const float* samples, const float* base, const float* scale, int rng_kind,
                                float* parts, bool log, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
int ctk_g_mppi_update_max_parts();   // records the update launch merges itself
hipError_t ctk_launch_g_mppi_update(hipStream_t st, const float* parts, int n_parts, float neg_inv_lbd, int P, int C, int H,
                                    const InterpEntry* interp, const float* u_nom_in, float* u_nom_out, const RolloutArgs& a, float* u_dev,
                                    float* u_host, uint32_t seq);
// CEM post-loop (optimizer_cem_tf.py:99-102: clip std, shift by one step, refill the tail) and u = first input of the best elite,
// or of the mean with the stdev clipped to [min, std_max] (optimizer_cem_naive_grad_tf.py:101-104); every environment, CartPole: C = 1
hipError_t ctk_launch_g_cem_finish(hipStream_t st, const float* Q, const int* idx, int H, int C, float* mu, float* sd, float std_min,
                                   float init_std, const RolloutArgs& a, float* u_dev, float* u_host, uint32_t seq, int ldq,
                                   float std_max = 1.0e8f, int u_from_mu = 0);
// random-action: u = Q[argmin J, 0, :]  (optimizer_random_action_tf.py:65-68)
hipError_t ctk_launch_g_pick_best_first(hipStream_t st, const float* Q, const int* idx, int C, float* u_dev, float* u_host, uint32_t seq,
                                        int ldq);
size_t ctk_g_rpgd_descent_lds(int env, int H, bool* tape_in_lds);
size_t ctk_g_rpgd_scratch_floats(int env, int N, int H);
const char* ctk_g_rpgd_descent_name(int env);
hipError_t ctk_launch_g_rpgd_descent(hipStream_t st, int env, const RolloutArgs& a, const float* params, float dt, int isteps, float lr,
                                     float b1, float b2, float eps, float clip, float* Q, float* m, float* v, const float* bc_table,
                                     int bc_len, int t0, int iters, float* scratch, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr,
                                     int rule = 0);
// n_problems step records from `steps_dev` on as ONE launch of ctk_g_rpgd_batch<env>: descent, keep-k selection and warm start of every
// problem.  a: the shared template (limits, sizes; s0 / u_prev / J / seed / call come from the records and descriptors); f: keep_k, P,
// shift_previous, the sampling constants and interp (its pointers, n_new and gather are the records' and descriptors').
// k_steps_dev == nullptr: ctk_g_rpgd_batch, every problem with the constants of `params`; else the per-problem form ctk_g_rpgd_batch_pp<env>,
// record j of steps_dev with element j of k_steps_dev (stride ctk_mppi_batch_k_stride(env), filled by ctk_mppi_batch_derive_k; `params` unused)
const char* ctk_g_rpgd_batch_name(int env, bool per_problem = false);
hipError_t ctk_launch_g_rpgd_batch(hipStream_t st, int env, const RolloutArgs& a, const float* params, float dt, int isteps, float lr,
                                   float b1, float b2, float eps, float clip, int rule, const float* bc_table, int bc_len,
                                   const RpgdFusedWarm& f, const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* steps_dev, int n_problems,
                                   const void* k_steps_dev = nullptr);
// The form with per-problem hyper-parameters and limits (include/ctk_hip_family_hyper.h; ctk_g_rpgd_batch_hp<ENV>).  Behind the step
// records lies one two-part element per record, in record order, [K (ctk_mppi_batch_k_stride bytes) | hyper block] at stride
// ctk_rpgd_batch_kh_stride(env): the block (the Adam constants, formed by the function behind every launch's; the device address of the
// bias-correction table of the problem's betas; the four sampling constants; the limits) stands in place of lr .. clip, bc_table, f's
// sampling constants and a's limits.  ctk_rpgd_batch_fill_hyper writes a block.
size_t ctk_rpgd_batch_hyper_bytes();
size_t ctk_rpgd_batch_kh_stride(int env);
void ctk_rpgd_batch_fill_hyper(void* dst, float lr, float b1, float b2, float eps, float clip, int rule, const float* bc_table_dev,
                               float sample_stdev, float sample_mean, float sample_min, float sample_max, const float* lo, const float* hi, int C);
const char* ctk_g_rpgd_batch_hp_name(int env);
hipError_t ctk_launch_g_rpgd_batch_hp(hipStream_t st, int env, const RolloutArgs& a, int bc_len, const RpgdFusedWarm& f,
                                      const CtkRpgdBatchDesc* desc_dev, const CtkRpgdBatchStep* steps_dev, int n_problems,
                                      const void* kh_steps_dev);

// ---- ctk_generic_net.hip : the template kernels with a network predictor (net = CTK_PRED_MLP | CTK_PRED_GRU; ctk_net.h) -----
// wperm: the policy's per-lane operand tables (forward | reverse), followed by the GRU's carried hidden state [64]
size_t ctk_g_net_table_floats(int net);
size_t ctk_g_net_hidden_floats(int net);
const char* ctk_g_rollout_net_name(int env, int net, int mode, bool log, int N, int P, int H);
int ctk_g_rollout_net_cols(int env, int mode, int P, int H);
int ctk_g_rollout_net_blocks(int env, int net, int mode, int N, int P, int H);   // workgroups = block records of one MPPI launch
size_t ctk_g_rollout_net_lds(int env, int net, int N, int cols, int H, int C);
hipError_t ctk_launch_g_rollout_net(hipStream_t st, int env, int net, int mode, const RolloutArgs& a, const float* params, float dt, int isteps,
                                    const MppiK& mk, const float* samples, const float* base, const float* scale, int rng_kind,
                                    const float* wperm, float* parts, bool log, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr,
                                    const MppiFuse* fuse = nullptr);   // MPPI mode: the in-launch hand-off (modes 1, 2) when it fits
size_t ctk_g_rpgd_descent_net_lds(int env, int net, int N, int H);
size_t ctk_g_rpgd_scratch_floats_net(int net, int N, int H);
const char* ctk_g_rpgd_descent_net_name(int env, int net, int N, int H);
// ctk_net_split.hip: the network predictors with one 16-trajectory tile spread over several waves of a workgroup (GRU: four, forward and
// BPTT; MLP: two), for the populations that leave SIMDs idle with one wave per tile
struct AdamK;
bool ctk_g_rpgd_split_ok(int env, int net, int N, int H);
size_t ctk_g_rpgd_descent_split_lds(int net, int H, int C);
size_t ctk_g_rpgd_scratch_floats_split(int net, int N, int H);
const char* ctk_g_rpgd_descent_split_name(int env, int net);
hipError_t ctk_launch_g_rpgd_descent_split(hipStream_t st, int env, int net, const RolloutArgs& a, const float* params, float dt, int isteps,
                                           const AdamK& ad, float* Q, float* m, float* v, const float* bc_table, int bc_len, int t0, int iters,
                                           const float* wperm, const float* wperm_bwd, const float* hidden, float* scratch,
                                           hipEvent_t e0, hipEvent_t e1);
bool ctk_g_rpgd_wide_ok(int env, int net, int N, int H);          // the MLP descent as phase + Jacobian launches (N <= 4 096)
size_t ctk_g_rpgd_scratch_floats_wide(int N, int H);
const char* ctk_g_rpgd_wide_name(int env, int N = 0, int H = 0);
hipError_t ctk_launch_g_rpgd_wide_split(hipStream_t st, int env, const RolloutArgs& a, const float* params, float dt, int isteps, const AdamK& ad,
                                        float* Q, float* m, float* v, const float* bc_table, int bc_len, int t0, int iters, const float* wperm,
                                        float* scratch, hipEvent_t e0, hipEvent_t e1, uint32_t* err_word, RpgdPersist* pers = nullptr);
bool ctk_g_rpgd_persist64_ok(int env, int N, int H);          // ... and of the 64-unit network's (no phase-launch form exists for that width)
const char* ctk_g_rpgd_persist64_name(int env);
hipError_t ctk_launch_g_rpgd_persist64(hipStream_t st, int env, const RolloutArgs& a, const float* params, float dt, int isteps, const AdamK& ad,
                                       float* Q, float* m, float* v, const float* bc_table, int bc_len, int t0, int iters, const float* wperm,
                                       float* scratch, hipEvent_t e0, hipEvent_t e1, uint32_t* err_word, RpgdPersist* pers);
bool ctk_g_rpgd_persist_ok(int env, int net, int N, int H);   // the wide form as one launch per MPC step (ctk_g_rpgd_persist)
bool ctk_g_rollout_split_ok(int env, int net, int N, int H, int cols);
size_t ctk_g_rollout_split_lds(int net, int cols, int H, int C);
int ctk_g_rollout_split_blocks(int N);
const char* ctk_g_rollout_split_name(int env, int net, int mode, bool log, int N, int H, int cols);
hipError_t ctk_launch_g_rollout_split(hipStream_t st, int env, int net, int mode, const RolloutArgs& a, const float* params, float dt, int isteps,
                                      const MppiK& mk, const float* samples, const float* base, const float* scale, int rng_kind,
                                      const float* wperm, const float* hidden, float* parts, bool log, hipEvent_t e0, hipEvent_t e1,
                                      const MppiFuse* fuse = nullptr);
hipError_t ctk_launch_g_gru_advance4(hipStream_t st, int env, const RolloutArgs& a, const float* u_dev, const float* wperm, float* hidden);
bool ctk_g_rollout_net_fusable(int env, int net, int N, int P, int H);   // may an MPPI step with this network predictor run as ONE launch?
size_t ctk_g_rpgd_descent_gru4_lds(int H, int C);
size_t ctk_g_rpgd_scratch_floats_gru4(int N, int H);
const char* ctk_g_rpgd_descent_gru4_name(int env);
hipError_t ctk_launch_g_rpgd_descent_gru4(hipStream_t st, int env, const RolloutArgs& a, const float* params, float dt, int isteps,
                                          const AdamK& ad, float* Q, float* m, float* v, const float* bc_table, int bc_len, int t0, int iters,
                                          const float* wperm, const float* wperm_bwd, const float* hidden, float* scratch,
                                          hipEvent_t e0, hipEvent_t e1);
hipError_t ctk_launch_g_rpgd_descent_net(hipStream_t st, int env, int net, const RolloutArgs& a, const float* params, float dt, int isteps,
                                         float lr, float b1, float b2, float eps, float clip, float* Q, float* m, float* v,
                                         const float* bc_table, int bc_len, int t0, int iters, const float* wperm, float* scratch,
                                         hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, int rule = 0, uint32_t* err_word = nullptr,
                                         RpgdPersist* pers = nullptr);
// predictor.update(s, Q0) for the GRU under the template kernels: a.s0 = measured state, a.u_prev = applied input (u_dev overrides)
hipError_t ctk_launch_g_gru_advance(hipStream_t st, int env, const RolloutArgs& a, const float* u_dev, float* wperm);

// ---- ctk_batch_rollout.hip : caller-supplied plans rolled out per problem in ONE launch (include/ctk_hip_rollout.h: *_batch_rollout) ----
// predictor.predict_core + get_trajectory_cost of M plans for every listed problem of a batch, whatever the batch's optimizer: grid
// (workgroups of M rows, records).  Two kernels, because a handle's ctk_rollout launches one of two that sum the cost in different
// orders: ctk_batch_rollout<ENV, PRED, WTRAJ> wraps affine_rollout_body (ctk_affine_body.h; what a CartPole handle with
// generic_kernels == 0 launches: ODE, MLP, GRU), ctk_g_batch_rollout<ENV, WTRAJ> the affine mode of ctk_g_rollout (ctk_g_rollout_body.inc;
// every other handle).  Base 0, scale 1 and infinite limits: the plans are taken as given.  No flag, no wait, no atomics.
constexpr int CTK_G_TRAJ = 64;          // trajectories per workgroup of the template rollout kernels (ctk_generic.hip: G_TRAJ)
struct CtkBatchRolloutRec {             // one per listed problem, blockIdx.y
    int32_t id;                         // problem index: selects the network weights / hidden state
    int32_t m;                          // plans of this record (the same M for all records of a call)
    int32_t kidx;                       // element of the constants array: 0 (shared form), the record's index (per-problem form: the
                                        // constants lie behind the records) or the problem's index (model = plant: the plant table)
    uint32_t pad;
    const float* plans;                 // [M,H,C] device pointer: the uploaded plans, or the problem's own current plan (M = 1)
    float* J;                           // [M]
    float* traj;                        // [M,H+1,S] or nullptr
    float* Q_out;                       // [M,H,C] the body's copy of the plans (scratch)
    float s[CTK_MAX_STATES];
    float u_prev[CTK_MAX_INPUTS];
};
static_assert(sizeof(CtkBatchRolloutRec) % 16 == 0, "the per-problem constants and the plans lie behind the records, 16-aligned");
// generic: the batch's handles run the template kernels (any environment but CartPole, or cfg.generic_kernels); pred: CTK_PRED_* of the
// rollout (the plant model: CTK_PRED_ODE); a: the shared template (C, H, inv_Hp1, infinite limits); k_dev: constants at stride
// ctk_mppi_batch_k_stride(env), indexed by the records' kidx; zero_one_dev: [2][H*C] zeros | ones; w_dev / wstride: the per-problem
// network blocks of an MLP or GRU batch (floats), else nullptr / 0
const char* ctk_batch_rollout_name(int env, bool generic, int pred, bool traj);
int ctk_batch_rollout_blocks(bool generic, int pred, int M);
hipError_t ctk_launch_batch_rollout(hipStream_t st, int env, bool generic, int pred, const RolloutArgs& a, const CtkBatchRolloutRec* recs_dev,
                                    int n_records, int M, const void* k_dev, const float* zero_one_dev, const float* w_dev, size_t wstride,
                                    bool traj);
