// ctk_batch.hip — the batch families of the C ABI (include/ctk_hip.h, ctk_hip_run.h, ctk_hip_episode.h, ctk_hip_loop.h): ctk_batch_*, ctk_mlp_batch_*,
// ctk_gru_batch_*, ctk_cem_batch_*, ctk_rpgd_batch_*.  The single handle is in ctk_api.hip; what the two files share is declared in ctk_host.h.
// The file in order: the host core (BatchCore and the bodies every family shares), the two drivers — batch_step<F> for a step,
// batch_closed_loop<F> for runs and episodes —, batch_rollout<F> for rollouts of caller-supplied plans (include/ctk_hip_rollout.h) and the
// macros that write a family's C entries over them (CTK_BATCH_ENTRIES, CTK_LOOP_ENTRIES, CTK_ROLLOUT_ENTRY); then each family: its struct, its trait F (MppiFamily, MlpFamily, GruFamily, CemFamily, RpgdFamily: what the drivers ask of
// it), and the entries that are its own (create, samples_needed, step, reset, read).  A message names the entry that was called: every
// entry passes its exported name (`who`) to the body that builds the text, the MLP family included — it runs the MPPI family's code
// under its own names.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "ctk_launch.h"
#include "ctk_host.h"
#include "ctk_device.h"   // CTK_SINCOS_FAST_LIMIT

using namespace ctk_host;

// =============================================================================================
// The host core of the batch families (ctk_batch, ctk_cem_batch, ctk_rpgd_batch derive from it; ctk_mlp_batch is a ctk_batch): what
// every family keeps per batch and per problem, and the one copy of what they all do with it — the id checks, the owner of every device
// and pinned allocation, the staging of host draws, the step records' common fields, the completion poll, the read-out of u, the
// transfers of read / get_state / set_state, the parameter tables and the Philox positions.  Plain data and free functions, private to
// this file (ctk_batch.hip): a family's own entry points pass their name (`who`) for the messages.
// =============================================================================================
namespace {

// The closed loop on the device, what every family keeps for it (ctk_batch_run / ctk_batch_plant_step and their ctk_cem_batch_ /
// ctk_rpgd_batch_ forms; kernels ctk_batch_plant<ENV> ..., ctk_plant.hip).  Problem p's PLANT has, for parameter id, the override if one
// was set (*_plant_set_param), else the problem's own controller value table(p)[id]
struct PlantSide {
    std::vector<float> plant_over;          // [B][CTK_MAX_PARAMS] the overrides
    std::vector<unsigned char> plant_has;   // [B][CTK_MAX_PARAMS] an override was set
    std::vector<float> plant_tab;           // [B][CTK_MAX_PARAMS] the effective table the constants in h_kplant were derived from
    std::vector<int> plant_sub;             // [B] ... and their Euler sub-step count (0: nothing derived yet)
    unsigned char* h_kplant = nullptr;      // pinned [B][kstride] the plants' derived constants, the staging of the copy to d_kplant
    unsigned char* d_kplant = nullptr;      // [B][kstride]
    unsigned char* h_run = nullptr;         // pinned: the step records, plant operands and traces of one segment or plant step (LoopLayout)
    unsigned char* d_run = nullptr;         // the same on the device; both grow on demand (batch_run_buffers)
    size_t d_run_cap = 0, h_run_cap = 0;    // bytes
    int run_segment = 256;                  // steps per segment of a run: a diagnostic switch may lower it (batch_core_init)
    // the stochastic plant (include/ctk_hip_episode.h: ctk_batch_episodes / ctk_batch_plant_step_noisy; kernel ctk_batch_plant_noisy<ENV>)
    std::vector<float> noise_sigma;         // [B][2][CTK_MAX_STATES] process | measurement standard deviations (0: none)
    std::vector<uint64_t> noise_seed;       // [B] Philox key of the problem's noise (at creation: its controller seed)
    std::vector<uint32_t> noise_pos;        // [B] noise position: one per transition of the noisy plant
};

struct BatchCore : PlantSide {
    ctk_config cfg{};
    int B = 0, N = 0, H = 0, env = CTK_ENV_CARTPOLE, S = CTK_S, C = CTK_C, HC = 0;
    float params[CTK_MAX_PARAMS]{};         // the shared table: the last whole-batch value of every id (*_batch_set_param / get_param)
    std::vector<float> pparams;             // [B][CTK_MAX_PARAMS] every problem's own table
    std::vector<unsigned char> dirty;       // [B] the table changed since the problem's constants were last derived (MPPI: and copied to d_k)
    bool differ = false;                    // a *_problem_set_param has succeeded: the per-problem form of the kernel from now on
    size_t kstride = 0;                     // ctk_mppi_batch_k_stride(env): bytes of one problem's derived constants
    // the CEM and RPGD families' per-problem hyper-parameters and limits (include/ctk_hip_family_hyper.h; the MPPI families keep theirs in
    // ctk_batch): the table of primary values, initialised from cfg, and every problem's hyper block as the _hp form of the kernel
    // reads it, refreshed by the setters.  `fhyper` (sticky, as `differ`) once a setter has succeeded: the _hp form from then on, whose
    // records carry two-part elements [K | hyper block] (elem) in place of the _pp form's K
    std::vector<float> fhyp;                // [B][frow]: the family's enum values | low [CTK_MAX_INPUTS] | high [CTK_MAX_INPUTS]
    int fcount = 0, frow = 0;               // the family's CTK_*_HYPER_COUNT; fcount + 2 * CTK_MAX_INPUTS
    std::vector<unsigned char> hcache;      // [B][hbytes] hyper blocks by problem id (host only; the step copies them behind the K parts)
    size_t hbytes = 0;                      // ctk_cem_batch_hyper_bytes() / ctk_rpgd_batch_hyper_bytes()
    bool fhyper = false;
    bool carries() const { return differ || fhyper; }                         // the step records carry an element per record
    size_t elem() const { return kstride + (fhyper ? hbytes : 0); }           // ... of this many bytes
    float* frow_of(int p) { return fhyp.data() + (size_t)p * frow; }
    const float* frow_of(int p) const { return fhyp.data() + (size_t)p * frow; }
    float* flow(int p) { return frow_of(p) + fcount; }
    const float* flow(int p) const { return frow_of(p) + fcount; }
    float* fhigh(int p) { return frow_of(p) + fcount + CTK_MAX_INPUTS; }
    const float* fhigh(int p) const { return frow_of(p) + fcount + CTK_MAX_INPUTS; }
    hipStream_t stream = nullptr;
    float* d_u = nullptr;                   // [B][CTK_MAX_INPUTS]
    float* h_u = nullptr;                   // pinned [B][16]: {u, seq}, error words, u[C] (the layout of a handle's slot)
    float* h_u_dev = nullptr;
    float* d_samples = nullptr; size_t samples_cap = 0;   // staging for host-supplied draws
    float *d_J = nullptr, *d_Q = nullptr, *d_traj = nullptr;   // [B][N] | [B][N,H,C] | [B][N,H+1,S] (materialize_trajectories); RPGD has J alone
    float* d_zero_one = nullptr;            // [2][H,C] zeros | ones: base and scale of a rollout of given plans (batch_rollout; made at the first one)
    Owner own;                             // every device / pinned allocation of the batch, entered where it is made (ctk_host.h; batch_core_release)
    std::vector<uint32_t> seq, call;        // [B] the sequence number of the problem's next step, its Philox position
    std::string err, dominant;
    float* u(int p) const { return d_u + (size_t)p * CTK_MAX_INPUTS; }
    float* slot(int p) const { return h_u + (size_t)p * 16; }
    float* table(int p) { return pparams.data() + (size_t)p * CTK_MAX_PARAMS; }
    const float* table(int p) const { return pparams.data() + (size_t)p * CTK_MAX_PARAMS; }
    ~BatchCore();                           // batch_core_release: `delete` is every family's destroy and the end of a failed creation
};

int bfail(BatchCore* b, int code, const std::string& msg) {
    if (b) b->err = msg; else g_create_error = msg;
    return code;
}
#define BHIP_TRY(b, expr)                                                                       \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return bfail((b), CTK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

// a diagnostic switch of the environment that only lowers a limit (values from 1 up to the limit)
void batch_env_lowers(const char* name, int* limit) {
    const char* e = std::getenv(name);
    if (e && std::atoi(e) >= 1 && std::atoi(e) < *limit) *limit = std::atoi(e);
}
// the seed of problem p: the caller's, or consecutive ones from the configuration's
uint64_t batch_seed(const ctk_config* cfg, const uint64_t* seeds, int p) { return seeds ? seeds[p] : cfg->seed + (uint64_t)p; }

// the fields of the core that depend on the configuration alone (every family's create, after its refusals)
void batch_core_init(BatchCore* b, const ctk_config* cfg, const EnvInfo* einfo, int n_problems, const uint64_t* seeds) {
    b->cfg = *cfg;
    b->B = n_problems; b->N = cfg->num_rollouts; b->H = cfg->mpc_horizon;
    b->env = cfg->environment; b->S = einfo->S; b->C = einfo->C; b->HC = b->H * b->C;
    default_params(b->env, b->params);
    b->pparams.resize((size_t)n_problems * CTK_MAX_PARAMS);
    for (int p = 0; p < n_problems; ++p) std::memcpy(b->table(p), b->params, sizeof(b->params));
    b->dirty.assign((size_t)n_problems, 1);            // nothing derived yet: the per-problem form derives what it steps (MPPI: all of them)
    b->kstride = ctk_mppi_batch_k_stride(b->env);
    b->seq.assign((size_t)n_problems, 1u); b->call.assign((size_t)n_problems, 0u);
    // A long run goes in segments of this many steps, so that its record buffer stays bounded (256 steps of 128 problems: 2.5 MiB of
    // records).  CTK_BATCH_RUN_SEGMENT_STEPS (diagnostic) only lowers it; the results do not depend on it.
    batch_env_lowers("CTK_BATCH_RUN_SEGMENT_STEPS", &b->run_segment);
    b->plant_over.assign((size_t)n_problems * CTK_MAX_PARAMS, 0.0f);
    b->plant_has.assign((size_t)n_problems * CTK_MAX_PARAMS, 0);
    b->plant_tab.assign((size_t)n_problems * CTK_MAX_PARAMS, 0.0f);
    b->plant_sub.assign((size_t)n_problems, 0);
    b->noise_sigma.assign((size_t)n_problems * 2 * CTK_MAX_STATES, 0.0f);
    b->noise_seed.resize((size_t)n_problems);
    for (int p = 0; p < n_problems; ++p) b->noise_seed[(size_t)p] = batch_seed(cfg, seeds, p);   // the controller's
    b->noise_pos.assign((size_t)n_problems, 0u);
}

// everything a batch owns on the device and in pinned memory; no HIP call for a batch that was refused before it opened anything
void batch_core_release(BatchCore* b) {
    if (!b->stream && b->own.empty()) return;
    hipSetDevice(b->cfg.device);
    if (b->stream) hipStreamSynchronize(b->stream);
    b->own.release();
    if (b->stream) hipStreamDestroy(b->stream);
}
BatchCore::~BatchCore() { batch_core_release(this); }

// what every family's creation starts its device state with: the stream, u of every problem, the mapped result slots (HIP_CREATE and
// Creating<>, the creation macro and guard of ctk_host.h: a failure stores its text, and the batch is deleted on the way out)
int batch_core_open(BatchCore* b) {
    HIP_CREATE(hipSetDevice(b->cfg.device));
    HIP_CREATE(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    HIP_CREATE(b->own.dev_zero(&b->d_u, (size_t)b->B * CTK_MAX_INPUTS * sizeof(float), b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_u, (size_t)b->B * 64, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_CREATE(hipHostGetDevicePointer((void**)&b->h_u_dev, b->h_u, 0));
    HIP_CREATE(b->own.dev_zero(&b->d_kplant, (size_t)b->B * b->kstride, b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_kplant, (size_t)b->B * b->kstride));
    return CTK_OK;
}

// the problems a call addresses: ids[0..n) ascending without repeats, or all of them (ids == NULL)
int batch_ids(BatchCore* b, const char* who, int n_ids, const int32_t* ids, int* n_out) {
    if (!ids) { *n_out = b->B; return CTK_OK; }
    if (n_ids < 1 || n_ids > b->B) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": n_ids must be 1 .. " + std::to_string(b->B) + " (the batch size)");
    for (int j = 0; j < n_ids; ++j) {
        if (ids[j] < 0 || ids[j] >= b->B)
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": problem index " + std::to_string(ids[j]) + " is outside 0 .. " + std::to_string(b->B - 1));
        if (j > 0 && ids[j] <= ids[j - 1]) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": ids must be strictly ascending");
    }
    *n_out = n_ids;
    return CTK_OK;
}
int batch_problem(BatchCore* b, const char* who, int p) {
    if (p < 0 || p >= b->B) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": problem index " + std::to_string(p) + " is outside 0 .. " + std::to_string(b->B - 1));
    return CTK_OK;
}

// what every family's launches share of RolloutArgs (ctk_api.hip: make_args of a handle without what the step records and descriptors supply); P,
// p_magic, interp and identity_interp are the family's
RolloutArgs batch_common_args(const BatchCore* b) {
    RolloutArgs a{};
    for (int c = 0; c < b->C; ++c) { a.lo[c] = b->cfg.action_low[c]; a.hi[c] = b->cfg.action_high[c]; }
    a.C = b->C;
    a.N = b->N; a.H = b->H;
    a.inv_Hp1 = 1.0f / (float)(b->H + 1);
    a.stream_id = 0;
    a.global_row0 = b->cfg.global_rollout_offset;
    return a;
}

// host-supplied draws into the staging buffer (ctk_api.hip: resolve_samples of a handle): n floats
int batch_stage(BatchCore* b, const float* src, size_t n) {
    BHIP_TRY(b, b->own.grow_dev(b->d_samples, b->samples_cap, n));
    BHIP_TRY(b, hipMemcpyAsync(b->d_samples, src, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
    return CTK_OK;
}

// row j of the call's states and previous inputs into a step record: they travel with the records
template <class Rec>
void batch_record_io(const BatchCore* b, Rec& q, int j, const float* s, const float* u_prev) {
    q.dev_uprev = u_prev ? 0u : 1u;
    for (int i = 0; i < b->S; ++i) q.s[i] = s[(size_t)j * b->S + i];
    for (int c = 0; c < b->C; ++c) q.u_prev[c] = u_prev ? u_prev[(size_t)j * b->C + c] : 0.0f;
}

// The per-problem forms of the CEM and RPGD kernels take the constants by record index: those of the n listed problems into h_k, in
// listed order.  A problem whose table changed is re-derived here, when it is stepped, with the function a handle uses; kcache is by
// problem id.  In the _hp form (fhyper) an element has two parts, [K | hyper block], at stride elem(): the block is the problem's
// current one (hcache, which the setters refresh), and the K part is current even where no parameter was ever set (`dirty` starts set).
void batch_stage_constants(BatchCore* b, unsigned char* kcache, const int32_t* ids, int n, unsigned char* h_k) {
    const size_t stride = b->elem();
    for (int j = 0; j < n; ++j) {
        const size_t z = (size_t)(ids ? ids[j] : j);
        if (b->dirty[z]) {
            ctk_mppi_batch_derive_k(b->env, b->table((int)z), b->cfg.dt, b->cfg.intermediate_steps, kcache + z * b->kstride);
            b->dirty[z] = 0;
        }
        std::memcpy(h_k + (size_t)j * stride, kcache + z * b->kstride, b->kstride);
        if (b->fhyper) std::memcpy(h_k + (size_t)j * stride + b->kstride, b->hcache.data() + z * b->hbytes, b->hbytes);
    }
}

// The step records of the CEM and RPGD steps to the device, n of `rec` bytes each.  In the per-problem form the constants of the n
// problems lie right behind the n records, in the records' order, so that ONE transfer carries both (*d_ksteps: where they land, else
// NULL).  A problem whose table changed is re-derived here, when it is stepped, with the function a handle uses (ctk_set_param ->
// derive_constants / Env<>::derive at its launch); kcache is by problem id, the block behind the records by launch order.
hipError_t batch_send_records(BatchCore* b, unsigned char* kcache, const int32_t* ids, int n, size_t rec, void* h_steps, void* d_steps,
                              const unsigned char** d_ksteps) {
    size_t bytes = (size_t)n * rec;
    *d_ksteps = nullptr;
    if (b->carries()) {
        batch_stage_constants(b, kcache, ids, n, static_cast<unsigned char*>(h_steps) + bytes);
        *d_ksteps = static_cast<const unsigned char*>(d_steps) + bytes;
        bytes += (size_t)n * b->elem();
    }
    const hipError_t e = hipMemcpyAsync(d_steps, h_steps, bytes, hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess && b->carries())               // nothing reached the device: derive and copy again at the next step
        for (int j = 0; j < n; ++j) b->dirty[(size_t)(ids ? ids[j] : j)] = 1;
    return e;
}

// problem p onto a message's list of problems ("3, 7, 12")
void list_problem(std::string& list, int p) { list += (list.empty() ? "" : ", ") + std::to_string(p); }

// completion of a step: the {u, seq} store of each of the first `launched` listed problems landing in its pinned slot (ctk_api.hip: finish_step's
// bounded spin: one budget of pauses for the whole call, then one synchronise, then give up).  Returns the problems that never published.
std::string batch_poll(BatchCore* b, const int32_t* ids, int launched) {
    bool synced = false;
    int spins = 0;
    std::string late;
    for (int j = 0; j < launched; ++j) {
        const int p = ids ? ids[j] : j;
        const uint32_t want = b->seq[(size_t)p];
        volatile uint32_t* slot = reinterpret_cast<volatile uint32_t*>(b->slot(p)) + 1;
        while (*slot != want) {
            if (!synced && ++spins < 4000000) { __builtin_ia32_pause(); continue; }
            if (!synced) { synced = true; if (hipStreamSynchronize(b->stream) != hipSuccess) break; continue; }
            break;
        }
        if (*slot != want) list_problem(late, p);
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return late;
}

// u of problem p from its slot into row j of u_out (publish_u_vec: u[0] beside seq, the other inputs behind the error words)
void batch_read_u(const BatchCore* b, int p, int j, float* u_out) {
    if (!u_out) return;
    volatile float* sl = reinterpret_cast<volatile float*>(b->slot(p));
    u_out[(size_t)j * b->C] = sl[0];
    for (int c = 1; c < b->C; ++c) u_out[(size_t)j * b->C + c] = sl[4 + c];
}

// ---- the parameter tables and Philox positions: the bodies of every family's *_set_param ... *_rng_set_position ----
int batch_param_id(BatchCore* b, const char* who, int id) {
    if (id < 0 || id >= env_info(b->env)->n_params) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown parameter id for this environment");
    return CTK_OK;
}
int batch_set_param(BatchCore* b, const char* who, int id, float value) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (int rc = batch_param_id(b, who, id)) return rc;
    b->params[id] = value;                             // the shared table: the shared form derives its constants from it at each launch
    for (int p = 0; p < b->B; ++p) { b->table(p)[id] = value; b->dirty[(size_t)p] = 1; }   // column id of every problem; the other ids stay
    return CTK_OK;
}
int batch_get_param(const BatchCore* b, int id, float* value) {
    if (!b || !value || id < 0 || id >= env_info(b->env)->n_params) return CTK_ERR_INVALID_ARGUMENT;
    *value = b->params[id];
    return CTK_OK;
}
// the call that turns `differ` on names the family's per-problem kernel in `dominant` (F::per_problem_kernel)
template <class F>
int batch_problem_set_param(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, int id, const float* values) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (int rc = batch_param_id(b, who, id)) return rc;
    if (!values) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL values (one value per listed problem)");
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        b->table(p)[id] = values[j];
        b->dirty[(size_t)p] = 1;                       // derived at a later step (MPPI: the next one, CEM and RPGD: the problem's next one)
    }
    if (!b->differ) b->dominant = F::per_problem_kernel(b);
    b->differ = true;                                  // sticky: the tables are never compared again
    return CTK_OK;
}
int batch_problem_get_param(const BatchCore* b, int problem, int id, float* value) {
    if (!b || !value || problem < 0 || problem >= b->B || id < 0 || id >= env_info(b->env)->n_params) return CTK_ERR_INVALID_ARGUMENT;
    *value = b->table(problem)[id];
    return CTK_OK;
}
int batch_params_differ(const BatchCore* b) { return b && b->differ ? 1 : 0; }
int batch_rng_get_position(const BatchCore* b, int problem, uint32_t* call) {
    if (!b || !call || problem < 0 || problem >= b->B) return CTK_ERR_INVALID_ARGUMENT;
    *call = b->call[(size_t)problem];
    return CTK_OK;
}
int batch_rng_set_position(BatchCore* b, const char* who, int problem, uint32_t call) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (int rc = batch_problem(b, who, problem)) return rc;
    b->call[(size_t)problem] = call;
    return CTK_OK;
}

// ---- the transfers of every family's *_get_state / *_set_state and *_read ----
// A problem's state as a family describes it: the state list of ctk_host.h (segments on the device in the order of the state's layout,
// then — the batch families' case of that list — its host-side counters last).  `mark`: a flag that set_state raises (RPGD: the problem
// counts as reset).
struct BatchState { std::vector<StateItem> items; unsigned char* mark = nullptr; };

// get (device to host) or set (host to device) of a problem's state (F::state) through host[n]: the checks here, the transfers in
// state_walk.  F::state_size_named: the size messages name the size (RPGD's do)
template <class F>
int batch_state_io(typename F::Batch* b, const char* who, int problem, float* host, size_t n, bool get) {
    if (!b || !host) return CTK_ERR_INVALID_ARGUMENT;
    if (int rc = batch_problem(b, who, problem)) return rc;
    const BatchState st = F::state(b, problem);
    const size_t size = state_floats(st.items);
    if (get ? n < size : n != size)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + (get ? ": destination too small" : ": wrong state size") +
                     (F::state_size_named ? " (" + std::to_string(size) + " floats)" : std::string()));
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    BHIP_TRY(b, state_walk(st.items, host, get, b->stream));
    if (!get && st.mark) *st.mark = 1;
    return CTK_OK;
}

// what every *_read checks before the family resolves the buffer
int batch_read_check(BatchCore* b, const char* who, int problem, const float* dst) {
    if (!b || !dst) return b ? bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL destination") : CTK_ERR_INVALID_ARGUMENT;
    return batch_problem(b, who, problem);
}
// the Q / J / TRAJ cases of the MPPI and CEM families' reads; *src stays NULL for every other buffer
int batch_locate_rollouts(BatchCore* b, const char* who, int problem, int buffer, const float** src, size_t* n) {
    const size_t z = (size_t)problem, N = (size_t)b->N;
    switch (buffer) {
        case CTK_BUF_Q: *src = b->d_Q + z * N * b->HC; *n = N * b->HC; break;
        case CTK_BUF_J: *src = b->d_J + z * N; *n = N; break;
        case CTK_BUF_TRAJ:
            if (!b->d_traj) return bfail(b, CTK_ERR_STATE, std::string(who) + ": trajectories not materialised (cfg.materialize_trajectories == 0)");
            *n = N * ((size_t)b->H + 1) * b->S; *src = b->d_traj + z * *n; break;
        default: break;
    }
    return CTK_OK;
}
// the n floats (is_int: 32-bit indices, converted) at src into dst[cap]; `before_copy` runs between hipSetDevice and the copy
int batch_read_out(BatchCore* b, const char* who, const float* src, size_t n, bool is_int, float* dst, size_t cap,
                   const std::function<int()>& before_copy = nullptr) {
    if (cap < n) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": destination too small (" + std::to_string(n) + " floats)");
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    if (before_copy) if (int rc = before_copy()) return rc;
    BHIP_TRY(b, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    if (is_int) for (size_t i = 0; i < n; ++i) { int v; std::memcpy(&v, &dst[i], 4); dst[i] = (float)v; }
    return CTK_OK;
}

// =============================================================================================
// The two drivers: ONE step (batch_step, the *_step entries) and ONE closed loop on the device (batch_closed_loop: *_run, *_episodes;
// include/ctk_hip_run.h, ctk_hip_episode.h, ctk_hip_loop.h) for every family.  What is a family's own is a small trait (MppiFamily and
// its MLP form MlpFamily, CemFamily, RpgdFamily, each below its family's struct):
//   Batch, Rec            the handle and its step record (every record type has id, seq, s[], u_prev[] and dev_uprev)
//   carries_k             the per-problem form's constants travel behind the step records and are taken by record index (CEM, RPGD);
//                         else they live in an array by problem id that `constants` refreshes (MPPI)
//   error_word            the kernel has an in-launch hand-off whose error word is read and cleared (MPPI, CEM); `handoff_outputs`:
//                         what a step's message says of the outputs then
//   refuse(b, who, n, ids)               the family's own refusal, before anything is launched
//   context(b)                           what all its launches share
//   constants(b, ids, n, h_k)            the per-problem form's constants ahead of a segment's records
//   fill(b, q, p, t)                     the record of the step problem p takes t steps from now: every counter, no draws
//   launch(b, ctx, d_rec, n, d_k, &launched)   the controller launches of n records of ONE step, split as the family's step splits them
//   advance(b, p, ctrl, tried, issued)   the family's counter rule, stated once: problem p after `ctrl` steps that were launched in full
//                                        and, if `tried`, one more whose launches failed, this problem's among them (`issued`) or not
//   unpublished_keeps_position           where a step and the closed loop differ (see the families): batch_step takes back the one
//                                        position that `advance` counted for a launched problem whose slot never shows the step's seq
// and, of the step alone, a caller's draws (StepDraws):
//   device_ahead_of_draws                hipSetDevice runs ahead of the check of the draws (MPPI), else behind it
//   draws_of(b, p)                       floats of problem p's row: row j starts where the rows of the listed problems before it end
//   check_draws(b, who, n, ids, d, total)   the family's checks of a caller's draws and their messages; total: the rows' sum
//   draws(q)                             the record's pointer to its row
// and of the entries that CTK_BATCH_ENTRIES writes: state(b, p), state_size_named, per_problem_kernel(b).
// =============================================================================================

// a caller's draws for a step: the pointer, where it points (CTK_LOC_*), and the count the caller states (RPGD's entry alone has one)
struct StepDraws { const float* samples; size_t n_samples; int loc; };

// what the MPPI and CEM steps check of a caller's draws (the RPGD step has its own order and a count to check)
int batch_check_draws(BatchCore* b, const StepDraws& d) {
    if (d.loc == CTK_LOC_NONE) return CTK_OK;
    if (d.samples == nullptr) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "samples pointer is NULL but samples_loc != CTK_LOC_NONE");
    if (d.loc != CTK_LOC_DEVICE && d.loc != CTK_LOC_HOST) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "bad samples_loc");
    return CTK_OK;
}

// One step of the listed problems (every family's *_step): the step records — states and previous inputs travel with them — in ONE
// transfer ahead of the launch(es), the completion poll, then the counters and u of every listed problem.  The call is synchronous:
// h_steps is both the source of the transfer and, afterwards, the host's memory of id and seq for the bookkeeping (nothing refills
// it before the call returns; an asynchronous step would need its own copy).
template <class F>
int batch_step(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, const float* s, const float* u_prev, const StepDraws& d,
               float* u_out) {
    using Rec = typename F::Rec;
    if (!b || !s) return b ? bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL state") : CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (int rc = F::refuse(b, who, n, ids)) return rc;
    if (F::device_ahead_of_draws) BHIP_TRY(b, hipSetDevice(b->cfg.device));    // by history: the MPPI step; behind the check in the CEM and RPGD steps
    size_t total = 0;
    for (int j = 0; j < n; ++j) total += F::draws_of(b, ids ? ids[j] : j);
    if (int rc = F::check_draws(b, who, n, ids, d, total)) return rc;          // refused before a sample is read, anything is launched or consumed
    if (!F::device_ahead_of_draws) BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const float* d_s = nullptr;                        // the first row; the rows follow one another in the order of the listed problems
    if (d.loc == CTK_LOC_DEVICE && total) d_s = d.samples;
    else if (d.loc == CTK_LOC_HOST && total) {
        if (int rc = batch_stage(b, d.samples, total)) return rc;
        d_s = b->d_samples;
    }
    size_t off = 0;
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        Rec& q = b->h_steps[j];
        F::fill(b, q, p, 0);
        const size_t cnt = F::draws_of(b, p);
        F::draws(q) = (d_s && cnt) ? d_s + off : nullptr;
        off += cnt;
        batch_record_io(b, q, j, s, u_prev);
    }
    const unsigned char* d_k = nullptr;                // carries_k, the per-problem form: the constants behind the records, in the same transfer
    hipError_t le;
    if constexpr (F::carries_k) le = batch_send_records(b, b->kcache.data(), ids, n, sizeof(Rec), b->h_steps, b->d_steps, &d_k);
    else {
        le = F::constants(b, ids, n, nullptr);         // MPPI: the constants' transfer goes ahead of the step records'
        if (le == hipSuccess) le = hipMemcpyAsync(b->d_steps, b->h_steps, (size_t)n * sizeof(Rec), hipMemcpyHostToDevice, b->stream);
    }
    const auto ctx = F::context(b);
    int launched = 0;
    if (le == hipSuccess) le = F::launch(b, ctx, b->d_steps, n, d_k, &launched);
    const std::string late = batch_poll(b, ids, launched);
    std::string timed_out;
    for (int j = 0; j < n; ++j) {                      // the counters reflect what was launched (F::advance)
        const int p = b->h_steps[j].id;
        volatile uint32_t* slot = reinterpret_cast<volatile uint32_t*>(b->slot(p));
        F::advance(b, p, j < launched ? 1 : 0, j >= launched, false);
        if (j >= launched) continue;
        // a launched problem that never published: where the family says so (unpublished_keeps_position), the Philox position that
        // advance has just moved with the launch is taken back, and neither u nor the error word is read
        if (F::unpublished_keeps_position && slot[1] != b->h_steps[j].seq) { --b->call[(size_t)p]; continue; }
        batch_read_u(b, p, j, u_out);
        if (F::error_word && slot[2]) { slot[2] = 0; list_problem(timed_out, p); }   // the hand-off's error word, read and cleared
    }
    if (le != hipSuccess) return bfail(b, CTK_ERR_HIP, std::string(who) + ": " + hipGetErrorString(le));
    if (!late.empty()) return bfail(b, CTK_ERR_HIP, std::string(who) + ": the step finished without publishing the result of problem(s) " + late);
    if constexpr (F::error_word)
        if (!timed_out.empty())
            return bfail(b, CTK_ERR_STATE, std::string(who) + ": in-launch record hand-off timed out (a workgroup's record never arrived) for problem(s) " +
                         timed_out + F::handoff_outputs);
    return CTK_OK;
}

// The plants' constants ahead of a run or a plant step: problem p's effective table (override, else its own controller value) and the
// sub-step count against what h_kplant was derived from; those that changed are re-derived with the function the controller's
// constants come from, and the span from the first to the last of them travels in ONE transfer on the batch's stream (none when
// nothing changed).  The caller synchronises before it returns, so the staging is free again at the next call.
hipError_t batch_plant_flush(BatchCore* b, int substeps) {
    int lo = b->B, hi = -1;
    float eff[CTK_MAX_PARAMS];
    for (int p = 0; p < b->B; ++p) {
        const size_t z = (size_t)p * CTK_MAX_PARAMS;
        for (int i = 0; i < CTK_MAX_PARAMS; ++i) eff[i] = b->plant_has[z + i] ? b->plant_over[z + i] : b->table(p)[i];
        if (b->plant_sub[(size_t)p] == substeps && std::memcmp(eff, &b->plant_tab[z], sizeof(eff)) == 0) continue;
        ctk_mppi_batch_derive_k(b->env, eff, b->cfg.dt, substeps, b->h_kplant + (size_t)p * b->kstride);
        std::memcpy(&b->plant_tab[z], eff, sizeof(eff));
        b->plant_sub[(size_t)p] = substeps;
        lo = std::min(lo, p); hi = p;
    }
    if (hi < 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(b->d_kplant + (size_t)lo * b->kstride, b->h_kplant + (size_t)lo * b->kstride, (size_t)(hi - lo + 1) * b->kstride,
                                        hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess) for (int p = lo; p <= hi; ++p) b->plant_sub[(size_t)p] = 0;      // nothing reached the device: derive and copy again
    return e;
}

// Where the parts of the run buffer lie for a segment of n problems and L steps (bytes from its start; every part 16-aligned).  What
// travels to the device in ONE transfer lies in front (up to `states`), what comes back in ONE copy behind it:
//   step records [L][n] | per-problem constants [n] | inputs of a plant step [n][C] | true start states [n][S] |
//   previous inputs of the first step [n][C] | noise records [n] || state trace [n][L][S] | observation trace [n][L][S] |
//   input trace [n][L][C] | realised costs [n][L]
// The constants are there only in the per-problem form of a family whose kernels take them by record index (kbytes, else 0): ONE block
// of n elements in listed order behind all L * n records, which every step's launches read.  The parts only the noisy plant has
// (s_start, u_start, noise, obs, costs) are empty without it: what then remains is
//   step records | constants | inputs of a plant step || state trace | input trace.
struct LoopLayout {
    size_t k, u_in, s_start, u_start, noise, states, obs, inputs, costs, total;
    LoopLayout(const BatchCore* b, size_t rec, size_t kbytes, int n, int L, bool noisy) {
        auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
        auto ep = [&](size_t x) { return noisy ? x : 0; };
        k = (size_t)L * n * rec;
        u_in = k + up(kbytes);
        s_start = u_in + up((size_t)n * b->C * sizeof(float));
        u_start = s_start + ep(up((size_t)n * b->S * sizeof(float)));
        noise = u_start + ep(up((size_t)n * b->C * sizeof(float)));
        states = noise + ep((size_t)n * sizeof(CtkPlantNoise));
        obs = states + up((size_t)n * L * b->S * sizeof(float));
        inputs = obs + ep(up((size_t)n * L * b->S * sizeof(float)));
        costs = inputs + up((size_t)n * L * b->C * sizeof(float));
        total = costs + ep(up((size_t)n * L * sizeof(float)));
    }
};
static_assert(sizeof(CtkBatchStep) % 16 == 0 && sizeof(CtkCemBatchStep) % 16 == 0 && sizeof(CtkRpgdBatchStep) % 16 == 0,
              "the parts of the run buffer lie behind the step records, 16-aligned");
static_assert(sizeof(CtkPlantNoise) % 16 == 0, "the traces lie behind the noise records, 16-aligned");

// the run buffer (device and pinned), grown to the layout's bytes on demand
int batch_run_buffers(BatchCore* b, const LoopLayout& lay) {
    BHIP_TRY(b, b->own.grow_dev(b->d_run, b->d_run_cap, lay.total));
    BHIP_TRY(b, b->own.grow_pin(b->h_run, b->h_run_cap, lay.total));
    return CTK_OK;
}

// problem p's noise record at its current position
void batch_noise_record(const BatchCore* b, int p, CtkPlantNoise* q) {
    const float* sg = &b->noise_sigma[(size_t)p * 2 * CTK_MAX_STATES];
    q->any = 0u;
    for (int i = 0; i < CTK_MAX_STATES; ++i) {
        q->sigma_w[i] = i < b->S ? sg[i] : 0.0f;
        q->sigma_v[i] = i < b->S ? sg[CTK_MAX_STATES + i] : 0.0f;
        if (q->sigma_w[i] != 0.0f || q->sigma_v[i] != 0.0f) q->any = 1u;
    }
    q->seed_lo = (uint32_t)(b->noise_seed[(size_t)p] & 0xFFFFFFFFull); q->seed_hi = (uint32_t)(b->noise_seed[(size_t)p] >> 32);
    q->pos = b->noise_pos[(size_t)p];
}

int batch_substeps(BatchCore* b, const char* who, int substeps, int* out) {
    if (substeps < 0) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": the plant's sub-step count must be >= 1, or 0 for cfg.intermediate_steps (" + std::to_string(substeps) + ")");
    *out = substeps ? substeps : b->cfg.intermediate_steps;
    return CTK_OK;
}

// One plant step of the listed problems (*_plant_step; with y_next, *_plant_step_noisy): the records, the inputs and what the noisy
// plant reads besides travel in ONE transfer, one launch, one copy back, one synchronisation.
template <class F>
int batch_plant_step(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev,
                     int substeps, float* s_next, float* y_next, float* cost) {
    using Rec = typename F::Rec;
    const bool noisy = y_next != nullptr;
    int n = 0, sub = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (int rc = batch_substeps(b, who, substeps, &sub)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const int S = b->S, C = b->C;
    const LoopLayout lay(b, sizeof(Rec), 0, n, 1, noisy);
    if (int rc = batch_run_buffers(b, lay)) return rc;
    // the records carry the problem and, for the plain plant, its state; the noisy plant reads the state from a row of its own
    Rec* rec = reinterpret_cast<Rec*>(b->h_run);
    CtkPlantNoise* nz = reinterpret_cast<CtkPlantNoise*>(b->h_run + lay.noise);
    for (int j = 0; j < n; ++j) {
        std::memset(&rec[j], 0, sizeof(Rec));
        rec[j].id = ids ? ids[j] : j;
        if (noisy) batch_noise_record(b, rec[j].id, &nz[j]);
        else for (int i = 0; i < S; ++i) rec[j].s[i] = s[(size_t)j * S + i];
    }
    std::memcpy(b->h_run + lay.u_in, u, (size_t)n * C * sizeof(float));
    if (noisy) {
        std::memcpy(b->h_run + lay.s_start, s, (size_t)n * S * sizeof(float));
        std::memcpy(b->h_run + lay.u_start, u_prev, (size_t)n * C * sizeof(float));
    }
    const Rec* d_rec = reinterpret_cast<const Rec*>(b->d_run);
    auto dev = [&](size_t at) { return reinterpret_cast<float*>(b->d_run + at); };
    const size_t back = noisy ? lay.total - lay.states : (size_t)n * S * sizeof(float);      // the plain plant wrote the next states alone
    hipError_t le = batch_plant_flush(b, sub);
    if (le == hipSuccess) le = hipMemcpyAsync(b->d_run, b->h_run, lay.states, hipMemcpyHostToDevice, b->stream);
    bool launched = false;
    if (le == hipSuccess) {
        if (noisy)
            le = ctk_launch_batch_plant_noisy(b->stream, b->env, b->d_desc, d_rec, nullptr, b->d_kplant,
                                              reinterpret_cast<const CtkPlantNoise*>(b->d_run + lay.noise), dev(lay.u_in), dev(lay.s_start), (size_t)S,
                                              dev(lay.u_start), (size_t)C, 0u, dev(lay.states), dev(lay.obs), nullptr, dev(lay.costs), n, (size_t)S, 0, 1);
        else
            le = ctk_launch_batch_plant(b->stream, b->env, b->d_desc, d_rec, nullptr, b->d_kplant, dev(lay.u_in), dev(lay.states), nullptr, n,
                                        (size_t)S, 0);
        launched = le == hipSuccess;
    }
    if (le == hipSuccess) le = hipMemcpyAsync(b->h_run + lay.states, b->d_run + lay.states, back, hipMemcpyDeviceToHost, b->stream);
    const hipError_t se = hipStreamSynchronize(b->stream);                     // the stagings are free again, whatever happened
    if (le == hipSuccess) le = se;
    if (noisy && launched)
        for (int j = 0; j < n; ++j) ++b->noise_pos[(size_t)rec[j].id];         // by the plant launch that was issued
    if (le != hipSuccess) return bfail(b, CTK_ERR_HIP, std::string(who) + ": " + hipGetErrorString(le));
    std::memcpy(s_next, b->h_run + lay.states, (size_t)n * S * sizeof(float));
    if (noisy) {
        std::memcpy(y_next, b->h_run + lay.obs, (size_t)n * S * sizeof(float));
        std::memcpy(cost, b->h_run + lay.costs, (size_t)n * sizeof(float));
    }
    return CTK_OK;
}

// The counters after a segment of L steps whose launches ended with `le`.  `ctrl` steps had the controllers of all n listed problems
// launched; if the launches of the step after them failed (part >= 0), those of its first `part` problems were; `plants` launches of
// the noisy plant were issued (a run: 0).  The family's counters and noise_pos are left as if exactly these had run, by the rule of the
// family's step (F::advance).  Only where nothing failed, a problem whose slot does not show the segment's last step is listed in
// `late`; the hand-off's error word, where the family has one, is read and cleared into timed[j] whatever happened.
template <class F>
void batch_loop_account(typename F::Batch* b, int n, const int32_t* ids, hipError_t le, int L, int ctrl, int part, int plants, std::string& late,
                        std::vector<unsigned char>& timed) {
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        volatile uint32_t* slot = reinterpret_cast<volatile uint32_t*>(b->slot(p));
        if (le == hipSuccess && slot[1] != b->seq[(size_t)p] + (uint32_t)(L - 1)) list_problem(late, p);
        if (F::error_word && slot[2]) { slot[2] = 0; timed[(size_t)j] = 1; }  // the hand-off's error word, read and cleared
        F::advance(b, p, ctrl, part >= 0, j < part);
        b->noise_pos[(size_t)p] += (uint32_t)plants;
    }
}

// a closed-loop call: *_run, or with obs_out (and costs_out) *_episodes
struct LoopCall {
    const char* who;                        // the entry point, for the messages
    const char* noun;                       // "a run" / "an episode"
    int n_ids; const int32_t* ids;
    const float *s0, *y0, *u_prev;
    int n_steps, plant_substeps;
    float *states_out, *obs_out, *inputs_out, *costs_out;
    int32_t* first_bad;
};

// The closed loop on the device, in segments of at most run_segment steps.  A segment is ONE transfer of its step records (and what the
// noisy plant reads at its first step), per step the controller launches and one plant launch, ONE copy of the traces back and ONE
// synchronisation; the plant launch of step t writes the state (the noisy plant: the observation) into the records of step t + 1 on the
// device.  The noisy plant differs in where it reads from (the true state and the previous input have rows of their own, see
// ctk_plant.hip), in its noise positions and in the two further traces.
template <class F>
int batch_closed_loop(typename F::Batch* b, const LoopCall& c) {
    using Rec = typename F::Rec;
    const bool noisy = c.obs_out != nullptr;
    const int32_t* ids = c.ids;
    const float* u_prev = c.u_prev;
    const int n_steps = c.n_steps;
    int n = 0, sub = 0;
    if (int rc = batch_ids(b, c.who, c.n_ids, ids, &n)) return rc;
    if (n_steps < 1)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(c.who) + ": " + c.noun + " has at least one step (n_steps == " + std::to_string(n_steps) + ")");
    if (int rc = batch_substeps(b, c.who, c.plant_substeps, &sub)) return rc;
    if (int rc = F::refuse(b, c.who, n, ids)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const int S = b->S, C = b->C;
    const size_t srow = ((size_t)n_steps + 1) * S, urow = (size_t)n_steps * C;       // one problem's rows of the traces
    for (int j = 0; j < n; ++j) {
        std::memcpy(c.states_out + (size_t)j * srow, c.s0 + (size_t)j * S, (size_t)S * sizeof(float));
        if (noisy) std::memcpy(c.obs_out + (size_t)j * srow, (c.y0 ? c.y0 : c.s0) + (size_t)j * S, (size_t)S * sizeof(float));
        if (c.first_bad) c.first_bad[j] = -1;
    }
    // The noisy plant without u_prev: the first step's previous input is what the first controller launch reads as its own — the problem's
    // last output in d_u (*_set_state writes it too, the pinned result slot only holds what a step published).  That launch
    // overwrites it, so the span of the listed problems is read here, once per call, ahead of everything else.  A run has no use for it.
    const int p_lo = ids ? ids[0] : 0, p_hi = ids ? ids[n - 1] : n - 1;
    std::vector<float> own_u;
    if (noisy && !u_prev) {
        own_u.resize((size_t)(p_hi - p_lo + 1) * CTK_MAX_INPUTS);
        BHIP_TRY(b, hipMemcpyAsync(own_u.data(), b->d_u + (size_t)p_lo * CTK_MAX_INPUTS, own_u.size() * sizeof(float), hipMemcpyDeviceToHost, b->stream));
        BHIP_TRY(b, hipStreamSynchronize(b->stream));
    }
    const float* first_s = noisy ? c.obs_out : c.states_out;                   // what the controllers see: of a run the state itself
    std::vector<unsigned char> timed((size_t)n, 0);
    std::string late;
    const auto ctx = F::context(b);
    const size_t kbytes = (F::carries_k && b->carries()) ? (size_t)n * b->elem() : 0;
    hipError_t le = batch_plant_flush(b, sub);
    for (int k0 = 0; le == hipSuccess && k0 < n_steps;) {
        const int L = std::min(b->run_segment, n_steps - k0);                  // this segment: steps k0 .. k0 + L - 1
        const LoopLayout lay(b, sizeof(Rec), kbytes, n, L, noisy);
        if (int rc = batch_run_buffers(b, lay)) { hipStreamSynchronize(b->stream); return rc; }
        // every record of the segment: all but the state is known in advance.  The state of the segment's first step is the host's (the
        // start state or observation, or the previous segment's last one from the copied trace); the later ones the plant launches write
        // on the device.
        Rec* rec = reinterpret_cast<Rec*>(b->h_run);
        for (int t = 0; t < L; ++t) {
            const bool given = k0 + t == 0 && u_prev;                          // from the second step on: the problem's own last output
            for (int j = 0; j < n; ++j) {
                Rec& q = rec[(size_t)t * n + j];
                F::fill(b, q, ids ? ids[j] : j, t);
                q.dev_uprev = given ? 0u : 1u;
                for (int i = 0; i < CTK_MAX_STATES; ++i) q.s[i] = (t == 0 && i < S) ? first_s[(size_t)j * srow + (size_t)k0 * S + i] : 0.0f;
                for (int i = 0; i < CTK_MAX_INPUTS; ++i) q.u_prev[i] = (given && i < C) ? u_prev[(size_t)j * C + i] : 0.0f;
            }
        }
        // what the first noisy plant launch of the segment reads in place of trace rows: the true state, and the input before the
        // segment's first one — the given u_prev, the previous segment's last input, or the problem's own last output (read above)
        if (noisy) {
            float* h_s = reinterpret_cast<float*>(b->h_run + lay.s_start);
            float* h_up = reinterpret_cast<float*>(b->h_run + lay.u_start);
            CtkPlantNoise* nz = reinterpret_cast<CtkPlantNoise*>(b->h_run + lay.noise);
            for (int j = 0; j < n; ++j) {
                const int p = ids ? ids[j] : j;
                std::memcpy(h_s + (size_t)j * S, c.states_out + (size_t)j * srow + (size_t)k0 * S, (size_t)S * sizeof(float));
                if (k0 > 0) std::memcpy(h_up + (size_t)j * C, c.inputs_out + (size_t)j * urow + ((size_t)k0 - 1) * C, (size_t)C * sizeof(float));
                else if (u_prev) std::memcpy(h_up + (size_t)j * C, u_prev + (size_t)j * C, (size_t)C * sizeof(float));
                else std::memcpy(h_up + (size_t)j * C, &own_u[(size_t)(p - p_lo) * CTK_MAX_INPUTS], (size_t)C * sizeof(float));
                batch_noise_record(b, p, &nz[j]);
            }
        }
        Rec* d_rec = reinterpret_cast<Rec*>(b->d_run);
        auto dev = [&](size_t at) { return reinterpret_cast<float*>(b->d_run + at); };
        const CtkPlantNoise* d_nz = reinterpret_cast<const CtkPlantNoise*>(b->d_run + lay.noise);
        const unsigned char* d_k = kbytes ? b->d_run + lay.k : nullptr;        // behind all L * n records: every step's launches read it
        float *d_st = dev(lay.states), *d_ob = dev(lay.obs), *d_in = dev(lay.inputs), *d_co = dev(lay.costs);
        le = F::constants(b, ids, n, b->h_run + lay.k);                        // MPPI: a transfer of its own, ahead of the step records'
        if (le == hipSuccess) le = hipMemcpyAsync(b->d_run, b->h_run, noisy ? lay.states : lay.u_in, hipMemcpyHostToDevice, b->stream);
        int ctrl = 0, part = -1, plants = 0;           // steps whose controllers were all launched; of the step whose launches failed, how
                                                       // many were; the noisy plant launches that were issued
        for (int t = 0; le == hipSuccess && t < L; ++t) {
            int launched = 0;
            le = F::launch(b, ctx, d_rec + (size_t)t * n, n, d_k, &launched);
            if (le != hipSuccess) { part = launched; break; }
            ++ctrl;
            Rec* next = t + 1 < L ? d_rec + (size_t)(t + 1) * n : nullptr;
            if (noisy) {
                le = ctk_launch_batch_plant_noisy(b->stream, b->env, b->d_desc, d_rec + (size_t)t * n, next, b->d_kplant, d_nz, nullptr,
                                                  t ? d_st + (size_t)(t - 1) * S : dev(lay.s_start), t ? (size_t)L * S : (size_t)S,
                                                  t ? d_in + (size_t)(t - 1) * C : dev(lay.u_start), t ? (size_t)L * C : (size_t)C, (uint32_t)t,
                                                  d_st + (size_t)t * S, d_ob + (size_t)t * S, d_in + (size_t)t * C, d_co + t, n, (size_t)L * S, (size_t)L * C,
                                                  (size_t)L);
                if (le == hipSuccess) ++plants;
            } else {
                le = ctk_launch_batch_plant(b->stream, b->env, b->d_desc, d_rec + (size_t)t * n, next, b->d_kplant, nullptr, d_st + (size_t)t * S,
                                            d_in + (size_t)t * C, n, (size_t)L * S, (size_t)L * C);
            }
        }
        if (le == hipSuccess) le = hipMemcpyAsync(b->h_run + lay.states, b->d_run + lay.states, lay.total - lay.states, hipMemcpyDeviceToHost, b->stream);
        const hipError_t se = hipStreamSynchronize(b->stream);                 // ONE synchronisation per segment, whatever happened
        if (le == hipSuccess) le = se;
        std::atomic_thread_fence(std::memory_order_acquire);
        batch_loop_account<F>(b, n, ids, le, L, ctrl, part, plants, late, timed);  // the counters reflect what was launched
        if (le != hipSuccess) break;
        auto host = [&](size_t at) { return reinterpret_cast<const float*>(b->h_run + at); };
        const float *h_st = host(lay.states), *h_ob = host(lay.obs), *h_in = host(lay.inputs), *h_co = host(lay.costs);
        for (int j = 0; j < n; ++j) {
            std::memcpy(c.states_out + (size_t)j * srow + ((size_t)k0 + 1) * S, h_st + (size_t)j * L * S, (size_t)L * S * sizeof(float));
            std::memcpy(c.inputs_out + (size_t)j * urow + (size_t)k0 * C, h_in + (size_t)j * L * C, (size_t)L * C * sizeof(float));
            if (noisy) {
                std::memcpy(c.obs_out + (size_t)j * srow + ((size_t)k0 + 1) * S, h_ob + (size_t)j * L * S, (size_t)L * S * sizeof(float));
                std::memcpy(c.costs_out + (size_t)j * n_steps + (size_t)k0, h_co + (size_t)j * L, (size_t)L * sizeof(float));
            }
            if (c.first_bad && c.first_bad[j] < 0)
                for (int i = 0; i < L * C; ++i)
                    if (!std::isfinite(h_in[(size_t)j * L * C + i])) { c.first_bad[j] = k0 + i / C; break; }
        }
        k0 += L;
    }
    if (le != hipSuccess)
        return bfail(b, CTK_ERR_HIP, std::string(c.who) + ": " + hipGetErrorString(le) + " (the counters reflect the steps that were launched; the traces are not valid)");
    if (!late.empty()) return bfail(b, CTK_ERR_HIP, std::string(c.who) + ": a segment finished without publishing the last result of problem(s) " + late);
    std::string timed_out;
    for (int j = 0; j < n; ++j)
        if (timed[(size_t)j]) list_problem(timed_out, ids ? ids[j] : j);
    if (!timed_out.empty())
        return bfail(b, CTK_ERR_STATE, std::string(c.who) + ": in-launch record hand-off timed out (a workgroup's record never arrived) for problem(s) " + timed_out +
                     "; such a step publishes NaN and the plant propagates it: their traces show where (first_bad), the other problems' traces are valid");
    return CTK_OK;
}

// ---- the bodies of every family's plant and noise entries (include/ctk_hip_run.h, ctk_hip_episode.h, ctk_hip_loop.h); `who` is the entry's name ----
int plant_set_param(BatchCore* b, const char* who, int n_ids, const int32_t* ids, int id, const float* values) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (int rc = batch_param_id(b, who, id)) return rc;
    if (!values) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL values (one value per listed problem)");
    for (int j = 0; j < n; ++j) {
        const size_t z = (size_t)(ids ? ids[j] : j) * CTK_MAX_PARAMS + (size_t)id;
        b->plant_over[z] = values[j];                  // derived at the next run or plant step (batch_plant_flush compares the tables)
        b->plant_has[z] = 1;
    }
    return CTK_OK;
}
int plant_get_param(const BatchCore* b, int problem, int id, float* value) {
    if (!b || !value || problem < 0 || problem >= b->B || id < 0 || id >= env_info(b->env)->n_params) return CTK_ERR_INVALID_ARGUMENT;
    const size_t z = (size_t)problem * CTK_MAX_PARAMS + (size_t)id;
    *value = b->plant_has[z] ? b->plant_over[z] : b->table(problem)[id];
    return CTK_OK;
}
int plant_clear_params(BatchCore* b) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    std::fill(b->plant_has.begin(), b->plant_has.end(), (unsigned char)0);
    return CTK_OK;
}
int plant_set_noise(BatchCore* b, const char* who, int n_ids, const int32_t* ids, int kind, const float* sigma) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (kind != 0 && kind != 1) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": kind is 0 (process noise) or 1 (measurement noise), not " + std::to_string(kind));
    if (!sigma) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL sigma (one row of num_states values per listed problem)");
    for (int i = 0; i < n * b->S; ++i)
        if (!(std::isfinite(sigma[i]) && sigma[i] >= 0.0f))
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": a standard deviation is finite and >= 0 (" + std::to_string(sigma[i]) + " for problem " +
                         std::to_string(ids ? ids[i / b->S] : i / b->S) + ", state " + std::to_string(i % b->S) + "); nothing was written");
    for (int j = 0; j < n; ++j) {
        float* dst = &b->noise_sigma[((size_t)(ids ? ids[j] : j) * 2 + (size_t)kind) * CTK_MAX_STATES];
        for (int i = 0; i < b->S; ++i) dst[i] = sigma[(size_t)j * b->S + i] == 0.0f ? 0.0f : sigma[(size_t)j * b->S + i];   // -0.0 is "none" too
    }
    return CTK_OK;
}
int plant_get_noise(const BatchCore* b, int problem, int kind, float* sigma) {
    if (!b || !sigma || problem < 0 || problem >= b->B || (kind != 0 && kind != 1)) return CTK_ERR_INVALID_ARGUMENT;
    std::memcpy(sigma, &b->noise_sigma[((size_t)problem * 2 + (size_t)kind) * CTK_MAX_STATES], (size_t)b->S * sizeof(float));
    return CTK_OK;
}
int plant_clear_noise(BatchCore* b) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    std::fill(b->noise_sigma.begin(), b->noise_sigma.end(), 0.0f);
    return CTK_OK;
}
int plant_set_noise_seed(BatchCore* b, const char* who, int n_ids, const int32_t* ids, const uint64_t* seeds) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (!seeds) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL seeds (one per listed problem)");
    for (int j = 0; j < n; ++j) b->noise_seed[(size_t)(ids ? ids[j] : j)] = seeds[j];
    return CTK_OK;
}
int plant_get_noise_seed(const BatchCore* b, int problem, uint64_t* seed) {
    if (!b || !seed || problem < 0 || problem >= b->B) return CTK_ERR_INVALID_ARGUMENT;
    *seed = b->noise_seed[(size_t)problem];
    return CTK_OK;
}
int plant_noise_get_position(const BatchCore* b, int problem, uint32_t* pos) {
    if (!b || !pos || problem < 0 || problem >= b->B) return CTK_ERR_INVALID_ARGUMENT;
    *pos = b->noise_pos[(size_t)problem];
    return CTK_OK;
}
int plant_noise_set_position(BatchCore* b, const char* who, int problem, uint32_t pos) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (int rc = batch_problem(b, who, problem)) return rc;
    b->noise_pos[(size_t)problem] = pos;
    return CTK_OK;
}

// ---- rollouts of caller-supplied plans (include/ctk_hip_rollout.h: *_batch_rollout; kernels in ctk_batch_rollout.hip) ----
// a rollout call: the entry's arguments
struct RolloutCall {
    const char* who;                        // the entry point, for the messages
    int n; const int32_t* ids;
    const float *S, *u_prev, *plans;
    int plans_loc, m, model, plant_substeps;
    float *traj_out, *J_out;
};

// Where the parts of the run buffer lie for a rollout of n records of m plans (bytes from its start; every part 16-aligned).  What
// travels to the device in ONE transfer lies in front (up to `J`), what comes back in ONE copy behind it, and behind that what stays
// on the device:
//   records [n] | per-problem constants [kelems] | plans [n][m][H,C] (host plans only) || J [n][m] | trajectories [n][m][H+1][S] (if asked) ||
//   the body's copy of the plans [n][m][H,C]
struct RolloutLayout {
    size_t k, plans, J, traj, Q, back, total;
    RolloutLayout(const BatchCore* b, size_t kelems, int n, int m, bool host_plans, bool want_traj) {
        auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
        const size_t rows = (size_t)n * m;
        k = (size_t)n * sizeof(CtkBatchRolloutRec);
        plans = k + kelems * b->kstride;
        J = plans + (host_plans ? up(rows * b->HC * sizeof(float)) : 0);
        traj = J + up(rows * sizeof(float));
        Q = traj + (want_traj ? up(rows * ((size_t)b->H + 1) * b->S * sizeof(float)) : 0);
        back = Q;
        total = Q + up(rows * b->HC * sizeof(float));
    }
};

// The rollout of the listed problems' plans, for every family: the checks, n records (with the constants and the caller's plans behind
// them) in ONE transfer, ONE launch, ONE copy back, ONE synchronisation.  It works in the run buffer, which no call keeps anything in:
// the problems' J, Q, TRAJ, plans, outputs, hidden states, counters and Philox positions are not touched.  What is a family's own:
//   rollout_pred(b)                      the predictor of model = controller (CTK_PRED_*)
//   rollout_weights(b, &stride)          the per-problem network blocks and their stride in floats (nullptr: analytic)
//   rollout_refuse(b, who, n, ids, own, net)   its refusals: a problem without weights where the network rolls out, an RPGD problem that
//                                        was never reset where its own plan is asked for
//   own_plan(b, p)                       where read(U_NOM, p) reads from
// ids may come in any order here (rows are independent), but each problem once.
template <class F>
int batch_rollout(typename F::Batch* b, const RolloutCall& c) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    const std::string who = c.who;
    if (!c.S) return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": NULL states (one row per listed problem)");
    int n = b->B;
    if (c.ids) {
        if (c.n < 1 || c.n > b->B) return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": n must be 1 .. " + std::to_string(b->B) + " (the batch size)");
        std::vector<unsigned char> seen((size_t)b->B, 0);
        for (int j = 0; j < c.n; ++j) {
            if (c.ids[j] < 0 || c.ids[j] >= b->B)
                return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": problem index " + std::to_string(c.ids[j]) + " is outside 0 .. " + std::to_string(b->B - 1));
            if (seen[(size_t)c.ids[j]]++) return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": problem " + std::to_string(c.ids[j]) + " is listed twice");
        }
        n = c.n;
    }
    const int32_t* ids = c.ids;
    if (c.m < 1 || c.m > b->N)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": need 1 <= m <= num_rollouts (" + std::to_string(b->N) + "), the bound of a handle's ctk_rollout (m == " + std::to_string(c.m) + ")");
    const bool own = c.plans == nullptr;
    if (own && c.m != 1) return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": plans == NULL rolls out every listed problem's own current plan: m must be 1");
    if (!own && c.plans_loc != CTK_LOC_HOST && c.plans_loc != CTK_LOC_DEVICE) return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": plans_loc must be CTK_LOC_HOST or CTK_LOC_DEVICE");
    if (c.model != CTK_ROLLOUT_MODEL_CONTROLLER && c.model != CTK_ROLLOUT_MODEL_PLANT)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, who + ": model is CTK_ROLLOUT_MODEL_CONTROLLER or CTK_ROLLOUT_MODEL_PLANT, not " + std::to_string(c.model));
    const bool plant = c.model == CTK_ROLLOUT_MODEL_PLANT;
    int sub = 0;
    if (plant) if (int rc = batch_substeps(b, c.who, c.plant_substeps, &sub)) return rc;
    const int pred = plant ? CTK_PRED_ODE : F::rollout_pred(b);
    if (int rc = F::rollout_refuse(b, c.who, n, ids, own, pred != CTK_PRED_ODE)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const int S = b->S, C = b->C, HC = b->HC, m = c.m;
    if (!b->d_zero_one) {                              // base 0, scale 1: once per batch
        std::vector<float> zo((size_t)2 * HC, 0.0f);
        std::fill(zo.begin() + HC, zo.end(), 1.0f);
        BHIP_TRY(b, b->own.dev_zero(&b->d_zero_one, zo.size() * sizeof(float), b->stream));
        const hipError_t e = hipMemcpyAsync(b->d_zero_one, zo.data(), zo.size() * sizeof(float), hipMemcpyHostToDevice, b->stream);
        const hipError_t se = hipStreamSynchronize(b->stream);     // zo goes out of scope
        if (e != hipSuccess || se != hipSuccess) { b->own.free_dev(b->d_zero_one); BHIP_TRY(b, e); BHIP_TRY(b, se); }
    }
    // the constants: the plants' live in d_kplant by problem id (the closed loop's table, flushed by its helper); the controller's travel
    // behind the records — one element in the shared form, else one per record, derived from the problem's CURRENT table with the
    // function a step uses (nothing is cached or marked here, so a later step derives what it would have derived)
    const bool host_plans = !own && c.plans_loc == CTK_LOC_HOST, want_traj = c.traj_out != nullptr;
    const size_t kelems = plant ? 0 : b->differ ? (size_t)n : 1;
    const RolloutLayout lay(b, kelems, n, m, host_plans, want_traj);
    BHIP_TRY(b, b->own.grow_dev(b->d_run, b->d_run_cap, lay.total));
    BHIP_TRY(b, b->own.grow_pin(b->h_run, b->h_run_cap, lay.back));
    CtkBatchRolloutRec* rec = reinterpret_cast<CtkBatchRolloutRec*>(b->h_run);
    const size_t prow = (size_t)m * HC, trow = (size_t)m * ((size_t)b->H + 1) * S;
    auto dev = [&](size_t at) { return reinterpret_cast<float*>(b->d_run + at); };
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        CtkBatchRolloutRec& q = rec[j];
        std::memset(&q, 0, sizeof(q));
        q.id = p; q.m = m;
        q.kidx = plant ? p : b->differ ? j : 0;
        q.plans = own ? F::own_plan(b, p) : host_plans ? dev(lay.plans) + (size_t)j * prow : c.plans + (size_t)j * prow;
        q.J = dev(lay.J) + (size_t)j * m;
        q.traj = want_traj ? dev(lay.traj) + (size_t)j * trow : nullptr;
        q.Q_out = dev(lay.Q) + (size_t)j * prow;
        for (int i = 0; i < S; ++i) q.s[i] = c.S[(size_t)j * S + i];
        for (int i = 0; i < C; ++i) q.u_prev[i] = c.u_prev ? c.u_prev[(size_t)j * C + i] : 0.0f;
        if (!plant && (j == 0 || b->differ))
            ctk_mppi_batch_derive_k(b->env, b->differ ? b->table(p) : b->params, b->cfg.dt, b->cfg.intermediate_steps, b->h_run + lay.k + (size_t)q.kidx * b->kstride);
    }
    if (host_plans) std::memcpy(b->h_run + lay.plans, c.plans, (size_t)n * prow * sizeof(float));
    RolloutArgs a = batch_common_args(b);
    for (int i = 0; i < C; ++i) { a.lo[i] = -INFINITY; a.hi[i] = INFINITY; }
    a.N = m;
    const bool generic = b->env != CTK_ENV_CARTPOLE || b->cfg.generic_kernels != 0;
    size_t wstride = 0;
    const float* w_dev = pred != CTK_PRED_ODE ? F::rollout_weights(b, &wstride) : nullptr;
    hipError_t le = plant ? batch_plant_flush(b, sub) : hipSuccess;
    if (le == hipSuccess) le = hipMemcpyAsync(b->d_run, b->h_run, lay.J, hipMemcpyHostToDevice, b->stream);
    if (le == hipSuccess)
        le = ctk_launch_batch_rollout(b->stream, b->env, generic, pred, a, reinterpret_cast<const CtkBatchRolloutRec*>(b->d_run), n, m,
                                      plant ? b->d_kplant : b->d_run + lay.k, b->d_zero_one, w_dev, wstride, want_traj);
    if (le == hipSuccess) le = hipMemcpyAsync(b->h_run + lay.J, b->d_run + lay.J, lay.back - lay.J, hipMemcpyDeviceToHost, b->stream);
    const hipError_t se = hipStreamSynchronize(b->stream);                     // the stagings are free again, whatever happened
    if (le == hipSuccess) le = se;
    if (le != hipSuccess) return bfail(b, CTK_ERR_HIP, who + ": " + hipGetErrorString(le));
    if (c.J_out) std::memcpy(c.J_out, b->h_run + lay.J, (size_t)n * m * sizeof(float));
    if (want_traj) std::memcpy(c.traj_out, b->h_run + lay.traj, (size_t)n * trow * sizeof(float));
    return CTK_OK;
}

// the entry of a family over it
#define CTK_ROLLOUT_ENTRY(FAM, TRAIT)                                                                                                                 \
    int FAM##_rollout(FAM* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,    \
                      int plant_substeps, float* traj_out, float* J_out) {                                                                            \
        return batch_rollout<TRAIT>(b, RolloutCall{#FAM "_rollout", n, ids, S, u_prev, plans, plans_loc, m, model, plant_substeps, traj_out, J_out}); \
    }

// The thirteen entries of a family that are one line over a shared body, FAM in {ctk_batch, ctk_mlp_batch, ctk_gru_batch, ctk_cem_batch, ctk_rpgd_batch}
// with the prefix PROB of its per-problem parameter entries and its trait: the bodies above under the family's names
#define CTK_BATCH_ENTRIES(FAM, PROB, TRAIT)                                                                                                           \
    const char* FAM##_last_error(const FAM* b) { return b ? b->err.c_str() : g_create_error.c_str(); }                                                \
    int FAM##_size(const FAM* b) { return b ? b->B : 0; }                                                                                             \
    const char* FAM##_dominant_kernel(const FAM* b) { return b ? b->dominant.c_str() : ""; }                                                          \
    void FAM##_destroy(FAM* b) { delete b; }                                                                                                          \
    int FAM##_set_param(FAM* b, int id, float value) { return batch_set_param(b, #FAM "_set_param", id, value); }                                     \
    int FAM##_get_param(const FAM* b, int id, float* value) { return batch_get_param(b, id, value); }                                                 \
    int PROB##_set_param(FAM* b, int n_ids, const int32_t* ids, int id, const float* values) {                                                        \
        return batch_problem_set_param<TRAIT>(b, #PROB "_set_param", n_ids, ids, id, values);                                                         \
    }                                                                                                                                                 \
    int PROB##_get_param(const FAM* b, int problem, int id, float* value) { return batch_problem_get_param(b, problem, id, value); }                  \
    int PROB##_params_differ(const FAM* b) { return batch_params_differ(b); }                                                                         \
    int FAM##_rng_get_position(const FAM* b, int problem, uint32_t* call) { return batch_rng_get_position(b, problem, call); }                        \
    int FAM##_rng_set_position(FAM* b, int problem, uint32_t call) { return batch_rng_set_position(b, #FAM "_rng_set_position", problem, call); }     \
    int FAM##_get_state(FAM* b, int problem, float* dst, size_t cap) { return batch_state_io<TRAIT>(b, #FAM "_get_state", problem, dst, cap, true); } \
    int FAM##_set_state(FAM* b, int problem, const float* src, size_t n) {                                                                            \
        return batch_state_io<TRAIT>(b, #FAM "_set_state", problem, const_cast<float*>(src), n, false);                                               \
    }

// The fourteen closed-loop entries of a family, FAM and its trait as above: the bodies above under the family's names
#define CTK_LOOP_ENTRIES(FAM, TRAIT)                                                                                                                  \
    int FAM##_plant_set_param(FAM* b, int n_ids, const int32_t* ids, int id, const float* values) {                                                   \
        return plant_set_param(b, #FAM "_plant_set_param", n_ids, ids, id, values);                                                                   \
    }                                                                                                                                                 \
    int FAM##_plant_get_param(const FAM* b, int problem, int id, float* value) { return plant_get_param(b, problem, id, value); }                     \
    int FAM##_plant_clear_params(FAM* b) { return plant_clear_params(b); }                                                                            \
    int FAM##_plant_step(FAM* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps, float* s_next) {                        \
        if (!b) return CTK_ERR_INVALID_ARGUMENT;                                                                                                      \
        if (!s || !u || !s_next) return bfail(b, CTK_ERR_INVALID_ARGUMENT, #FAM "_plant_step: NULL state, input or destination");                     \
        return batch_plant_step<TRAIT>(b, #FAM "_plant_step", n_ids, ids, s, u, nullptr, substeps, s_next, nullptr, nullptr);                         \
    }                                                                                                                                                 \
    int FAM##_run(FAM* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev, int n_steps, int plant_substeps, float* states_out,    \
                  float* inputs_out, int32_t* first_bad) {                                                                                            \
        if (!b) return CTK_ERR_INVALID_ARGUMENT;                                                                                                      \
        if (!s0 || !states_out || !inputs_out) return bfail(b, CTK_ERR_INVALID_ARGUMENT, #FAM "_run: NULL start states or trace destination");        \
        return batch_closed_loop<TRAIT>(b, LoopCall{#FAM "_run", "a run", n_ids, ids, s0, nullptr, u_prev, n_steps, plant_substeps, states_out,       \
                                                    nullptr, inputs_out, nullptr, first_bad});                                                        \
    }                                                                                                                                                 \
    int FAM##_plant_set_noise(FAM* b, int n_ids, const int32_t* ids, int kind, const float* sigma) {                                                  \
        return plant_set_noise(b, #FAM "_plant_set_noise", n_ids, ids, kind, sigma);                                                                  \
    }                                                                                                                                                 \
    int FAM##_plant_get_noise(const FAM* b, int problem, int kind, float* sigma) { return plant_get_noise(b, problem, kind, sigma); }                 \
    int FAM##_plant_clear_noise(FAM* b) { return plant_clear_noise(b); }                                                                              \
    int FAM##_plant_set_noise_seed(FAM* b, int n_ids, const int32_t* ids, const uint64_t* seeds) {                                                    \
        return plant_set_noise_seed(b, #FAM "_plant_set_noise_seed", n_ids, ids, seeds);                                                              \
    }                                                                                                                                                 \
    int FAM##_plant_get_noise_seed(const FAM* b, int problem, uint64_t* seed) { return plant_get_noise_seed(b, problem, seed); }                      \
    int FAM##_plant_noise_get_position(const FAM* b, int problem, uint32_t* pos) { return plant_noise_get_position(b, problem, pos); }                \
    int FAM##_plant_noise_set_position(FAM* b, int problem, uint32_t pos) {                                                                           \
        return plant_noise_set_position(b, #FAM "_plant_noise_set_position", problem, pos);                                                           \
    }                                                                                                                                                 \
    int FAM##_plant_step_noisy(FAM* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev, int substeps,              \
                               float* s_next, float* y_next, float* cost) {                                                                           \
        if (!b) return CTK_ERR_INVALID_ARGUMENT;                                                                                                      \
        if (!s || !u || !u_prev || !s_next || !y_next || !cost)                                                                                       \
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, #FAM "_plant_step_noisy: NULL state, input, previous input or destination");                    \
        return batch_plant_step<TRAIT>(b, #FAM "_plant_step_noisy", n_ids, ids, s, u, u_prev, substeps, s_next, y_next, cost);                        \
    }                                                                                                                                                 \
    int FAM##_episodes(FAM* b, int n_ids, const int32_t* ids, const float* s0, const float* y0, const float* u_prev, int n_steps, int plant_substeps, \
                       float* states_out, float* obs_out, float* inputs_out, float* costs_out, int32_t* first_bad) {                                  \
        if (!b) return CTK_ERR_INVALID_ARGUMENT;                                                                                                      \
        if (!s0 || !states_out || !obs_out || !inputs_out || !costs_out)                                                                              \
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, #FAM "_episodes: NULL start states or trace destination");                                      \
        return batch_closed_loop<TRAIT>(b, LoopCall{#FAM "_episodes", "an episode", n_ids, ids, s0, y0, u_prev, n_steps, plant_substeps, states_out,  \
                                                    obs_out, inputs_out, costs_out, first_bad});                                                      \
    }

}  // namespace

// =============================================================================================
// Batched MPPI (include/ctk_hip.h: ctk_batch_*): B independent problems of one configuration, stepped by ONE launch of
// ctk_mppi_batch<ENV, LOG> per step (ctk_mppi.hip).  One allocation per buffer kind with a problem stride — no handles inside.
// Per-problem host state is what a handle keeps: the sequence number of its next step, its Philox position, which u_nom buffer is current,
// its parameter table.  While no ctk_problem_set_param has succeeded the launches take the constants of the shared table by value; from
// then on (`differ`, sticky) they read every problem's constants from d_k, which ctk_batch_step refreshes for the problems marked dirty.
// The optimizer's own numbers go the same way (include/ctk_hip_hyper.h): the five MPPI hyper-parameters and the input limits are the
// configuration's until a *_problem_set_hyper / *_problem_set_limits / *_batch_set_hyper has succeeded; from then on (`hyper`, sticky) the
// launches take the _hp form, which reads every problem's constants AND its MppiK and limits from the two-part elements of d_kh (batch_flush_kh).
// =============================================================================================
struct ctk_batch : BatchCore {
    int P = 0, PC = 0, blocks = 0;
    unsigned char* h_k = nullptr;           // pinned [B][kstride] derived constants, the staging of the copy to d_k
    unsigned char* d_k = nullptr;           // [B][kstride]
    MppiK mk{};
    int max_per_launch = 1;                 // problems per launch: half the device's CUs (ctk_batch_create), a diagnostic switch may lower it
    InterpEntry* d_interp = nullptr;
    float* d_parts = nullptr;               // [B][blocks][2+PC]
    unsigned long long* d_ll = nullptr;     // [B][blocks][2+PC] {value, seq} words
    float* d_unom = nullptr;                // [B][2][H,C]
    CtkBatchDesc* d_desc = nullptr;         // [B]
    CtkBatchStep* h_steps = nullptr;        // pinned [B]: the step records of the step being issued
    CtkBatchStep* d_steps = nullptr;        // [B]
    std::vector<int> cur;
    // the MLP family (include/ctk_hip.h: ctk_mlp_batch_*): the same struct with a predictor field and per-problem weight tables
    int pred = CTK_PRED_ODE;                // CTK_PRED_MLP: ctk_mppi_batch_mlp<LOG> / ctk_mppi_batch_mlp_pp<LOG>
    int hid1 = 32, hid2 = 32;               // the network's hidden widths (cfg.predictor_hidden1/2, 0 = 32): narrower ones are embedded
    size_t wtab = 0;                        // floats of one per-lane weight table (ctk_mppi_batch_mlp_table_floats)
    float* d_w = nullptr;                   // [B][wtab] problem p's table, in the layout of a handle's d_wperm
    float* h_w = nullptr;                   // pinned [B][wtab]: the staging of ONE transfer per weight call
    std::vector<unsigned char> have_w;      // [B] the problem has received weights
    // the GRU family (include/ctk_hip.h: ctk_gru_batch_*): pred == CTK_PRED_GRU, ctk_mppi_batch_gru<LOG, FORM> / ctk_mppi_batch_gru_pp<LOG, FORM>.
    // Problem p's block of d_w (wtab floats) is [table (wrow) | carried hidden state (64) | fast-cosine word | pad]: the kernels write
    // the hidden state, so the block has NO host mirror — h_w stages tables alone ([B][wrow]), and every transfer names its part
    int form = 0;                           // CTK_MPPI_FORM_* of every launch: what a handle of this configuration launches (ctk_mppi_batch_gru_fit)
    size_t wrow = 0;                        // floats of the table part of a block (ctk_mppi_batch_gru_table_floats)
    float* h_hid = nullptr;                 // pinned [B][64]: the staging of a hidden-state call (rows by problem id)
    uint32_t* h_flag = nullptr;             // pinned [B]: net_out_bound * hidden_scale <= CTK_SINCOS_FAST_LIMIT, the word of every block
    std::vector<float> net_out_bound;       // [B] what a handle keeps under these names (ctk_api.hip): INFINITY until weights arrive,
    std::vector<float> hidden_scale;        // [B] 1, or max(1, max |h|) of a caller-set hidden state
    // per-problem optimizer hyper-parameters and input limits (include/ctk_hip_hyper.h): the table of primary values, initialised from
    // cfg; `hyper` (sticky, as `differ`) once a setter has succeeded: the _hp form of the kernel from then on, fed from d_kh
    std::vector<float> hyp;                 // [B][HYP_ROW]: the five of enum ctk_hyper | low [CTK_MAX_INPUTS] | high [CTK_MAX_INPUTS]
    std::vector<unsigned char> hdirty;      // [B] the row changed since the problem's element was last derived and copied to d_kh
    bool hyper = false;
    size_t khstride = 0;                    // ctk_mppi_batch_kh_stride(env): bytes of one two-part element [K | CtkBatchHyper]
    unsigned char* h_kh = nullptr;          // pinned [B][khstride]: the staging of the copy to d_kh, and its mirror
    unsigned char* d_kh = nullptr;          // [B][khstride] what the _hp form takes in the place of d_k
    static constexpr int HYP_LOW = CTK_HYPER_COUNT, HYP_HIGH = CTK_HYPER_COUNT + CTK_MAX_INPUTS, HYP_ROW = CTK_HYPER_COUNT + 2 * CTK_MAX_INPUTS;
    float* hrow(int p) { return hyp.data() + (size_t)p * HYP_ROW; }
    const float* hrow(int p) const { return hyp.data() + (size_t)p * HYP_ROW; }
    size_t unom_stride() const { return (size_t)2 * HC; }
    float* unom(int p, int which) const { return d_unom + (size_t)p * unom_stride() + (size_t)which * HC; }
};

namespace {

// the shared template of a launch's RolloutArgs (ctk_api.hip: make_args without what the step records and descriptors supply)
RolloutArgs batch_args(const ctk_batch* b) {
    RolloutArgs a = batch_common_args(b);
    a.P = b->P;
    a.p_magic = ctk_magic_of(b->P);
    a.identity_interp = (b->cfg.period_interpolation_inducing_points == 1 && b->P == b->H) ? 1 : 0;
    a.interp = b->d_interp;
    return a;
}

// The per-problem form's constants: re-derive those of every dirty problem (stepped now or not) with the function a handle uses
// (ctk_set_param -> derive_constants / Env<>::derive at its launch), and copy the span from the first to the last dirty problem in ONE
// transfer on the batch's stream; no transfer when nothing is dirty.  h_k mirrors d_k, so what lies between two dirty problems is current.
// The caller synchronises before it returns (ctk_batch_step), so the staging is free again at the next call.
hipError_t batch_flush_constants(ctk_batch* b) {
    int lo = b->B, hi = -1;
    for (int p = 0; p < b->B; ++p) {
        if (!b->dirty[(size_t)p]) continue;
        ctk_mppi_batch_derive_k(b->env, b->table(p), b->cfg.dt, b->cfg.intermediate_steps, b->h_k + (size_t)p * b->kstride);
        b->dirty[(size_t)p] = 0;
        lo = std::min(lo, p); hi = p;
    }
    if (hi < 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(b->d_k + (size_t)lo * b->kstride, b->h_k + (size_t)lo * b->kstride, (size_t)(hi - lo + 1) * b->kstride,
                                        hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess) for (int p = lo; p <= hi; ++p) b->dirty[(size_t)p] = 1;       // nothing reached the device: derive and copy again
    return e;
}

// the five hyper-parameters of a configuration in the order of enum ctk_hyper, and back into a copy of it
void hyper_from_config(const ctk_config& c, float* v) {
    v[CTK_HYPER_CC_WEIGHT] = c.cc_weight; v[CTK_HYPER_R] = c.R; v[CTK_HYPER_LBD] = c.LBD; v[CTK_HYPER_NU] = c.NU; v[CTK_HYPER_SQRTRHOINV] = c.SQRTRHOINV;
}
void hyper_into_config(const float* v, ctk_config* c) {
    c->cc_weight = v[CTK_HYPER_CC_WEIGHT]; c->R = v[CTK_HYPER_R]; c->LBD = v[CTK_HYPER_LBD]; c->NU = v[CTK_HYPER_NU]; c->SQRTRHOINV = v[CTK_HYPER_SQRTRHOINV];
}

// The _hp form's per-problem array, by the scheme of batch_flush_constants.  Element p is [K | CtkBatchHyper]: the first part is
// re-derived where the problem's parameter table changed (`dirty`, with the function a handle uses), the second where its
// hyper-parameters or limits did (`hdirty`: MppiK by mppi_constants, the function behind a handle's, on a copy of the configuration
// that carries the problem's values); the span from the first to the last such problem (stepped now or not) travels in ONE transfer
// on the batch's stream, none when nothing changed.  h_kh mirrors d_kh.  The caller synchronises before it returns, so the staging
// is free again at the next call.
hipError_t batch_flush_kh(ctk_batch* b) {
    int lo = b->B, hi = -1;
    for (int p = 0; p < b->B; ++p) {
        if (!b->dirty[(size_t)p] && !b->hdirty[(size_t)p]) continue;
        unsigned char* elem = b->h_kh + (size_t)p * b->khstride;
        if (b->dirty[(size_t)p]) ctk_mppi_batch_derive_k(b->env, b->table(p), b->cfg.dt, b->cfg.intermediate_steps, elem);
        if (b->hdirty[(size_t)p]) {
            const float* row = b->hrow(p);
            ctk_config c = b->cfg;
            hyper_into_config(row, &c);
            CtkBatchHyper e{};
            e.m = mppi_constants(c);
            for (int i = 0; i < CTK_MAX_INPUTS; ++i) { e.lo[i] = row[ctk_batch::HYP_LOW + i]; e.hi[i] = row[ctk_batch::HYP_HIGH + i]; }
            std::memcpy(elem + b->kstride, &e, sizeof(e));
        }
        b->dirty[(size_t)p] = 0; b->hdirty[(size_t)p] = 0;
        lo = std::min(lo, p); hi = p;
    }
    if (hi < 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(b->d_kh + (size_t)lo * b->khstride, b->h_kh + (size_t)lo * b->khstride, (size_t)(hi - lo + 1) * b->khstride,
                                        hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess) for (int p = lo; p <= hi; ++p) b->dirty[(size_t)p] = b->hdirty[(size_t)p] = 1;   // nothing reached the device: derive and copy again
    return e;
}

// The controller launches of n step records from steps_dev on (ctk_batch_step; every step of ctk_batch_run): consecutive launches of at
// most max_per_launch problems — the results do not depend on the split.  *launched: the records that were launched.
hipError_t batch_launch_records(ctk_batch* b, const RolloutArgs& a, const CtkBatchStep* steps_dev, int n, int* launched) {
    const bool log = b->cfg.materialize_trajectories != 0;
    hipError_t le = hipSuccess;
    *launched = 0;
    const void* d_k = b->hyper ? b->d_kh : b->differ ? b->d_k : nullptr;     // the _hp form: the two-part elements in d_k's place
    while (le == hipSuccess && *launched < n) {
        const int cnt = std::min(b->max_per_launch, n - *launched);
        if (b->pred == CTK_PRED_GRU)
            le = ctk_launch_mppi_batch_gru(b->stream, b->params, b->cfg.dt, b->cfg.intermediate_steps, a, b->mk, b->d_desc, steps_dev + *launched, cnt, log,
                                           b->form, b->d_w, d_k, b->hyper);
        else if (b->pred == CTK_PRED_MLP)
            le = ctk_launch_mppi_batch_mlp(b->stream, b->params, b->cfg.dt, b->cfg.intermediate_steps, a, b->mk, b->d_desc, steps_dev + *launched, cnt, log,
                                           b->d_w, d_k, b->hyper);
        else
            le = ctk_launch_mppi_batch(b->stream, b->env, b->params, b->cfg.dt, b->cfg.intermediate_steps, a, b->mk, b->d_desc, steps_dev + *launched, cnt, log,
                                       d_k, b->hyper);
        if (le == hipSuccess) *launched += cnt;
    }
    return le;
}

// optimizer_reset() of problem p (ctk_reset of an MPPI handle): the plan at mid-range in buffer 0; u, the Philox position stay
int batch_reset_one(ctk_batch* b, int p) {
    std::vector<float> tmp((size_t)b->HC);
    const float* row = b->hrow(p);                     // the problem's own limits (the configuration's until *_problem_set_limits)
    for (int i = 0; i < b->HC; ++i) tmp[(size_t)i] = 0.5f * (row[ctk_batch::HYP_LOW + i % b->C] + row[ctk_batch::HYP_HIGH + i % b->C]);
    b->cur[(size_t)p] = 0;
    BHIP_TRY(b, hipMemcpyAsync(b->unom(p, 0), tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    return CTK_OK;
}

// what a step record says of the step that problem p takes t steps from now (ctk_batch_step: t == 0; a segment of the closed loop: t in
// [0, L)): its counters, and no draws.  The state and the previous input are the caller's.
void batch_fill_record(const ctk_batch* b, CtkBatchStep& q, int p, int t) {
    q.id = p; q.seq = b->seq[(size_t)p] + (uint32_t)t; q.call = b->call[(size_t)p] + (uint32_t)t;
    q.cur = (uint32_t)(b->cur[(size_t)p] ^ (t & 1));
    q.pad = 0u; q.samples = nullptr;
}

// the MPPI family's part of the drivers (the trait of batch_step and batch_closed_loop, above)
struct MppiFamily {
    using Batch = ctk_batch;
    using Rec = CtkBatchStep;
    static constexpr bool carries_k = false, error_word = true, device_ahead_of_draws = true, state_size_named = false;
    static constexpr const char* handoff_outputs = "; their outputs are NaN, the other problems' outputs are valid and written";   // this family's text alone says "their outputs are NaN"
    static int refuse(Batch*, const char*, int, const int32_t*) { return CTK_OK; }       // (the MLP family's missing weights: MlpFamily)
    static size_t draws_of(const Batch* b, int) { return (size_t)b->N * b->PC; }
    static int check_draws(Batch* b, const char*, int, const int32_t*, const StepDraws& d, size_t) { return batch_check_draws(b, d); }
    static const float*& draws(Rec& q) { return q.samples; }
    static RolloutArgs context(const Batch* b) { return batch_args(b); }
    // (the _hp form reads every problem's k too, from d_kh: entering it marks them all dirty, hyper_enter)
    static hipError_t constants(Batch* b, const int32_t*, int, unsigned char*) {
        return b->hyper ? batch_flush_kh(b) : b->differ ? batch_flush_constants(b) : hipSuccess;
    }
    static void fill(const Batch* b, Rec& q, int p, int t) { batch_fill_record(b, q, p, t); }
    static hipError_t launch(Batch* b, const RolloutArgs& a, const Rec* d_rec, int n, const unsigned char*, int* launched) {
        return batch_launch_records(b, a, d_rec, n, launched);
    }
    // The counter rule: every listed problem, launched or not, consumes its sequence number (ctk_api.hip: guarded(); as CEM, RPGD
    // differs on purpose); its Philox position and plan buffer only if launched
    static void advance(Batch* b, int p, int ctrl, bool tried, bool issued) {
        const size_t z = (size_t)p;
        b->seq[z] += (uint32_t)ctrl; b->call[z] += (uint32_t)ctrl; b->cur[z] ^= ctrl & 1;
        if (tried) {
            ++b->seq[z];
            if (issued) { ++b->call[z]; b->cur[z] ^= 1; }
        }
    }
    // A launched step whose slot never shows the step's seq (a device fault).  By history this family's step advances the Philox
    // position and reads u for every launched problem, published or not (CEM and RPGD: only if its slot shows the step's seq); the
    // closed loop does not look per step in any family.
    static constexpr bool unpublished_keeps_position = false;
    // ---- the family's part of batch_rollout ----
    static int rollout_pred(const ctk_batch* b) { return b->pred; }
    static const float* rollout_weights(const ctk_batch* b, size_t* stride) { *stride = b->wtab; return b->d_w; }
    static int rollout_refuse(ctk_batch*, const char*, int, const int32_t*, bool, bool) { return CTK_OK; }   // (missing weights: MlpFamily, GruFamily)
    static const float* own_plan(const ctk_batch* b, int p) { return b->unom(p, b->cur[(size_t)p]); }
    // the state of a problem: its current plan, its last output
    static BatchState state(Batch* b, int p) { return {{state_seg(b->unom(p, b->cur[(size_t)p]), (size_t)b->HC), state_seg(b->u(p), (size_t)b->C)}}; }
    static const char* per_problem_kernel(const Batch* b) {     // (the _hp form stays the _hp form)
        return b->pred == CTK_PRED_GRU ? ctk_mppi_batch_gru_name(b->cfg.materialize_trajectories != 0, b->form, true, b->hyper)
             : b->pred == CTK_PRED_MLP ? ctk_mppi_batch_mlp_name(b->cfg.materialize_trajectories != 0, true, b->hyper)
                                       : ctk_mppi_batch_name(b->env, b->cfg.materialize_trajectories != 0, true, b->hyper);
    }
};

// ctk_batch_create (pred == CTK_PRED_ODE), ctk_mlp_batch_create (CTK_PRED_MLP) and ctk_gru_batch_create (CTK_PRED_GRU) into the caller's fresh struct: the refusals that need
// only the configuration, the device probe, the buffers.  On failure the message is in g_create_error and the caller deletes the struct.
int batch_create_in(ctk_batch* b, const char* who, int pred, const ctk_config* cfg, int n_problems, const uint64_t* seeds) {
    const bool mlp = pred == CTK_PRED_MLP, gru = pred == CTK_PRED_GRU;
    auto refuse = [&](int code, const std::string& msg) { return bfail(nullptr, code, std::string(who) + ": " + msg); };
    if (n_problems < 1) return refuse(CTK_ERR_UNSUPPORTED, "a batch holds at least one problem (n_problems == " + std::to_string(n_problems) + ")");
    const EnvInfo* einfo = nullptr;
    if (int rc = check_config(who, cfg, &einfo)) return rc;
    const int N = cfg->num_rollouts, H = cfg->mpc_horizon, P = num_inducing_points(H, cfg->period_interpolation_inducing_points);
    const int hw1 = cfg->predictor_hidden1 ? cfg->predictor_hidden1 : 32, hw2 = cfg->predictor_hidden2 ? cfg->predictor_hidden2 : 32;
    // the network families' refusals name the sizes refused: population, horizon, inducing points and the network as the reference names it
    const std::string sizes = !(mlp || gru) ? std::string()
        : " (num_rollouts " + std::to_string(N) + ", mpc_horizon " + std::to_string(H) + ", " + std::to_string(P) + " inducing points, network " +
          std::to_string(einfo->S + einfo->C) + "IN-" + std::to_string(hw1) + "H1-" + std::to_string(hw2) + "H2-" + std::to_string(einfo->S) + "OUT)";
    if (cfg->optimizer != CTK_OPT_MPPI)
        return refuse(CTK_ERR_UNSUPPORTED, "a batch steps MPPI controllers only (cfg.optimizer == " + std::to_string(cfg->optimizer) +
                      "); the other optimizers run as single handles (ctk_create)" + sizes);
    if (!mlp && !gru && cfg->predictor != CTK_PRED_ODE)
        return refuse(CTK_ERR_UNSUPPORTED, "the batch kernel rolls out the analytic (ODE) predictor only (cfg.predictor == " +
                      std::to_string(cfg->predictor) + "); network predictors run as single handles (ctk_create)");
    if (mlp) {                                         // this family's own refusals, under its name; the first one names ctk_batch_create
        if (cfg->predictor == CTK_PRED_ODE)
            return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_mlp_batch_create: this family rolls out the MLP predictor (cfg.predictor == " + std::to_string(cfg->predictor) +
                         " is the analytic one: use ctk_batch_create)" + sizes);
        if (cfg->predictor != CTK_PRED_MLP)
            return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_mlp_batch_create: this family rolls out the MLP predictor only (cfg.predictor == " + std::to_string(cfg->predictor) +
                         "); the GRU's carried hidden state has no batch form, such a controller runs as a single handle (ctk_create)" + sizes);
        if (cfg->environment != CTK_ENV_CARTPOLE || cfg->generic_kernels != 0)
            return bfail(nullptr, CTK_ERR_UNSUPPORTED, std::string("ctk_mlp_batch_create: the batch kernel is CartPole's matrix-core MLP kernel (environment ") + einfo->name +
                         ", generic_kernels == " + std::to_string(cfg->generic_kernels) + "): such handles run the one-wave template network kernels, which have no batch form (ctk_create)" + sizes);
        if (hw1 < 1 || hw2 < 1) return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_mlp_batch_create: predictor_hidden1 / predictor_hidden2 must be >= 1 (0 = 32)");
        if (std::max(hw1, hw2) > 32)
            return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_mlp_batch_create: the batch kernel holds 32 units per hidden layer (narrower layers are embedded exactly); wider "
                         "networks run the 64-unit template kernels, which have no batch form (ctk_create)" + sizes);
    }
    if (gru) {                                         // the GRU family's refusals: every one CTK_ERR_UNSUPPORTED, each other predictor's names its family
        if (cfg->predictor == CTK_PRED_ODE)
            return refuse(CTK_ERR_UNSUPPORTED, "this family rolls out the GRU predictor (cfg.predictor == " + std::to_string(cfg->predictor) +
                          " is the analytic one: use ctk_batch_create)" + sizes);
        if (cfg->predictor == CTK_PRED_MLP)
            return refuse(CTK_ERR_UNSUPPORTED, "this family rolls out the GRU predictor (cfg.predictor == " + std::to_string(cfg->predictor) +
                          " is the MLP: use ctk_mlp_batch_create)" + sizes);
        if (cfg->predictor != CTK_PRED_GRU)
            return refuse(CTK_ERR_UNSUPPORTED, "this family rolls out the GRU predictor only (cfg.predictor == " + std::to_string(cfg->predictor) + ")" + sizes);
        if (cfg->environment != CTK_ENV_CARTPOLE || cfg->generic_kernels != 0)
            return refuse(CTK_ERR_UNSUPPORTED, std::string("the batch kernel is CartPole's four-wave matrix-core GRU kernel (environment ") + einfo->name +
                          ", generic_kernels == " + std::to_string(cfg->generic_kernels) + "): such handles run the template network kernels, which have no batch form (ctk_create)" + sizes);
        if (hw1 < 1 || hw2 < 1 || std::max(hw1, hw2) > 32)
            return refuse(CTK_ERR_UNSUPPORTED, "the batch kernel holds 1 to 32 units per hidden layer (narrower layers are embedded exactly); no GRU kernel is "
                          "built for other widths" + sizes);
    }
    if (!(cfg->LBD > 0.0f && cfg->NU != 0.0f)) return refuse(CTK_ERR_INVALID_ARGUMENT, "MPPI needs LBD > 0 and NU != 0");
    size_t lds = 0;
    int blocks = 0, form = 0;
    if (const int why = gru ? ctk_mppi_batch_gru_fit(N, H, P, &lds, &blocks, &form)
                      : mlp ? ctk_mppi_batch_mlp_fit(N, H, P, &lds, &blocks) : ctk_mppi_batch_fit(cfg->environment, N, H, P, &lds, &blocks)) {
        const std::string sizes = "num_rollouts " + std::to_string(N) + ", mpc_horizon " + std::to_string(H) + ", " + std::to_string(P) + " inducing points x " +
                                  std::to_string(einfo->C) + " inputs = " + std::to_string(blocks) + " block records of " + std::to_string(2 + P * einfo->C) + " words";
        const char* reason = why == 1 ? (mlp ? ": a handle of this size does not run the pair form of the MLP kernel (more than 8192 rollouts, or CTK_MPPI_NO_PAIR is set), the only one a batch has"
                                             : ": populations from 32768 rollouts on run the throughput kernels, which a batch does not have")
                           : why == 2 ? (gru ? ": a handle of this size does not hand its block records over in-launch (more than 128 records that hold more than 4096 words, or more "
                                               "than 512 records) but runs rollout, merge and update as separate launches, a path the batch does not have"
                                             : ": the batch kernel has the narrow in-launch hand-off only (at most 128 records and 2048 record words per problem)")
                           : why == 3 ? ": the block records do not fit the hand-off's LDS staging"
                                      : ": the rollout tiles need more than 160 KiB of LDS";
        return refuse(CTK_ERR_UNSUPPORTED, "per-problem population outside the batch kernel's sizes (" + sizes + ")" + reason +
                      (why == 4 ? " (" + std::to_string(lds) + " bytes)" : std::string()) + "; such a controller runs as a single handle (ctk_create)");
    }

    hipDeviceProp_t prop;
    if (int rc = probe_device(who, cfg->device, &prop)) return rc;

    batch_core_init(b, cfg, einfo, n_problems, seeds);        // dirty: no constants in d_k yet, the first step of the per-problem form derives them all
    b->pred = pred; b->hid1 = hw1; b->hid2 = hw2; b->form = form;
    b->P = P; b->PC = P * b->C; b->blocks = blocks;
    b->mk = mppi_constants(b->cfg);
    b->hyp.assign((size_t)n_problems * ctk_batch::HYP_ROW, 0.0f);
    for (int p = 0; p < n_problems; ++p) {
        hyper_from_config(b->cfg, b->hrow(p));
        for (int c = 0; c < b->C; ++c) { b->hrow(p)[ctk_batch::HYP_LOW + c] = cfg->action_low[c]; b->hrow(p)[ctk_batch::HYP_HIGH + c] = cfg->action_high[c]; }
    }
    b->hdirty.assign((size_t)n_problems, 1);               // nothing in d_kh yet: the first step of the _hp form derives them all
    // Progress: the only workgroup of a launch that ever waits is block 0 of a problem, for workgroups of its own problem.  With at most
    // CUs / 2 problems in a launch the waiting workgroups cannot fill the machine (every CU holds at least one workgroup of this kernel),
    // so every other workgroup finds a place whatever the dispatch order.  CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH (diagnostic) only lowers it.
    b->max_per_launch = std::max(1, prop.multiProcessorCount / 2);
    batch_env_lowers("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH", &b->max_per_launch);
    b->cur.assign((size_t)n_problems, 0);
    b->dominant = gru ? ctk_mppi_batch_gru_name(cfg->materialize_trajectories != 0, form)
                : mlp ? ctk_mppi_batch_mlp_name(cfg->materialize_trajectories != 0) : ctk_mppi_batch_name(b->env, cfg->materialize_trajectories != 0);
    if (mlp) { b->wtab = b->wrow = ctk_mppi_batch_mlp_table_floats(); b->have_w.assign((size_t)n_problems, 0); }
    if (gru) {
        b->wtab = ctk_mppi_batch_gru_block_floats(); b->wrow = ctk_mppi_batch_gru_table_floats(); b->have_w.assign((size_t)n_problems, 0);
        b->net_out_bound.assign((size_t)n_problems, INFINITY); b->hidden_scale.assign((size_t)n_problems, 1.0f);
    }

    if (int rc = batch_core_open(b)) return rc;
    const size_t Bz = (size_t)n_problems, rec = (size_t)blocks * (2 + b->PC);
    HIP_CREATE(b->own.dev_zero(&b->d_interp, (size_t)H * sizeof(InterpEntry), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_J, Bz * N * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_Q, Bz * N * b->HC * sizeof(float), b->stream));
    if (cfg->materialize_trajectories) HIP_CREATE(b->own.dev_zero(&b->d_traj, Bz * N * (H + 1) * b->S * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_parts, Bz * rec * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_ll, Bz * rec * sizeof(unsigned long long), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_unom, Bz * b->unom_stride() * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_desc, Bz * sizeof(CtkBatchDesc), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_steps, Bz * sizeof(CtkBatchStep), b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_steps, Bz * sizeof(CtkBatchStep)));
    HIP_CREATE(b->own.dev_zero(&b->d_k, Bz * b->kstride, b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_k, Bz * b->kstride));
    b->khstride = ctk_mppi_batch_kh_stride(b->env);
    HIP_CREATE(b->own.dev_zero(&b->d_kh, Bz * b->khstride, b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_kh, Bz * b->khstride));
    if (mlp || gru) {
        HIP_CREATE(b->own.dev_zero(&b->d_w, Bz * b->wtab * sizeof(float), b->stream));
        HIP_CREATE(b->own.pinned_zero(&b->h_w, Bz * b->wrow * sizeof(float)));
    }
    if (gru) {
        HIP_CREATE(b->own.pinned_zero(&b->h_hid, Bz * ctk_mppi_batch_gru_hidden_floats() * sizeof(float)));
        HIP_CREATE(b->own.pinned_zero(&b->h_flag, Bz * sizeof(uint32_t)));
    }

    const std::vector<InterpEntry> tab = build_interp_table(H, cfg->period_interpolation_inducing_points, P);
    std::vector<CtkBatchDesc> desc(Bz);
    std::vector<float> plan(Bz * b->unom_stride(), 0.0f);          // optimizer_reset(): buffer 0 of every problem at mid-range
    for (int p = 0; p < n_problems; ++p) {
        const size_t z = (size_t)p;
        const uint64_t seed = batch_seed(cfg, seeds, p);
        CtkBatchDesc& d = desc[z];
        d.parts = b->d_parts + z * rec; d.ll = b->d_ll + z * rec;
        d.J = b->d_J + z * N; d.Q_out = b->d_Q + z * N * b->HC;
        d.traj_out = b->d_traj ? b->d_traj + z * N * (H + 1) * b->S : nullptr;
        d.unom[0] = b->unom(p, 0); d.unom[1] = b->unom(p, 1);
        d.u_dev = b->d_u + z * CTK_MAX_INPUTS; d.u_host = b->h_u_dev + z * 16;
        d.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull); d.seed_hi = (uint32_t)(seed >> 32);
        for (int i = 0; i < b->HC; ++i) plan[z * b->unom_stride() + i] = 0.5f * (cfg->action_low[i % b->C] + cfg->action_high[i % b->C]);
    }
    HIP_CREATE(hipMemcpyAsync(b->d_interp, tab.data(), (size_t)H * sizeof(InterpEntry), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_desc, desc.data(), Bz * sizeof(CtkBatchDesc), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_unom, plan.data(), plan.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipStreamSynchronize(b->stream));               // the host vectors go out of scope below
    return CTK_OK;
}

// *_create of the family's three forms (FAM: ctk_batch, ctk_mlp_batch, ctk_gru_batch)
template <class FAM>
int mppi_batch_create(const char* who, int pred, const ctk_config* cfg, int n_problems, const uint64_t* seeds, FAM** out) {
    if (out) *out = nullptr;
    if (!cfg || !out) return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
    FAM* b = new FAM();
    if (int rc = batch_create_in(b, who, pred, cfg, n_problems, seeds)) { delete b; return rc; }
    *out = b;
    return CTK_OK;
}

// *_reset: optimizer_reset() of the listed problems
int mppi_batch_reset(ctk_batch* b, const char* who, int n_ids, const int32_t* ids) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    for (int j = 0; j < n; ++j)
        if (int rc = batch_reset_one(b, ids ? ids[j] : j)) return rc;
    return CTK_OK;
}

int mppi_batch_read(ctk_batch* b, const char* who, int problem, int buffer, float* dst, size_t cap) {
    if (int rc = batch_read_check(b, who, problem, dst)) return rc;
    const float* src = nullptr; size_t n = 0;
    if (int rc = batch_locate_rollouts(b, who, problem, buffer, &src, &n)) return rc;
    if (!src) {
        if (buffer != CTK_BUF_U_NOM) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": a batch has Q, J, TRAJ and U_NOM");
        src = b->unom(problem, b->cur[(size_t)problem]); n = (size_t)b->HC;
    }
    return batch_read_out(b, who, src, n, false, dst, cap);
}

// ---- per-problem hyper-parameters and limits (include/ctk_hip_hyper.h): the bodies of the three forms' entries; `who` is the entry's name ----
// the rules ctk_batch_create applies to the same fields (check_config, batch_create_in), and finiteness
int hyper_check(ctk_batch* b, const char* who, int hyper, float v, int p) {
    static const char* const names[CTK_HYPER_COUNT] = {"cc_weight", "R", "LBD", "NU", "SQRTRHOINV"};
    const char* why = !std::isfinite(v) ? ": a hyper-parameter is finite"
                    : hyper == CTK_HYPER_LBD && !(v > 0.0f) ? ": MPPI needs LBD > 0"
                    : hyper == CTK_HYPER_NU && v == 0.0f ? ": MPPI needs NU != 0" : nullptr;
    if (!why) return CTK_OK;                           // the text is built for a refused value only
    return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + why + " (" + names[hyper] + " == " + std::to_string(v) + " for problem " + std::to_string(p) +
                 "); nothing was written");
}
// the first successful setter: the _hp form from now on (sticky)
void hyper_enter(ctk_batch* b) {
    if (b->hyper) return;
    b->hyper = true;
    b->dominant = MppiFamily::per_problem_kernel(b);
    std::fill(b->dirty.begin(), b->dirty.end(), (unsigned char)1);            // every problem's k into d_kh, whatever d_k holds
    std::fill(b->hdirty.begin(), b->hdirty.end(), (unsigned char)1);
}
// values == NULL: `all` for every listed problem (the whole-batch entry)
int batch_set_hyper(ctk_batch* b, const char* who, int n_ids, const int32_t* ids, int hyper, const float* values, float all) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (hyper < 0 || hyper >= CTK_HYPER_COUNT)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown hyper-parameter " + std::to_string(hyper) + " (enum ctk_hyper: cc_weight, R, LBD, NU, SQRTRHOINV)");
    for (int j = 0; j < n; ++j)
        if (int rc = hyper_check(b, who, hyper, values ? values[j] : all, ids ? ids[j] : j)) return rc;
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        b->hrow(p)[hyper] = values ? values[j] : all;
        b->hdirty[(size_t)p] = 1;                      // derived and copied ahead of the next step's launches (batch_flush_kh)
    }
    hyper_enter(b);
    return CTK_OK;
}
int batch_problem_set_hyper(ctk_batch* b, const char* who, int n_ids, const int32_t* ids, int hyper, const float* values) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (!values) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL values (one value per listed problem)");
    return batch_set_hyper(b, who, n_ids, ids, hyper, values, 0.0f);
}
int batch_problem_get_hyper(const ctk_batch* b, int problem, int hyper, float* out) {
    if (!b || !out || problem < 0 || problem >= b->B || hyper < 0 || hyper >= CTK_HYPER_COUNT) return CTK_ERR_INVALID_ARGUMENT;
    *out = b->hrow(problem)[hyper];
    return CTK_OK;
}
int batch_problem_set_limits(ctk_batch* b, const char* who, int n_ids, const int32_t* ids, const float* low, const float* high) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (!low || !high) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL limits (one row of num_control_inputs values per listed problem)");
    for (int i = 0; i < n * b->C; ++i) {
        const bool finite = std::isfinite(low[i]) && std::isfinite(high[i]);
        if (finite && low[i] <= high[i]) continue;
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + (finite ? ": action_low must be <= action_high for every control input" : ": a limit is finite") +
                     " (" + std::to_string(low[i]) + ", " + std::to_string(high[i]) + " for problem " + std::to_string(ids ? ids[i / b->C] : i / b->C) +
                     ", input " + std::to_string(i % b->C) + "); nothing was written");
    }
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        for (int c = 0; c < b->C; ++c) {
            b->hrow(p)[ctk_batch::HYP_LOW + c] = low[(size_t)j * b->C + c];
            b->hrow(p)[ctk_batch::HYP_HIGH + c] = high[(size_t)j * b->C + c];
        }
        b->hdirty[(size_t)p] = 1;
    }
    hyper_enter(b);
    return CTK_OK;
}
int batch_problem_get_limits(const ctk_batch* b, int problem, float* low, float* high) {
    if (!b || !low || !high || problem < 0 || problem >= b->B) return CTK_ERR_INVALID_ARGUMENT;
    std::memcpy(low, b->hrow(problem) + ctk_batch::HYP_LOW, (size_t)b->C * sizeof(float));
    std::memcpy(high, b->hrow(problem) + ctk_batch::HYP_HIGH, (size_t)b->C * sizeof(float));
    return CTK_OK;
}

}  // namespace

// =============================================================================================
// Batched MPPI with the MLP predictor (include/ctk_hip.h: ctk_mlp_batch_* / ctk_mlp_problem_*): the ctk_batch above with pred == CTK_PRED_MLP
// — the same struct, step records, completion poll, constants flush, reset and read paths — launched as ctk_mppi_batch_mlp<LOG> /
// ctk_mppi_batch_mlp_pp<LOG>, plus what a learned plant adds: one per-lane weight table per problem (d_w [B][wtab], permute_mlp_weights as
// for a handle's d_wperm), written by ctk_mlp_batch_set_weights / ctk_mlp_problem_set_weights through ONE transfer per call, and
// `have_w`, without which a problem is not stepped (MlpFamily::refuse: its one difference from MppiFamily).  Its entries come from the
// macros that write ctk_batch's, under its own names.
// =============================================================================================
struct ctk_mlp_batch : ctk_batch {};

namespace {

size_t mlp_batch_weight_count(const ctk_batch* b) { return shaped_weight_count(CTK_PRED_MLP, b->S, b->C, b->hid1, b->hid2); }

// tables of the n listed problems (ids == NULL: problems 0 .. n-1) from w [n][cnt] (each_own) or from the one network w [cnt]: permuted
// into the pinned staging at the problems' places, then the span from the first to the last listed problem in ONE transfer.  The staging
// mirrors d_w (both start as zeros and change only here), so what lies between two listed problems is rewritten with what it holds.
int mlp_batch_put_weights(ctk_batch* b, int n, const int32_t* ids, const float* w, size_t cnt, bool each_own) {
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    std::vector<float> full(weight_count(CTK_PRED_MLP, b->S, b->C, 32));
    std::vector<float> perm;
    for (int j = 0; j < n; ++j) {
        if (j == 0 || each_own) {
            const float* src = w + (each_own ? (size_t)j * cnt : 0);
            if (b->hid1 == 32 && b->hid2 == 32) perm = permute_mlp_weights(src, b->S, b->C);
            else {
                std::fill(full.begin(), full.end(), 0.0f);
                embed_mlp_rows(src, b->S, b->S + b->C, b->hid1, b->hid2, 32, full.data());
                perm = permute_mlp_weights(full.data(), b->S, b->C);
            }
        }
        std::memcpy(b->h_w + (size_t)(ids ? ids[j] : j) * b->wtab, perm.data(), b->wtab * sizeof(float));
    }
    const int lo = ids ? ids[0] : 0, hi = ids ? ids[n - 1] : n - 1;         // (ids are ascending: batch_ids)
    BHIP_TRY(b, hipMemcpyAsync(b->d_w + (size_t)lo * b->wtab, b->h_w + (size_t)lo * b->wtab, (size_t)(hi - lo + 1) * b->wtab * sizeof(float),
                               hipMemcpyHostToDevice, b->stream));
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < n; ++j) b->have_w[(size_t)(ids ? ids[j] : j)] = 1;
    return CTK_OK;
}

// the MPPI family under the MLP family's names, and its one refusal: a problem without a network is not stepped, and then none of the
// listed ones is: nothing is launched, no plan, output or Philox position moves (a handle's ctk_step fails the same way: check_predictor)
struct MlpFamily : MppiFamily {
    using Batch = ctk_mlp_batch;
    static int refuse(ctk_batch* b, const char* who, int n, const int32_t* ids) {
        std::string missing;
        for (int j = 0; j < n; ++j) {
            const int p = ids ? ids[j] : j;
            if (!b->have_w[(size_t)p]) list_problem(missing, p);
        }
        if (!missing.empty())
            return bfail(b, CTK_ERR_STATE, std::string(who) + ": no network weights for problem(s) " + missing +
                         " (ctk_mlp_batch_set_weights / ctk_mlp_problem_set_weights before stepping); nothing was launched");
        return CTK_OK;
    }
    // a rollout through the network needs it; one through the analytic plant (model = plant) does not
    static int rollout_refuse(ctk_batch* b, const char* who, int n, const int32_t* ids, bool, bool net) { return net ? refuse(b, who, n, ids) : CTK_OK; }
};

}  // namespace

extern "C" {

// create, samples_needed, step, reset and read of the family's three forms, FAM in {ctk_batch, ctk_mlp_batch, ctk_gru_batch}, and the six
// hyper-parameter entries of include/ctk_hip_hyper.h under the prefix PROB of its per-problem entries
#define CTK_MPPI_ENTRIES(FAM, PROB, TRAIT, PRED)                                                                                                            \
    int FAM##_create(const ctk_config* cfg, int n_problems, const uint64_t* seeds, FAM** out) {                                                       \
        return mppi_batch_create(#FAM "_create", PRED, cfg, n_problems, seeds, out);                                                                  \
    }                                                                                                                                                 \
    size_t FAM##_samples_needed(const FAM* b) { return b ? (size_t)b->N * b->PC : 0; }                                                                \
    int FAM##_step(FAM* b, int n_ids, const int32_t* ids, const float* s, const float* u_prev, const float* samples, int samples_loc, float* u_out) { \
        return batch_step<TRAIT>(b, #FAM "_step", n_ids, ids, s, u_prev, StepDraws{samples, 0, samples_loc}, u_out);                                  \
    }                                                                                                                                                 \
    int FAM##_reset(FAM* b, int n_ids, const int32_t* ids) { return mppi_batch_reset(b, #FAM "_reset", n_ids, ids); }                                 \
    int FAM##_read(FAM* b, int problem, int buffer, float* dst, size_t cap) { return mppi_batch_read(b, #FAM "_read", problem, buffer, dst, cap); } \
    int PROB##_set_hyper(FAM* b, int n_ids, const int32_t* ids, int hyper, const float* values) {                                                     \
        return batch_problem_set_hyper(b, #PROB "_set_hyper", n_ids, ids, hyper, values);                                                             \
    }                                                                                                                                                 \
    int PROB##_get_hyper(const FAM* b, int problem, int hyper, float* out) { return batch_problem_get_hyper(b, problem, hyper, out); }                \
    int PROB##_set_limits(FAM* b, int n_ids, const int32_t* ids, const float* low, const float* high) {                                               \
        return batch_problem_set_limits(b, #PROB "_set_limits", n_ids, ids, low, high);                                                               \
    }                                                                                                                                                 \
    int PROB##_get_limits(const FAM* b, int problem, float* low, float* high) { return batch_problem_get_limits(b, problem, low, high); }             \
    int PROB##_hypers_differ(const FAM* b) { return b && b->hyper ? 1 : 0; }                                                                          \
    int FAM##_set_hyper(FAM* b, int hyper, float value) { return batch_set_hyper(b, #FAM "_set_hyper", 0, nullptr, hyper, nullptr, value); }

CTK_MPPI_ENTRIES(ctk_batch, ctk_problem, MppiFamily, CTK_PRED_ODE)
CTK_BATCH_ENTRIES(ctk_batch, ctk_problem, MppiFamily)
// the closed loop on the device (include/ctk_hip_run.h: ctk_batch_plant_* / ctk_batch_run) and the stochastic plant with the realised
// cost (include/ctk_hip_episode.h: ctk_batch_plant_*noise* / ctk_batch_plant_step_noisy / ctk_batch_episodes)
CTK_LOOP_ENTRIES(ctk_batch, MppiFamily)
// rollouts of caller-supplied plans (include/ctk_hip_rollout.h), every family by the same macro
CTK_ROLLOUT_ENTRY(ctk_batch, MppiFamily)

// the same under the MLP family's names: the network plans, the plant of its closed loop is the analytic CartPole with the problem's
// parameter table (and the overrides set there)
CTK_MPPI_ENTRIES(ctk_mlp_batch, ctk_mlp_problem, MlpFamily, CTK_PRED_MLP)
CTK_BATCH_ENTRIES(ctk_mlp_batch, ctk_mlp_problem, MlpFamily)
CTK_LOOP_ENTRIES(ctk_mlp_batch, MlpFamily)
CTK_ROLLOUT_ENTRY(ctk_mlp_batch, MlpFamily)

size_t ctk_mlp_batch_weight_count(const ctk_mlp_batch* b) { return b ? mlp_batch_weight_count(b) : 0; }

int ctk_mlp_batch_set_weights(ctk_mlp_batch* b, const float* w, size_t n) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (!w) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_mlp_batch_set_weights: NULL weights");
    if (n != mlp_batch_weight_count(b))
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_mlp_batch_set_weights: expected " + std::to_string(mlp_batch_weight_count(b)) + " floats for the " +
                     std::to_string(b->S + b->C) + "IN-" + std::to_string(b->hid1) + "H1-" + std::to_string(b->hid2) + "H2-" + std::to_string(b->S) +
                     "OUT network (ctk_mlp_batch_weight_count), got " + std::to_string(n));
    return mlp_batch_put_weights(b, b->B, nullptr, w, n, false);
}

int ctk_mlp_problem_set_weights(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* w, size_t n) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int cnt = 0;
    if (int rc = batch_ids(b, "ctk_mlp_problem_set_weights", n_ids, ids, &cnt)) return rc;
    if (!w) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_mlp_problem_set_weights: NULL weights (one network per listed problem)");
    if (n != mlp_batch_weight_count(b))
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_mlp_problem_set_weights: expected " + std::to_string(mlp_batch_weight_count(b)) + " floats per problem for the " +
                     std::to_string(b->S + b->C) + "IN-" + std::to_string(b->hid1) + "H1-" + std::to_string(b->hid2) + "H2-" + std::to_string(b->S) +
                     "OUT network (ctk_mlp_batch_weight_count), got " + std::to_string(n));
    return mlp_batch_put_weights(b, cnt, ids, w, n, true);
}

int ctk_mlp_problem_have_weights(const ctk_mlp_batch* b, int problem) { return (b && problem >= 0 && problem < b->B && b->have_w[(size_t)problem]) ? 1 : 0; }

}  // extern "C"

// =============================================================================================
// Batched MPPI with the GRU predictor (include/ctk_hip.h: ctk_gru_batch_* / ctk_gru_problem_*): the ctk_batch above with pred == CTK_PRED_GRU,
// launched as ctk_mppi_batch_gru<LOG, FORM> / ctk_mppi_batch_gru_pp<LOG, FORM> in the form a handle of the configuration launches, plus
// what a recurrent plant model adds.  Problem p's block of d_w is [per-lane table | carried hidden state | fast-cosine word | pad]
// (ctk_launch.h).  The hidden state is advanced ON THE DEVICE behind every step (ctk_gru_advance_batch, one workgroup per step record,
// issued once behind the step's rollout launches: GruFamily::launch), so the host has no copy of it and no transfer may span a block:
// a weight call moves table parts, zeroes the hidden parts and rewrites the words of the LISTED problems only, by pitched copies, one per
// run of consecutive ids.  The fast-cosine word is the half of a handle's per-step decision (ctk_api.hip: make_args, a.fast_cos_ok) that
// does not depend on the state: net_out_bound * hidden_scale <= CTK_SINCOS_FAST_LIMIT, kept per problem as a handle keeps them; the
// kernel joins it with |s[2]| of the step record, so the decision is also a handle's inside a run, whose states exist on the device only.
// =============================================================================================
struct ctk_gru_batch : ctk_batch {};

namespace {

size_t gru_batch_weight_count(const ctk_batch* b) { return shaped_weight_count(CTK_PRED_GRU, b->S, b->C, b->hid1, b->hid2); }
float* gru_batch_hidden(const ctk_batch* b, int p) { return b->d_w + (size_t)p * b->wtab + b->wrow; }
uint32_t gru_batch_flag(const ctk_batch* b, int p) {
    return b->net_out_bound[(size_t)p] * b->hidden_scale[(size_t)p] <= CTK_SINCOS_FAST_LIMIT ? 1u : 0u;
}

// fn(first problem, count) for every run of consecutive problems among the n listed ones (ids ascending: batch_ids; NULL: all in one run)
template <class Fn>
hipError_t gru_batch_runs(int n, const int32_t* ids, Fn&& fn) {
    for (int j = 0; j < n;) {
        int e = j + 1;
        while (ids && e < n && ids[e] == ids[e - 1] + 1) ++e;
        if (!ids) e = n;
        if (const hipError_t err = fn(ids ? ids[j] : 0, e - j)) return err;
        j = e;
    }
    return hipSuccess;
}

// the hidden rows (h_hid, by problem id) and the fast-cosine words (from the host's bounds) of the listed problems into their blocks
hipError_t gru_batch_send_hidden(ctk_batch* b, int n, const int32_t* ids) {
    const size_t hid = ctk_mppi_batch_gru_hidden_floats() * sizeof(float), pitch = b->wtab * sizeof(float);
    for (int j = 0; j < n; ++j) { const int p = ids ? ids[j] : j; b->h_flag[p] = gru_batch_flag(b, p); }
    return gru_batch_runs(n, ids, [&](int p0, int cnt) {
        hipError_t e = hipMemcpy2DAsync(gru_batch_hidden(b, p0), pitch, b->h_hid + (size_t)p0 * ctk_mppi_batch_gru_hidden_floats(), hid, hid, (size_t)cnt,
                                        hipMemcpyHostToDevice, b->stream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(gru_batch_hidden(b, p0) + ctk_mppi_batch_gru_hidden_floats(), pitch, b->h_flag + p0, sizeof(uint32_t), sizeof(uint32_t),
                                 (size_t)cnt, hipMemcpyHostToDevice, b->stream);
        return e;
    });
}

// networks of the n listed problems (ids == NULL: problems 0 .. n-1) from w [n][cnt] (each_own) or from the one network w [cnt], as
// ctk_set_predictor_weights[_shaped] gives a handle one: the table, a zero hidden state, net_out_bound (hidden_scale stays).  Table parts,
// hidden parts and words of the listed problems only: what lies between two runs of ids is not touched (the other problems' hidden states
// live on the device alone)
int gru_batch_put_weights(ctk_batch* b, int n, const int32_t* ids, const float* w, size_t cnt, bool each_own) {
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const size_t HF = ctk_mppi_batch_gru_hidden_floats();
    std::vector<float> full(weight_count(CTK_PRED_GRU, b->S, b->C, 32));
    std::vector<float> perm, bound((size_t)n);
    const bool narrow = b->hid1 != 32 || b->hid2 != 32;
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        if (j == 0 || each_own) {
            const float* src = w + (each_own ? (size_t)j * cnt : 0);
            if (narrow) {
                std::fill(full.begin(), full.end(), 0.0f);
                embed_gru_rows(src, b->S, b->S + b->C, b->hid1, b->hid2, full.data());
                src = full.data();
            }
            perm = permute_gru_weights(src);
            bound[(size_t)j] = gru_out_bound(src);
        } else bound[(size_t)j] = bound[0];
        std::memcpy(b->h_w + (size_t)p * b->wrow, perm.data(), b->wrow * sizeof(float));
        std::memset(b->h_hid + (size_t)p * HF, 0, HF * sizeof(float));
    }
    const std::vector<float> before = b->net_out_bound;
    for (int j = 0; j < n; ++j) b->net_out_bound[(size_t)(ids ? ids[j] : j)] = bound[(size_t)j];
    const size_t row = b->wrow * sizeof(float), pitch = b->wtab * sizeof(float);
    hipError_t e = gru_batch_runs(n, ids, [&](int p0, int c) {
        return hipMemcpy2DAsync(b->d_w + (size_t)p0 * b->wtab, pitch, b->h_w + (size_t)p0 * b->wrow, row, row, (size_t)c, hipMemcpyHostToDevice, b->stream);
    });
    if (e == hipSuccess) e = gru_batch_send_hidden(b, n, ids);
    const hipError_t se = hipStreamSynchronize(b->stream);                     // the stagings are free again, whatever happened
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) { b->net_out_bound = before; return bfail(b, CTK_ERR_HIP, std::string("the GRU batch's weight transfer: ") + hipGetErrorString(e)); }
    for (int j = 0; j < n; ++j) b->have_w[(size_t)(ids ? ids[j] : j)] = 1;
    return CTK_OK;
}

int gru_batch_weight_args(ctk_batch* b, const char* who, const float* w, size_t n, const char* each) {
    if (!w) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL weights" + each);
    if (n != gru_batch_weight_count(b))
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": expected " + std::to_string(gru_batch_weight_count(b)) + " floats for the GRU-" +
                     std::to_string(b->S + b->C) + "IN-" + std::to_string(b->hid1) + "H1-" + std::to_string(b->hid2) + "H2-" + std::to_string(b->S) +
                     "OUT network (ctk_gru_batch_weight_count), got " + std::to_string(n));
    return CTK_OK;
}

// the MPPI family under the GRU family's names: a problem without a network is not stepped (as the MLP family's), and the launches of a
// step end with the advance of the stepped problems' hidden states
struct GruFamily : MppiFamily {
    using Batch = ctk_gru_batch;
    static int refuse(ctk_batch* b, const char* who, int n, const int32_t* ids) {
        std::string missing;
        for (int j = 0; j < n; ++j) {
            const int p = ids ? ids[j] : j;
            if (!b->have_w[(size_t)p]) list_problem(missing, p);
        }
        if (!missing.empty())
            return bfail(b, CTK_ERR_STATE, std::string(who) + ": no network weights for problem(s) " + missing +
                         " (ctk_gru_batch_set_weights / ctk_gru_problem_set_weights before stepping); nothing was launched, no hidden state moved");
        return CTK_OK;
    }
    // a rollout through the network needs it; one through the analytic plant (model = plant) does not
    static int rollout_refuse(ctk_batch* b, const char* who, int n, const int32_t* ids, bool, bool net) { return net ? refuse(b, who, n, ids) : CTK_OK; }
    // the rollout launches of the n records (split at max_per_launch), then ONE advance of the launched records' hidden states, each by
    // (the state of its record, the u its rollout launch published): mppi_advance_hidden of a handle (ctk_api.hip).  In a closed loop the
    // plant launch follows on the stream and writes the NEXT step's records, so the advance has read this step's state by then
    static hipError_t launch(ctk_batch* b, const RolloutArgs& a, const Rec* d_rec, int n, const unsigned char*, int* launched) {
        hipError_t le = batch_launch_records(b, a, d_rec, n, launched);
        if (*launched > 0) {
            const hipError_t ae = ctk_launch_gru_advance_batch(b->stream, b->d_desc, d_rec, *launched, b->d_w);
            if (le == hipSuccess) le = ae;
        }
        return le;
    }
};

}  // namespace

extern "C" {

// the MPPI family's entries under the GRU family's names; ctk_gru_batch_reset is ctk_reset of an MPPI handle, which leaves the hidden
// state alone; the plant of the closed loop is the analytic CartPole with the problem's parameter table, as for the MLP batch
CTK_MPPI_ENTRIES(ctk_gru_batch, ctk_gru_problem, GruFamily, CTK_PRED_GRU)
CTK_BATCH_ENTRIES(ctk_gru_batch, ctk_gru_problem, GruFamily)
CTK_LOOP_ENTRIES(ctk_gru_batch, GruFamily)
CTK_ROLLOUT_ENTRY(ctk_gru_batch, GruFamily)

int ctk_gru_batch_fit(int num_rollouts, int mpc_horizon, int period, int* blocks, int* record_words, int* wide_tail, size_t* lds_bytes) {
    if (num_rollouts < 1 || mpc_horizon < 1 || period < 1) return CTK_ERR_INVALID_ARGUMENT;
    const int P = num_inducing_points(mpc_horizon, period);
    size_t lds = 0;
    int nb = 0, form = 0;
    const int why = ctk_mppi_batch_gru_fit(num_rollouts, mpc_horizon, P, &lds, &nb, &form);
    if (blocks) *blocks = nb;
    if (record_words) *record_words = 2 + P;
    if (wide_tail) *wide_tail = (!why && (form & CTK_MPPI_FORM_WIDE_TAIL)) ? 1 : 0;
    if (lds_bytes) *lds_bytes = lds;
    return why ? CTK_ERR_UNSUPPORTED : CTK_OK;
}

size_t ctk_gru_batch_weight_count(const ctk_gru_batch* b) { return b ? gru_batch_weight_count(b) : 0; }

int ctk_gru_batch_set_weights(ctk_gru_batch* b, const float* w, size_t n) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (int rc = gru_batch_weight_args(b, "ctk_gru_batch_set_weights", w, n, "")) return rc;
    return gru_batch_put_weights(b, b->B, nullptr, w, n, false);
}

int ctk_gru_problem_set_weights(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* w, size_t n) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int cnt = 0;
    if (int rc = batch_ids(b, "ctk_gru_problem_set_weights", n_ids, ids, &cnt)) return rc;
    if (int rc = gru_batch_weight_args(b, "ctk_gru_problem_set_weights", w, n, " (one network per listed problem)")) return rc;
    return gru_batch_put_weights(b, cnt, ids, w, n, true);
}

int ctk_gru_problem_have_weights(const ctk_gru_batch* b, int problem) { return (b && problem >= 0 && problem < b->B && b->have_w[(size_t)problem]) ? 1 : 0; }

// ctk_predictor_get_hidden of every listed problem: dst [n][64], rows in the order of ids
int ctk_gru_problem_get_hidden(ctk_gru_batch* b, int n_ids, const int32_t* ids, float* dst) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, "ctk_gru_problem_get_hidden", n_ids, ids, &n)) return rc;
    if (!dst) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_gru_problem_get_hidden: NULL destination (64 floats per listed problem)");
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const size_t HF = ctk_mppi_batch_gru_hidden_floats(), hid = HF * sizeof(float);
    BHIP_TRY(b, gru_batch_runs(n, ids, [&](int p0, int c) {
        return hipMemcpy2DAsync(b->h_hid + (size_t)p0 * HF, hid, gru_batch_hidden(b, p0), b->wtab * sizeof(float), hid, (size_t)c, hipMemcpyDeviceToHost, b->stream);
    }));
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < n; ++j) std::memcpy(dst + (size_t)j * HF, b->h_hid + (size_t)(ids ? ids[j] : j) * HF, hid);
    return CTK_OK;
}

// ctk_predictor_set_hidden of every listed problem: src [n][64], or NULL for zeros; hidden_scale as a handle's entry leaves it
int ctk_gru_problem_set_hidden(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* src) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, "ctk_gru_problem_set_hidden", n_ids, ids, &n)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const size_t HF = ctk_mppi_batch_gru_hidden_floats();
    const std::vector<float> before = b->hidden_scale;
    for (int j = 0; j < n; ++j) {
        const size_t p = (size_t)(ids ? ids[j] : j);
        float* row = b->h_hid + p * HF;
        b->hidden_scale[p] = 1.0f;
        for (size_t i = 0; i < HF; ++i) {
            row[i] = src ? src[(size_t)j * HF + i] : 0.0f;
            b->hidden_scale[p] = std::max(b->hidden_scale[p], std::fabs(row[i]));
        }
    }
    hipError_t e = gru_batch_send_hidden(b, n, ids);
    const hipError_t se = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) { b->hidden_scale = before; return bfail(b, CTK_ERR_HIP, std::string("ctk_gru_problem_set_hidden: ") + hipGetErrorString(e)); }
    return CTK_OK;
}

}  // extern "C"

// =============================================================================================
// Per-problem hyper-parameters and input limits of the CEM and RPGD batches (include/ctk_hip_family_hyper.h): the bodies of the two
// families' entries over the core's table of primary values (BatchCore::fhyp).  What is a family's own is part of its trait F:
//   hyper_names, hyper_list        the names of enum ctk_cem_hyper / ctk_rpgd_hyper in its order, and the list a message shows
//   hyper_rule(b, hyper, v)        the rule *_create applies to the field, and integrality for a count: why v is refused, or NULL
//   hyper_prepare(b, who, n, ids, hyper, values, all)   what has to exist before the values are written (RPGD: the bias-correction
//                                  tables of beta pairs that appear with this call); may fail, and then nothing was written
//   hyper_block(b, p)              problem p's hyper block into hcache, from its row (RPGD: CTK_ERR_STATE, and the block stays, if its betas have no table)
//   hyper_changed(b, p, hyper)     what else a new value invalidates (CEM: BEST_IDX when cem_best_k changes)
// `who` is the entry's name.  The first successful setter turns the _hp form on (sticky): from then on every step record carries a
// two-part element, and F::per_problem_kernel names the _hp kernel.
// =============================================================================================
namespace {

template <class F>
void fhyper_enter(typename F::Batch* b) {
    if (b->fhyper) return;
    b->fhyper = true;
    b->dominant = F::per_problem_kernel(b);
}
// the core's table and blocks at creation: every problem with the configuration's values (first[]: the family's enum values)
void fhyper_init(BatchCore* b, int count, size_t hbytes, const float* first) {
    b->fcount = count; b->frow = count + 2 * CTK_MAX_INPUTS; b->hbytes = hbytes;
    b->fhyp.assign((size_t)b->B * b->frow, 0.0f);
    b->hcache.assign((size_t)b->B * hbytes, 0);
    for (int p = 0; p < b->B; ++p) {
        std::memcpy(b->frow_of(p), first, (size_t)count * sizeof(float));
        for (int c = 0; c < b->C; ++c) { b->flow(p)[c] = b->cfg.action_low[c]; b->fhigh(p)[c] = b->cfg.action_high[c]; }
    }
}
// values == NULL: `all` for every listed problem (the whole-batch entry)
template <class F>
int fam_set_hyper(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, int hyper, const float* values, float all) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (hyper < 0 || hyper >= b->fcount)
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown hyper-parameter " + std::to_string(hyper) + " (" + F::hyper_list + ")");
    for (int j = 0; j < n; ++j) {
        const float v = values ? values[j] : all;
        const char* why = !std::isfinite(v) ? ": a hyper-parameter is finite" : F::hyper_rule(b, hyper, v);
        if (why)
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + why + " (" + F::hyper_names[hyper] + " == " + std::to_string(v) + " for problem " +
                         std::to_string(ids ? ids[j] : j) + "); nothing was written");
    }
    if (int rc = F::hyper_prepare(b, who, n, ids, hyper, values, all)) return rc;
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        b->frow_of(p)[hyper] = values ? values[j] : all;
        F::hyper_changed(b, p, hyper);
        if (int rc = F::hyper_block(b, p)) return rc;  // travels behind the problem's next step record (batch_stage_constants)
    }
    fhyper_enter<F>(b);
    return CTK_OK;
}
template <class F>
int fam_problem_set_hyper(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, int hyper, const float* values) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    if (!values) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL values (one value per listed problem)");
    return fam_set_hyper<F>(b, who, n_ids, ids, hyper, values, 0.0f);
}
int fam_problem_get_hyper(const BatchCore* b, int problem, int hyper, float* out) {
    if (!b || !out || problem < 0 || problem >= b->B || hyper < 0 || hyper >= b->fcount) return CTK_ERR_INVALID_ARGUMENT;
    *out = b->frow_of(problem)[hyper];
    return CTK_OK;
}
template <class F>
int fam_problem_set_limits(typename F::Batch* b, const char* who, int n_ids, const int32_t* ids, const float* low, const float* high) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, who, n_ids, ids, &n)) return rc;
    if (!low || !high) return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL limits (one row of num_control_inputs values per listed problem)");
    for (int i = 0; i < n * b->C; ++i) {
        const bool finite = std::isfinite(low[i]) && std::isfinite(high[i]);
        if (finite && low[i] <= high[i]) continue;
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + (finite ? ": action_low must be <= action_high for every control input" : ": a limit is finite") +
                     " (" + std::to_string(low[i]) + ", " + std::to_string(high[i]) + " for problem " + std::to_string(ids ? ids[i / b->C] : i / b->C) +
                     ", input " + std::to_string(i % b->C) + "); nothing was written");
    }
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        for (int c = 0; c < b->C; ++c) { b->flow(p)[c] = low[(size_t)j * b->C + c]; b->fhigh(p)[c] = high[(size_t)j * b->C + c]; }
        if (int rc = F::hyper_block(b, p)) return rc;
    }
    fhyper_enter<F>(b);
    return CTK_OK;
}
int fam_problem_get_limits(const BatchCore* b, int problem, float* low, float* high) {
    if (!b || !low || !high || problem < 0 || problem >= b->B) return CTK_ERR_INVALID_ARGUMENT;
    std::memcpy(low, b->flow(problem), (size_t)b->C * sizeof(float));
    std::memcpy(high, b->fhigh(problem), (size_t)b->C * sizeof(float));
    return CTK_OK;
}
const char* const COUNT_IS_INTEGRAL = ": a count is integral (values cross the ABI as float, and every admissible count is exact in fp32)";

// the six entries of include/ctk_hip_family_hyper.h for FAM in {ctk_cem_batch, ctk_rpgd_batch} with the prefix PROB of its per-problem entries
#define CTK_FAMILY_HYPER_ENTRIES(FAM, PROB, TRAIT)                                                                                                    \
    int PROB##_set_hyper(FAM* b, int n_ids, const int32_t* ids, int hyper, const float* values) {                                                     \
        return fam_problem_set_hyper<TRAIT>(b, #PROB "_set_hyper", n_ids, ids, hyper, values);                                                        \
    }                                                                                                                                                 \
    int PROB##_get_hyper(const FAM* b, int problem, int hyper, float* out) { return fam_problem_get_hyper(b, problem, hyper, out); }                  \
    int PROB##_set_limits(FAM* b, int n_ids, const int32_t* ids, const float* low, const float* high) {                                               \
        return fam_problem_set_limits<TRAIT>(b, #PROB "_set_limits", n_ids, ids, low, high);                                                          \
    }                                                                                                                                                 \
    int PROB##_get_limits(const FAM* b, int problem, float* low, float* high) { return fam_problem_get_limits(b, problem, low, high); }               \
    int PROB##_hypers_differ(const FAM* b) { return b && b->fhyper ? 1 : 0; }                                                                         \
    int FAM##_set_hyper(FAM* b, int hyper, float value) { return fam_set_hyper<TRAIT>(b, #FAM "_set_hyper", 0, nullptr, hyper, nullptr, value); }

}  // namespace

// =============================================================================================
// Batched CEM (include/ctk_hip.h: ctk_cem_batch_*): B independent CEM problems of one configuration, stepped by launches of
// ctk_cem_batch<ENV, TRAJ> (ctk_cem_fused.hip).  One allocation per buffer kind with a problem stride — no handles inside.  Per-problem
// host state is what a CEM handle keeps: the sequence number of its next step, its Philox position, its step count (which decides the
// outer iterations of its next step: cem_iterations), the next hand-off tag, whether BEST_IDX has to be rebuilt from J, and its parameter
// table.  While no ctk_cem_problem_set_param has succeeded the launches take the constants of the shared table by value; from then on
// (`differ`, sticky) every step writes the constants of the problems it steps BEHIND their step records, in the records' order, so they
// travel in the records' transfer (no constants array in device memory, no second transfer).
// The optimizer's own numbers go the same way (include/ctk_hip_family_hyper.h): cem_best_k, the two deviations, cem_outer_it and the
// input limits are the configuration's until a ctk_cem_problem_set_hyper / _set_limits / ctk_cem_batch_set_hyper has succeeded; from
// then on (`fhyper`, sticky) the launches take ctk_cem_batch_hp<ENV, TRAJ>, and behind every step record travels the two-part element
// [K | hyper block] of its problem.  cem_outer_it never reaches the kernel but through the record's `its`.
// =============================================================================================
struct ctk_cem_batch : BatchCore {
    int K = 0, nblk = 0;
    std::vector<unsigned char> kcache;      // [B][kstride] derived constants by problem id (host only; the step copies them into h_steps)
    int max_per_launch = 1;                 // problems per launch: max(1, CUs / nblk) (ctk_cem_batch_create), a diagnostic switch may lower it
    size_t llw = 0;                         // ctk_cem_fused_ll_words(N, HC): hand-off words per problem
    unsigned long long* d_ll = nullptr;     // [B][llw], zero at allocation
    float* d_mu = nullptr;                  // [B][H,C]
    float* d_sd = nullptr;                  // [B][H,C]
    int* d_idx = nullptr;                   // [B][N]
    CtkCemBatchDesc* d_desc = nullptr;      // [B]
    CtkCemBatchStep* h_steps = nullptr;     // pinned, B * (sizeof(CtkCemBatchStep) + kstride) bytes: the n step records of the step being
    CtkCemBatchStep* d_steps = nullptr;     // issued and, in the per-problem form, the constants of those n problems right behind them
    std::vector<uint32_t> cem_tag;
    std::vector<int> count;
    std::vector<unsigned char> idx_stale;
    float* mu(int p) const { return d_mu + (size_t)p * HC; }
    float* sd(int p) const { return d_sd + (size_t)p * HC; }
    // cem_iterations of the step the problem takes t steps from now: the warm-up count exactly at its first step after creation or reset
    // (cem_outer_it: the problem's own, the configuration's until a setter changed it)
    int its_at(int p, int t) const { return (cfg.warmup && count[(size_t)p] + t == 0) ? cfg.warmup_iterations : (int)frow_of(p)[CTK_CEM_HYPER_OUTER_IT]; }
    int its(int p) const { return its_at(p, 0); }
    int K_of(int p) const { return (int)frow_of(p)[CTK_CEM_HYPER_BEST_K]; }   // the problem's cem_best_k
};

namespace {

// the shared template of a launch's RolloutArgs (ctk_api.hip: make_args of a CEM handle without what the step records and descriptors supply)
RolloutArgs cem_batch_args(const ctk_cem_batch* b) {
    RolloutArgs a = batch_common_args(b);
    a.P = b->H;
    a.p_magic = ctk_magic_of(b->H);
    return a;
}

// the first hand-off tag of a step of `its` iterations for a problem whose next unused tag is `tag` (cem_step: a step's tags are
// consecutive; where tag + its would wrap, the step restarts at 1, so that tag 0 stays the never-written value)
uint32_t cem_tag0(uint32_t tag, int its) { return (uint32_t)(tag + (uint32_t)its) < tag ? 1u : tag; }

// what all launches of a CEM batch share
struct CemBatchCtx { RolloutArgs a; CemFusedLaunch cl; bool log; };
CemBatchCtx cem_batch_context(const ctk_cem_batch* b) {
    return {cem_batch_args(b),
            CemFusedLaunch{0, b->K, nullptr, 0u, b->cfg.cem_stdev_min, 1.0e8f, b->cfg.cem_initial_action_stdev, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0.5},
            b->cfg.materialize_trajectories != 0};
}

// The controller launches of n step records from steps_dev on (ctk_cem_batch_step; every step of ctk_cem_batch_run): consecutive launches
// of at most max_per_launch problems; a problem never spans launches.  d_ksteps: the per-problem form's constants by record index (else
// NULL).  *launched: the records that were launched.
hipError_t cem_batch_launch_records(ctk_cem_batch* b, const CemBatchCtx& x, const CtkCemBatchStep* steps_dev, int n, const unsigned char* d_ksteps,
                                    int* launched) {
    hipError_t le = hipSuccess;
    *launched = 0;
    while (le == hipSuccess && *launched < n) {
        const int cnt = std::min(b->max_per_launch, n - *launched);
        // (the elements are indexed by the launch's record offset, as the records are)
        const unsigned char* d_k = d_ksteps ? d_ksteps + (size_t)*launched * b->elem() : nullptr;
        le = b->fhyper ? ctk_launch_cem_batch_hp(b->stream, b->env, x.a, x.cl, b->d_desc, steps_dev + *launched, cnt, x.log, d_k)
                       : ctk_launch_cem_batch(b->stream, b->env, b->params, b->cfg.dt, b->cfg.intermediate_steps, x.a, x.cl, b->d_desc, steps_dev + *launched, cnt,
                                              x.log, d_k);
        if (le == hipSuccess) *launched += cnt;
    }
    return le;
}

// the CEM family's part of the drivers (the trait of batch_step and batch_closed_loop)
struct CemFamily {
    using Batch = ctk_cem_batch;
    using Rec = CtkCemBatchStep;
    static constexpr bool carries_k = true, error_word = true, device_ahead_of_draws = false, state_size_named = false;
    static constexpr const char* handoff_outputs = "; the other problems' outputs are valid and written";
    static int refuse(Batch*, const char*, int, const int32_t*) { return CTK_OK; }
    static size_t draws_of(const Batch* b, int p) { return (size_t)b->its(p) * b->N * b->HC; }
    // the rows of a caller's buffer have ONE length: mixed iteration counts are refused before anything is launched or consumed
    static int check_draws(Batch* b, const char* who, int n, const int32_t* ids, const StepDraws& d, size_t) {
        if (int rc = batch_check_draws(b, d)) return rc;
        if (d.loc == CTK_LOC_NONE) return CTK_OK;
        const int its0 = b->its(ids ? ids[0] : 0);
        bool mixed = false;
        for (int j = 1; j < n; ++j) mixed |= b->its(ids ? ids[j] : j) != its0;
        if (!mixed) return CTK_OK;
        std::string each;
        for (int j = 0; j < n; ++j) {
            const int p = ids ? ids[j] : j;
            each += (j ? ", " : "") + std::to_string(p) + ": " + std::to_string(b->its(p));
        }
        return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": with caller-supplied samples every listed problem must run the same number of outer "
                     "iterations, but (problem: iterations) " + each + " — the warm-up step of a problem after its creation or reset is longer; step them in "
                     "separate calls (the in-kernel sampler has no such restriction)");
    }
    static const float*& draws(Rec& q) { return q.samples; }
    static CemBatchCtx context(const Batch* b) { return cem_batch_context(b); }
    static hipError_t constants(Batch* b, const int32_t* ids, int n, unsigned char* h_k) {
        if (b->carries()) batch_stage_constants(b, b->kcache.data(), ids, n, h_k);
        return hipSuccess;
    }
    // its from count + t; the tags of the t steps before it consumed one after the other, each by the wrap rule; seq and call + 1 per step
    static void fill(const Batch* b, Rec& q, int p, int t) {
        const size_t z = (size_t)p;
        uint32_t tag = b->cem_tag[z];
        for (int i = 0; i < t; ++i) tag = cem_tag0(tag, b->its_at(p, i)) + (uint32_t)b->its_at(p, i);
        q = Rec{};
        q.id = p; q.seq = b->seq[z] + (uint32_t)t; q.call = b->call[z] + (uint32_t)t;
        q.its = b->its_at(p, t); q.tag0 = cem_tag0(tag, q.its);
    }
    static hipError_t launch(Batch* b, const CemBatchCtx& x, const Rec* d_rec, int n, const unsigned char* d_k, int* launched) {
        return cem_batch_launch_records(b, x, d_rec, n, d_k, launched);
    }
    // The counter rule: every listed problem, launched or not, consumes its sequence number (ctk_api.hip: guarded(); as MPPI, RPGD
    // differs on purpose) and, as every launch attempt does, its tags (cem_step: the wrap rule keeps tag 0 the never-written value);
    // its step count and Philox position advance, and BEST_IDX goes stale, only if launched (as cem_step: with the launch)
    static void advance(Batch* b, int p, int ctrl, bool tried, bool issued) {
        const size_t z = (size_t)p;
        const int listed = ctrl + (tried ? 1 : 0), ran = ctrl + (tried && issued ? 1 : 0);
        for (int i = 0; i < listed; ++i) b->cem_tag[z] = cem_tag0(b->cem_tag[z], b->its_at(p, i)) + (uint32_t)b->its_at(p, i);
        b->seq[z] += (uint32_t)listed; b->call[z] += (uint32_t)ran; b->count[z] += ran;
        if (ran) b->idx_stale[z] = 1;
    }
    // A launched step whose slot never shows the step's seq (a device fault): ctk_api.hip's finish_step returns before it advances the
    // Philox position or reads u, and so does this family's step (as RPGD; MPPI advances it regardless, by history); the closed loop
    // does not look per step in any family.
    static constexpr bool unpublished_keeps_position = true;
    // ---- the family's part of batch_rollout: the analytic predictor; a problem's plan is its mean, where read(U_NOM) reads ----
    static int rollout_pred(const Batch*) { return CTK_PRED_ODE; }
    static const float* rollout_weights(const Batch*, size_t* stride) { *stride = 0; return nullptr; }
    static int rollout_refuse(Batch*, const char*, int, const int32_t*, bool, bool) { return CTK_OK; }
    static const float* own_plan(const Batch* b, int p) { return b->mu(p); }
    // the state of a problem: mean, standard deviation, last output; its step count
    static BatchState state(Batch* b, int p) {
        return {{state_seg(b->mu(p), (size_t)b->HC), state_seg(b->sd(p), (size_t)b->HC), state_seg(b->u(p), (size_t)b->C), state_counter(&b->count[(size_t)p])}};
    }
    static const char* per_problem_kernel(const Batch* b) {     // (the _hp form stays the _hp form)
        return b->fhyper ? ctk_cem_batch_hp_name(b->env, b->cfg.materialize_trajectories != 0) : ctk_cem_batch_name(b->env, b->cfg.materialize_trajectories != 0, true);
    }
    // ---- per-problem hyper-parameters (include/ctk_hip_family_hyper.h: enum ctk_cem_hyper) ----
    static constexpr const char* hyper_names[CTK_CEM_HYPER_COUNT] = {"cem_best_k", "cem_initial_action_stdev", "cem_stdev_min", "cem_outer_it"};
    static constexpr const char* hyper_list = "enum ctk_cem_hyper: cem_best_k, cem_initial_action_stdev, cem_stdev_min, cem_outer_it";
    // the rules ctk_cem_batch_create applies to the same fields
    static const char* hyper_rule(const Batch* b, int hyper, float v) {
        if (hyper != CTK_CEM_HYPER_BEST_K && hyper != CTK_CEM_HYPER_OUTER_IT) return nullptr;
        if (v != std::floor(v)) return COUNT_IS_INTEGRAL;
        if (hyper == CTK_CEM_HYPER_BEST_K) return v >= 1.0f && v <= (float)b->N ? nullptr : ": CEM needs 1 <= cem_best_k <= num_rollouts";
        return v >= 1.0f && v <= 2147483520.0f ? nullptr : ": CEM needs cem_outer_it >= 1";
    }
    static int hyper_prepare(Batch*, const char*, int, const int32_t*, int, const float*, float) { return CTK_OK; }
    static int hyper_block(Batch* b, int p) {
        const float* row = b->frow_of(p);
        ctk_cem_batch_fill_hyper(b->hcache.data() + (size_t)p * b->hbytes, b->K_of(p), row[CTK_CEM_HYPER_STDEV_MIN], row[CTK_CEM_HYPER_INITIAL_ACTION_STDEV],
                                 b->flow(p), b->fhigh(p), b->C);
        return CTK_OK;
    }
    // BEST_IDX is materialised on demand with the problem's K: a new K makes what a step left there stale (before the problem's first
    // step after its creation or reset there is nothing to select from, as in a handle)
    static void hyper_changed(Batch* b, int p, int hyper) { if (hyper == CTK_CEM_HYPER_BEST_K && b->count[(size_t)p] > 0) b->idx_stale[(size_t)p] = 1; }
};

// mean at the middle of problem p's limits, std = its cem_initial_action_stdev (the configuration's until a setter changed them) into
// the host images (ctk_reset of a CEM handle created with p's values)
void cem_batch_initial(const ctk_cem_batch* b, int p, float* mu, float* sd) {
    for (int i = 0; i < b->HC; ++i) {
        mu[i] = 0.5f * (b->flow(p)[i % b->C] + b->fhigh(p)[i % b->C]);
        sd[i] = b->frow_of(p)[CTK_CEM_HYPER_INITIAL_ACTION_STDEV];
    }
}

}  // namespace

extern "C" {

CTK_BATCH_ENTRIES(ctk_cem_batch, ctk_cem_problem, CemFamily)
// ---- the closed loop on the device (include/ctk_hip_loop.h: ctk_cem_batch_plant_* / ctk_cem_batch_run / ctk_cem_batch_episodes) ----
CTK_LOOP_ENTRIES(ctk_cem_batch, CemFamily)
CTK_ROLLOUT_ENTRY(ctk_cem_batch, CemFamily)
// ---- per-problem hyper-parameters and limits (include/ctk_hip_family_hyper.h: ctk_cem_problem_*_hyper / _limits, ctk_cem_batch_set_hyper) ----
CTK_FAMILY_HYPER_ENTRIES(ctk_cem_batch, ctk_cem_problem, CemFamily)

size_t ctk_cem_batch_samples_needed(const ctk_cem_batch* b, int problem) { return (b && problem >= 0 && problem < b->B) ? CemFamily::draws_of(b, problem) : 0; }

int ctk_cem_batch_create(const ctk_config* cfg, int n_problems, const uint64_t* seeds, ctk_cem_batch** out) {
    if (out) *out = nullptr;
    if (!cfg || !out) return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_cem_batch_create: NULL argument");
    if (n_problems < 1) return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_cem_batch_create: a batch holds at least one problem (n_problems == " + std::to_string(n_problems) + ")");
    const EnvInfo* einfo = nullptr;
    if (int rc = check_config("ctk_cem_batch_create", cfg, &einfo)) return rc;
    if (cfg->optimizer != CTK_OPT_CEM)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_cem_batch_create: a CEM batch steps plain CEM controllers only (cfg.optimizer == " + std::to_string(cfg->optimizer) +
                     "); MPPI has ctk_batch_create, the CEM variants (naive-grad, Bharadhwaj, GMM) and the other optimizers run as single handles (ctk_create)");
    if (cfg->predictor != CTK_PRED_ODE)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_cem_batch_create: the batch kernel rolls out the analytic (ODE) predictor only (cfg.predictor == " +
                     std::to_string(cfg->predictor) + "); network predictors run as single handles (ctk_create)");
    const int N = cfg->num_rollouts, H = cfg->mpc_horizon, HC = H * einfo->C, nblk = ctk_cem_fused_blocks(N);
    if (!ctk_cem_fusable(cfg->predictor, N, HC))
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_cem_batch_create: per-problem population outside the one-launch CEM step's sizes (num_rollouts " + std::to_string(N) +
                     " = " + std::to_string(nblk) + " workgroups of 64 rollouts, mpc_horizon " + std::to_string(H) + " x " + std::to_string(einfo->C) + " inputs = " +
                     std::to_string(HC) + " columns, " + std::to_string(ctk_cem_fused_lds(N, HC)) + " bytes of LDS): the batch kernel takes at most " +
                     std::to_string(CTK_CEM_FUSED_MAX_BLOCKS) + " workgroups per problem and 131072 bytes (128 KiB) of LDS; such a controller runs as a single handle (ctk_create)");
    if (cfg->cem_best_k > N)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_cem_batch_create: cem_best_k " + std::to_string(cfg->cem_best_k) + " exceeds num_rollouts " + std::to_string(N) +
                     ": the elite set of a problem is part of its population");
    if (cfg->cem_best_k < 1 || cfg->cem_outer_it < 1 || (cfg->warmup && cfg->warmup_iterations < 1))
        return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_cem_batch_create: need cem_best_k >= 1, cem_outer_it >= 1 and, with warmup, warmup_iterations >= 1");

    hipDeviceProp_t prop;
    if (int rc = probe_device("ctk_cem_batch_create", cfg->device, &prop)) return rc;

    Creating<ctk_cem_batch> made;
    ctk_cem_batch* b = made.p;
    batch_core_init(b, cfg, einfo, n_problems, seeds);
    b->K = cfg->cem_best_k; b->nblk = nblk;
    b->llw = ctk_cem_fused_ll_words(N, HC);
    b->kcache.assign((size_t)n_problems * b->kstride, 0);
    // Progress (the proof stands above ctk_cem_batch, ctk_cem_fused.hip): every workgroup of a problem waits for all workgroups of that
    // problem, so a launch holds at most max(1, CUs / nblk) problems — problems * nblk <= CUs, every CU admits at least one workgroup of
    // this kernel (LDS <= 128 KiB), so all workgroups of a launch are co-resident whatever the dispatch order or placement.  One problem
    // alone is the single kernel's case (nblk <= CTK_CEM_FUSED_MAX_BLOCKS).  CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH (diagnostic) only lowers it.
    b->max_per_launch = std::max(1, prop.multiProcessorCount / nblk);
    batch_env_lowers("CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH", &b->max_per_launch);
    b->cem_tag.assign((size_t)n_problems, 1u);
    b->count.assign((size_t)n_problems, 0); b->idx_stale.assign((size_t)n_problems, 0);
    b->dominant = ctk_cem_batch_name(b->env, cfg->materialize_trajectories != 0);
    const float first[CTK_CEM_HYPER_COUNT] = {(float)cfg->cem_best_k, cfg->cem_initial_action_stdev, cfg->cem_stdev_min, (float)cfg->cem_outer_it};
    fhyper_init(b, CTK_CEM_HYPER_COUNT, ctk_cem_batch_hyper_bytes(), first);
    for (int p = 0; p < n_problems; ++p) CemFamily::hyper_block(b, p);   // (cannot fail)

    if (int rc = batch_core_open(b)) return rc;
    const size_t Bz = (size_t)n_problems;
    HIP_CREATE(b->own.dev_zero(&b->d_ll, Bz * b->llw * sizeof(unsigned long long), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_mu, Bz * HC * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_sd, Bz * HC * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_J, Bz * N * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_Q, Bz * N * HC * sizeof(float), b->stream));
    if (cfg->materialize_trajectories) HIP_CREATE(b->own.dev_zero(&b->d_traj, Bz * N * (H + 1) * b->S * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_idx, Bz * N * sizeof(int), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_desc, Bz * sizeof(CtkCemBatchDesc), b->stream));
    const size_t steps_bytes = Bz * (sizeof(CtkCemBatchStep) + b->kstride + b->hbytes);   // the records, then room for as many two-part elements
    HIP_CREATE(b->own.dev_zero(&b->d_steps, steps_bytes, b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_steps, steps_bytes));

    std::vector<CtkCemBatchDesc> desc(Bz);
    std::vector<float> mu(Bz * HC), sd(Bz * HC);                   // optimizer_reset() of every problem
    for (int p = 0; p < n_problems; ++p) {
        const size_t z = (size_t)p;
        const uint64_t seed = batch_seed(cfg, seeds, p);
        CtkCemBatchDesc& d = desc[z];
        d.ll = b->d_ll + z * b->llw;
        d.mu = b->mu(p); d.sd = b->sd(p);
        d.J = b->d_J + z * N; d.Q_out = b->d_Q + z * N * HC;
        d.traj_out = b->d_traj ? b->d_traj + z * N * (H + 1) * b->S : nullptr;
        d.u_dev = b->u(p); d.u_host = b->h_u_dev + z * 16; d.idx_out = b->d_idx + z * N;
        d.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull); d.seed_hi = (uint32_t)(seed >> 32);
        cem_batch_initial(b, p, mu.data() + z * HC, sd.data() + z * HC);
    }
    HIP_CREATE(hipMemcpyAsync(b->d_desc, desc.data(), Bz * sizeof(CtkCemBatchDesc), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_mu, mu.data(), mu.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_sd, sd.data(), sd.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipStreamSynchronize(b->stream));               // the host vectors go out of scope below
    *out = made.release();
    return CTK_OK;
}

int ctk_cem_batch_step(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u_prev, const float* samples, int samples_loc,
                       float* u_out) {
    return batch_step<CemFamily>(b, "ctk_cem_batch_step", n_ids, ids, s, u_prev, StepDraws{samples, 0, samples_loc}, u_out);
}

int ctk_cem_batch_reset(ctk_cem_batch* b, int n_ids, const int32_t* ids) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, "ctk_cem_batch_reset", n_ids, ids, &n)) return rc;
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    const size_t HC = (size_t)b->HC;                   // every listed problem's own images: the copies below read them until the synchronisation
    std::vector<float> mu((size_t)n * HC), sd((size_t)n * HC), zero((size_t)b->C, 0.0f);
    for (int j = 0; j < n; ++j) {                      // ctk_reset of a CEM handle: parameters, hyper-parameters, tags and the Philox position stay
        const int p = ids ? ids[j] : j;
        cem_batch_initial(b, p, mu.data() + (size_t)j * HC, sd.data() + (size_t)j * HC);
        b->count[(size_t)p] = 0;
        BHIP_TRY(b, hipMemcpyAsync(b->mu(p), mu.data() + (size_t)j * HC, HC * sizeof(float), hipMemcpyHostToDevice, b->stream));
        BHIP_TRY(b, hipMemcpyAsync(b->sd(p), sd.data() + (size_t)j * HC, HC * sizeof(float), hipMemcpyHostToDevice, b->stream));
        BHIP_TRY(b, hipMemcpyAsync(b->u(p), zero.data(), zero.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    }
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    return CTK_OK;
}

int ctk_cem_batch_read(ctk_cem_batch* b, int problem, int buffer, float* dst, size_t cap) {
    if (int rc = batch_read_check(b, "ctk_cem_batch_read", problem, dst)) return rc;
    const size_t z = (size_t)problem, N = (size_t)b->N;
    const float* src = nullptr; size_t n = 0; bool is_int = false;
    if (int rc = batch_locate_rollouts(b, "ctk_cem_batch_read", problem, buffer, &src, &n)) return rc;
    if (!src) switch (buffer) {
        case CTK_BUF_U_NOM: src = b->mu(problem); n = (size_t)b->HC; break;
        case CTK_BUF_STD: src = b->sd(problem); n = (size_t)b->HC; break;
        case CTK_BUF_BEST_IDX: src = reinterpret_cast<const float*>(b->d_idx + z * N); n = (size_t)b->K_of(problem); is_int = true; break;
        default: return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_cem_batch_read: a CEM batch has Q, J, TRAJ, U_NOM, STD and BEST_IDX");
    }
    return batch_read_out(b, "ctk_cem_batch_read", src, n, is_int, dst, cap, [&]() -> int {
        if (!is_int || !b->idx_stale[z]) return CTK_OK;
        // the sorted elite indices are materialised from the last iteration's costs (ctk_api.hip: locate_buffer)
        BHIP_TRY(b, ctk_launch_select_topk(b->stream, b->d_J + z * N, b->N, b->K_of(problem), b->d_idx + z * N));
        b->idx_stale[z] = 0;
        return CTK_OK;
    });
}

}  // extern "C"

// =============================================================================================
// Batched RPGD (include/ctk_hip.h: ctk_rpgd_batch_*): B independent RPGD problems of one configuration with at most
// CTK_RPGD_FUSED_MAX_N plans each, stepped by launches of ctk_g_rpgd_batch<ENV> (ctk_generic.hip) — one workgroup per problem runs the
// descent, the keep-k selection and the warm start that a template handle runs as three launches.  One allocation per buffer kind with a
// problem stride — no handles inside.  Per-problem host state is what an RPGD handle keeps: the sequence number of its next step, its
// Philox position, its step count (which decides the iterations of its next step and whether it resamples), its Adam step number, which
// buffer holds its population, whether it has been reset, and its parameter table.  No workgroup of the kernel waits for another, so a
// call is split into launches only at the grid's y limit.  While no ctk_rpgd_problem_set_param has succeeded the launches take the
// constants of the shared table by value; from then on (`differ`, sticky) every step writes the constants of the problems it steps
// BEHIND their step records, in the records' order, so they travel in the records' transfer (no constants array in device memory, no
// second transfer).
// The optimizer's own numbers go the same way (include/ctk_hip_family_hyper.h): the Adam constants, the clip, the sampling constants,
// outer_its, resamp_per and the input limits are the configuration's until a ctk_rpgd_problem_set_hyper / _set_limits /
// ctk_rpgd_batch_set_hyper has succeeded; from then on (`fhyper`, sticky) the launches take ctk_g_rpgd_batch_hp<ENV>, and behind every
// step record travels the two-part element [K | hyper block] of its problem.  The block names the problem's bias-correction table: one
// device table per distinct (adam_beta_1, adam_beta_2) in use (bc_tabs), each adam_bias_corrections of its pair, the function behind a
// handle's table.  outer_its and resamp_per never reach the kernel but through the record's iters / resample.
// =============================================================================================
struct ctk_rpgd_batch : BatchCore {
    int P = 0, PC = 0, K = 0;
    std::vector<unsigned char> kcache;      // [B][kstride] derived constants by problem id (host only; the step copies them into h_steps)
    InterpEntry* d_interp = nullptr;        // [H] shared
    float* d_bc = nullptr; int bc_len = 0;  // the bias-correction table of the configuration's betas (bc_tabs[0])
    struct BcTab { float b1, b2; float* d; };
    std::vector<BcTab> bc_tabs;             // the device tables, [2 * bc_len] floats each; one that no problem names is written over by the next new pair
    std::vector<int> bc_of;                 // [B] the problem's table
    float* d_pop[2] = {nullptr, nullptr};   // [B][N,H,C] each
    float* d_m[2] = {nullptr, nullptr};
    float* d_v[2] = {nullptr, nullptr};
    float* d_ages[2] = {nullptr, nullptr};  // [B][N] each
    int* d_idx = nullptr;                   // [B][N]
    float* d_unom = nullptr;                // [B][H,C]
    float* d_scratch = nullptr; size_t scratch_stride = 0;   // [B][H * NT * 64] state tapes that do not fit in LDS
    CtkRpgdBatchDesc* d_desc = nullptr;     // [B]
    CtkRpgdBatchStep* h_steps = nullptr;    // pinned, B * (sizeof(CtkRpgdBatchStep) + kstride) bytes: the n records of the step (or reset) being
    CtkRpgdBatchStep* d_steps = nullptr;    // issued and, in the per-problem form of a step, the constants of those n problems right behind them
    std::vector<int> count, adam_step;
    std::vector<unsigned char> cur, ready;
    size_t NHC() const { return (size_t)N * HC; }
    // rpgd_iterations and the resampling rule (optimizer_rpgd.py:449) of the step the problem takes t steps from now: both from count + t
    // (outer_its, resamp_per: the problem's own, the configuration's until a setter changed them)
    int its_at(int p, int t) const {
        const int outer = (int)frow_of(p)[CTK_RPGD_HYPER_OUTER_ITS];
        const int first = cfg.warmup ? cfg.warmup_iterations : outer;
        return count[(size_t)p] + t == 0 ? first : outer;
    }
    bool resamples_at(int p, int t) const { return (count[(size_t)p] + t) % (int)frow_of(p)[CTK_RPGD_HYPER_RESAMP_PER] == 0; }
    int its(int p) const { return its_at(p, 0); }
    bool resamples(int p) const { return resamples_at(p, 0); }
    size_t needs(int p) const { return (resamples(p) && K < N) ? (size_t)(N - K) * PC : 0; }   // samples_needed of an RPGD handle
};

namespace {

// the shared template of a launch's RolloutArgs (ctk_api.hip: make_args of an RPGD handle's descent without what the step records and descriptors supply)
RolloutArgs rpgd_batch_args(const ctk_rpgd_batch* b) {
    RolloutArgs a = batch_common_args(b);
    a.P = b->H;
    a.p_magic = ctk_magic_of(b->H);
    a.identity_interp = b->cfg.period_interpolation_inducing_points == 1 ? 1 : 0;
    a.interp = b->d_interp;
    return a;
}
// what the launches take of the warm start's description: keep_k, P, the sampling constants, the interpolation table
RpgdFusedWarm rpgd_batch_warm(const ctk_rpgd_batch* b) {
    const ctk_config& c = b->cfg;
    return RpgdFusedWarm{b->K, nullptr, b->P, 0, 0, c.shift_previous, c.sampling_distribution, 0, c.sample_whole_control_space, c.sample_stdev,
                         c.sample_mean, c.sample_min, c.sample_max, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, b->d_interp,
                         nullptr, nullptr, nullptr, 0u};
}

constexpr int RPGD_BATCH_MAX_GRID_Y = 65535;   // problems of one launch: the grid's y limit, nothing else bounds it

// what all launches of an RPGD batch share
struct RpgdBatchCtx { RolloutArgs a; RpgdFusedWarm f; };

// The controller launches of n step records from steps_dev on (ctk_rpgd_batch_step; every step of ctk_rpgd_batch_run): consecutive
// launches only past the grid's y limit; a problem never spans launches.  d_ksteps: the per-problem form's constants by record index
// (else NULL).  *launched: the records that were launched.
hipError_t rpgd_batch_launch_records(ctk_rpgd_batch* b, const RpgdBatchCtx& x, const CtkRpgdBatchStep* steps_dev, int n, const unsigned char* d_ksteps,
                                     int* launched) {
    const ctk_config& c = b->cfg;
    hipError_t le = hipSuccess;
    *launched = 0;
    while (le == hipSuccess && *launched < n) {
        const int cnt = std::min(RPGD_BATCH_MAX_GRID_Y, n - *launched);
        // (the elements are indexed by the launch's record offset, as the records are)
        const unsigned char* d_k = d_ksteps ? d_ksteps + (size_t)*launched * b->elem() : nullptr;
        le = b->fhyper ? ctk_launch_g_rpgd_batch_hp(b->stream, b->env, x.a, b->bc_len, x.f, b->d_desc, steps_dev + *launched, cnt, d_k)
                       : ctk_launch_g_rpgd_batch(b->stream, b->env, x.a, b->params, c.dt, c.intermediate_steps, c.learning_rate, c.adam_beta_1, c.adam_beta_2,
                                                 c.adam_epsilon, c.gradmax_clip, c.adam_rule == 1 ? 1 : 0, b->d_bc, b->bc_len, x.f, b->d_desc,
                                                 steps_dev + *launched, cnt, d_k);
        if (le == hipSuccess) *launched += cnt;
    }
    return le;
}

// a listed problem that was never reset: nothing is launched (ctk_rpgd_batch_step and the closed loop)
int rpgd_batch_ready(ctk_rpgd_batch* b, const char* who, int n, const int32_t* ids) {
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        if (!b->ready[(size_t)p])
            return bfail(b, CTK_ERR_STATE, std::string(who) + ": problem " + std::to_string(p) + " was never reset: call ctk_rpgd_batch_reset (optimizer_reset) "
                         "before its first step; nothing was launched");
    }
    return CTK_OK;
}

// the RPGD family's part of the drivers (the trait of batch_step and batch_closed_loop)
struct RpgdFamily {
    using Batch = ctk_rpgd_batch;
    using Rec = CtkRpgdBatchStep;
    static constexpr bool carries_k = true, error_word = false;      // this kernel has no in-launch hand-off
    static constexpr bool device_ahead_of_draws = false, state_size_named = true;
    static int refuse(Batch* b, const char* who, int n, const int32_t* ids) { return rpgd_batch_ready(b, who, n, ids); }
    // one [num_rollouts - opt_keep_k, P, C] block for every listed problem that resamples at this step, none for the others
    static size_t draws_of(const Batch* b, int p) { return b->needs(p); }
    static int check_draws(Batch* b, const char* who, int, const int32_t*, const StepDraws& d, size_t need) {
        if (d.loc == CTK_LOC_NONE) return CTK_OK;
        if (d.loc != CTK_LOC_DEVICE && d.loc != CTK_LOC_HOST) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "bad samples_loc");
        if (d.n_samples != need)                       // refused before a sample is read
            return bfail(b, CTK_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(d.n_samples) + " samples given, the listed problems need " +
                         std::to_string(need) + " (one [num_rollouts - opt_keep_k, P, C] block for every listed problem whose ctk_rpgd_batch_samples_needed is "
                         "non-zero, in id order); nothing was launched");
        if (need != 0 && d.samples == nullptr) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "samples pointer is NULL but samples_loc != CTK_LOC_NONE");
        return CTK_OK;
    }
    static const float*& draws(Rec& q) { return q.draws; }
    static RpgdBatchCtx context(const Batch* b) { return {rpgd_batch_args(b), rpgd_batch_warm(b)}; }
    static hipError_t constants(Batch* b, const int32_t* ids, int n, unsigned char* h_k) {
        if (b->carries()) batch_stage_constants(b, b->kcache.data(), ids, n, h_k);
        return hipSuccess;
    }
    // iters and resample from count + t; t0 = the Adam steps taken plus those of the t steps before it; cur flips, seq and call + 1 per
    // step; the draws are the in-kernel Philox's
    static void fill(const Batch* b, Rec& q, int p, int t) {
        const size_t z = (size_t)p;
        q = Rec{};
        q.id = p; q.seq = b->seq[z] + (uint32_t)t; q.call = b->call[z] + (uint32_t)t; q.cur = (uint32_t)(b->cur[z] ^ (t & 1));
        q.iters = b->its_at(p, t); q.t0 = b->adam_step[z];
        for (int i = 0; i < t; ++i) q.t0 += b->its_at(p, i);
        q.resample = b->resamples_at(p, t) ? 1 : 0;
    }
    static hipError_t launch(Batch* b, const RpgdBatchCtx& x, const Rec* d_rec, int n, const unsigned char* d_k, int* launched) {
        return rpgd_batch_launch_records(b, x, d_rec, n, d_k, launched);
    }
    // The counter rule, on purpose: a problem never issued consumes nothing, not even its sequence number (the MPPI and CEM families
    // consume seq for every listed problem); the Adam step number, the buffer and the step count move with the launch (as rpgd_descent /
    // rpgd_step)
    static void advance(Batch* b, int p, int ctrl, bool tried, bool issued) {
        const size_t z = (size_t)p;
        const int ran = ctrl + (tried && issued ? 1 : 0);
        for (int i = 0; i < ran; ++i) b->adam_step[z] += b->its_at(p, i);      // (ahead of count, which its_at reads)
        b->seq[z] += (uint32_t)ran; b->call[z] += (uint32_t)ran; b->cur[z] ^= ran & 1; b->count[z] += ran;
    }
    // A launched step whose slot never shows the step's seq (a device fault): ctk_api.hip's finish_step returns before it advances the
    // Philox position or reads u, and so does this family's step (as CEM; MPPI advances it regardless, by history); the closed loop
    // does not look per step in any family.
    static constexpr bool unpublished_keeps_position = true;
    // ---- the family's part of batch_rollout: the analytic predictor; a problem's plan is u_nom, which its first reset writes ----
    static int rollout_pred(const Batch*) { return CTK_PRED_ODE; }
    static const float* rollout_weights(const Batch*, size_t* stride) { *stride = 0; return nullptr; }
    static int rollout_refuse(Batch* b, const char* who, int n, const int32_t* ids, bool own, bool) { return own ? rpgd_batch_ready(b, who, n, ids) : CTK_OK; }
    static const float* own_plan(const Batch* b, int p) { return b->d_unom + (size_t)p * b->HC; }
    // the state of a problem (ctk_state_size of an RPGD handle): population, Adam moments, ages, last output; Adam step and step count.
    // A problem whose state was set counts as reset.
    static BatchState state(Batch* b, int p) {
        const size_t z = (size_t)p, N = (size_t)b->N, NHC = b->NHC();
        const int cur = b->cur[z];
        return {{state_seg(b->d_pop[cur] + z * NHC, NHC), state_seg(b->d_m[cur] + z * NHC, NHC), state_seg(b->d_v[cur] + z * NHC, NHC),
                 state_seg(b->d_ages[cur] + z * N, N), state_seg(b->u(p), (size_t)b->C), state_counter(&b->adam_step[z]), state_counter(&b->count[z])},
                &b->ready[z]};
    }
    static const char* per_problem_kernel(const Batch* b) {     // (the _hp form stays the _hp form)
        return b->fhyper ? ctk_g_rpgd_batch_hp_name(b->env) : ctk_g_rpgd_batch_name(b->env, true);
    }
    // ---- per-problem hyper-parameters (include/ctk_hip_family_hyper.h: enum ctk_rpgd_hyper) ----
    static constexpr const char* hyper_names[CTK_RPGD_HYPER_COUNT] = {"learning_rate", "adam_beta_1", "adam_beta_2", "adam_epsilon", "gradmax_clip", "sample_stdev",
                                                                      "sample_mean", "uniform_dist_min", "uniform_dist_max", "outer_its", "resamp_per"};
    static constexpr const char* hyper_list = "enum ctk_rpgd_hyper: learning_rate, adam_beta_1, adam_beta_2, adam_epsilon, gradmax_clip, sample_stdev, sample_mean, "
                                              "uniform_dist_min, uniform_dist_max, outer_its, resamp_per";
    // the rules ctk_rpgd_batch_create applies to the same fields
    static const char* hyper_rule(const Batch*, int hyper, float v) {
        if (hyper != CTK_RPGD_HYPER_OUTER_ITS && hyper != CTK_RPGD_HYPER_RESAMP_PER) return nullptr;
        if (v != std::floor(v)) return COUNT_IS_INTEGRAL;
        if (hyper == CTK_RPGD_HYPER_OUTER_ITS) return v >= 0.0f && v <= 2147483520.0f ? nullptr : ": RPGD needs outer_its >= 0";
        return v >= 1.0f && v <= 2147483520.0f ? nullptr : ": RPGD needs resamp_per >= 1";
    }
    // the table of (b1, b2), or -1
    static int bc_find(const Batch* b, float b1, float b2) {
        for (size_t i = 0; i < b->bc_tabs.size(); ++i)
            if (b->bc_tabs[i].b1 == b1 && b->bc_tabs[i].b2 == b2) return (int)i;
        return -1;
    }
    // A new beta makes a new (beta_1, beta_2) pair for its problem: every pair that appears with this call gets its device table here,
    // before anything is written — adam_bias_corrections of the pair, into a table that no problem names (the configuration's, table 0,
    // is kept) or a new allocation.  No launch is in flight between two calls (every step, run and reset ends synchronised), so such
    // a table may be written over — but never one that a problem of THIS call is about to name: `needed` holds every table the call has
    // found or written for a listed problem, whether or not a problem names it yet.
    static int hyper_prepare(Batch* b, const char*, int n, const int32_t* ids, int hyper, const float* values, float all) {
        if (hyper != CTK_RPGD_HYPER_ADAM_BETA_1 && hyper != CTK_RPGD_HYPER_ADAM_BETA_2) return CTK_OK;
        std::vector<int> needed;
        for (int j = 0; j < n; ++j) {
            const int p = ids ? ids[j] : j;
            const float v = values ? values[j] : all;
            const float b1 = hyper == CTK_RPGD_HYPER_ADAM_BETA_1 ? v : b->frow_of(p)[CTK_RPGD_HYPER_ADAM_BETA_1];
            const float b2 = hyper == CTK_RPGD_HYPER_ADAM_BETA_2 ? v : b->frow_of(p)[CTK_RPGD_HYPER_ADAM_BETA_2];
            const int have = bc_find(b, b1, b2);
            if (have >= 0) { needed.push_back(have); continue; }             // (it may be named by no problem at this moment)
            int slot = -1;
            for (size_t i = 1; i < b->bc_tabs.size() && slot < 0; ++i)
                if (std::find(b->bc_of.begin(), b->bc_of.end(), (int)i) == b->bc_of.end() && std::find(needed.begin(), needed.end(), (int)i) == needed.end())
                    slot = (int)i;
            BHIP_TRY(b, hipSetDevice(b->cfg.device));
            const std::vector<float> bc = adam_bias_corrections(b1, b2);       // the table of a handle created with the pair (ctk_host.h)
            if (slot < 0) {
                float* d = nullptr;
                BHIP_TRY(b, b->own.dev_zero(&d, bc.size() * sizeof(float), b->stream));
                b->bc_tabs.push_back({NAN, NAN, d});   // (no pair yet: found by nobody until the copy below has succeeded)
                slot = (int)b->bc_tabs.size() - 1;
            }
            b->bc_tabs[(size_t)slot].b1 = b->bc_tabs[(size_t)slot].b2 = NAN;
            BHIP_TRY(b, hipMemcpyAsync(b->bc_tabs[(size_t)slot].d, bc.data(), bc.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
            BHIP_TRY(b, hipStreamSynchronize(b->stream));                      // bc goes out of scope
            b->bc_tabs[(size_t)slot].b1 = b1; b->bc_tabs[(size_t)slot].b2 = b2;
            needed.push_back(slot);
        }
        return CTK_OK;
    }
    static int hyper_block(Batch* b, int p) {
        const float* r = b->frow_of(p);
        const int tab = bc_find(b, r[CTK_RPGD_HYPER_ADAM_BETA_1], r[CTK_RPGD_HYPER_ADAM_BETA_2]);   // (hyper_prepare has made it)
        if (tab < 0)                                   // never an address that is not a table's: the problem keeps the block and table it had
            return bfail(b, CTK_ERR_STATE, "no bias-correction table for adam_beta_1 " + std::to_string(r[CTK_RPGD_HYPER_ADAM_BETA_1]) + ", adam_beta_2 " +
                         std::to_string(r[CTK_RPGD_HYPER_ADAM_BETA_2]) + " of problem " + std::to_string(p) + " (hyper_prepare makes one for every pair a call brings)");
        b->bc_of[(size_t)p] = tab;
        ctk_rpgd_batch_fill_hyper(b->hcache.data() + (size_t)p * b->hbytes, r[CTK_RPGD_HYPER_LEARNING_RATE], r[CTK_RPGD_HYPER_ADAM_BETA_1],
                                  r[CTK_RPGD_HYPER_ADAM_BETA_2], r[CTK_RPGD_HYPER_ADAM_EPSILON], r[CTK_RPGD_HYPER_GRADMAX_CLIP], b->cfg.adam_rule == 1 ? 1 : 0,
                                  b->bc_tabs[(size_t)tab].d, r[CTK_RPGD_HYPER_SAMPLE_STDEV], r[CTK_RPGD_HYPER_SAMPLE_MEAN], r[CTK_RPGD_HYPER_UNIFORM_DIST_MIN],
                                  r[CTK_RPGD_HYPER_UNIFORM_DIST_MAX], b->flow(p), b->fhigh(p), b->C);
        return CTK_OK;
    }
    static void hyper_changed(Batch*, int, int) {}
};

}  // namespace

extern "C" {

size_t ctk_rpgd_template_descent_lds(int environment, int mpc_horizon, int* tape_in_lds) {
    if (tape_in_lds) *tape_in_lds = 0;
    if (!env_info(environment) || mpc_horizon < 1) return 0;
    bool fits = false;
    const size_t lds = ctk_g_rpgd_descent_lds(environment, mpc_horizon, &fits);
    if (tape_in_lds) *tape_in_lds = fits ? 1 : 0;
    return lds;
}

CTK_BATCH_ENTRIES(ctk_rpgd_batch, ctk_rpgd_problem, RpgdFamily)
// ---- the closed loop on the device (include/ctk_hip_loop.h: ctk_rpgd_batch_plant_* / ctk_rpgd_batch_run / ctk_rpgd_batch_episodes) ----
CTK_LOOP_ENTRIES(ctk_rpgd_batch, RpgdFamily)
CTK_ROLLOUT_ENTRY(ctk_rpgd_batch, RpgdFamily)
// ---- per-problem hyper-parameters and limits (include/ctk_hip_family_hyper.h: ctk_rpgd_problem_*_hyper / _limits, ctk_rpgd_batch_set_hyper) ----
CTK_FAMILY_HYPER_ENTRIES(ctk_rpgd_batch, ctk_rpgd_problem, RpgdFamily)

size_t ctk_rpgd_batch_samples_needed(const ctk_rpgd_batch* b, int problem) { return (b && problem >= 0 && problem < b->B) ? b->needs(problem) : 0; }

int ctk_rpgd_batch_create(const ctk_config* cfg, int n_problems, const uint64_t* seeds, ctk_rpgd_batch** out) {
    if (out) *out = nullptr;
    if (!cfg || !out) return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_rpgd_batch_create: NULL argument");
    if (n_problems < 1) return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: a batch holds at least one problem (n_problems == " + std::to_string(n_problems) + ")");
    const EnvInfo* einfo = nullptr;
    if (int rc = check_config("ctk_rpgd_batch_create", cfg, &einfo)) return rc;
    const int N = cfg->num_rollouts, H = cfg->mpc_horizon, HC = H * einfo->C;
    if (cfg->optimizer != CTK_OPT_RPGD)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: an RPGD batch steps RPGD controllers only (cfg.optimizer == " + std::to_string(cfg->optimizer) +
                     ", num_rollouts " + std::to_string(N) + ", mpc_horizon " + std::to_string(H) + "); MPPI has ctk_batch_create, plain CEM ctk_cem_batch_create, the "
                     "gradient variant (CTK_OPT_GRADIENT) and the other optimizers run as single handles (ctk_create)");
    if (cfg->predictor != CTK_PRED_ODE)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: the batch kernel descends through the analytic (ODE) predictor only (cfg.predictor == " +
                     std::to_string(cfg->predictor) + ", num_rollouts " + std::to_string(N) + ", mpc_horizon " + std::to_string(H) +
                     "); network predictors run as single handles (ctk_create)");
    if (cfg->environment == CTK_ENV_CARTPOLE && cfg->generic_kernels == 0)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: CartPole's tuned descent (ctk_rpgd_descent, what a handle with generic_kernels == 0 runs) has no "
                     "batch form; the template kernels do: set cfg.generic_kernels = 1, and compare with handles created the same way (num_rollouts " +
                     std::to_string(N) + ", mpc_horizon " + std::to_string(H) + ")");
    if (N > CTK_RPGD_FUSED_MAX_N)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: num_rollouts " + std::to_string(N) + " exceeds " + std::to_string(CTK_RPGD_FUSED_MAX_N) +
                     ", the population one workgroup holds (a problem's whole step runs in one workgroup); such a controller runs as a single handle (ctk_create)");
    if (cfg->opt_keep_k > N)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: opt_keep_k " + std::to_string(cfg->opt_keep_k) + " exceeds num_rollouts " + std::to_string(N) +
                     ": the plans a problem keeps are part of its population");
    if (cfg->materialize_trajectories)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: materialize_trajectories is not built for a batch (num_rollouts " + std::to_string(N) +
                     ", mpc_horizon " + std::to_string(H) + "): the logging rollout sits between descent and warm start, and the one launch has no seam for it; "
                     "such a controller runs as a single handle (ctk_create)");
    bool tape_in_lds = false;
    const size_t lds = ctk_g_rpgd_descent_lds(cfg->environment, H, &tape_in_lds);
    if (lds > 160 * 1024)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: mpc_horizon " + std::to_string(H) + " x " + std::to_string(einfo->C) + " inputs = " +
                     std::to_string(HC) + " columns need " + std::to_string(lds) + " bytes of LDS without the state tape; a workgroup has 163840 (160 KiB)");
    if (cfg->opt_keep_k < 1 || cfg->outer_its < 0 || cfg->resamp_per < 1 || cfg->shift_previous < 0 || (cfg->warmup && cfg->warmup_iterations < 0) ||
        (cfg->sampling_distribution != 0 && cfg->sampling_distribution != 1))
        return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_rpgd_batch_create: RPGD needs opt_keep_k >= 1, outer_its >= 0, resamp_per >= 1, shift_previous >= 0, "
                     "warmup_iterations >= 0, sampling_distribution in {0,1}");
    if (cfg->intermediate_steps != 1)
        return bfail(nullptr, CTK_ERR_UNSUPPORTED, "ctk_rpgd_batch_create: the RPGD adjoint is built for intermediate_steps == 1 (given " + std::to_string(cfg->intermediate_steps) + ")");
    if (cfg->adam_rule != 0 && cfg->adam_rule != 1)
        return bfail(nullptr, CTK_ERR_INVALID_ARGUMENT, "ctk_rpgd_batch_create: adam_rule must be 0 (the reference's torch ADAM) or 1 (tf.keras.optimizers.Adam)");

    hipDeviceProp_t prop;
    if (int rc = probe_device("ctk_rpgd_batch_create", cfg->device, &prop)) return rc;

    Creating<ctk_rpgd_batch> made;
    ctk_rpgd_batch* b = made.p;
    batch_core_init(b, cfg, einfo, n_problems, seeds);
    b->K = cfg->opt_keep_k;
    b->P = num_inducing_points(H, cfg->period_interpolation_inducing_points);
    b->PC = b->P * einfo->C;
    b->kcache.assign((size_t)n_problems * b->kstride, 0);
    b->scratch_stride = tape_in_lds ? 0 : ctk_g_rpgd_scratch_floats(b->env, N, H);
    b->count.assign((size_t)n_problems, 0); b->adam_step.assign((size_t)n_problems, 0);
    b->cur.assign((size_t)n_problems, 0); b->ready.assign((size_t)n_problems, 0);
    b->dominant = ctk_g_rpgd_batch_name(b->env);
    const float first[CTK_RPGD_HYPER_COUNT] = {cfg->learning_rate, cfg->adam_beta_1, cfg->adam_beta_2, cfg->adam_epsilon, cfg->gradmax_clip, cfg->sample_stdev,
                                               cfg->sample_mean, cfg->sample_min, cfg->sample_max, (float)cfg->outer_its, (float)cfg->resamp_per};
    fhyper_init(b, CTK_RPGD_HYPER_COUNT, ctk_rpgd_batch_hyper_bytes(), first);
    b->bc_of.assign((size_t)n_problems, 0);

    if (int rc = batch_core_open(b)) return rc;
    const size_t Bz = (size_t)n_problems, NHC = b->NHC();
    for (int i = 0; i < 2; ++i) {
        HIP_CREATE(b->own.dev_zero(&b->d_pop[i], Bz * NHC * sizeof(float), b->stream));
        HIP_CREATE(b->own.dev_zero(&b->d_m[i], Bz * NHC * sizeof(float), b->stream));
        HIP_CREATE(b->own.dev_zero(&b->d_v[i], Bz * NHC * sizeof(float), b->stream));
        HIP_CREATE(b->own.dev_zero(&b->d_ages[i], Bz * N * sizeof(float), b->stream));
    }
    HIP_CREATE(b->own.dev_zero(&b->d_J, Bz * N * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_idx, Bz * N * sizeof(int), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_unom, Bz * HC * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_scratch, Bz * b->scratch_stride * sizeof(float), b->stream));
    HIP_CREATE(b->own.dev_zero(&b->d_desc, Bz * sizeof(CtkRpgdBatchDesc), b->stream));
    const size_t steps_bytes = Bz * (sizeof(CtkRpgdBatchStep) + b->kstride + b->hbytes);   // the records, then room for as many two-part elements
    HIP_CREATE(b->own.dev_zero(&b->d_steps, steps_bytes, b->stream));
    HIP_CREATE(b->own.pinned_zero(&b->h_steps, steps_bytes));

    std::vector<InterpEntry> tab = build_interp_table(H, cfg->period_interpolation_inducing_points, b->P);
    HIP_CREATE(b->own.dev_zero(&b->d_interp, (size_t)H * sizeof(InterpEntry), b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_interp, tab.data(), (size_t)H * sizeof(InterpEntry), hipMemcpyHostToDevice, b->stream));
    const std::vector<float> bc = adam_bias_corrections(cfg->adam_beta_1, cfg->adam_beta_2);   // the table of a handle (ctk_host.h)
    b->bc_len = (int)(bc.size() / 2);
    HIP_CREATE(b->own.dev_zero(&b->d_bc, bc.size() * sizeof(float), b->stream));
    HIP_CREATE(hipMemcpyAsync(b->d_bc, bc.data(), bc.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    b->bc_tabs.push_back({cfg->adam_beta_1, cfg->adam_beta_2, b->d_bc});
    for (int p = 0; p < n_problems; ++p)
        if (int rc = RpgdFamily::hyper_block(b, p)) { g_create_error = "ctk_rpgd_batch_create: " + b->err; return rc; }

    std::vector<CtkRpgdBatchDesc> desc(Bz);
    for (int p = 0; p < n_problems; ++p) {
        const size_t z = (size_t)p;
        const uint64_t seed = batch_seed(cfg, seeds, p);
        CtkRpgdBatchDesc& d = desc[z];
        for (int i = 0; i < 2; ++i) {
            d.pop[i] = b->d_pop[i] + z * NHC; d.m[i] = b->d_m[i] + z * NHC; d.v[i] = b->d_v[i] + z * NHC;
            d.ages[i] = b->d_ages[i] + z * N;
        }
        d.J = b->d_J + z * N; d.idx = b->d_idx + z * N; d.u_nom = b->d_unom + z * HC;
        d.u_dev = b->u(p); d.u_host = b->h_u_dev + z * 16;
        d.scratch = b->d_scratch + z * b->scratch_stride;
        d.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull); d.seed_hi = (uint32_t)(seed >> 32);
    }
    HIP_CREATE(hipMemcpyAsync(b->d_desc, desc.data(), Bz * sizeof(CtkRpgdBatchDesc), hipMemcpyHostToDevice, b->stream));
    HIP_CREATE(hipStreamSynchronize(b->stream));               // the host vectors go out of scope below
    *out = made.release();
    return CTK_OK;
}

int ctk_rpgd_batch_reset(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* draws, int draws_loc) {
    if (!b) return CTK_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (int rc = batch_ids(b, "ctk_rpgd_batch_reset", n_ids, ids, &n)) return rc;
    const size_t per = (size_t)b->N * b->PC;           // sample_actions of a whole population: [N,P,C] per problem
    const float* d_draws = nullptr;
    if (draws_loc != CTK_LOC_NONE) {
        if (draws == nullptr) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "draws pointer is NULL but draws_loc != CTK_LOC_NONE");
        if (draws_loc != CTK_LOC_DEVICE && draws_loc != CTK_LOC_HOST) return bfail(b, CTK_ERR_INVALID_ARGUMENT, "bad draws_loc");
    }
    BHIP_TRY(b, hipSetDevice(b->cfg.device));
    if (draws_loc == CTK_LOC_DEVICE) d_draws = draws;
    else if (draws_loc == CTK_LOC_HOST) {
        if (int rc = batch_stage(b, draws, (size_t)n * per)) return rc;
        d_draws = b->d_samples;
    }
    for (int j = 0; j < n; ++j) {
        const int p = ids ? ids[j] : j;
        CtkRpgdBatchStep& q = b->h_steps[j];
        q = CtkRpgdBatchStep{};
        q.id = p; q.call = b->call[(size_t)p]; q.cur = b->cur[(size_t)p];
        q.draws = d_draws ? d_draws + (size_t)j * per : nullptr;
    }
    BHIP_TRY(b, hipMemcpyAsync(b->d_steps, b->h_steps, (size_t)n * sizeof(CtkRpgdBatchStep), hipMemcpyHostToDevice, b->stream));
    RolloutArgs a = rpgd_batch_args(b);
    RpgdFusedWarm f = rpgd_batch_warm(b);
    for (int done = 0; done < n;) {                    // ONE launch for the call (more only past the grid's y limit)
        // ... but with per-problem hyper-parameters one per listed problem: the reset kernel takes the sampling constants and the
        // limits by value, and a problem's draws are mapped with ITS values (a reset is not a step: no form of its own for it)
        const int cnt = b->fhyper ? 1 : std::min(RPGD_BATCH_MAX_GRID_Y, n - done);
        if (b->fhyper) {
            const int p = ids ? ids[done] : done;
            const float* r = b->frow_of(p);
            f.sample_stdev = r[CTK_RPGD_HYPER_SAMPLE_STDEV]; f.sample_mean = r[CTK_RPGD_HYPER_SAMPLE_MEAN];
            f.sample_min = r[CTK_RPGD_HYPER_UNIFORM_DIST_MIN]; f.sample_max = r[CTK_RPGD_HYPER_UNIFORM_DIST_MAX];
            for (int c = 0; c < b->C; ++c) { a.lo[c] = b->flow(p)[c]; a.hi[c] = b->fhigh(p)[c]; }
        }
        BHIP_TRY(b, ctk_launch_rpgd_batch_reset(b->stream, a, f, b->d_desc, b->d_steps + done, cnt));
        done += cnt;
    }
    BHIP_TRY(b, hipStreamSynchronize(b->stream));
    for (int j = 0; j < n; ++j) {                      // rpgd_reset of a handle: parameters, the sequence number and the buffer index stay
        const size_t z = (size_t)(ids ? ids[j] : j);
        b->count[z] = 0; b->adam_step[z] = 0; b->ready[z] = 1;
        ++b->call[z];
    }
    return CTK_OK;
}

int ctk_rpgd_batch_step(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u_prev, const float* samples,
                        size_t n_samples, int samples_loc, float* u_out) {
    return batch_step<RpgdFamily>(b, "ctk_rpgd_batch_step", n_ids, ids, s, u_prev, StepDraws{samples, n_samples, samples_loc}, u_out);
}

int ctk_rpgd_batch_read(ctk_rpgd_batch* b, int problem, int buffer, float* dst, size_t cap) {
    if (int rc = batch_read_check(b, "ctk_rpgd_batch_read", problem, dst)) return rc;
    const size_t z = (size_t)problem, N = (size_t)b->N, NHC = b->NHC();
    const int cur = b->cur[z];
    const float* src = nullptr; size_t n = 0; bool is_int = false;
    switch (buffer) {                                  // ctk_api.hip: locate_buffer of an RPGD handle
        case CTK_BUF_Q: src = b->d_pop[cur ^ 1] + z * NHC; n = NHC; break;
        case CTK_BUF_PLAN: src = b->d_pop[cur] + z * NHC; n = NHC; break;
        case CTK_BUF_ADAM_M: src = b->d_m[cur] + z * NHC; n = NHC; break;
        case CTK_BUF_ADAM_V: src = b->d_v[cur] + z * NHC; n = NHC; break;
        case CTK_BUF_AGES: src = b->d_ages[cur] + z * N; n = N; break;
        case CTK_BUF_AGES_LOGGED: src = b->d_ages[cur ^ 1] + z * N; n = N; break;
        case CTK_BUF_J: src = b->d_J + z * N; n = N; break;
        case CTK_BUF_U_NOM: src = b->d_unom + z * b->HC; n = (size_t)b->HC; break;
        case CTK_BUF_BEST_IDX: src = reinterpret_cast<const float*>(b->d_idx + z * N); n = (size_t)b->K; is_int = true; break;
        default: return bfail(b, CTK_ERR_INVALID_ARGUMENT, "ctk_rpgd_batch_read: an RPGD batch has Q, J, U_NOM, PLAN, ADAM_M, ADAM_V, AGES, AGES_LOGGED and BEST_IDX");
    }
    return batch_read_out(b, "ctk_rpgd_batch_read", src, n, is_int, dst, cap);
}

}  // extern "C"
