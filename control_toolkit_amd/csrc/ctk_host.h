// ctk_host.h — host helpers that the two host translation units share: ctk_api.hip (the single handle) defines them, ctk_batch.hip (the
// batch families) uses them; and what both are built from, inline: the owner of every allocation, the scoped device temporary, the
// creation guard and macro, the state list and its walk.  Private to the library: hidden visibility, so none of them is an exported symbol.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctk_launch.h"
#include "ctk_env.h"      // EnvInfo

#pragma GCC visibility push(hidden)
namespace ctk_host {

// the text of a refused creation, of a handle or of a batch of any family: ONE thread-local, read by every *_last_error(NULL)
extern thread_local std::string g_create_error;

const EnvInfo* env_info(int env);   // NULL: not an environment of this library
int num_inducing_points(int H, int p);
std::vector<InterpEntry> build_interp_table(int H, int p, int P);
MppiK mppi_constants(const ctk_config& c);
void default_params(int env, float* p);
std::vector<float> permute_mlp_weights(const float* raw, int S = CTK_S, int C = CTK_C);
size_t weight_count(int predictor, int S, int C, int hid = 32);
size_t shaped_weight_count(int predictor, int S, int C, int h1, int h2);
void embed_mlp_rows(const float* w, int S, int I, int h1, int h2, int W, float* full);
// CartPole's 2 x 32 GRU: a narrower network into the raw layout of the full one, the per-lane table of the full one
// (ctk_launch.h: ctk_mppi_batch_gru_table_floats() floats), the bound on its outputs behind a handle's net_out_bound
void embed_gru_rows(const float* w, int S, int I, int h1, int h2, float* full);
std::vector<float> permute_gru_weights(const float* raw);
float gru_out_bound(const float* raw);
int check_config(const char* who, const ctk_config* cfg, const EnvInfo** einfo_out);
int probe_device(const char* who, int device, hipDeviceProp_t* prop);

// Adam's bias corrections {1 - beta_1^t, 1 - beta_2^t}, t = 1 .. 32768, in double, rounded to fp32 (optimizer_rpgd.py:73-74); beyond the
// table both are exactly 1.0f in fp32
inline std::vector<float> adam_bias_corrections(float beta_1, float beta_2) {
    std::vector<float> bc((size_t)2 * 32768);
    for (size_t tt = 1; 2 * tt <= bc.size(); ++tt) {
        bc[2 * (tt - 1)] = (float)(1.0 - std::pow((double)beta_1, (double)tt));
        bc[2 * (tt - 1) + 1] = (float)(1.0 - std::pow((double)beta_2, (double)tt));
    }
    return bc;
}

// ---- the owner: every device and pinned allocation of a handle or a batch is entered here where it is made; release() frees them ----
struct Owner {
    std::vector<void*> dev, pin;
    bool empty() const { return dev.empty() && pin.empty(); }
    void* own_dev(void* p) { if (p) dev.push_back(p); return p; }
    void* own_pin(void* p) { if (p) pin.push_back(p); return p; }
    void disown(void* p) {
        dev.erase(std::remove(dev.begin(), dev.end(), p), dev.end());
        pin.erase(std::remove(pin.begin(), pin.end(), p), pin.end());
    }
    // a zeroed device allocation of at least one byte (the memset on `stream`); a zeroed pinned allocation with the caller's flags
    template <class T>
    hipError_t dev_zero(T** p, size_t bytes, hipStream_t stream) {
        const hipError_t e = hipMalloc((void**)p, bytes ? bytes : 1);
        if (e == hipSuccess) own_dev(*p);
        return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes ? bytes : 1, stream);
    }
    template <class T>
    hipError_t pinned_zero(T** p, size_t bytes, unsigned flags = hipHostMallocDefault) {
        const hipError_t e = hipHostMalloc((void**)p, bytes, flags);
        if (e == hipSuccess) { own_pin(*p); std::memset(*p, 0, bytes); }
        return e;
    }
    // an early free: the block leaves the owner, the pointer is nulled
    template <class T>
    hipError_t free_dev(T*& p) {
        if (!p) return hipSuccess;
        disown(p);
        const hipError_t e = hipFree(p);
        p = nullptr;
        return e;
    }
    // A buffer that grows on demand, to n elements: the old block is freed and leaves the owner, the new one is allocated and entered.
    // No copy of the contents, no over-allocation; after a failure the buffer is empty (p == nullptr, cap == 0).
    template <class T>
    hipError_t grow_dev(T*& p, size_t& cap, size_t n) {
        if (n <= cap) return hipSuccess;
        cap = 0;
        hipError_t e = free_dev(p);
        if (e == hipSuccess) e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) { own_dev(p); cap = n; }
        return e;
    }
    template <class T>
    hipError_t grow_pin(T*& p, size_t& cap, size_t n) {
        if (n <= cap) return hipSuccess;
        cap = 0;
        disown(p);
        hipError_t e = p ? hipHostFree(p) : hipSuccess;
        p = nullptr;
        if (e == hipSuccess) e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) { own_pin(p); cap = n; }
        return e;
    }
    void release() {
        for (void* p : dev) hipFree(p);
        for (void* p : pin) hipHostFree(p);
        dev.clear(); pin.clear();
    }
};

// a device temporary that ends with its scope, unless it is handed on (release)
struct ScopedDev {
    void* p = nullptr;
    ScopedDev() = default;
    ScopedDev(const ScopedDev&) = delete;
    ScopedDev& operator=(const ScopedDev&) = delete;
    ~ScopedDev() { if (p) hipFree(p); }
    void* release() { void* r = p; p = nullptr; return r; }
};

// a handle or batch under creation: deleted on every return but the one that hands it over
template <class T>
struct Creating { T* p = new T(); ~Creating() { delete p; } T* release() { T* r = p; p = nullptr; return r; } };
// a HIP call of a creation: a failure stores a text that names the call where every *_last_error(NULL) reads it; `Creating` deletes the object
#define HIP_CREATE(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { ctk_host::g_create_error = std::string(#expr) + ": " + hipGetErrorString(_e); return CTK_ERR_HIP; } } while (0)

// ---- a state as an ordered list of items: a device segment {dev, n} or one host counter {counter} stored as one float ----
struct StateItem { float* dev; size_t n; int* counter; };
inline StateItem state_seg(float* dev, size_t n) { return {dev, n, nullptr}; }
inline StateItem state_counter(int* c) { return {nullptr, 1, c}; }
inline size_t state_floats(const std::vector<StateItem>& items) {
    size_t n = 0;
    for (const StateItem& it : items) n += it.n;
    return n;
}
// get (device to host) or set (host to device) through host[state_floats(items)]: the copies in the list's order, ONE synchronisation;
// set writes the counters ahead of it, get reads them behind it (host writes to other addresses than the copies')
inline hipError_t state_walk(const std::vector<StateItem>& items, float* host, bool get, hipStream_t stream) {
    float* at = host;
    for (const StateItem& it : items) {
        if (it.counter) { if (!get) *it.counter = (int)*at; }
        else if (hipError_t e = hipMemcpyAsync(get ? at : it.dev, get ? it.dev : at, it.n * sizeof(float), get ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, stream)) return e;
        at += it.n;
    }
    if (hipError_t e = hipStreamSynchronize(stream)) return e;
    at = host;
    for (const StateItem& it : items) { if (get && it.counter) *at = (float)*it.counter; at += it.n; }
    return hipSuccess;
}

}  // namespace ctk_host
#pragma GCC visibility pop
