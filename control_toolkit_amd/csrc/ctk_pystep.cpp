// control_toolkit_amd._ctk_pystep: a pre-bound call of ctk_step for CtkEngine.step (control_toolkit_amd/_capi.py).
//
// The ctypes path marshals six arguments per step and copies the state through two ndarray temporaries; everything but the
// state's (and u_prev's) few floats is the same every call.  bind() fixes the function address, the handle, S, C and the output
// buffer once; the returned object is called with (s, u_prev, samples_ptr, samples_loc) through vectorcall, copies the floats
// out of the arguments' buffers into its own arrays and calls ctk_step with the GIL released.
//
// CPython C API + buffer protocol only (no numpy C API); the module does not link libctk_hip.so: the address comes from
// whichever library the engine loaded, so libraries with a user environment compiled in work unchanged.
//
// Anything that is not a C-contiguous float32 buffer of the right size makes the call return NotImplemented WITHOUT calling
// ctk_step: the Python wrapper then runs its ctypes path with its conversions and error texts.
//
// Two more bound objects sit above it, with the same rule (NotImplemented = nothing has happened, the Python body runs):
// bind_optimizer() -> the MPPI optimizer's whole step, bind_controller() -> controller_mpc.step.  They are further down.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <climits>
#include <cstddef>
#include <cstring>

namespace {

typedef int (*step_fn)(void* h, const float* s, const float* u_prev, const float* samples, int samples_loc, float* u_out);

constexpr int MAX_DIM = 64;   // well above include/ctk_hip.h's CTK_MAX_STATES / CTK_MAX_INPUTS; bind() refuses more

struct BoundStep {
    PyObject_HEAD
    vectorcallfunc vectorcall;
    step_fn fn;
    void* handle;          // NULL after invalidate()
    int S, C;
    Py_buffer out;         // the engine's u_out array: one reference for the object's lifetime
    float s[MAX_DIM];
    float up[MAX_DIM];
};

// native-order 4-byte float: numpy exports "f"; "@f" / "=f" / "<f" name the same thing on the little-endian hosts this runs on
bool is_f32(const Py_buffer& v) {
    if (v.itemsize != (Py_ssize_t)sizeof(float)) return false;
    const char* f = v.format;
    if (!f) return false;   // no format = unsigned bytes
    if (*f == '@' || *f == '=' || *f == '<') ++f;
    return f[0] == 'f' && f[1] == '\0';
}

// 1: copied n floats into dst; 0: not a fast-path argument (no exception set); the view is released on every path
int take_floats(PyObject* obj, Py_ssize_t at_least, bool exact, int n, float* dst) {
    if (!PyObject_CheckBuffer(obj)) return 0;
    Py_buffer v;
    if (PyObject_GetBuffer(obj, &v, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) != 0) {   // non-contiguous, or an exporter without formats
        PyErr_Clear();
        return 0;
    }
    int ok = 0;
    if (is_f32(v)) {
        const Py_ssize_t count = v.len / (Py_ssize_t)sizeof(float);
        if (exact ? count == at_least : count >= at_least) {
            std::memcpy(dst, v.buf, (size_t)n * sizeof(float));
            ok = 1;
        }
    }
    PyBuffer_Release(&v);
    return ok;
}

PyObject* not_fast() { Py_RETURN_NOTIMPLEMENTED; }

PyObject* bound_call(PyObject* self_, PyObject* const* args, size_t nargsf, PyObject* kwnames) {
    BoundStep* self = (BoundStep*)self_;
    if (PyVectorcall_NARGS(nargsf) != 4 || (kwnames && PyTuple_GET_SIZE(kwnames) != 0)) {
        PyErr_SetString(PyExc_TypeError, "bound step takes (s, u_prev, samples_ptr, samples_loc)");
        return nullptr;
    }
    void* const handle = self->handle;
    if (!handle) return not_fast();
    // samples_ptr: None or an int address; samples_loc: int
    const float* samples = nullptr;
    if (args[2] != Py_None) {
        if (!PyLong_Check(args[2])) { PyErr_SetString(PyExc_TypeError, "samples_ptr must be None or an int"); return nullptr; }
        samples = (const float*)PyLong_AsVoidPtr(args[2]);
        if (!samples && PyErr_Occurred()) return nullptr;
    }
    const long loc = PyLong_AsLong(args[3]);
    if (loc == -1 && PyErr_Occurred()) return nullptr;
    if (!take_floats(args[0], self->S, true, self->S, self->s)) return not_fast();
    const float* up = nullptr;
    if (args[1] != Py_None) {
        if (!take_floats(args[1], self->C, false, self->C, self->up)) return not_fast();
        up = self->up;
    }
    const step_fn fn = self->fn;
    float* const u_out = (float*)self->out.buf;
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = fn(handle, self->s, up, samples, (int)loc, u_out);
    Py_END_ALLOW_THREADS
    return PyLong_FromLong(rc);
}

PyObject* bound_invalidate(PyObject* self, PyObject*) {
    ((BoundStep*)self)->handle = nullptr;
    Py_RETURN_NONE;
}

PyObject* bound_valid(PyObject* self, void*) { return PyBool_FromLong(((BoundStep*)self)->handle != nullptr); }

void bound_dealloc(PyObject* self_) {
    BoundStep* self = (BoundStep*)self_;
    if (self->out.obj) PyBuffer_Release(&self->out);
    Py_TYPE(self_)->tp_free(self_);
}

PyMethodDef bound_methods[] = {
    {"invalidate", bound_invalidate, METH_NOARGS, "forget the handle: later calls return NotImplemented and never reach ctk_step"},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef bound_getset[] = {
    {"valid", bound_valid, nullptr, "False after invalidate()", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject BoundStepType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* bind(PyObject*, PyObject* args) {
    PyObject *fn_addr, *handle_addr, *u_out;
    int S, C;
    if (!PyArg_ParseTuple(args, "O!O!iiO:bind", &PyLong_Type, &fn_addr, &PyLong_Type, &handle_addr, &S, &C, &u_out)) return nullptr;
    void* fn = PyLong_AsVoidPtr(fn_addr);
    if (!fn) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, "bind: step_fn_addr is 0"); return nullptr; }
    void* handle = PyLong_AsVoidPtr(handle_addr);
    if (!handle) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, "bind: handle_addr is 0"); return nullptr; }
    if (S < 1 || S > MAX_DIM || C < 1 || C > MAX_DIM) { PyErr_Format(PyExc_ValueError, "bind: S and C must be in 1..%d", MAX_DIM); return nullptr; }
    BoundStep* self = (BoundStep*)BoundStepType.tp_alloc(&BoundStepType, 0);
    if (!self) return nullptr;
    self->out.obj = nullptr;
    if (PyObject_GetBuffer(u_out, &self->out, PyBUF_WRITABLE | PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) != 0) { Py_DECREF(self); return nullptr; }
    if (!is_f32(self->out) || self->out.len != (Py_ssize_t)(C * sizeof(float))) {
        PyErr_Format(PyExc_ValueError, "bind: u_out must be a writable float32 buffer of %d entries", C);
        Py_DECREF(self);
        return nullptr;
    }
    self->vectorcall = bound_call;
    self->fn = (step_fn)fn;
    self->handle = handle;
    self->S = S; self->C = C;
    return (PyObject*)self;
}

// ---- the optimizer's whole step in one call (Optimizers/optimizer_mppi_hip.py: step) ---------------------------------------------------
//
// BoundOptimizerStep does what optimizer_mppi_hip.step does when nothing special is going on: guards, samples from the rng object,
// u_prev, ctk_step with the GIL released, publish, _lazy.clear().  The CEM and random-action steps are the same sequence with two
// flagged differences (STEP_* below).  It is called as fast(s) and returns the u object, or NotImplemented
// BEFORE any side effect (no cursor moved, ctk_step not called); the Python body then runs unchanged.  The per-step key of
// template_optimizer._sync_parameters is replaced by a snapshot (below) that is compared value by value without building tuples.

constexpr int MAX_PARAMS = 64;   // entries of one parameter dictionary a snapshot can hold; more: the snapshot is invalid (Python path)

PyObject *s_optimizer_logging, *s_calculate_optimal_trajectory, *s_engine, *s_step, *s_u, *s_u_public, *s_u_vec, *s_rng, *s_lazy,
         *s_cost_function, *s_predictor, *s_version, *s_parameters, *s_variable_parameters, *s_pointers, *s_i, *s_check, *s_copy,
         *s_reload_flag, *s_controller_logging, *s_optimizer, *s_count, *s_warmup;

// borrowed, nullptr when absent (no exception left behind)
PyObject* dict_get(PyObject* d, PyObject* key) {
    PyObject* v = PyDict_GetItemWithError(d, key);
    if (!v && PyErr_Occurred()) PyErr_Clear();
    return v;
}

// new reference, nullptr when absent (no exception left behind)
PyObject* attr_or_null(PyObject* o, PyObject* name) {
    PyObject* v = PyObject_GetAttr(o, name);
    if (!v) PyErr_Clear();
    return v;
}

// 1 / 0 / 0 with the error cleared: a value whose truth cannot be told is left to the Python path
bool is_true(PyObject* v) {
    const int t = PyObject_IsTrue(v);
    if (t < 0) PyErr_Clear();
    return t != 0;
}

// the double of an exact float, int or bool, or of a 0-d float32 / float64 buffer (NumPy scalars and 0-d arrays); false for anything
// else and for NaN, which never compares equal
bool as_double(PyObject* v, double* out) {
    double x;
    if (PyFloat_CheckExact(v)) x = PyFloat_AS_DOUBLE(v);
    else if (PyBool_Check(v)) x = (v == Py_True) ? 1.0 : 0.0;
    else if (PyLong_CheckExact(v)) {
        x = PyLong_AsDouble(v);
        if (x == -1.0 && PyErr_Occurred()) { PyErr_Clear(); return false; }
    } else if (PyObject_CheckBuffer(v)) {
        Py_buffer b;
        if (PyObject_GetBuffer(v, &b, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) != 0) { PyErr_Clear(); return false; }
        bool ok = false;
        const char* f = b.format;
        if (b.ndim == 0 && f) {
            if (*f == '@' || *f == '=' || *f == '<') ++f;
            if (f[0] == 'f' && !f[1] && b.len == (Py_ssize_t)sizeof(float)) { float t; std::memcpy(&t, b.buf, sizeof t); x = t; ok = true; }
            else if (f[0] == 'd' && !f[1] && b.len == (Py_ssize_t)sizeof(double)) { std::memcpy(&x, b.buf, sizeof x); ok = true; }
        }
        PyBuffer_Release(&b);
        if (!ok) return false;
    } else return false;
    if (x != x) return false;
    *out = x;
    return true;
}

// identity, length and values (in iteration order) of one parameter dictionary
struct DictSnap {
    PyObject* dict;   // strong
    Py_ssize_t n;
    double vals[MAX_PARAMS];
};

bool dictsnap_take(DictSnap* d, PyObject* dict) {   // dict: borrowed; d->dict must be nullptr
    if (!dict || !PyDict_CheckExact(dict) || PyDict_GET_SIZE(dict) > MAX_PARAMS) return false;
    Py_ssize_t pos = 0, i = 0;
    PyObject *k, *v;
    while (PyDict_Next(dict, &pos, &k, &v))
        if (!as_double(v, &d->vals[i++])) return false;
    d->n = i;
    Py_INCREF(dict);
    d->dict = dict;
    return true;
}

bool dictsnap_same(const DictSnap* d, PyObject* dict) {
    if (dict != d->dict || PyDict_GET_SIZE(dict) != d->n) return false;
    Py_ssize_t pos = 0, i = 0;
    PyObject *k, *v;
    double x;
    while (PyDict_Next(dict, &pos, &k, &v)) {
        if (i >= d->n || !as_double(v, &x) || x != d->vals[i]) return false;
        ++i;
    }
    return i == d->n;
}

struct BoundOptimizerStep {
    PyObject_HEAD
    vectorcallfunc vectorcall;
    // fixed at bind_optimizer(); all strong
    PyObject *opt, *opt_dict, *engine, *engine_dict, *u_arr, *param_names, *rng_device, *rng_buffer;
    BoundStep* bound;
    int flags;   // STEP_* below: what the optimizer's step does around the sequence they all share
    // the parameter snapshot (resync())
    PyObject *cf, *pred, *vp, *vp_dict;
    PyObject* vp_names[MAX_PARAMS];   // the engine parameter names found in vp_dict: strong
    double vp_vals[MAX_PARAMS];
    Py_ssize_t vp_n, vp_len;
    double version;
    DictSnap cf_params, pred_params;
    bool snap_valid, stale, closed, last_native;
    unsigned long long native_steps, declined_steps;
};

// the steps differ in two places only (Optimizers/optimizer_mppi_hip.py, optimizer_cem_hip.py, optimizer_random_action_hip.py)
constexpr int STEP_CLEARS_LAZY = 1;   // MPPI: _lazy.clear() after the publish
constexpr int STEP_COUNTS = 2;        // CEM: count += 1 at the end; the first step of a warm-up run (warmup and count == 0) stays in Python

// cost_function.variable_parameters or predictor.variable_parameters, as _sync_parameters picks it: new reference or nullptr (none)
PyObject* pick_vp(PyObject* cf, PyObject* pred) {
    PyObject* vp = attr_or_null(cf, s_variable_parameters);
    if (vp && !is_true(vp)) Py_CLEAR(vp);
    if (!vp) {
        vp = attr_or_null(pred, s_variable_parameters);
        if (vp && (vp == Py_None || !is_true(vp))) Py_CLEAR(vp);
    }
    return vp;
}

void snap_clear(BoundOptimizerStep* self) {
    Py_CLEAR(self->cf); Py_CLEAR(self->pred); Py_CLEAR(self->vp); Py_CLEAR(self->vp_dict);
    Py_CLEAR(self->cf_params.dict); Py_CLEAR(self->pred_params.dict);
    for (Py_ssize_t i = 0; i < self->vp_n; ++i) Py_CLEAR(self->vp_names[i]);
    self->vp_n = 0;
    self->snap_valid = false;
}

// takes the snapshot again from the objects the optimizer holds now; anything outside the build's own wrappers leaves it invalid, and
// every step is then declined (the Python path keys the parameters itself)
void snap_take(BoundOptimizerStep* self) {
    snap_clear(self);
    self->stale = false;
    PyObject* cf = dict_get(self->opt_dict, s_cost_function);
    PyObject* pred = dict_get(self->opt_dict, s_predictor);
    if (!cf || !pred) return;
    Py_INCREF(cf); self->cf = cf;
    Py_INCREF(pred); self->pred = pred;
    PyObject* ver = attr_or_null(cf, s_version);
    bool ok = ver && as_double(ver, &self->version);
    Py_XDECREF(ver);
    if (!ok) return;
    PyObject* p = attr_or_null(cf, s_parameters);
    ok = dictsnap_take(&self->cf_params, p);
    Py_XDECREF(p);
    if (!ok) return;
    p = attr_or_null(pred, s_parameters);
    ok = dictsnap_take(&self->pred_params, p);
    Py_XDECREF(p);
    if (!ok) return;
    self->vp = pick_vp(cf, pred);
    self->vp_len = 0;
    if (self->vp) {
        self->vp_dict = PyObject_GenericGetDict(self->vp, nullptr);
        if (!self->vp_dict) { PyErr_Clear(); return; }
        if (!PyDict_CheckExact(self->vp_dict)) return;
        self->vp_len = PyDict_GET_SIZE(self->vp_dict);
        const Py_ssize_t n = PyTuple_GET_SIZE(self->param_names);
        for (Py_ssize_t i = 0; i < n; ++i) {
            PyObject* name = PyTuple_GET_ITEM(self->param_names, i);
            PyObject* v = dict_get(self->vp_dict, name);
            if (!v) continue;
            if (self->vp_n >= MAX_PARAMS || !as_double(v, &self->vp_vals[self->vp_n])) return;
            Py_INCREF(name);
            self->vp_names[self->vp_n++] = name;
        }
    }
    self->snap_valid = true;
}

bool snap_same(BoundOptimizerStep* self) {
    PyObject* const cf = dict_get(self->opt_dict, s_cost_function);
    PyObject* const pred = dict_get(self->opt_dict, s_predictor);
    if (cf != self->cf || pred != self->pred) return false;
    double x;
    PyObject* o = attr_or_null(cf, s_version);
    bool ok = o && as_double(o, &x) && x == self->version;
    Py_XDECREF(o);
    if (!ok) return false;
    o = attr_or_null(cf, s_parameters);
    ok = o && dictsnap_same(&self->cf_params, o);
    Py_XDECREF(o);
    if (!ok) return false;
    o = attr_or_null(pred, s_parameters);
    ok = o && dictsnap_same(&self->pred_params, o);
    Py_XDECREF(o);
    if (!ok) return false;
    o = pick_vp(cf, pred);
    ok = (o == self->vp);
    Py_XDECREF(o);
    if (!ok) return false;
    if (self->vp) {
        if (PyDict_GET_SIZE(self->vp_dict) != self->vp_len) return false;
        for (Py_ssize_t i = 0; i < self->vp_n; ++i) {
            PyObject* v = dict_get(self->vp_dict, self->vp_names[i]);
            if (!v || !as_double(v, &x) || x != self->vp_vals[i]) return false;
        }
    }
    return true;
}

// a strong reference for a scope: what a step borrowed from the optimizer's __dict__ must outlive the attribute reads and the GIL-free call
struct Hold {
    PyObject* o;
    explicit Hold(PyObject* p) : o(p) { Py_XINCREF(o); }
    ~Hold() { Py_XDECREF(o); }
    Hold(const Hold&) = delete;
    Hold& operator=(const Hold&) = delete;
};

PyObject* opt_declined(BoundOptimizerStep* self) {
    self->last_native = false;
    ++self->declined_steps;
    return not_fast();
}

// one step; s: borrowed.  Returns u (new reference), NotImplemented (nothing has happened) or nullptr with an exception set.
PyObject* opt_step(BoundOptimizerStep* self, PyObject* s) {
    BoundStep* const bs = self->bound;
    PyObject* const d = self->opt_dict;
    if (self->closed || !self->snap_valid) return opt_declined(self);
    PyObject* v = dict_get(d, s_optimizer_logging);
    if (!v || is_true(v)) return opt_declined(self);
    v = dict_get(d, s_calculate_optimal_trajectory);
    if (!v || is_true(v)) return opt_declined(self);
    if (dict_get(d, s_engine) != self->engine) return opt_declined(self);
    if (dict_get(self->engine_dict, s_step)) return opt_declined(self);   // somebody wrapped engine.step: theirs must run
    void* const handle = bs->handle;
    if (!handle) return opt_declined(self);
    PyObject* const u_now = dict_get(d, s_u);
    if (!u_now || u_now != dict_get(d, s_u_public)) return opt_declined(self);   // a caller assigned u: _u_prev() converts it
    PyObject* const rng = dict_get(d, s_rng);
    if (!rng) return opt_declined(self);
    const Hold hold_rng(rng);
    const bool from_buffer = (PyObject*)Py_TYPE(rng) == self->rng_buffer;
    if (!from_buffer && (PyObject*)Py_TYPE(rng) != self->rng_device) return opt_declined(self);
    PyObject* lazy = nullptr;
    if (self->flags & STEP_CLEARS_LAZY) {
        lazy = dict_get(d, s_lazy);
        if (!lazy || !PyDict_CheckExact(lazy)) return opt_declined(self);
    }
    const Hold hold_lazy(lazy);
    long count = 0;
    if (self->flags & STEP_COUNTS) {
        PyObject* const c = dict_get(d, s_count);
        PyObject* const w = dict_get(d, s_warmup);
        if (!c || !w || !PyLong_CheckExact(c)) return opt_declined(self);
        count = PyLong_AsLong(c);
        if (count == -1 && PyErr_Occurred()) { PyErr_Clear(); return opt_declined(self); }
        if (count < 0 || count == LONG_MAX || (count == 0 && is_true(w))) return opt_declined(self);
    }
    if (!PyObject_CheckBuffer(s)) return opt_declined(self);
    {   // exactly [S] float32, C-contiguous; anything else goes through _prepare_state
        Py_buffer b;
        if (PyObject_GetBuffer(s, &b, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) != 0) { PyErr_Clear(); return opt_declined(self); }
        const bool ok = b.ndim == 1 && is_f32(b) && b.len == (Py_ssize_t)(bs->S * sizeof(float));
        if (ok) std::memcpy(bs->s, b.buf, (size_t)bs->S * sizeof(float));
        PyBuffer_Release(&b);
        if (!ok) return opt_declined(self);
    }
    const float* up = nullptr;
    v = dict_get(d, s_u_vec);
    if (!v) return opt_declined(self);
    if (v != Py_None) {
        if (!take_floats(v, bs->C, false, bs->C, bs->up)) return opt_declined(self);
        up = bs->up;
    }
    // DeviceBufferRng.normal(): pointers[_i], then _i = (_i + 1) % len(pointers); the object keeps the cursor
    const float* samples = nullptr;
    int loc = 0;   // LOC_NONE
    PyObject* next_i = nullptr;
    if (from_buffer) {
        PyObject* ptrs = attr_or_null(rng, s_pointers);
        PyObject* cur = attr_or_null(rng, s_i);
        bool ok = ptrs && cur && PyList_CheckExact(ptrs) && PyLong_CheckExact(cur) && PyList_GET_SIZE(ptrs) > 0;
        if (ok) {
            const Py_ssize_t n = PyList_GET_SIZE(ptrs), i = PyLong_AsSsize_t(cur);
            if (i == -1 && PyErr_Occurred()) PyErr_Clear();
            ok = i >= 0 && i < n && PyLong_CheckExact(PyList_GET_ITEM(ptrs, i));
            if (ok) {
                samples = (const float*)PyLong_AsVoidPtr(PyList_GET_ITEM(ptrs, i));
                if (!samples && PyErr_Occurred()) { PyErr_Clear(); ok = false; }
            }
            if (ok) {
                next_i = PyLong_FromSsize_t((i + 1) % n);
                if (!next_i) { PyErr_Clear(); ok = false; }
            }
        }
        Py_XDECREF(ptrs); Py_XDECREF(cur);
        if (!ok) return opt_declined(self);
        loc = 2;   // LOC_DEVICE
    }
    if (!snap_same(self)) {
        Py_XDECREF(next_i);
        self->stale = true;
        return opt_declined(self);
    }
    // every guard has passed: from here on the step happens
    if (next_i) {
        const int rc = PyObject_SetAttr(rng, s_i, next_i);
        Py_DECREF(next_i);
        if (rc != 0) return nullptr;
    }
    self->last_native = true;
    ++self->native_steps;
    const step_fn fn = bs->fn;
    float* const u_out = (float*)bs->out.buf;
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = fn(handle, bs->s, up, samples, loc, u_out);
    Py_END_ALLOW_THREADS
    PyObject *u_vec = nullptr, *u = nullptr;
    if (rc) {   // the engine's own exception and text
        PyObject* code = PyLong_FromLong(rc);
        PyObject* r = code ? PyObject_CallMethodOneArg(self->engine, s_check, code) : nullptr;
        Py_XDECREF(code);
        if (!r) goto fail;
        Py_DECREF(r);
    }
    u_vec = PyObject_CallMethodNoArgs(self->u_arr, s_copy);
    if (!u_vec) goto fail;
    if (bs->C == 1) u = PySequence_GetItem(u_vec, 0);
    else { u = u_vec; Py_INCREF(u); }
    if (!u) goto fail;
    if (PyObject_SetAttr(self->opt, s_u_vec, u_vec) != 0 || PyObject_SetAttr(self->opt, s_u, u) != 0 ||
        PyObject_SetAttr(self->opt, s_u_public, u) != 0) goto fail;
    if (lazy) PyDict_Clear(lazy);
    if (self->flags & STEP_COUNTS) {
        PyObject* next = PyLong_FromLong(count + 1);
        const int failed = next ? PyObject_SetAttr(self->opt, s_count, next) : -1;
        Py_XDECREF(next);
        if (failed) goto fail;
    }
    Py_DECREF(u_vec);
    return u;
fail:
    Py_XDECREF(u_vec);
    Py_XDECREF(u);
    return nullptr;
}

PyObject* opt_call(PyObject* self, PyObject* const* args, size_t nargsf, PyObject* kwnames) {
    if (PyVectorcall_NARGS(nargsf) != 1 || (kwnames && PyTuple_GET_SIZE(kwnames) != 0)) {
        PyErr_SetString(PyExc_TypeError, "bound optimizer step takes (s)");
        return nullptr;
    }
    return opt_step((BoundOptimizerStep*)self, args[0]);
}

PyObject* opt_resync(PyObject* self, PyObject*) {
    snap_take((BoundOptimizerStep*)self);
    return PyBool_FromLong(((BoundOptimizerStep*)self)->snap_valid);
}

PyObject* opt_invalidate(PyObject* self, PyObject*) {
    ((BoundOptimizerStep*)self)->closed = true;
    Py_RETURN_NONE;
}

PyObject* opt_get_valid(PyObject* self, void*) {
    BoundOptimizerStep* o = (BoundOptimizerStep*)self;
    return PyBool_FromLong(!o->closed && o->bound && o->bound->handle);
}
PyObject* opt_get_snapshot_valid(PyObject* self, void*) { return PyBool_FromLong(((BoundOptimizerStep*)self)->snap_valid); }
PyObject* opt_get_stale(PyObject* self, void*) { return PyBool_FromLong(((BoundOptimizerStep*)self)->stale); }
PyObject* opt_get_last_native(PyObject* self, void*) { return PyBool_FromLong(((BoundOptimizerStep*)self)->last_native); }
PyObject* opt_get_native_steps(PyObject* self, void*) { return PyLong_FromUnsignedLongLong(((BoundOptimizerStep*)self)->native_steps); }
PyObject* opt_get_declined_steps(PyObject* self, void*) { return PyLong_FromUnsignedLongLong(((BoundOptimizerStep*)self)->declined_steps); }

int opt_traverse(PyObject* self_, visitproc visit, void* arg) {
    BoundOptimizerStep* self = (BoundOptimizerStep*)self_;
    Py_VISIT(self->opt); Py_VISIT(self->opt_dict); Py_VISIT(self->engine); Py_VISIT(self->engine_dict); Py_VISIT(self->u_arr);
    Py_VISIT(self->param_names); Py_VISIT(self->rng_device); Py_VISIT(self->rng_buffer); Py_VISIT((PyObject*)self->bound);
    Py_VISIT(self->cf); Py_VISIT(self->pred); Py_VISIT(self->vp); Py_VISIT(self->vp_dict);
    Py_VISIT(self->cf_params.dict); Py_VISIT(self->pred_params.dict);
    return 0;
}

int opt_clear(PyObject* self_) {
    BoundOptimizerStep* self = (BoundOptimizerStep*)self_;
    self->closed = true;
    snap_clear(self);
    Py_CLEAR(self->opt); Py_CLEAR(self->opt_dict); Py_CLEAR(self->engine); Py_CLEAR(self->engine_dict); Py_CLEAR(self->u_arr);
    Py_CLEAR(self->param_names); Py_CLEAR(self->rng_device); Py_CLEAR(self->rng_buffer);
    BoundStep* b = self->bound;
    self->bound = nullptr;
    Py_XDECREF((PyObject*)b);
    return 0;
}

void opt_dealloc(PyObject* self) {
    PyObject_GC_UnTrack(self);
    opt_clear(self);
    Py_TYPE(self)->tp_free(self);
}

PyMethodDef opt_methods[] = {
    {"resync", opt_resync, METH_NOARGS, "take the parameter snapshot again (after _sync_parameters uploaded); returns whether it is usable"},
    {"invalidate", opt_invalidate, METH_NOARGS, "the engine is closing: later calls return NotImplemented and never reach ctk_step"},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef opt_getset[] = {
    {"valid", opt_get_valid, nullptr, "False after invalidate() or once the engine's bound call is closed", nullptr},
    {"snapshot_valid", opt_get_snapshot_valid, nullptr, "False: the parameter objects are not the build's own wrappers' (every step declined)", nullptr},
    {"stale", opt_get_stale, nullptr, "a step was declined because the snapshot differed; cleared by resync()", nullptr},
    {"last_native", opt_get_last_native, nullptr, "the last call stepped here (False: it returned NotImplemented)", nullptr},
    {"native_steps", opt_get_native_steps, nullptr, "calls that stepped here", nullptr},
    {"declined_steps", opt_get_declined_steps, nullptr, "calls that returned NotImplemented", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject BoundOptimizerStepType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* bind_optimizer(PyObject*, PyObject* args) {
    PyObject *opt, *engine, *bound, *u_arr, *param_names, *rng_device, *rng_buffer;
    int flags;
    if (!PyArg_ParseTuple(args, "OOO!OO!O!O!i:bind_optimizer", &opt, &engine, &BoundStepType, &bound, &u_arr, &PyTuple_Type, &param_names,
                          &PyType_Type, &rng_device, &PyType_Type, &rng_buffer, &flags)) return nullptr;
    if (flags & ~(STEP_CLEARS_LAZY | STEP_COUNTS)) { PyErr_SetString(PyExc_ValueError, "bind_optimizer: unknown step flags"); return nullptr; }
    BoundStep* bs = (BoundStep*)bound;
    if (!bs->handle) { PyErr_SetString(PyExc_ValueError, "bind_optimizer: the engine's bound step is closed"); return nullptr; }
    for (Py_ssize_t i = 0; i < PyTuple_GET_SIZE(param_names); ++i)
        if (!PyUnicode_CheckExact(PyTuple_GET_ITEM(param_names, i))) { PyErr_SetString(PyExc_TypeError, "bind_optimizer: param_names must be a tuple of str"); return nullptr; }
    {   // u_arr must be the array whose memory the bound step writes: its copy() is what a step publishes
        Py_buffer b;
        if (PyObject_GetBuffer(u_arr, &b, PyBUF_SIMPLE) != 0) return nullptr;
        const bool same = b.buf == bs->out.buf && b.len == bs->out.len;
        PyBuffer_Release(&b);
        if (!same) { PyErr_SetString(PyExc_ValueError, "bind_optimizer: u_out is not the bound step's output array"); return nullptr; }
    }
    PyObject* opt_dict = PyObject_GenericGetDict(opt, nullptr);
    if (!opt_dict) return nullptr;
    PyObject* engine_dict = PyObject_GenericGetDict(engine, nullptr);
    if (!engine_dict) { Py_DECREF(opt_dict); return nullptr; }
    if (!PyDict_CheckExact(opt_dict) || !PyDict_CheckExact(engine_dict)) {
        Py_DECREF(opt_dict); Py_DECREF(engine_dict);
        PyErr_SetString(PyExc_TypeError, "bind_optimizer: optimizer and engine must keep their attributes in a plain __dict__");
        return nullptr;
    }
    BoundOptimizerStep* self = (BoundOptimizerStep*)BoundOptimizerStepType.tp_alloc(&BoundOptimizerStepType, 0);   // zero-filled
    if (!self) { Py_DECREF(opt_dict); Py_DECREF(engine_dict); return nullptr; }
    self->vectorcall = opt_call;
    Py_INCREF(opt); self->opt = opt;
    self->opt_dict = opt_dict;
    Py_INCREF(engine); self->engine = engine;
    self->engine_dict = engine_dict;
    Py_INCREF(u_arr); self->u_arr = u_arr;
    Py_INCREF(param_names); self->param_names = param_names;
    Py_INCREF(rng_device); self->rng_device = rng_device;
    Py_INCREF(rng_buffer); self->rng_buffer = rng_buffer;
    Py_INCREF(bound); self->bound = bs;
    self->flags = flags;
    snap_take(self);
    return (PyObject*)self;
}

// ---- controller_mpc.step (Controllers/controller_mpc.py) ---------------------------------------------------------------------------------
//
// BoundControllerStep stands where controller_mpc.configure puts its step: (s, time=None, updated_attributes={}).  With no cost reload
// pending, no updated attributes and no logging, the Python step is the optimizer's step and three calls that do nothing; then the
// optimizer's bound step is called directly.  Everything else, and NotImplemented from there, is the original method with the
// caller's own arguments.
struct BoundControllerStep {
    PyObject_HEAD
    vectorcallfunc vectorcall;
    PyObject *ctrl_dict, *opt, *py_step;   // strong
    BoundOptimizerStep* fast;              // strong
    unsigned long long native_steps, python_steps;
};

PyObject* ctrl_call(PyObject* self_, PyObject* const* args, size_t nargsf, PyObject* kwnames) {
    BoundControllerStep* self = (BoundControllerStep*)self_;
    const Py_ssize_t nargs = PyVectorcall_NARGS(nargsf), nkw = kwnames ? PyTuple_GET_SIZE(kwnames) : 0;
    PyObject *s = nargs >= 1 ? args[0] : nullptr, *ua = nargs >= 3 ? args[2] : nullptr;
    bool plain = nargs <= 3;
    for (Py_ssize_t k = 0; plain && k < nkw; ++k) {
        PyObject* name = PyTuple_GET_ITEM(kwnames, k);
        if (PyUnicode_CompareWithASCIIString(name, "time") == 0) plain = nargs < 2;
        else if (PyUnicode_CompareWithASCIIString(name, "updated_attributes") == 0) { plain = nargs < 3; ua = args[nargs + k]; }
        else if (PyUnicode_CompareWithASCIIString(name, "s") == 0) { plain = nargs < 1; s = args[nargs + k]; }
        else plain = false;
    }
    if (plain && s && self->fast && !self->fast->closed && self->ctrl_dict && (!ua || (PyDict_CheckExact(ua) && PyDict_GET_SIZE(ua) == 0))) {
        PyObject* cf = dict_get(self->ctrl_dict, s_cost_function);
        PyObject* flag = cf ? attr_or_null(cf, s_reload_flag) : nullptr;
        PyObject* logging = dict_get(self->ctrl_dict, s_controller_logging);
        const bool ok = flag && !is_true(flag) && logging && !is_true(logging) && dict_get(self->ctrl_dict, s_optimizer) == self->opt &&
                        !dict_get(self->fast->opt_dict, s_step);
        Py_XDECREF(flag);
        if (ok) {
            PyObject* u = opt_step(self->fast, s);
            if (u != Py_NotImplemented) {
                if (u) ++self->native_steps;
                return u;
            }
            Py_DECREF(u);
        }
    }
    ++self->python_steps;
    if (!self->py_step) { PyErr_SetString(PyExc_RuntimeError, "the controller of this bound step is gone"); return nullptr; }
    return PyObject_Vectorcall(self->py_step, args, (size_t)nargs, kwnames);
}

PyObject* ctrl_get_native_steps(PyObject* self, void*) { return PyLong_FromUnsignedLongLong(((BoundControllerStep*)self)->native_steps); }
PyObject* ctrl_get_python_steps(PyObject* self, void*) { return PyLong_FromUnsignedLongLong(((BoundControllerStep*)self)->python_steps); }
PyObject* ctrl_get_wrapped(PyObject* self, void*) {
    PyObject* f = ((BoundControllerStep*)self)->py_step;
    if (!f) Py_RETURN_NONE;
    Py_INCREF(f);
    return f;
}

int ctrl_traverse(PyObject* self_, visitproc visit, void* arg) {
    BoundControllerStep* self = (BoundControllerStep*)self_;
    Py_VISIT(self->ctrl_dict); Py_VISIT(self->opt); Py_VISIT(self->py_step); Py_VISIT((PyObject*)self->fast);
    return 0;
}

int ctrl_clear(PyObject* self_) {
    BoundControllerStep* self = (BoundControllerStep*)self_;
    Py_CLEAR(self->ctrl_dict); Py_CLEAR(self->opt); Py_CLEAR(self->py_step);
    BoundOptimizerStep* f = self->fast;
    self->fast = nullptr;
    Py_XDECREF((PyObject*)f);
    return 0;
}

void ctrl_dealloc(PyObject* self) {
    PyObject_GC_UnTrack(self);
    ctrl_clear(self);
    Py_TYPE(self)->tp_free(self);
}

PyGetSetDef ctrl_getset[] = {
    {"native_steps", ctrl_get_native_steps, nullptr, "calls that went straight to the optimizer's bound step", nullptr},
    {"python_steps", ctrl_get_python_steps, nullptr, "calls handed to the Python method", nullptr},
    {"__wrapped__", ctrl_get_wrapped, nullptr, "the Python method that takes every other call", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject BoundControllerStepType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* bind_controller(PyObject*, PyObject* args) {
    PyObject *ctrl, *opt, *fast, *py_step;
    if (!PyArg_ParseTuple(args, "OOO!O:bind_controller", &ctrl, &opt, &BoundOptimizerStepType, &fast, &py_step)) return nullptr;
    if (!PyCallable_Check(py_step)) { PyErr_SetString(PyExc_TypeError, "bind_controller: step must be callable"); return nullptr; }
    if (((BoundOptimizerStep*)fast)->opt != opt) { PyErr_SetString(PyExc_ValueError, "bind_controller: the bound step belongs to another optimizer"); return nullptr; }
    PyObject* ctrl_dict = PyObject_GenericGetDict(ctrl, nullptr);
    if (!ctrl_dict) return nullptr;
    if (!PyDict_CheckExact(ctrl_dict)) {
        Py_DECREF(ctrl_dict);
        PyErr_SetString(PyExc_TypeError, "bind_controller: the controller must keep its attributes in a plain __dict__");
        return nullptr;
    }
    BoundControllerStep* self = (BoundControllerStep*)BoundControllerStepType.tp_alloc(&BoundControllerStepType, 0);
    if (!self) { Py_DECREF(ctrl_dict); return nullptr; }
    self->vectorcall = ctrl_call;
    self->ctrl_dict = ctrl_dict;
    Py_INCREF(opt); self->opt = opt;
    Py_INCREF(py_step); self->py_step = py_step;
    Py_INCREF(fast); self->fast = (BoundOptimizerStep*)fast;
    return (PyObject*)self;
}

PyMethodDef module_methods[] = {
    {"bind", bind, METH_VARARGS,
     "bind(step_fn_addr, handle_addr, S, C, u_out) -> callable(s, u_prev, samples_ptr, samples_loc) -> int status | NotImplemented"},
    {"bind_optimizer", bind_optimizer, METH_VARARGS,
     "bind_optimizer(optimizer, engine, bound_step, u_out, param_names, DeviceRng, DeviceBufferRng, flags) -> callable(s) -> u | NotImplemented"},
    {"bind_controller", bind_controller, METH_VARARGS,
     "bind_controller(controller, optimizer, bound_optimizer_step, step) -> callable(s, time=None, updated_attributes={}) -> u"},
    {nullptr, nullptr, 0, nullptr},
};

bool intern_names() {
    struct { PyObject** at; const char* text; } names[] = {
        {&s_optimizer_logging, "optimizer_logging"}, {&s_calculate_optimal_trajectory, "calculate_optimal_trajectory"}, {&s_engine, "engine"},
        {&s_step, "step"}, {&s_u, "u"}, {&s_u_public, "_u_public"}, {&s_u_vec, "_u_vec"}, {&s_rng, "rng"}, {&s_lazy, "_lazy"},
        {&s_cost_function, "cost_function"}, {&s_predictor, "predictor"}, {&s_version, "version"}, {&s_parameters, "parameters"},
        {&s_variable_parameters, "variable_parameters"}, {&s_pointers, "pointers"}, {&s_i, "_i"}, {&s_check, "_check"}, {&s_copy, "copy"},
        {&s_reload_flag, "reload_cost_parameters_from_config_flag"}, {&s_controller_logging, "controller_logging"}, {&s_optimizer, "optimizer"},
        {&s_count, "count"}, {&s_warmup, "warmup"},
    };
    for (auto& n : names)
        if (!(*n.at = PyUnicode_InternFromString(n.text))) return false;
    return true;
}

bool ready_gc_type(PyTypeObject* t, const char* name, size_t size, destructor dealloc, traverseproc traverse, inquiry clear,
                   size_t vectorcall_offset, PyMethodDef* methods, PyGetSetDef* getset, const char* doc) {
    t->tp_name = name;
    t->tp_basicsize = (Py_ssize_t)size;
    t->tp_dealloc = dealloc;
    t->tp_traverse = traverse;
    t->tp_clear = clear;
    t->tp_free = PyObject_GC_Del;
    t->tp_vectorcall_offset = (Py_ssize_t)vectorcall_offset;
    t->tp_call = PyVectorcall_Call;
    t->tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_VECTORCALL | Py_TPFLAGS_HAVE_GC;
    t->tp_methods = methods;
    t->tp_getset = getset;
    t->tp_doc = doc;
    return PyType_Ready(t) == 0;
}

PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "_ctk_pystep", "pre-bound ctk_step call for CtkEngine.step", -1, module_methods,
                          nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__ctk_pystep(void) {
    BoundStepType.tp_name = "control_toolkit_amd._ctk_pystep.BoundStep";
    BoundStepType.tp_basicsize = sizeof(BoundStep);
    BoundStepType.tp_dealloc = bound_dealloc;
    BoundStepType.tp_vectorcall_offset = offsetof(BoundStep, vectorcall);
    BoundStepType.tp_call = PyVectorcall_Call;
    BoundStepType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_VECTORCALL;
    BoundStepType.tp_methods = bound_methods;
    BoundStepType.tp_getset = bound_getset;
    BoundStepType.tp_doc = "ctk_step with the handle, the sizes and the output buffer bound";
    if (PyType_Ready(&BoundStepType) < 0) return nullptr;
    if (!intern_names()) return nullptr;
    if (!ready_gc_type(&BoundOptimizerStepType, "control_toolkit_amd._ctk_pystep.BoundOptimizerStep", sizeof(BoundOptimizerStep), opt_dealloc,
                       opt_traverse, opt_clear, offsetof(BoundOptimizerStep, vectorcall), opt_methods, opt_getset,
                       "an optimizer's step with its guards, samples, ctk_step and publish bound")) return nullptr;
    if (!ready_gc_type(&BoundControllerStepType, "control_toolkit_amd._ctk_pystep.BoundControllerStep", sizeof(BoundControllerStep), ctrl_dealloc,
                       ctrl_traverse, ctrl_clear, offsetof(BoundControllerStep, vectorcall), nullptr, ctrl_getset,
                       "controller_mpc.step: the optimizer's bound step when nothing else is to do, else the Python method")) return nullptr;
    return PyModule_Create(&module_def);
}
