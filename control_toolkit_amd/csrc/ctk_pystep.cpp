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
#define PY_SSIZE_T_CLEAN
#include <Python.h>
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

PyMethodDef module_methods[] = {
    {"bind", bind, METH_VARARGS,
     "bind(step_fn_addr, handle_addr, S, C, u_out) -> callable(s, u_prev, samples_ptr, samples_loc) -> int status | NotImplemented"},
    {nullptr, nullptr, 0, nullptr},
};

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
    return PyModule_Create(&module_def);
}
