"""Shared by tests/test_pystep_cpu.py and the child processes it starts: a stub library with ctk_step's signature (compiled with the
host C compiler at test time) and a CtkEngine built around it without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

STUB_SRC = r"""
#include <stddef.h>
#include <string.h>
#include <time.h>
#define MAXD 16
static void* g_handle; static float g_s[MAXD], g_up[MAXD]; static int g_up_null; static const void* g_samples; static int g_loc;
static long g_calls; static int g_S = 4, g_C = 1, g_status = 0, g_sleep_ms = 0;
int ctk_step(void* h, const float* s, const float* u_prev, const float* samples, int samples_loc, float* u_out) {
    g_handle = h; g_samples = samples; g_loc = samples_loc; g_up_null = (u_prev == NULL); ++g_calls;
    memcpy(g_s, s, g_S * sizeof(float));
    if (u_prev) memcpy(g_up, u_prev, g_C * sizeof(float));
    if (g_sleep_ms) { struct timespec t = {g_sleep_ms / 1000, (g_sleep_ms % 1000) * 1000000L}; nanosleep(&t, NULL); }
    for (int c = 0; c < g_C; ++c) u_out[c] = 10.0f + (float)c;
    return g_status;
}
void stub_config(int S, int Cn, int status, int sleep_ms) { g_S = S; g_C = Cn; g_status = status; g_sleep_ms = sleep_ms; }
long stub_calls(void) { return g_calls; }
void* stub_handle(void) { return g_handle; }
const void* stub_samples(void) { return g_samples; }
int stub_loc(void) { return g_loc; }
int stub_up_null(void) { return g_up_null; }
void stub_state(float* dst) { memcpy(dst, g_s, g_S * sizeof(float)); }
void stub_u_prev(float* dst) { memcpy(dst, g_up, g_C * sizeof(float)); }
/* what CtkEngine's wrapper asks of its library besides ctk_step */
const char* ctk_last_error(void* h) { (void)h; return "stub error"; }
size_t ctk_samples_needed(void* h) { (void)h; return 8; }
void ctk_destroy(void* h) { (void)h; }
"""


def build_stub(directory) -> str:
    src, lib = os.path.join(directory, "pystep_stub.c"), os.path.join(directory, "libpystep_stub.so")
    with open(src, "w") as f:
        f.write(STUB_SRC)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-shared", "-fPIC", "-o", lib, src], check=True)
    return lib


def load_stub(path):
    lib = C.CDLL(path)
    lib.ctk_step.restype, lib.ctk_step.argtypes = C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    lib.stub_config.restype, lib.stub_config.argtypes = None, [C.c_int] * 4
    lib.stub_calls.restype = C.c_long
    lib.stub_handle.restype = C.c_void_p
    lib.stub_samples.restype = C.c_void_p
    lib.stub_state.argtypes = lib.stub_u_prev.argtypes = [C.c_void_p]
    lib.ctk_last_error.restype, lib.ctk_last_error.argtypes = C.c_char_p, [C.c_void_p]
    lib.ctk_samples_needed.restype, lib.ctk_samples_needed.argtypes = C.c_size_t, [C.c_void_p]
    lib.ctk_destroy.restype, lib.ctk_destroy.argtypes = None, [C.c_void_p]
    return lib


def step_address(lib) -> int:
    return C.cast(lib.ctk_step, C.c_void_p).value


def received(lib, S, Cn):
    s, up = np.zeros(S, np.float32), np.zeros(Cn, np.float32)
    lib.stub_state(s.ctypes.data); lib.stub_u_prev(up.ctypes.data)
    return {"handle": lib.stub_handle(), "s": s, "u_prev": None if lib.stub_up_null() else up,
            "samples": lib.stub_samples(), "loc": lib.stub_loc()}


def stub_engine(lib, S=4, Cn=1, handle=0x5EED0):
    """a CtkEngine as its constructor leaves it behind ctk_create, with the stub where the library and the handle would be"""
    from control_toolkit_amd import _capi
    e = object.__new__(_capi.CtkEngine)
    e._lib, e.S, e.C = lib, S, Cn
    e._h = C.c_void_p(handle)
    e._u, e._s, e._up = np.zeros(Cn, np.float32), np.zeros(S, np.float32), np.zeros(Cn, np.float32)
    e._u_p, e._s_p, e._up_p = e._u.ctypes.data, e._s.ctypes.data, e._up.ctypes.data
    e._step_fn = lib.ctk_step
    e._bound = None
    e._bind_step()
    return e
