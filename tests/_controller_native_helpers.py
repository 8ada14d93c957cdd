"""Shared by tests/test_controller_native_cpu.py and tools/controller_overhead.py: a stub library with the entry points a stepping
controller_mpc asks of libctk_hip.so (compiled with the host C compiler when asked for), which records what ctk_step received and counts
parameter uploads, and a real controller_mpc / optimizer built around it without a GPU."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

STUB_SRC = r"""
#include <stddef.h>
#include <string.h>
#include <time.h>
#define MAXD 16
#define MAXP 64
static void* g_handle; static float g_s[MAXD], g_up[MAXD]; static int g_up_null; static const void* g_samples; static int g_loc;
static long g_calls, g_uploads, g_uploads_at_step, g_upload_count[MAXP]; static float g_param[MAXP];
static int g_S = 4, g_C = 1, g_status = 0, g_sleep_ms = 0;
/* u_out depends on everything the step received, so that two paths that hand over different arguments give different outputs */
int ctk_step(void* h, const float* s, const float* u_prev, const float* samples, int samples_loc, float* u_out) {
    g_handle = h; g_samples = samples; g_loc = samples_loc; g_up_null = (u_prev == NULL); ++g_calls;
    g_uploads_at_step = g_uploads;
    memcpy(g_s, s, g_S * sizeof(float));
    if (u_prev) memcpy(g_up, u_prev, g_C * sizeof(float));
    if (g_sleep_ms) { struct timespec t = {g_sleep_ms / 1000, (g_sleep_ms % 1000) * 1000000L}; nanosleep(&t, NULL); }
    float acc = 0.0f;
    for (int i = 0; i < g_S; ++i) acc += s[i] * (float)(i + 1);
    for (int c = 0; c < g_C; ++c)
        u_out[c] = 0.125f * acc + (float)c + (u_prev ? 0.5f * u_prev[c] : -1.0f) + (float)(((size_t)samples >> 12) & 7) + 0.25f * (float)samples_loc;
    return g_status;
}
int ctk_set_param(void* h, int id, float v) { (void)h; if (id < 0 || id >= MAXP) return 1; g_param[id] = v; ++g_upload_count[id]; ++g_uploads; return 0; }
void stub_config(int S, int Cn, int status, int sleep_ms) { g_S = S; g_C = Cn; g_status = status; g_sleep_ms = sleep_ms; }
long stub_calls(void) { return g_calls; }
long stub_uploads(void) { return g_uploads; }
long stub_uploads_at_step(void) { return g_uploads_at_step; }   /* uploads made before the last ctk_step began */
long stub_upload_count(int id) { return g_upload_count[id]; }
float stub_param(int id) { return g_param[id]; }
void* stub_handle(void) { return g_handle; }
const void* stub_samples(void) { return g_samples; }
int stub_loc(void) { return g_loc; }
int stub_up_null(void) { return g_up_null; }
void stub_state(float* dst) { memcpy(dst, g_s, g_S * sizeof(float)); }
void stub_u_prev(float* dst) { memcpy(dst, g_up, g_C * sizeof(float)); }
const char* ctk_last_error(void* h) { (void)h; return "stub error"; }
size_t ctk_samples_needed(void* h) { (void)h; return 8; }
void ctk_destroy(void* h) { (void)h; }
"""

HANDLE = 0x7F00C0DEB000


def build_stub(directory) -> str:
    src, lib = os.path.join(directory, "controller_stub.c"), os.path.join(directory, "libcontroller_stub.so")
    with open(src, "w") as f:
        f.write(STUB_SRC)
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-shared", "-fPIC", "-o", lib, src], check=True)
    return lib


def load_stub(path):
    lib = C.CDLL(path)
    lib.ctk_step.restype, lib.ctk_step.argtypes = C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    lib.ctk_set_param.restype, lib.ctk_set_param.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_float]
    lib.stub_config.restype, lib.stub_config.argtypes = None, [C.c_int] * 4
    lib.stub_calls.restype = lib.stub_uploads.restype = lib.stub_uploads_at_step.restype = C.c_long
    lib.stub_upload_count.restype, lib.stub_upload_count.argtypes = C.c_long, [C.c_int]
    lib.stub_param.restype, lib.stub_param.argtypes = C.c_float, [C.c_int]
    lib.stub_handle.restype = C.c_void_p
    lib.stub_samples.restype = C.c_void_p
    lib.stub_state.argtypes = lib.stub_u_prev.argtypes = [C.c_void_p]
    lib.ctk_last_error.restype, lib.ctk_last_error.argtypes = C.c_char_p, [C.c_void_p]
    lib.ctk_samples_needed.restype, lib.ctk_samples_needed.argtypes = C.c_size_t, [C.c_void_p]
    lib.ctk_destroy.restype, lib.ctk_destroy.argtypes = None, [C.c_void_p]
    return lib


def received(lib, S=4, Cn=1):
    s, up = np.zeros(S, np.float32), np.zeros(Cn, np.float32)
    lib.stub_state(s.ctypes.data); lib.stub_u_prev(up.ctypes.data)
    return {"handle": lib.stub_handle(), "s": s.tobytes(), "u_prev": None if lib.stub_up_null() else up.tobytes(),
            "samples": lib.stub_samples(), "loc": lib.stub_loc()}


def stub_engine_class(lib):
    """a CtkEngine whose constructor stops short of ctk_create: the stub where the library and the handle would be (CartPole's sizes
    and parameter names), everything a stepping MPPI, CEM or random-action optimizer calls answered on the host"""
    from control_toolkit_amd import _capi

    class StubEngine(_capi.CtkEngine):
        def __init__(self, optimizer, predictor, *, num_rollouts, mpc_horizon, period_interpolation_inducing_points=1, pystep=None, **kw):
            self._lib, self.S, self.C, self.param_names = lib, 4, 1, tuple(_capi.PARAMS)
            self.environment, self.optimizer, self.predictor = "CartPole", optimizer, predictor
            self.N, self.H, self._P = int(num_rollouts), int(mpc_horizon), int(period_interpolation_inducing_points)
            self._h = C.c_void_p(HANDLE)
            self._u, self._s, self._up = np.zeros(self.C, np.float32), np.zeros(self.S, np.float32), np.zeros(self.C, np.float32)
            self._u_p, self._s_p, self._up_p = self._u.ctypes.data, self._s.ctypes.data, self._up.ctypes.data
            self._step_fn = lib.ctk_step
            self._bound = self._fast_step = None
            if pystep is None or pystep:
                self._bind_step()

        def reset(self, draws=None, loc=0):
            pass

        def inducing_points(self):
            return self._P

        def read(self, name):
            return np.zeros((1, self.H, self.C), np.float32)

        def rollout(self, s, Q, u_prev=0.0, want_traj=True):
            return np.zeros((1, self.H + 1, self.S), np.float32), np.zeros(1, np.float32)

    return StubEngine


@contextlib.contextmanager
def stubbed(lib):
    """inside: optimizers build their engine as a StubEngine around `lib`"""
    from control_toolkit_amd import Optimizers, _capi
    saved = Optimizers.CtkEngine, Optimizers.environment_info
    Optimizers.CtkEngine = stub_engine_class(lib)
    Optimizers.environment_info = lambda env: (4, 1, tuple(_capi.PARAMS))
    try:
        yield
    finally:
        Optimizers.CtkEngine, Optimizers.environment_info = saved


def make_controller(lib, native_step=True, controller_logging=False, N=64, H=8, optimizer="mppi-hip", **optimizer_keys):
    """controller_mpc around mppi-hip (or cem-hip / random-action-hip) as bench.py builds it, on the stub"""
    from control_toolkit_amd.Controllers.controller_mpc import controller_mpc
    from control_toolkit_amd.Predictors import PredictorWrapper
    from control_toolkit_amd.Cost_Functions import CostFunctionWrapper
    oc = dict(seed=1, mpc_horizon=H, num_rollouts=N, mpc_timestep=0.02, rng_mode="device", native_step=native_step)
    if optimizer == "mppi-hip":
        oc.update(cc_weight=1.0, R=1.0, LBD=100.0, NU=1000.0, SQRTRHOINV=0.03, period_interpolation_inducing_points=1)
    elif optimizer == "cem-hip":
        oc.update(cem_outer_it=3, cem_initial_action_stdev=0.5, cem_stdev_min=0.01, cem_best_k=8, warmup=False, warmup_iterations=0)
    oc.update(optimizer_keys)
    cc = {"mpc": {"optimizer": optimizer, "predictor_specification": "ODE", "cost_function_specification": "default",
                  "computation_library": "hip", "controller_logging": controller_logging, "calculate_optimal_trajectory": False,
                  "device": "gpu:0"}}
    c = controller_mpc("CartPole", (np.array([-1.0], np.float32), np.array([1.0], np.float32)),
                       {"target_position": 0.0, "target_equilibrium": 1.0}, config_controllers=cc, config_optimizers={optimizer: oc},
                       predictor=PredictorWrapper(), cost_function=CostFunctionWrapper(watch=False))
    with stubbed(lib):
        c.configure()
    return c
