"""The bound optimizer and controller steps (control_toolkit_amd/csrc/ctk_pystep.cpp: bind_optimizer, bind_controller) against the
Python bodies they restate: no GPU.  A real controller_mpc around mppi-hip steps a stub library (tests/_controller_native_helpers.py)
that records what ctk_step received and counts parameter uploads; `native_step: false` in the optimizer's entry keeps the second
controller on Python."""
import os
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _controller_native_helpers as H  # noqa: E402

from control_toolkit_amd._capi import CtkError, PARAMS  # noqa: E402
from control_toolkit_amd.others.globals_and_utils import DeviceBufferRng, DeviceRng  # noqa: E402

pytest.importorskip("control_toolkit_amd._ctk_pystep")
pytestmark = pytest.mark.skipif(os.environ.get("CTK_PYSTEP", "1") == "0", reason="CTK_PYSTEP=0 switches the bound steps off")

POOL = [0x7E0000001000, 0x7E0000002000, 0x7E0000003000]
STATES = [np.array([0.05 * k, -0.1 + 0.02 * k, 2.8 - 0.3 * k, 0.4 * (-1) ** k], np.float32) for k in range(12)]


@pytest.fixture(scope="module")
def stub_path(tmp_path_factory):
    return H.build_stub(str(tmp_path_factory.mktemp("controller_stub")))


@pytest.fixture()
def lib(stub_path):
    lib = H.load_stub(stub_path)
    lib.stub_config(4, 1, 0, 0)
    yield lib
    lib.stub_config(4, 1, 0, 0)


def controller(lib, native=True, rng="buffer", **kw):
    c = H.make_controller(lib, native_step=native, **kw)
    c.optimizer.rng = DeviceBufferRng(POOL, seed=1) if rng == "buffer" else DeviceRng(1)   # after configure, as bench.py does
    return c


def warmed(lib, **kw):
    """a native controller two steps in: the first step is Python's (u is still the constructor's 0.0), the second is native"""
    c = controller(lib, **kw)
    c.step(STATES[0]); c.step(STATES[1])
    assert c.optimizer.step_path == "native"
    return c


def observe(lib, c, u):
    o = c.optimizer
    return {"received": H.received(lib), "type": type(u), "dtype": np.asarray(u).dtype, "value": np.asarray(u).tobytes(),
            "u_is_returned": o.u is u, "public_is_returned": o._u_public is u, "u_vec": (o._u_vec.dtype, o._u_vec.shape, o._u_vec.tobytes()),
            "u_vec_owns": o._u_vec.base is None and o._u_vec is not o.engine._u, "lazy": dict(o._lazy), "cursor": getattr(o.rng, "_i", None)}


# ---- the two paths hand ctk_step the same and publish the same ------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["controller", "optimizer"])
@pytest.mark.parametrize("rng", ["buffer", "device"])
def test_native_and_python_paths_agree(lib, rng, boundary):
    a, b = controller(lib, True, rng), controller(lib, False, rng)
    assert type(a.step).__name__ == "BoundControllerStep" and type(b.step).__name__ == "method"
    assert a.optimizer._fast is not None and b.optimizer._fast is None
    for k, s in enumerate(STATES):
        seen = []
        for c in (a, b):
            c.optimizer._lazy["U_NOM"] = "stale"          # what a reader of u_nom left behind: the step drops it
            n0 = lib.stub_calls()
            u = c.step(s.copy()) if boundary == "controller" else c.optimizer.step(s.copy())
            assert lib.stub_calls() == n0 + 1
            seen.append(observe(lib, c, u))
        assert seen[0] == seen[1], k
        assert seen[0]["lazy"] == {} and seen[0]["type"] is np.float32 and seen[0]["u_is_returned"] and seen[0]["u_vec_owns"]
        assert seen[0]["received"]["loc"] == (2 if rng == "buffer" else 0)
        assert seen[0]["received"]["samples"] == (POOL[k % 3] if rng == "buffer" else None)
        assert a.optimizer.step_path == ("python" if k == 0 else "native") and b.optimizer.step_path == "python"
    assert a.optimizer.native_step_count == len(STATES) - 1 and b.optimizer.native_step_count == 0
    if boundary == "controller":
        assert a.step.native_steps == len(STATES) - 1 and a.step.python_steps == 1


def test_keyword_arguments_of_the_controller_step(lib):
    c = warmed(lib)
    n0 = c.optimizer.native_step_count
    c.step(STATES[2], None); c.step(STATES[3], time=0.1); c.step(s=STATES[4], time=None, updated_attributes={}); c.step(STATES[5], None, {})
    assert c.optimizer.native_step_count == n0 + 4
    with pytest.raises(TypeError):
        c.step(STATES[6], nonsense=1)
    with pytest.raises(TypeError):
        c.step()


# ---- CEM and random-action: the same sequence; CEM counts its steps and keeps a warm-up run's first step in Python -------------------------
@pytest.mark.parametrize("optimizer", ["cem-hip", "random-action-hip"])
def test_cem_and_random_action_paths_agree(lib, optimizer):
    a, b = (controller(lib, native, optimizer=optimizer) for native in (True, False))
    assert a.optimizer._fast is not None and b.optimizer._fast is None
    for k, s in enumerate(STATES):
        seen = []
        for c in (a, b):
            c.optimizer._lazy["U_NOM"] = "kept"            # these steps do not clear _lazy, on either path
            n0 = lib.stub_calls()
            u = c.step(s.copy())
            assert lib.stub_calls() == n0 + 1
            seen.append(dict(observe(lib, c, u), count=getattr(c.optimizer, "count", None)))
        assert seen[0] == seen[1], k
        assert seen[0]["lazy"] == {"U_NOM": "kept"} and seen[0]["count"] == (k + 1 if optimizer == "cem-hip" else None)
        assert a.optimizer.step_path == ("python" if k == 0 else "native") and b.optimizer.step_path == "python"
    a.controller_reset(); b.controller_reset()             # CEM: count = 0 and u = 0.0 again, so the next step is Python's
    ua, ub = a.step(STATES[0]), b.step(STATES[0])
    assert ua == ub and a.optimizer.step_path == ("python" if optimizer == "cem-hip" else "native")


def test_cem_warm_up_step_stays_in_python(lib):
    c = controller(lib, optimizer="cem-hip", warmup=True, warmup_iterations=5)
    o = c.optimizer
    c.step(STATES[0]); c.step(STATES[1])
    assert o.step_path == "native" and o.count == 2
    o.count = 0                                            # as optimizer_reset leaves it, but with u still the published one
    n0 = lib.stub_calls()
    c.step(STATES[2])
    assert o.step_path == "python" and o.count == 1 and lib.stub_calls() == n0 + 1
    c.step(STATES[3])
    assert o.step_path == "native" and o.count == 2


def test_rpgd_and_gradient_optimizers_have_no_bound_step():
    from control_toolkit_amd.Optimizers.optimizer_rpgd_hip import optimizer_rpgd_hip
    from control_toolkit_amd.Optimizers.optimizer_gradient_hip import optimizer_gradient_hip
    assert optimizer_rpgd_hip._native_step_fn is None and optimizer_gradient_hip._native_step_fn is None


# ---- every fallback trigger: one ctk_step call, the cursor advanced once, the Python path ---------------------------------------------------
def _subclassed_rng(c):
    class PoolRng(DeviceBufferRng):
        pass
    r = PoolRng(POOL, seed=1)
    r._i = c.optimizer.rng._i
    c.optimizer.rng = r


def _wrapped_engine_step(c):
    e = c.optimizer.engine
    e.step = lambda *a, **kw: type(e).step(e, *a, **kw)


def _other_engine(c, lib):
    c.optimizer.engine = H.stub_engine_class(lib)("mppi", "ODE", num_rollouts=64, mpc_horizon=8)


TRIGGERS = {
    "optimizer_logging": lambda c, lib: setattr(c.optimizer, "optimizer_logging", True),
    "calculate_optimal_trajectory": lambda c, lib: setattr(c.optimizer, "calculate_optimal_trajectory", True),
    "another_engine": _other_engine,
    "engine_step_wrapped": lambda c, lib: _wrapped_engine_step(c),
    "bound_step_closed": lambda c, lib: c.optimizer.engine._bound.invalidate(),
    "u_assigned": lambda c, lib: setattr(c.optimizer, "u", np.float32(0.375)),
    "rng_subclass": lambda c, lib: _subclassed_rng(c),
    "native_step_object_invalidated": lambda c, lib: c.optimizer._fast.invalidate(),
}


@pytest.mark.parametrize("trigger", sorted(TRIGGERS))
def test_fallback_trigger(lib, trigger):
    c = warmed(lib)
    TRIGGERS[trigger](c, lib)
    n0, i0, native0 = lib.stub_calls(), c.optimizer.rng._i, c.optimizer.native_step_count
    u = c.step(STATES[2])
    assert lib.stub_calls() == n0 + 1 and c.optimizer.rng._i == (i0 + 1) % 3
    assert c.optimizer.step_path == "python" and c.optimizer.native_step_count == native0
    assert type(u) is np.float32 and H.received(lib)["s"] == STATES[2].tobytes()
    if trigger == "u_assigned":
        assert H.received(lib)["u_prev"] == np.float32(0.375).tobytes()
        c.step(STATES[3])
        assert c.optimizer.step_path == "native"     # the step published u again


@pytest.mark.parametrize("state", ["float64", "row", "strided", "list", "too_long"])
def test_fallback_state_that_needs_prepare_state(lib, state):
    c = warmed(lib)
    s = {"float64": STATES[2].astype(np.float64), "row": STATES[2].reshape(1, 4), "strided": np.repeat(STATES[2], 2)[::2],
         "list": [float(x) for x in STATES[2]], "too_long": np.zeros(5, np.float32)}[state]
    n0, i0 = lib.stub_calls(), c.optimizer.rng._i
    if state == "too_long":
        with pytest.raises(ValueError, match="state must have shape"):
            c.step(s)
        assert lib.stub_calls() == n0 and c.optimizer.rng._i == i0 and c.optimizer.step_path == "python"
        return
    c.step(s)
    assert lib.stub_calls() == n0 + 1 and c.optimizer.rng._i == (i0 + 1) % 3 and c.optimizer.step_path == "python"
    assert H.received(lib)["s"] == STATES[2].tobytes()
    c.step(STATES[3])
    assert c.optimizer.step_path == "native"


def test_fallback_updated_attributes_and_cost_reload_and_logging(lib):
    c = warmed(lib)
    tp = PARAMS.index("target_position")
    n0, i0, up0 = lib.stub_calls(), c.optimizer.rng._i, lib.stub_upload_count(tp)
    c.step(STATES[2], updated_attributes={"target_position": 0.25})
    assert lib.stub_calls() == n0 + 1 and c.optimizer.rng._i == (i0 + 1) % 3 and c.optimizer.step_path == "python"
    assert lib.stub_upload_count(tp) == up0 + 1 and lib.stub_param(tp) == 0.25
    c.step(STATES[3])
    assert c.optimizer.step_path == "native"
    c.cost_function.set_parameters(dd_weight=321.0)            # sets the reload flag the controller step looks at
    n0, i0 = lib.stub_calls(), c.optimizer.rng._i
    c.step(STATES[4])
    assert lib.stub_calls() == n0 + 1 and c.optimizer.rng._i == (i0 + 1) % 3 and c.optimizer.step_path == "python"
    assert lib.stub_param(PARAMS.index("dd_weight")) == 321.0 and lib.stub_uploads_at_step() == lib.stub_uploads()
    c.step(STATES[5])
    assert c.optimizer.step_path == "native"
    logged = controller(lib, controller_logging=True)
    for s in STATES[:3]:
        n0 = lib.stub_calls()
        logged.step(s)
        assert lib.stub_calls() == n0 + 1 and logged.optimizer.step_path == "python"
    assert len(logged.logs["u_logged"]) == 3


def test_reference_shaped_cost_wrapper_gets_no_bound_step(lib):
    c = controller(lib)
    o = c.optimizer
    del o.cost_function.version                               # no version counter: _sync_parameters keys _parameter_values
    with H.stubbed(lib):
        o.configure(num_states=4, num_control_inputs=1, dt=0.02, predictor_specification="ODE")
    assert o._fast is None
    o.step(STATES[0]); o.step(STATES[1])
    assert o.step_path == "python"


# ---- parameter changes: uploaded before the step that follows, as often as on the Python path, and native again after ----------------------
def _cost_reload(c):
    c.cost_function.set_parameters(ep_weight=12345.0)


def _in_place(c):
    c.cost_function.parameters["ekp_weight"] = 81.5


def _dynamics(c):
    c.predictor.parameters["m_pole"] = 0.125


def _variable_parameter(c):
    c.variable_parameters.target_position = np.float32(-0.5)


def _variable_parameter_in_place(c):
    c.variable_parameters.target_equilibrium[...] = -1.0     # the 0-d array controller_mpc put there, written in place


def _new_cost_key(c):
    c.cost_function.parameters["g"] = 9.5                     # a cost entry overrides the predictor's value of the same name


def _new_variable_parameter(c):
    c.variable_parameters.L = 0.5


def _version_alone(c):
    c.cost_function.version += 1                              # nothing to upload, but the key differs


CHANGES = {"cost_reload_version_bump": (_cost_reload, "ep_weight", 12345.0), "cost_in_place": (_in_place, "ekp_weight", 81.5),
           "predictor_parameters": (_dynamics, "m_pole", 0.125), "variable_parameter": (_variable_parameter, "target_position", -0.5),
           "variable_parameter_in_place": (_variable_parameter_in_place, "target_equilibrium", -1.0),
           "new_cost_key": (_new_cost_key, "g", 9.5), "new_variable_parameter": (_new_variable_parameter, "L", 0.5),
           "version_alone": (_version_alone, None, None)}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_parameter_change_uploads_before_the_next_step(lib, change):
    apply, name, value = CHANGES[change]
    counts = []
    for native in (True, False):
        c = controller(lib, native)
        c.step(STATES[0]); c.step(STATES[1])
        per_id0, n0 = [lib.stub_upload_count(i) for i in range(len(PARAMS))], lib.stub_calls()
        apply(c)
        c.step(STATES[2])
        assert lib.stub_calls() == n0 + 1 and c.optimizer.step_path == "python"
        assert lib.stub_uploads_at_step() == lib.stub_uploads()                   # nothing was uploaded after ctk_step began
        counts.append([lib.stub_upload_count(i) - per_id0[i] for i in range(len(PARAMS))])
        if name is not None:
            assert lib.stub_param(PARAMS.index(name)) == np.float32(value)
        up = lib.stub_uploads()
        c.step(STATES[3])
        assert lib.stub_uploads() == up
        assert c.optimizer.step_path == ("native" if native else "python")
    assert counts[0] == counts[1]
    assert sum(counts[0]) == (0 if name is None else 1) and (name is None or counts[0][PARAMS.index(name)] == 1)


def test_replaced_dictionary_and_unsupported_values(lib):
    c = warmed(lib)
    c.cost_function.parameters = dict(c.cost_function.parameters)     # equal values in a new dictionary: the Python key does not move
    up = lib.stub_uploads()
    c.step(STATES[2])
    assert c.optimizer.step_path == "python" and lib.stub_uploads() == up
    c.step(STATES[3])
    assert c.optimizer.step_path == "native"                          # the declined step had the snapshot taken again
    c.cost_function.parameters["R"] = "1.5"                           # a string: float() takes it on the Python path, the snapshot does not
    c.step(STATES[4]); c.step(STATES[5])
    assert c.optimizer.step_path == "python" and not c.optimizer._fast.snapshot_valid
    assert lib.stub_param(PARAMS.index("R")) == 1.5
    c.cost_function.parameters["R"] = 2.0
    c.step(STATES[6]); c.step(STATES[7])
    assert c.optimizer.step_path == "native" and lib.stub_param(PARAMS.index("R")) == 2.0
    c.cost_function.parameters["R"] = float("nan")
    c.step(STATES[8])
    assert c.optimizer.step_path == "python"


# ---- status, closing -------------------------------------------------------------------------------------------------------------------------
def test_non_zero_status_raises_the_engines_error_on_both_paths(lib):
    texts = []
    for native in (True, False):
        c = controller(lib, native)
        c.step(STATES[0]); c.step(STATES[1])
        lib.stub_config(4, 1, 3, 0)
        u0, i0, n0 = c.optimizer.u, c.optimizer.rng._i, lib.stub_calls()
        with pytest.raises(CtkError) as e:
            c.step(STATES[2])
        texts.append(str(e.value))
        assert lib.stub_calls() == n0 + 1 and c.optimizer.rng._i == (i0 + 1) % 3 and c.optimizer.u is u0   # nothing published
        lib.stub_config(4, 1, 0, 0)
        c.step(STATES[3])
        assert c.optimizer.step_path == ("native" if native else "python")
    assert texts[0] == texts[1] == "[ctk 3] stub error"


def test_closed_engine_never_reaches_the_library(lib):
    c = warmed(lib)
    fast, step = c.optimizer._fast, c.step
    assert fast.valid
    c.optimizer.engine.close()
    assert not fast.valid and c.optimizer.engine._fast_step is None
    n0, i0 = lib.stub_calls(), c.optimizer.rng._i
    assert fast(STATES[2]) is NotImplemented
    assert lib.stub_calls() == n0 and c.optimizer.rng._i == i0
    del step


# ---- references, the GIL ---------------------------------------------------------------------------------------------------------------------
def test_no_reference_leak_over_1e5_native_steps(lib):
    c = warmed(lib)
    o, s = c.optimizer, STATES[2].copy()
    held = (o, o.rng, o.cost_function.parameters, o.predictor.parameters, s, o.engine, c.variable_parameters, o._lazy, c, None, NotImplemented)
    for _ in range(10):
        c.step(s)
    before = [sys.getrefcount(x) for x in held]
    n0 = o.native_step_count
    for _ in range(100_000):
        c.step(s)
    assert o.native_step_count == n0 + 100_000
    after = [sys.getrefcount(x) for x in held]
    assert after[:-2] == before[:-2]
    assert abs(after[-2] - before[-2]) < 100 and abs(after[-1] - before[-1]) < 100     # None / NotImplemented: the interpreter's own traffic
    s64 = s.astype(np.float64)
    before = [sys.getrefcount(x) for x in held] + [sys.getrefcount(s64)]
    for _ in range(20_000):                                                            # the declined path
        c.step(s64)
    after = [sys.getrefcount(x) for x in held] + [sys.getrefcount(s64)]
    assert after[:-3] == before[:-3] and after[-1] == before[-1]


def test_bound_objects_are_collected_with_their_controller(lib):
    import gc
    import weakref
    c = warmed(lib)
    refs = [weakref.ref(c), weakref.ref(c.optimizer), weakref.ref(c.optimizer.engine)]
    del c
    gc.collect()
    assert [r() for r in refs] == [None, None, None]


def test_gil_is_released_while_the_native_step_runs(lib):
    c = warmed(lib)
    lib.stub_config(4, 1, 0, 50)
    count, stop = [0], threading.Event()

    def spin():
        while not stop.is_set():
            count[0] += 1

    t = threading.Thread(target=spin)
    t.start()
    try:
        while count[0] == 0:
            time.sleep(0)
        c0 = count[0]
        c.step(STATES[2])                           # 50 ms inside the stub
        advanced = count[0] - c0
    finally:
        stop.set()
        t.join()
    assert c.optimizer.step_path == "native"
    assert advanced > 1000                          # holding the GIL would let the other thread in only around the call
