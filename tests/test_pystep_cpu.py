"""The pre-bound step call (control_toolkit_amd/csrc/ctk_pystep.cpp) against a stub with ctk_step's signature: no GPU.

The stub records what it received and writes u_out[c] = 10 + c.  The module is optional (csrc/Makefile skips it without Python.h), so
without it the module-level tests skip and the wrapper tests check the ctypes path alone."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pystep_helpers as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = 0x7F00DEADB000
S, Cn = 4, 2
STATE = np.array([0.05, -0.1, 2.8, 0.4], np.float32)


@pytest.fixture(scope="module")
def stub_path(tmp_path_factory):
    return H.build_stub(str(tmp_path_factory.mktemp("pystep_stub")))


@pytest.fixture()
def stub(stub_path):
    lib = H.load_stub(stub_path)
    lib.stub_config(S, Cn, 0, 0)
    return lib


@pytest.fixture()
def mod():
    return pytest.importorskip("control_toolkit_amd._ctk_pystep")


@pytest.fixture()
def bound(mod, stub):
    u = np.zeros(Cn, np.float32)
    return mod.bind(H.step_address(stub), HANDLE, S, Cn, u), u


# ---- arguments arrive exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(S,), (1, S)])
def test_state_handle_and_output(bound, stub, shape):
    b, u = bound
    n0 = stub.stub_calls()
    assert b(STATE.reshape(shape), None, None, 0) == 0
    got = H.received(stub, S, Cn)
    assert stub.stub_calls() == n0 + 1
    assert got["handle"] == HANDLE
    assert got["s"].tobytes() == STATE.tobytes()
    assert got["u_prev"] is None and got["samples"] is None and got["loc"] == 0
    assert u.tolist() == [10.0, 11.0]          # written through u_out into the bound array's own memory


def test_u_prev_valued_takes_the_first_C(bound, stub):
    b, _ = bound
    up = np.array([0.25, -0.5, 9.0], np.float32)            # more than C entries: the first C, as reshape(-1)[:C] takes today
    assert b(STATE, up, None, 0) == 0
    assert H.received(stub, S, Cn)["u_prev"].tobytes() == up[:Cn].tobytes()
    assert b(STATE, up[:Cn].reshape(1, Cn), None, 0) == 0
    assert H.received(stub, S, Cn)["u_prev"].tobytes() == up[:Cn].tobytes()
    assert b(STATE, None, None, 0) == 0
    assert H.received(stub, S, Cn)["u_prev"] is None


def test_samples_pointer_and_loc(bound, stub):
    b, _ = bound
    for ptr, loc in ((None, 0), (0x7E0012345000, 2), (0x1000, 1), ((1 << 63) + 64, 2)):
        assert b(STATE, None, ptr, loc) == 0
        got = H.received(stub, S, Cn)
        assert got["samples"] == ptr and got["loc"] == loc


def test_other_buffer_exporters_are_taken(bound, stub):
    import array
    b, _ = bound
    assert b(array.array("f", STATE.tolist()), None, None, 0) == 0
    assert H.received(stub, S, Cn)["s"].tobytes() == STATE.tobytes()
    assert b(memoryview(STATE), None, None, 0) == 0


# ---- "not fast": NotImplemented, and the stub is never called -------------------------------------------------------------------------
NOT_FAST = {
    "float64 state": (STATE.astype(np.float64), None),
    "list": (STATE.tolist(), None),
    "non-contiguous float32 view": (np.zeros(2 * S, np.float32)[::2], None),
    "too few": (STATE[:3].copy(), None),
    "too many": (np.zeros(S + 1, np.float32), None),
    "int32 of the right size": (np.zeros(S, np.int32), None),
    "bytes": (STATE.tobytes(), None),
    "u_prev float64": (STATE, np.zeros(Cn, np.float64)),
    "u_prev list": (STATE, [0.0, 0.0]),
    "u_prev too short": (STATE, np.zeros(Cn - 1, np.float32)),
    "u_prev non-contiguous": (STATE, np.zeros(2 * Cn, np.float32)[::2]),
}


@pytest.mark.parametrize("case", sorted(NOT_FAST))
def test_not_fast_inputs_never_reach_the_stub(bound, stub, case):
    b, _ = bound
    s, up = NOT_FAST[case]
    n0 = stub.stub_calls()
    assert b(s, up, None, 0) is NotImplemented
    assert stub.stub_calls() == n0


def test_bad_calls_raise_and_never_reach_the_stub(mod, bound, stub):
    b, _ = bound
    n0 = stub.stub_calls()
    with pytest.raises(TypeError):
        b(STATE, None, None)
    with pytest.raises(TypeError):
        b(STATE, None, None, 0, 1)
    with pytest.raises(TypeError):
        b(STATE, None, 1.5, 0)
    with pytest.raises(TypeError):
        b(STATE, None, None, "host")
    with pytest.raises(ValueError):
        mod.bind(H.step_address(stub), HANDLE, S, Cn, np.zeros(Cn + 1, np.float32))     # u_out of the wrong size
    with pytest.raises(ValueError):
        mod.bind(H.step_address(stub), HANDLE, S, Cn, np.zeros(Cn, np.float64))
    ro = np.zeros(Cn, np.float32); ro.setflags(write=False)
    with pytest.raises((BufferError, ValueError)):
        mod.bind(H.step_address(stub), HANDLE, S, Cn, ro)
    with pytest.raises(ValueError):
        mod.bind(0, HANDLE, S, Cn, np.zeros(Cn, np.float32))
    assert stub.stub_calls() == n0


# ---- references -----------------------------------------------------------------------------------------------------------------------
def test_refcounts_stay_put_over_1e5_calls(mod, stub):
    u = np.zeros(Cn, np.float32)
    r_u0 = sys.getrefcount(u)
    b = mod.bind(H.step_address(stub), HANDLE, S, Cn, u)
    s, up, s64 = STATE.copy(), np.zeros(Cn, np.float32), STATE.astype(np.float64)
    before = [sys.getrefcount(x) for x in (s, up, s64, u)]
    r_ni = sys.getrefcount(NotImplemented)
    for _ in range(100_000):
        b(s, up, None, 0)
    assert [sys.getrefcount(x) for x in (s, up, s64, u)] == before
    for _ in range(100_000):                    # the "not fast" path: state refused, then u_prev refused after the state was taken
        b(s64, up, None, 0)
        b(s, s64, None, 0)
    assert [sys.getrefcount(x) for x in (s, up, s64, u)] == before
    assert abs(sys.getrefcount(NotImplemented) - r_ni) < 100            # each NotImplemented handed out was a new reference, dropped by us
    stub.stub_config(S, Cn, 3, 0)               # the error-status path
    for _ in range(100_000):
        b(s, up, None, 0)
    assert [sys.getrefcount(x) for x in (s, up, s64, u)] == before
    del b
    assert sys.getrefcount(u) == r_u0            # the object's one reference to u_out went with it


# ---- the GIL is released around the call -------------------------------------------------------------------------------------------------
def test_gil_is_released_while_the_step_runs(bound, stub):
    b, _ = bound
    stub.stub_config(S, Cn, 0, 50)
    count, stop = [0], threading.Event()

    def spin():
        while not stop.is_set():
            count[0] += 1

    t = threading.Thread(target=spin)
    t.start()
    try:
        while count[0] == 0:                     # the counter thread is running before the call starts
            time.sleep(0)
        c0 = count[0]
        assert b(STATE, None, None, 0) == 0      # 50 ms inside the stub
        advanced = count[0] - c0
    finally:
        stop.set()
        t.join()
    # holding the GIL for the 50 ms would let the other thread in only around the call (a handful of increments at most)
    assert advanced > 1000


# ---- status and invalidation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("status", [1, 2, 3, 7, -5])
def test_non_zero_status_is_returned_unchanged(bound, stub, status):
    b, _ = bound
    stub.stub_config(S, Cn, status, 0)
    assert b(STATE, None, None, 0) == status


def test_invalidate_stops_every_later_call(bound, stub):
    b, _ = bound
    assert b.valid
    assert b(STATE, None, None, 0) == 0
    n0 = stub.stub_calls()
    b.invalidate()
    assert not b.valid
    assert b(STATE, None, None, 0) is NotImplemented
    assert b(STATE, np.zeros(Cn, np.float32), 0x1000, 2) is NotImplemented
    assert stub.stub_calls() == n0


# ---- the wrapper: CtkEngine.step over the stub ------------------------------------------------------------------------------------------------
def have_module():
    try:
        import control_toolkit_amd._ctk_pystep  # noqa: F401
        return True
    except ImportError:
        return False


def engines(stub):
    """the engine on its default path and one held on the ctypes path"""
    from control_toolkit_amd import _capi
    e = H.stub_engine(stub, S, Cn, HANDLE)
    assert e.step_path == ("bound" if have_module() and os.environ.get("CTK_PYSTEP", "1") != "0" else "ctypes")
    c = H.stub_engine(stub, S, Cn, HANDLE)
    if c._bound is not None:
        c._bound.invalidate(); c._bound = None
    assert c.step_path == "ctypes"
    assert isinstance(e, _capi.CtkEngine)
    return e, c


def test_wrapper_steps_agree_on_both_paths(stub):
    for e in engines(stub):
        for s in (STATE, STATE.reshape(1, S), STATE.astype(np.float64), STATE.tolist()):
            n0 = stub.stub_calls()
            u = e.step(s, u_prev=[0.5, -0.5])
            assert stub.stub_calls() == n0 + 1 and u.tolist() == [10.0, 11.0] and u is not e._u
            got = H.received(stub, S, Cn)
            assert got["handle"] == HANDLE and got["s"].tobytes() == STATE.tobytes() and got["u_prev"].tolist() == [0.5, -0.5]
            assert got["samples"] is None and got["loc"] == 0
        e.step(STATE, 0x7E0000001000)
        got = H.received(stub, S, Cn)
        assert got["samples"] == 0x7E0000001000 and got["loc"] == 2 and got["u_prev"] is None
        host = np.arange(8, dtype=np.float32)                     # the stub's ctk_samples_needed
        e.step(STATE, host)
        got = H.received(stub, S, Cn)
        assert got["samples"] == host.ctypes.data and got["loc"] == 1


def test_wrapper_errors_have_todays_text_on_both_paths(stub):
    for e in engines(stub):
        n0 = stub.stub_calls()
        for bad in (np.zeros(S + 1, np.float32), np.zeros(S - 1, np.float64), [0.0] * (S + 2)):
            with pytest.raises(ValueError) as ei:
                e.step(bad)
            assert str(ei.value) == f"state must have {S} entries"
        with pytest.raises(ValueError) as ei:
            e.step(STATE, np.zeros(9, np.float32))
        assert str(ei.value) == "step consumes 8 draws, got 9"
        assert stub.stub_calls() == n0
        stub.stub_config(S, Cn, 3, 0)
        from control_toolkit_amd import CtkError
        with pytest.raises(CtkError) as ei:
            e.step(STATE)
        assert str(ei.value) == "[ctk 3] stub error"
        stub.stub_config(S, Cn, 1, 0)
        with pytest.raises(ValueError) as ei:
            e.step(STATE)
        assert str(ei.value) == "[ctk 1] stub error"
        stub.stub_config(S, Cn, 0, 0)


def test_wrapper_close_invalidates_before_destroy(stub):
    e, _ = engines(stub)
    b = e._bound
    e.close()
    assert e.step_path == "ctypes" and not e._h.value
    if b is not None:
        assert not b.valid
    e.close()                                                     # twice is fine, as before


def test_ctk_pystep_0_selects_ctypes_in_a_child_process(stub_path):
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            "import numpy as np, _pystep_helpers as H\n"
            "lib = H.load_stub(sys.argv[3]); lib.stub_config(4, 2, 0, 0)\n"
            "e = H.stub_engine(lib, 4, 2)\n"
            "u = e.step(np.zeros(4, np.float32))\n"
            "print(e.step_path, u.tolist(), lib.stub_calls())\n")
    out = {}
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests"), stub_path],
                           env=dict(os.environ, CTK_PYSTEP=flag), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[flag] = r.stdout.split()[0]
        assert r.stdout.strip().endswith("[10.0, 11.0] 1")
    assert out["0"] == "ctypes"
    assert out["1"] == ("bound" if have_module() else "ctypes")
