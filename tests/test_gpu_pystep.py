"""-m gpu: CtkEngine.step through the pre-bound call (_ctk_pystep) against the same step through ctypes.

Two engines with equal seeds, one per path (pystep=False holds the second on ctypes), take 12 closed-loop steps from the same states;
u, J and U_NOM must agree byte for byte: both paths hand ctk_step the same floats and pointers, so any difference is a marshalling
error.  Shapes: the smallest that cross the in-launch hand-off (N > 64: several blocks) and the single-block form."""
import numpy as np
import pytest

from control_toolkit_amd import CtkEngine, CtkError

pytestmark = pytest.mark.gpu

STEPS = 12
S0 = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
CASES = {
    "mppi N64 H4 p1": ("mppi", dict(num_rollouts=64, mpc_horizon=4, period_interpolation_inducing_points=1)),
    "mppi N192 H12 p3": ("mppi", dict(num_rollouts=192, mpc_horizon=12, period_interpolation_inducing_points=3)),
    "cem N64 H6": ("cem", dict(num_rollouts=64, mpc_horizon=6, cem_outer_it=2, cem_best_k=8)),
    "random_action N64 H4": ("random_action", dict(num_rollouts=64, mpc_horizon=4)),
    "rpgd N32 H8": ("rpgd", dict(num_rollouts=32, mpc_horizon=8, period_interpolation_inducing_points=1, outer_its=2, resamp_per=2, opt_keep_k=8)),
}


def have_module():
    try:
        import control_toolkit_amd._ctk_pystep  # noqa: F401
        return True
    except ImportError:
        return False


def pair(opt, kw):
    a = CtkEngine(opt, "ODE", dt=0.02, seed=7, **kw)
    b = CtkEngine(opt, "ODE", dt=0.02, seed=7, pystep=False, **kw)
    assert a.step_path == "bound" and b.step_path == "ctypes"
    if opt == "rpgd":
        a.reset(); b.reset()
    return a, b


def plant(s, u):
    """any deterministic float32 map closes the loop: the next state depends on every bit of u"""
    s = s.copy()
    s[0] += np.float32(0.02) * s[1]; s[1] += np.float32(0.3) * u[0]
    s[2] += np.float32(0.02) * s[3]; s[3] -= np.float32(0.5) * u[0] * np.cos(s[2])
    return s.astype(np.float32)


@pytest.fixture(scope="module", autouse=True)
def module_is_there():
    assert have_module(), "control_toolkit_amd._ctk_pystep is not built: `make -C control_toolkit_amd/csrc`"


@pytest.mark.parametrize("u_prev", ["given", "omitted"])
@pytest.mark.parametrize("mode", ["rng", "device", "host"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bound_step_equals_ctypes_step(case, mode, u_prev):
    import torch
    opt, kw = CASES[case]
    a, b = pair(opt, kw)
    rng = np.random.default_rng(5)
    try:
        s, up = S0.copy(), np.zeros(1, np.float32)
        for t in range(STEPS):
            need = a.samples_needed()
            assert b.samples_needed() == need
            smp_a = smp_b = None
            if mode != "rng" and need:
                host = (rng.random(need, dtype=np.float32) if opt == "random_action" else rng.standard_normal(need).astype(np.float32))
                if mode == "device":
                    dev = torch.from_numpy(host).to("cuda")
                    torch.cuda.synchronize()
                    smp_a = smp_b = dev.data_ptr()
                else:
                    smp_a, smp_b = host, host.copy()
            k = dict(u_prev=up) if u_prev == "given" else {}
            ua, ub = a.step(s, smp_a, **k), b.step(s, smp_b, **k)
            assert ua.dtype == np.float32 and ua is not a._u
            assert ua.tobytes() == ub.tobytes(), (case, mode, t, ua, ub)
            for name in ("J", "U_NOM") if opt != "random_action" else ("J",):
                assert a.read(name).tobytes() == b.read(name).tobytes(), (case, mode, t, name)
            s, up = plant(s, ua), ua
        assert a.step_path == "bound"
    finally:
        a.close(); b.close()


def test_row_state_takes_the_bound_path_and_float64_the_fallback():
    opt, kw = CASES["mppi N192 H12 p3"]
    a, b = pair(opt, kw)
    c = CtkEngine(opt, "ODE", dt=0.02, seed=7, **kw)
    try:
        calls = []
        inner = a._bound
        a._bound = lambda *args: (calls.append(inner(*args)), calls[-1])[1]      # what the bound call answered
        s = S0.copy()
        for t in range(4):
            ua = a.step(s.reshape(1, 4))                     # [1, S] float32: taken as it is
            assert calls[-1] == 0
            uc = c.step(s.astype(np.float64))                # float64: NotImplemented, then the ctypes body converts
            ub = b.step(s.reshape(1, 4))
            assert ua.tobytes() == ub.tobytes() == uc.tobytes()
            assert a.read("U_NOM").tobytes() == b.read("U_NOM").tobytes() == c.read("U_NOM").tobytes()
            s = plant(s, ua)
        a.step(s.astype(np.float64)); b.step(s.astype(np.float64))
        assert calls[-1] is NotImplemented
    finally:
        a._bound = inner
        a.close(); b.close(); c.close()


def raised(fn):
    with pytest.raises(Exception) as ei:
        fn()
    return type(ei.value), str(ei.value)


def test_error_status_and_closed_handle_raise_the_same_on_both_paths():
    import torch
    opt, kw = CASES["mppi N64 H4 p1"]
    a, b = pair(opt, kw)
    try:
        part = torch.zeros(a.mppi_partial_size(), device="cuda")
        for e in (a, b):
            e.step(S0)
            e.mppi_step_begin(S0, part.data_ptr())           # a sharded step is pending: ctk_step refuses
        ra, rb = raised(lambda: a.step(S0)), raised(lambda: b.step(S0))
        assert ra == rb and ra[0] is CtkError and "pending" in ra[1], (ra, rb)
        bad = np.zeros(a.samples_needed() + 1, np.float32)
        assert raised(lambda: a.step(S0, bad)) == raised(lambda: b.step(S0, bad))
        assert raised(lambda: a.step(np.zeros(5, np.float32))) == raised(lambda: b.step(np.zeros(5, np.float32))) == (ValueError, "state must have 4 entries")
        torch.cuda.synchronize()
    finally:
        a.close(); b.close()
    assert a.step_path == "ctypes"                            # the bound call is gone with the handle
    ra, rb = raised(lambda: a.step(S0)), raised(lambda: b.step(S0))
    assert ra == rb, (ra, rb)
