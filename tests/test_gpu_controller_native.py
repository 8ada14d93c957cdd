"""-m gpu: controller_mpc.step through the bound controller and optimizer steps (_ctk_pystep: bind_controller, bind_optimizer) against
the same controller held on the Python bodies by `native_step: false`.

Two controllers with equal seeds run a 30-step closed loop from the same state, with one cost-parameter change and one
`updated_attributes` in the middle; u of every step and the final u_nom must agree byte for byte: both paths hand ctk_step the same
floats and pointers and upload the same parameters before the same steps, so any difference is an error of the bound steps.
Shapes: N 64 (one workgroup) and N 192 (three records through the in-launch merge), H 8, CartPole ODE."""
import numpy as np
import pytest

from control_toolkit_amd.Controllers.controller_mpc import controller_mpc
from control_toolkit_amd.Cost_Functions import CostFunctionWrapper
from control_toolkit_amd.Predictors import PredictorWrapper
from control_toolkit_amd.others.globals_and_utils import DeviceBufferRng

pytestmark = pytest.mark.gpu

STEPS, CHANGE_COST_AT, UPDATE_ATTRIBUTES_AT = 30, 10, 20
S0 = np.array([0.05, -0.1, 2.8, 0.4], np.float32)


def have_module():
    try:
        import control_toolkit_amd._ctk_pystep  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.fixture(scope="module", autouse=True)
def module_is_there():
    assert have_module(), "control_toolkit_amd._ctk_pystep is not built: `make -C control_toolkit_amd/csrc`"


def build(optimizer, N, native):
    oc = dict(seed=3, mpc_horizon=8, num_rollouts=N, mpc_timestep=0.02, rng_mode="device", device=0, native_step=native)
    if optimizer == "mppi-hip":
        oc.update(cc_weight=1.0, R=1.0, LBD=100.0, NU=1000.0, SQRTRHOINV=0.03, period_interpolation_inducing_points=1)
    else:
        oc.update(cem_outer_it=3, cem_initial_action_stdev=0.5, cem_stdev_min=0.01, cem_best_k=8, warmup=False, warmup_iterations=0)
    cc = {"mpc": {"optimizer": optimizer, "predictor_specification": "ODE", "cost_function_specification": "default",
                  "computation_library": "hip", "controller_logging": False, "calculate_optimal_trajectory": False, "device": "gpu:0"}}
    c = controller_mpc("CartPole", (np.array([-1.0], np.float32), np.array([1.0], np.float32)),
                       {"target_position": 0.0, "target_equilibrium": 1.0}, config_controllers=cc, config_optimizers={optimizer: oc},
                       predictor=PredictorWrapper(), cost_function=CostFunctionWrapper(watch=False))
    c.configure()
    return c


def plant(s, u):
    """any deterministic float32 map closes the loop: the next state depends on every bit of u"""
    s = s.copy()
    s[0] += np.float32(0.02) * s[1]; s[1] += np.float32(0.3) * u
    s[2] += np.float32(0.02) * s[3]; s[3] -= np.float32(0.5) * u * np.cos(s[2])
    return s.astype(np.float32)


def closed_loop(optimizer, N, native, samples):
    import torch
    c = build(optimizer, N, native)
    o = c.optimizer
    try:
        assert (o._fast is not None) == native and type(c.step).__name__ == ("BoundControllerStep" if native else "method")
        pool = None
        if samples == "buffer":
            g = torch.Generator(device="cuda"); g.manual_seed(11)
            need = max(int(o.engine.samples_needed()), 3 * N * 8)     # at least what any step of either optimizer reads
            pool = [torch.randn((need,), generator=g, device="cuda", dtype=torch.float32) for _ in range(3)]
            torch.cuda.synchronize()
            o.rng = DeviceBufferRng([t.data_ptr() for t in pool], seed=1)
        s, us, paths = S0.copy(), [], []
        for t in range(STEPS):
            if t == CHANGE_COST_AT:
                c.cost_function.set_parameters(dd_weight=450.0, ep_weight=15000.0)
            u = c.step(s, updated_attributes={"target_position": 0.15}) if t == UPDATE_ATTRIBUTES_AT else c.step(s)
            assert type(u) is np.float32 and o.u is u
            us.append(u.tobytes()); paths.append(o.step_path)
            s = plant(s, u)
        u_nom = np.array(o.u_nom, np.float32)
        params = [o.engine.get_param(n) for n in ("dd_weight", "ep_weight", "target_position")]
        torch.cuda.synchronize()
        return us, u_nom, paths, params, pool
    finally:
        o.engine.close()


@pytest.mark.parametrize("samples", ["buffer", "device-rng"])
@pytest.mark.parametrize("N", [64, 192])
def test_mppi_closed_loop_native_equals_python(N, samples):
    ua, noma, pa, para, _ = closed_loop("mppi-hip", N, True, samples)
    ub, nomb, pb, parb, _ = closed_loop("mppi-hip", N, False, samples)
    assert [t for t in range(STEPS) if ua[t] != ub[t]] == []
    assert noma.shape == (1, 8, 1) and noma.tobytes() == nomb.tobytes()
    assert para == parb == [450.0, 15000.0, float(np.float32(0.15))]
    # the first step (u is the constructor's 0.0) and the two steps with something to upload are Python's, every other one is native
    assert [t for t in range(STEPS) if pa[t] == "python"] == [0, CHANGE_COST_AT, UPDATE_ATTRIBUTES_AT]
    assert set(pb) == {"python"}
    assert len(set(ua)) > STEPS // 2                           # a loop that moves: not thirty equal outputs


def test_cem_closed_loop_native_equals_python():
    ua, noma, pa, para, _ = closed_loop("cem-hip", 64, True, "buffer")
    ub, nomb, pb, parb, _ = closed_loop("cem-hip", 64, False, "buffer")
    assert [t for t in range(STEPS) if ua[t] != ub[t]] == []
    assert noma.tobytes() == nomb.tobytes() and para == parb
    assert [t for t in range(STEPS) if pa[t] == "python"] == [0, CHANGE_COST_AT, UPDATE_ATTRIBUTES_AT] and set(pb) == {"python"}
