"""CPU: the CEM-GMM optimizer (reference Optimizers/optimizer_cem_gmm_tf.py) — the NumPy restatement tests/gmm_oracle.py
against the reference-recorded fixtures, discovery of the host class, the draw layout of one step, and the engine name."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import ctk_oracle as O
from helpers import load, predictor_from
from gmm_oracle import CEMGMM, pack_draws, device_draws, UNIFORM_STREAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMM_CASES = ["default", "quad2d"]
# the template's `cem-gmm-tf` entry (Control_Toolkit_ASF_Template/config_optimizers.yml:15-22), verbatim
TEMPLATE_ENTRY = dict(seed=None, mpc_horizon=40, cem_outer_it=3, num_rollouts=200, cem_stdev_min=0.01, cem_initial_action_stdev=0.5,
                      cem_best_k=40)


def gmm_oracle_from(d) -> CEMGMM:
    pred = predictor_from(d)
    return CEMGMM(pred, O.Cost(pred.env, pred.dt), d["low"], d["high"], num_rollouts=int(d["num_rollouts"]),
                  mpc_horizon=int(d["mpc_horizon"]), cem_outer_it=int(d["cem_outer_it"]),
                  cem_initial_action_stdev=float(d["cem_initial_action_stdev"]), cem_stdev_min=float(d["cem_stdev_min"]),
                  cem_best_k=int(d["cem_best_k"]))


@pytest.mark.parametrize("case", GMM_CASES)
def test_cem_gmm_matches_reference(case):
    """optimizer_cem_gmm_tf.py:57-137 as the unmodified module computed it (tests/golden/make_golden_gmm.py); tolerances of
    test_oracle_golden.py::test_cem_matches_reference"""
    d = load(f"cem_gmm_{case}.npz")
    o = gmm_oracle_from(d)
    np.testing.assert_array_equal(o.dist_mue, d["dist_mue_init"])
    np.testing.assert_array_equal(o.stdev, d["stdev_init"])
    np.testing.assert_array_equal(o.probs, d["probs_init"])
    for t in range(int(d["steps"])):
        np.testing.assert_array_equal(np.broadcast_to(np.asarray(o.u, np.float32).reshape(-1), d[f"u_prev_{t}"].shape), d[f"u_prev_{t}"])
        u = o.step(d[f"s_{t}"], d[f"normals_{t}"], d[f"uniforms_{t}"])
        np.testing.assert_allclose(o.Q, d[f"Q_{t}"], rtol=1e-6, atol=2e-6)
        np.testing.assert_allclose(o.J, d[f"J_{t}"], rtol=2e-6)
        np.testing.assert_array_equal(o.probs, d[f"probs_{t}"])
        np.testing.assert_allclose(o.dist_mue, d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(o.stdev, d[f"stdev_{t}"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(np.asarray(u).reshape(-1), d[f"u_{t}"], rtol=1e-6, atol=1e-6)
        # the recorded closed loop continues from the reference's own distribution
        o.dist_mue, o.stdev, o.probs = d[f"dist_mue_{t}"].copy(), d[f"stdev_{t}"].copy(), d[f"probs_{t}"].copy()
        o.u = O._u_out(d[f"u_{t}"])
    assert o.min_margin > 1e-5     # no label of the recording was decided by rounding


def test_cem_gmm_discovery_and_constructor_keys():
    from control_toolkit_amd import _capi
    from control_toolkit_amd.others.globals_and_utils import import_optimizer_by_name, find_optimizer_if_it_exists
    from control_toolkit_amd.Cost_Functions import CostFunctionWrapper
    from control_toolkit_amd.Predictors import PredictorWrapper
    from control_toolkit_amd import HipLibrary
    cls = import_optimizer_by_name("cem-gmm-hip")
    full, path = find_optimizer_if_it_exists("cem-gmm-hip")
    assert cls.__name__ == full == os.path.splitext(os.path.basename(path))[0] == "optimizer_cem_gmm_hip"
    assert cls.engine_name == "cem_gmm"
    # the reference's ctor keys (optimizer_cem_gmm_tf.py:16-33), no warm-up keys, extra YAML keys swallowed by **kwargs
    params = inspect.signature(cls.__init__).parameters
    for k in ("predictor", "cost_function", "control_limits", "computation_library", "seed", "mpc_horizon", "cem_outer_it",
              "cem_initial_action_stdev", "num_rollouts", "cem_stdev_min", "cem_best_k", "optimizer_logging", "calculate_optimal_trajectory"):
        assert k in params
    assert "warmup" not in params and any(p.kind is p.VAR_KEYWORD for p in params.values())
    lim = (np.array([-1.0], np.float32), np.array([1.0], np.float32))
    opt = cls(predictor=PredictorWrapper(), cost_function=CostFunctionWrapper(), control_limits=lim, computation_library=HipLibrary(),
              optimizer_logging=True, calculate_optimal_trajectory=False, **dict(TEMPLATE_ENTRY, seed=5), some_future_key=1)
    assert (opt.cem_outer_it, opt.cem_best_k, opt.num_rollouts, opt.mpc_horizon) == (3, 40, 200, 40)
    assert opt.optimizer_name == "cem-gmm-hip"
    # engine name <-> enum value, in the binding and in the header
    assert _capi.OPTIMIZERS["cem_gmm"] == 7
    header = open(os.path.join(ROOT, "include", "ctk_hip.h")).read()
    assert re.search(r"CTK_OPT_CEM_GMM\s*=\s*7\b", header)
    for name in ("MIX_MU", "MIX_STD", "MIX_PROB", "MIX_LABEL"):
        assert re.search(rf"CTK_BUF_{name}\s*=\s*{_capi.BUFFERS[name]}\b", header)
    assert re.search(r"CTK_ABI_VERSION 6\b", header)


def test_cem_gmm_draw_layout():
    """one step consumes, per outer iteration, N*H*C normals (row-major [N,H,C]) FOLLOWED BY N uniforms"""
    from control_toolkit_amd.Optimizers.optimizer_cem_gmm_hip import optimizer_cem_gmm_hip, pack_gmm_draws, gmm_samples_needed
    from control_toolkit_amd.Cost_Functions import CostFunctionWrapper
    from control_toolkit_amd.Predictors import PredictorWrapper
    from control_toolkit_amd import HipLibrary
    its, N, H, C = 3, 7, 5, 2
    normals = np.arange(its * N * H * C, dtype=np.float32).reshape(its, N, H, C)
    uniforms = -1.0 - np.arange(its * N, dtype=np.float32).reshape(its, N)
    flat = pack_gmm_draws(normals, uniforms)
    assert flat.dtype == np.float32 and flat.size == gmm_samples_needed(its, N, H, C) == its * (N * H * C + N)
    per = N * H * C + N
    for it in range(its):
        np.testing.assert_array_equal(flat[it * per: it * per + N * H * C], normals[it].ravel())
        np.testing.assert_array_equal(flat[it * per + N * H * C: (it + 1) * per], uniforms[it])
    np.testing.assert_array_equal(flat, pack_draws(normals, uniforms))     # the restatement packs the same way

    class Rng:   # records what step() asks its generator for
        on_device = False
        calls = []

        def normal(self, shape, dtype=np.float32):
            self.calls.append(("normal", list(shape)))
            return normals

        def uniform(self, shape, dtype=np.float32):
            self.calls.append(("uniform", list(shape)))
            return uniforms
    lim = (np.array([-1.0, -1.0], np.float32), np.array([1.0, 1.0], np.float32))
    opt = optimizer_cem_gmm_hip(predictor=PredictorWrapper(), cost_function=CostFunctionWrapper(), control_limits=lim,
                                computation_library=HipLibrary(), seed=1, mpc_horizon=H, cem_outer_it=its, cem_initial_action_stdev=0.5,
                                num_rollouts=N, cem_stdev_min=0.01, cem_best_k=3, optimizer_logging=False, rng_mode="host")
    opt.num_control_inputs = C
    opt.rng = Rng()
    np.testing.assert_array_equal(opt._step_draws(), flat)
    assert Rng.calls == [("normal", [its, N, H, C]), ("uniform", [its, N])]
    opt.rng = type("Dev", (), {"on_device": True})()
    assert opt._step_draws() is None                                       # device mode: the engine draws


def test_cem_gmm_device_draw_streams():
    """the uniforms of a device-rng step live on a Philox stream of their own: distinct from every iteration's normals"""
    normals, uniforms = device_draws(seed=3, call=0, its=2, N=16, HC=6)
    assert normals.shape == (2, 16, 6) and uniforms.shape == (2, 16)
    assert np.all((uniforms >= 0.0) & (uniforms < 1.0))
    np.testing.assert_array_equal(uniforms[1], O.device_noise(3, UNIFORM_STREAM + 1, 0, 0, 16, 1, "uniform")[:, 0])
    assert not np.array_equal(uniforms[0], O.device_noise(3, 0, 0, 0, 16, 1, "uniform")[:, 0])


def test_cem_gmm_restatement_properties():
    """reset state, the K = 2 corner (two singleton clusters), the shift that repeats the last row, the K < 2 refusal"""
    env = O.EnvParams()
    pred = O.Predictor("ODE", dt=0.02, env=env)
    N, H = 32, 6
    with pytest.raises(ValueError):
        CEMGMM(pred, O.Cost(env), num_rollouts=N, mpc_horizon=H, cem_best_k=1)
    o = CEMGMM(pred, O.Cost(env), num_rollouts=N, mpc_horizon=H, cem_outer_it=2, cem_best_k=2, cem_stdev_min=0.05)
    assert o.dist_mue.shape == o.stdev.shape == (H, 1, 2)
    np.testing.assert_array_equal(o.probs, [0.5, 0.5])
    rng = np.random.default_rng(0)
    u = o.step(np.array([0.0, 0.0, 0.3, 0.0], np.float32), rng.standard_normal((2, N, H, 1)).astype(np.float32),
               rng.random((2, N), dtype=np.float32))
    np.testing.assert_array_equal(o.probs, [0.5, 0.5])
    np.testing.assert_array_equal(o.stdev, np.full((H, 1, 2), np.float32(0.05)))      # std 0 of a singleton, clipped up
    elite = o.Q[o.best_idx]
    np.testing.assert_array_equal(o.dist_mue[:-1, :, 0], elite[0, 1:])                 # shifted by one step ...
    np.testing.assert_array_equal(o.dist_mue[-1, :, 1], elite[1, -1])                  # ... repeating the last row
    np.testing.assert_array_equal(np.asarray(u).reshape(-1), elite[0, 0])
    assert o.state().size == 4 * H + 2 + 1 + 1
    # a larger K exercises both sides of the split, and the per-rollout component pick
    o = CEMGMM(pred, O.Cost(env), num_rollouts=64, mpc_horizon=H, cem_outer_it=3, cem_best_k=16)
    o.step(np.array([0.0, 0.0, 0.3, 0.0], np.float32), rng.standard_normal((3, 64, H, 1)).astype(np.float32), rng.random((3, 64), dtype=np.float32))
    n1 = int(np.sum(o.labels == 0))
    assert 1 <= n1 <= 15 and o.probs[0] == np.float32(n1) / np.float32(16) and o.probs[1] == np.float32(1) - o.probs[0]
    assert set(np.unique(o.comp)) <= {0, 1}


def test_cem_gmm_engine_name_reaches_the_library():
    """the binding knows the optimizer: without a GPU creation gets as far as the device check (not ValueError: unknown optimizer)"""
    import torch
    from control_toolkit_amd import CtkEngine, CtkError
    kw = dict(num_rollouts=32, mpc_horizon=10, dt=0.02, cem_outer_it=2, cem_best_k=4)
    if torch.cuda.is_available():
        CtkEngine("cem_gmm", "ODE", **kw).close()
    else:
        with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
            CtkEngine("cem_gmm", "ODE", **kw)
