"""CPU tests (-m "not gpu") of the closed loop on the device (CtkMppiBatch.closed_loop / CtkMppiMlpBatch.closed_loop; include/ctk_hip_run.h:
ctk_batch_plant_* / ctk_batch_run and the ctk_mlp_batch_ forms): every new entry point is declared, bound with argument types and exported;
the Python side checks shapes, ids, step and sub-step counts and refuses sample buffers BEFORE the library is touched; and a guard on the
inputs of test_gpu_batch_run.py — over its start states, the oracle's float32 step is far inside the bound the GPU tests assert the plant
kernel with, so that the bound is spent on the kernel and not on the reference."""
import os
import re

import numpy as np
import pytest

import batch_run_cases as K
from large_angle_cases import StepF64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_HEADER = os.path.join(ROOT, "include", "ctk_hip_run.h")
ENTRIES = ["plant_set_param", "plant_get_param", "plant_clear_params", "plant_step", "run"]
METHODS = ["run", "plant_step", "set_plant_params", "get_plant_params", "clear_plant_params"]


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", src)))


def test_every_new_symbol_is_declared_bound_and_exported():
    from control_toolkit_amd._capi import load_library, RUN_SYMBOLS, SYMBOLS
    want = sorted(f"{fam}_{e}" for fam in ("ctk_batch", "ctk_mlp_batch") for e in ENTRIES)
    assert declared(RUN_HEADER) == want == sorted(RUN_SYMBOLS)
    assert not set(RUN_SYMBOLS) & set(SYMBOLS)
    # ctk_hip.h brings them in: a caller includes one header
    assert re.search(r'^#include "ctk_hip_run.h"', open(os.path.join(ROOT, "include", "ctk_hip.h")).read(), flags=re.M)
    lib = load_library()
    for n in want:
        res, args = RUN_SYMBOLS[n]
        fn = getattr(lib, n)                                 # AttributeError: not exported
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
    for e in ENTRIES:                                        # the MLP family forwards under its own names, same signatures
        assert RUN_SYMBOLS["ctk_mlp_batch_" + e] == RUN_SYMBOLS["ctk_batch_" + e]
    assert len(RUN_SYMBOLS["ctk_batch_run"][1]) == 10 and len(RUN_SYMBOLS["ctk_batch_plant_step"][1]) == 7
    # NULL handles answer like the other entries'
    assert lib.ctk_batch_run(None, 0, None, None, None, 1, 0, None, None, None) == 1
    assert lib.ctk_mlp_batch_run(None, 0, None, None, None, 1, 0, None, None, None) == 1
    assert lib.ctk_batch_plant_step(None, 0, None, None, None, 0, None) == 1 and lib.ctk_batch_plant_clear_params(None) == 1


def test_the_header_compiles_as_c(tmp_path):
    import subprocess
    for first in ("ctk_hip.h", "ctk_hip_run.h"):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\nint main(void) {{ return ctk_batch_run(0, 0, 0, 0, 0, 1, 0, 0, 0, 0) + ctk_mlp_batch_plant_clear_params(0) > 99; }}\n')
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")], check=True)


def test_the_classes_have_the_closed_loop():
    import control_toolkit_amd
    from control_toolkit_amd._capi import BatchClosedLoop, CtkMppiBatch, CtkMppiMlpBatch, CtkCemBatch, CtkRpgdBatch
    assert control_toolkit_amd.BatchClosedLoop is BatchClosedLoop and "BatchClosedLoop" in control_toolkit_amd.__all__
    assert isinstance(CtkMppiBatch.closed_loop, property) and CtkMppiMlpBatch.closed_loop is CtkMppiBatch.closed_loop
    for m in METHODS:
        assert callable(getattr(BatchClosedLoop, m)), m
    assert isinstance(BatchClosedLoop.last_run_first_bad, property)
    assert not hasattr(CtkCemBatch, "closed_loop") and not hasattr(CtkRpgdBatch, "closed_loop")      # a follow-up on the same plant kernel


def test_arguments_are_checked_before_the_library_is_touched():
    from control_toolkit_amd._capi import BatchClosedLoop, batch_run_args

    class NoLibrary:                                          # stands in for a batch: any touch of the library or a buffer raises
        B, S, C = 3, 4, 1
        param_names = ("g", "m_cart", "m_pole")

        def __getattr__(self, name):
            raise AssertionError(f"the batch's {name} was touched before the arguments were checked")

    loop = BatchClosedLoop(NoLibrary())
    S0 = np.zeros((3, 4), np.float32)
    for bad in (np.zeros((3, 5)), np.zeros((2, 4)), np.zeros(4), np.zeros((3, 4, 1))):
        with pytest.raises(ValueError, match=r"states must have shape \(3, 4\)"):
            loop.run(bad, 6)
    with pytest.raises(ValueError, match=r"states must have shape \(2, 4\)"):
        loop.run(S0, 6, ids=[0, 2])
    with pytest.raises(ValueError, match=r"u_prev must have shape \(3, 1\)"):
        loop.run(S0, 6, u_prev=np.zeros((3, 2)))
    for bad in ([3], [-1, 0], [0, 3]):
        with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
            loop.run(S0[:len(bad)], 6, ids=bad)
    with pytest.raises(ValueError, match="strictly ascending"):
        loop.run(S0[:2], 6, ids=[1, 0])
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="at least one step"):
            loop.run(S0, bad)
    for bad in (0, -2, 1.5, False):
        with pytest.raises(ValueError, match="plant_substeps must be an integer >= 1 or None"):
            loop.run(S0, 6, plant_substeps=bad)
    for samples in (np.zeros((3, 70, 3, 1), np.float32), 0x7F0000001000):
        with pytest.raises(NotImplementedError, match="device Philox only"):
            loop.run(S0, 6, samples=samples)
    with pytest.raises(ValueError, match=r"S must have shape \(3, 4\)"):
        loop.plant_step(np.zeros((3, 3)), np.zeros((3, 1)))
    with pytest.raises(ValueError, match=r"U must have shape \(3, 1\)"):
        loop.plant_step(S0, np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"U must have shape \(3, 1\)"):
        loop.plant_step(S0, None)
    with pytest.raises(ValueError, match="plant_substeps"):
        loop.plant_step(S0, np.zeros((3, 1)), plant_substeps=0)
    with pytest.raises(ValueError, match="unknown parameter 'mass'"):
        loop.set_plant_params("mass", 1.0)
    with pytest.raises(ValueError, match="one value per listed problem"):
        loop.set_plant_params("m_pole", [0.1, 0.2])
    with pytest.raises(ValueError, match="must be finite"):
        loop.set_plant_params("m_pole", float("nan"))
    with pytest.raises(ValueError, match="unknown parameter 'mass'"):
        loop.get_plant_params("mass")
    assert batch_run_args(3, 4, 1, S0, 6) == (None, 3, 0) and batch_run_args(3, 4, 1, S0[:1], np.int64(2), ids=[1], plant_substeps=4)[1:] == (1, 4)


def test_cases_are_what_the_issue_names():
    assert K.CASES["CartPole"][:3] == (70, 7, 3) and K.CASES["Quad2D"][:3] == (128, 12, 5) and K.CASES["Hover"][:3] == (128, 12, 1)
    assert (K.B, K.B_SPLIT, K.STEPS, K.STEPS_SEGMENTS) == (3, 5, 6, 10) and K.SCALES == (0.8, 1.0, 1.3)
    assert [K.CASES[e][5] for e in K.ENVS] == ["m_pole", "mass", "mass"]
    for env in K.ENVS:
        name, vals = K.override_values(env, K.B_SPLIT)
        base = getattr(K.CASES[env][4](), name)
        np.testing.assert_allclose(vals / base, [0.8, 1.0, 1.3, 0.8, 1.0], rtol=1e-6)
        s = K.start_states(env, K.B)
        assert s.shape == (K.B, K.CASES[env][4].S) and s.dtype == np.float32
        if env == "CartPole":
            assert (np.abs(s[:, 2] - 2.6) <= 0.4 + 1e-6).all()
    # at the tested sub-step counts the library's sub-step length (fp32(double(fp32 dt) / n) or fp32(dt / n)) is the oracle's float32
    for n in K.SUBSTEPS:
        assert np.float32(K.DT / n) == np.float32(float(np.float32(K.DT)) / n)


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("env", K.ENVS)
def test_the_oracle_step_uses_a_small_part_of_the_bound(env, substeps):
    """The reference of the plant tests is the oracle's float32 Predictor.step.  Against the same step in float64 on the float32 state
    (large_angle_cases.StepF64: what another association of the same arithmetic may differ by), over the case start states and 300
    steps of uniform inputs with the per-problem overrides, it must use at most a tenth of the trajectory bound rtol 1e-4 / atol 2e-5.
    Measured: worst 1.0 % of the bound over the three environments at 1 and 4 sub-steps (Quad2D at 4)."""
    name, vals = K.override_values(env, K.B_SPLIT)
    worst = 0.0
    for p in range(K.B_SPLIT):
        pars = K.plant_oracle(env, substeps, **{name: vals[p]}).env
        f32_step = K.plant_oracle(env, substeps, **{name: vals[p]})
        f64_step = StepF64("ODE", dt=K.DT, intermediate_steps=substeps, env=pars)
        s = K.start_states(env, K.B_SPLIT)
        U = K.uniform_inputs(env, (300, K.B_SPLIT), seed=p)
        for k in range(300):
            a, b = f32_step.step(s, U[k]), f64_step.step(s, U[k])
            bound = K.TRAJ_TOL["atol"] + K.TRAJ_TOL["rtol"] * np.abs(b.astype(np.float64))
            worst = max(worst, float((np.abs(a.astype(np.float64) - b) / bound).max()))
            s = a
        assert np.isfinite(s).all()
    print(f"{env} substeps {substeps}: the oracle's float32 step uses {100 * worst:.2f} % of the bound")
    assert worst <= 0.1
