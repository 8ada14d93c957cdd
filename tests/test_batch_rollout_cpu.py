"""CPU tests (-m "not gpu") of the batch rollout (BatchRollout; include/ctk_hip_rollout.h): the header against the symbol table, the five
signatures, every refusal of batch_rollout_args with the library not loaded, and the guard of the case inputs.

The guard: for the inputs of batch_rollout_cases.py the oracle's float32 rollout (O.Predictor.predict_core + Cost.get_trajectory_cost)
must stay within SHARE of the GPU tests' tolerances (trajectories rtol 1e-4 / atol 2e-5, J rtol 3e-5: tests/test_gpu_env.py) against the
float64 statement of the same plant (param_cases.PlantF64, stepwise rounded) — else the inputs themselves would eat the bound the kernels
are held to.  Worst use measured on this file's cases (fraction of the bound; trajectories, J):
    CartPole 0.0112, 0.0234    Quad2D 0.0154, 0.0103    Hover 0.0067, 0.0082    (SHARE = 0.25)"""
import os
import re

import numpy as np
import pytest

import batch_rollout_cases as R
from param_cases import PlantF64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip_rollout.h")
SHARE = 0.25
TRAJ_TOL, J_RTOL = dict(rtol=1e-4, atol=2e-5), 3e-5


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_exactly_the_rollout_symbols():
    from control_toolkit_amd import _capi
    declared = sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", header_text())))
    assert declared == sorted(_capi.ROLLOUT_SYMBOLS) == sorted(f"{b}_rollout" for b, _ in _capi._BATCH_FAMILIES)
    others = [_capi.SYMBOLS, _capi.RUN_SYMBOLS, _capi.EPISODE_SYMBOLS, _capi.LOOP_SYMBOLS, _capi.GRU_LOOP_SYMBOLS, _capi.HYPER_SYMBOLS,
              _capi.FAMILY_HYPER_SYMBOLS, _capi.AHEAD_SYMBOLS]
    for table in others:
        assert not set(_capi.ROLLOUT_SYMBOLS) & set(table)
    main = open(os.path.join(ROOT, "include", "ctk_hip.h")).read()
    assert len(re.findall(r'^#include "ctk_hip_rollout.h"', main, flags=re.M)) == 1            # a caller includes one header
    assert not re.findall(r"\bctk_[a-z_]*batch_rollout\s*\(", main)                             # the entry text lives in the new header
    assert _capi.ROLLOUT_MODELS == {"controller": 0, "plant": 1}
    assert re.search(r"CTK_ROLLOUT_MODEL_CONTROLLER = 0", header_text()) and re.search(r"CTK_ROLLOUT_MODEL_PLANT = 1", header_text())


def test_the_five_signatures_are_equal_and_cite_what_they_replace():
    from control_toolkit_amd import _capi
    sigs = list(_capi.ROLLOUT_SYMBOLS.values())
    assert len(sigs) == 5 and all(s == sigs[0] for s in sigs) and len(sigs[0][1]) == 12
    text = re.sub(r"\s+", " ", header_text())
    shapes = set()
    for name in _capi.ROLLOUT_SYMBOLS:
        m = re.search(r"int " + name + r"\(ctk_[a-z_]+\* b, ([^)]*)\)", text)
        assert m, name
        shapes.add(m.group(1))
    assert len(shapes) == 1 and shapes.pop().count(",") == 10
    raw = open(HEADER).read()
    for name in _capi.ROLLOUT_SYMBOLS:                                                          # each cites the reference call it replaces
        assert re.search(name + r"\([^;]*;\s*/\* replaces: [^*]*(predict_core|predictor)", raw, flags=re.S), name


def test_view_class_and_exports():
    import control_toolkit_amd
    from control_toolkit_amd import _capi
    assert control_toolkit_amd.BatchRollout is _capi.BatchRollout and "BatchRollout" in control_toolkit_amd.__all__
    assert control_toolkit_amd.batch_rollout_args is _capi.batch_rollout_args
    assert _capi.BatchRollout.CALLS == ("rollout", "optimal_trajectory") and all(callable(getattr(_capi.BatchRollout, n)) for n in _capi.BatchRollout.CALLS)
    for cls in (_capi.CtkMppiBatch, _capi.CtkMppiMlpBatch, _capi.CtkMppiGruBatch, _capi.CtkCemBatch, _capi.CtkRpgdBatch):
        assert isinstance(getattr(cls, "rollouts"), property)                                   # a view, not a method: the method lists stay


def test_batch_rollout_args_checks_everything_without_the_library(monkeypatch):
    from control_toolkit_amd import _capi
    monkeypatch.setattr(_capi, "load_library", lambda *a, **k: pytest.fail("the library was touched"))
    B, S, C, H, N = 5, 4, 1, 7, 70
    A = lambda *a, **k: _capi.batch_rollout_args(B, S, C, H, N, *a, **k)
    st = np.zeros((B, S), np.float32)
    # what passes: all problems with their own plans; a permuted subset; a broadcast; the plant model
    idv, n, s2, up, pl, M, model, sub = A(st)
    assert idv is None and n == B and up is None and pl is None and (M, model, sub) == (1, 0, 0)
    idv, n, _, up, pl, M, model, sub = A(st[:3], np.zeros((3, 37, H, C)), 0.5, [4, 1, 3], "plant", 2)
    assert idv.dtype == np.int32 and list(idv) == [4, 1, 3] and n == 3 and up.shape == (3, 1) and pl.shape == (3, 37, H, C) and (M, model, sub) == (37, 1, 2)
    assert A(st, np.ones((9, H, C)))[4].shape == (B, 9, H, C) and A(st, np.ones((9, H)))[4].shape == (B, 9, H, C)
    assert A(st[0], np.ones((2, H)), ids=[3])[1] == 1
    ptr = A(st, (123456, 3))
    assert ptr[4] == 123456 and ptr[5] == 3 and A(st, 123456)[5] == 1
    # every refusal
    for bad in ([], [0, 0], [1, 2, 1], [5], [-1], [0.5]):
        with pytest.raises(ValueError, match="ids"):
            A(st[:max(1, len(bad))], ids=bad)
    with pytest.raises(ValueError, match="states must have shape"):
        A(st[:4])
    with pytest.raises(ValueError, match="states must have shape"):
        A(np.zeros((B, S + 1)))
    with pytest.raises(ValueError, match="u_prev must be"):
        A(st, None, np.zeros((B, 2)))
    with pytest.raises(ValueError, match="u_prev must be"):
        A(st, None, np.zeros(B - 1))
    for bad in (np.zeros((B, 3, H + 1, C)), np.zeros((B - 1, 3, H, C)), np.zeros((3, H, C + 1)), np.zeros(H), np.zeros((B, 3, H, C, 1))):
        with pytest.raises(ValueError, match="plans must have shape"):
            A(st, bad)
    with pytest.raises(ValueError, match="1 <= M <= num_rollouts"):
        A(st, np.zeros((B, N + 1, H, C)))
    with pytest.raises(ValueError, match="1 <= M <= num_rollouts"):
        A(st, np.zeros((B, 0, H, C)))
    with pytest.raises(ValueError, match="1 <= M <= num_rollouts"):
        A(st, (123456, N + 1))
    with pytest.raises(ValueError, match="integer M"):
        A(st, (123456, 2.0))
    with pytest.raises(ValueError, match="model must be"):
        A(st, model="true plant")
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="plant_substeps must be"):
            A(st, model="plant", plant_substeps=bad)
    with pytest.raises(ValueError, match="plant_substeps belongs to"):
        A(st, plant_substeps=2)
    # more than one input: [M, H] is not a plan
    with pytest.raises(ValueError, match="plans must have shape"):
        _capi.batch_rollout_args(3, 6, 2, H, N, np.zeros((3, 6)), np.zeros((4, H)))
    assert _capi.batch_rollout_args(3, 6, 2, H, N, np.zeros((3, 6)), np.zeros((4, H, 2)), [0.1, 0.2])[3].shape == (3, 2)


def use_of_the_bound(env):
    """the largest fraction of the GPU tolerances that float32 against float64 uses on the cases' inputs: (trajectories, J)"""
    worst_t = worst_j = 0.0
    for N, H, M in R.SHAPES:
        B = 3
        S, Q, up = R.states(env, B), R.plans(env, B, M, H), R.u_prev(env, B)
        for p in range(B):
            traj, J = R.oracle_rollout(env, p, S[p], Q[p], up[p])
            plant = PlantF64(env, R.params_of(env, p), dt=R.DT)
            t64 = plant.rollout(S[p], Q[p], rounded=True)
            j64 = plant.trajectory_cost(t64, Q[p], up[p]).numpy()
            t64 = t64.numpy()
            worst_t = max(worst_t, float(np.max(np.abs(traj - t64) / (TRAJ_TOL["atol"] + TRAJ_TOL["rtol"] * np.abs(t64)))))
            worst_j = max(worst_j, float(np.max(np.abs(J - j64) / (J_RTOL * np.abs(j64)))))
    return worst_t, worst_j


@pytest.mark.parametrize("env", sorted(R.INERTIAL))
def test_case_inputs_leave_the_bound_to_the_kernels(env):
    pytest.importorskip("torch")
    worst_t, worst_j = use_of_the_bound(env)
    print(f"{env}: float32 oracle against float64 uses {worst_t:.4f} of the trajectory bound, {worst_j:.4f} of the J bound")
    assert worst_t <= SHARE and worst_j <= SHARE


def test_cases_are_what_the_docstring_says():
    for env in R.INERTIAL:
        lo, hi = (np.asarray(a, np.float32) for a in R.LIMITS[env])
        q = R.plans(env, 3, 37, 7)
        inside = (q >= lo) & (q <= hi)
        assert not inside[0, 36].any() and inside[0, :36].all() and inside[1:].all()            # exactly one row outside the limits
        assert len({R.own_params(env, p) for p in range(5)}) == 5                                 # every problem its own parameters
        assert R.own_params(env, 1)[0][1] == float(np.float32(getattr(R.L.env_params(env), R.INERTIAL[env])))   # scale 1.0: the default
    assert sorted(len(v) for v in R.IDS.values()) == [3, 3] and all(v[0] is None and len(v[2]) == 1 for v in R.IDS.values())
