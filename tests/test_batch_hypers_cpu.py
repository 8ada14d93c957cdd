"""CPU tests (-m "not gpu") of the per-problem MPPI hyper-parameters and input limits of the MPPI batches (include/ctk_hip_hyper.h,
CtkMppiBatch.set_problem_hypers / set_hyper / set_problem_limits): the pure argument checker, the header against the Python tables and
the library's exports, and the guard that keeps tests/test_gpu_batch_hypers.py from being vacuous — every case of hyper_cases.MPPI_CASES
moves the tensor it shows in by more than the bound tests/test_gpu_hyper.py compares that tensor with, so a kernel that ignored a
problem's value could not equal the handle created with it."""
import os
import re

import numpy as np
import pytest

from control_toolkit_amd import _capi
from control_toolkit_amd._capi import batch_hyper_args, HYPERS, HYPER_SYMBOLS
import hyper_cases as Hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
HYPER_HEADER = os.path.join(ROOT, "include", "ctk_hip_hyper.h")
# the bounds tests/test_gpu_hyper.py compares J and u / U_NOM with (test_gpu_large_angles.J_TOL, test_gpu_mppi.U_TOL): restated, because
# importing a GPU test module here would load the device helpers
J_TOL = dict(rtol=3e-5, atol=1e-3)
U_TOL = dict(rtol=1e-4, atol=2e-5)
FAMILIES = (("ctk_batch", "ctk_problem"), ("ctk_mlp_batch", "ctk_mlp_problem"), ("ctk_gru_batch", "ctk_gru_problem"))


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------
def test_checker_accepts_scalars_and_one_value_per_listed_problem():
    hid, idv, n, vals = batch_hyper_args(4, "LBD", 30.0)
    assert (hid, idv, n) == (HYPERS["LBD"], None, 4) and vals.dtype == np.float32 and vals.tolist() == [30.0] * 4
    hid, idv, n, vals = batch_hyper_args(4, "NU", [2.0, -0.5], ids=[1, 3])
    assert hid == HYPERS["NU"] and idv.tolist() == [1, 3] and idv.dtype == np.int32 and n == 2 and vals.tolist() == [2.0, -0.5]
    for name in HYPERS:
        assert batch_hyper_args(2, name, 0.5)[0] == HYPERS[name]
    assert batch_hyper_args(2, "cc_weight", 0.0)[3].tolist() == [0.0, 0.0]        # only LBD and NU have a forbidden value
    assert batch_hyper_args(2, "R", -1.0)[3].tolist() == [-1.0, -1.0]


def test_checker_accepts_limits_as_scalars_rows_and_tables():
    hid, idv, n, (lo, hi) = batch_hyper_args(3, "limits", (-0.2, 0.4), Cn=2)
    assert hid is None and idv is None and n == 3 and lo.shape == hi.shape == (3, 2) and lo.dtype == np.float32
    _, _, _, (lo, hi) = batch_hyper_args(3, "limits", ([-0.2, -0.3], [0.35, 0.15]), Cn=2)
    assert lo.tolist() == [[np.float32(-0.2), np.float32(-0.3)]] * 3 and hi[2].tolist() == [np.float32(0.35), np.float32(0.15)]
    _, idv, n, (lo, hi) = batch_hyper_args(3, "limits", ([[-1.0], [0.0]], 0.5), ids=[0, 2], Cn=1)
    assert idv.tolist() == [0, 2] and n == 2 and lo.tolist() == [[-1.0], [0.0]] and hi.tolist() == [[0.5], [0.5]]
    assert batch_hyper_args(1, "limits", (0.3, 0.3))[3][0].tolist() == [[np.float32(0.3)]]          # low == high is allowed, as at creation


@pytest.mark.parametrize("args,kw,text", [
    ((4, "lambda", 1.0), {}, "unknown hyper-parameter 'lambda'"),
    ((4, "target_position", 1.0), {}, "unknown hyper-parameter"),                 # an environment parameter is not a hyper-parameter
    ((4, "LBD", [1.0, 2.0]), {}, r"one value per listed problem \(4\)"),
    ((4, "LBD", [1.0, 2.0, 3.0]), {"ids": [0, 2]}, r"one value per listed problem \(2\)"),
    ((4, "LBD", [[1.0, 2.0]]), {"ids": [0, 2]}, "one value per listed problem"),
    ((4, "LBD", "much"), {}, "must be a number"),
    ((4, "LBD", 1.0), {"ids": [0, 4]}, r"ids must lie in 0 \.\. 3"),
    ((4, "LBD", 1.0), {"ids": [2, 1]}, "strictly ascending"),
    ((4, "LBD", 1.0), {"ids": []}, "non-empty"),
    ((4, "R", [1.0, float("nan"), 1.0, 1.0]), {}, "finite in fp32.*problem 1"),
    ((4, "R", [1.0, float("inf")]), {"ids": [0, 3]}, "finite in fp32.*problem 3"),
    ((4, "SQRTRHOINV", 1e39), {}, "finite in fp32.*problem 0"),
    ((4, "LBD", [1.0, 1.0, 0.0, 1.0]), {}, "'LBD' must be > 0.*problem 2"),
    ((4, "LBD", [-3.0]), {"ids": [2]}, "'LBD' must be > 0.*problem 2"),
    ((4, "LBD", 1e-60), {}, "'LBD' must be > 0.*problem 0"),                      # rounds to 0 in fp32, which is what the library would see
    ((4, "NU", [1.0, 0.0]), {"ids": [1, 3]}, "'NU' must not be 0.*problem 3"),
    ((4, "limits", 1.0), {}, r"pair \(low, high\)"),
    ((4, "limits", ([0.0, 0.0], 1.0)), {"Cn": 1}, "low must be a scalar"),
    ((4, "limits", (0.0, [[1.0], [1.0]])), {"Cn": 1}, "high must be a scalar"),
    ((4, "limits", (0.0, float("nan"))), {}, "high must be finite in fp32.*problem 0, input 0"),
    ((4, "limits", ([[0.0, 0.2], [0.0, 0.6]], 0.5)), {"ids": [1, 2], "Cn": 2}, "low must be <= high.*problem 2, input 1"),
    ((4, "limits", (0.0, 1.0)), {"ids": [7]}, "ids must lie in"),
])
def test_checker_refuses(args, kw, text):
    with pytest.raises(ValueError, match=text):
        batch_hyper_args(*args, **kw)


def test_calls_are_on_the_mppi_batches_only():
    """the seven calls live on the view CtkMppiBatch.hypers (BatchHypers) and are reachable on an MPPI batch under its own name; the
    classes' attribute lists, which tests/test_batch_cpu.py pins, stay what they were, and CEM / RPGD batches and handles have neither"""
    import control_toolkit_amd
    names = ("set_problem_hypers", "set_hyper", "get_problem_hyper", "get_problem_hypers", "set_problem_limits", "get_problem_limits", "hypers_differ")
    assert _capi.BatchHypers.CALLS == names and all(callable(getattr(_capi.BatchHypers, n)) for n in names)
    for cls in (_capi.CtkMppiBatch, _capi.CtkMppiMlpBatch, _capi.CtkMppiGruBatch):
        assert isinstance(cls.hypers, property)
        b = cls.__new__(cls)                                        # no device: the forwarding needs no handle
        for n in names:
            m = getattr(b, n)
            assert m.__func__ is getattr(_capi.BatchHypers, n) and m.__self__._batch is b
        with pytest.raises(AttributeError):
            b.no_such_call
    for cls in (_capi.CtkCemBatch, _capi.CtkRpgdBatch, _capi.CtkEngine):
        assert not hasattr(cls, "hypers")
        b = cls.__new__(cls)
        assert not any(hasattr(b, n) for n in names), cls.__name__
    assert control_toolkit_amd.batch_hyper_args is batch_hyper_args and control_toolkit_amd.HYPERS is HYPERS
    assert control_toolkit_amd.BatchHypers is _capi.BatchHypers


# ---- the header -----------------------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HYPER_HEADER).read(), flags=re.S)


def test_header_declares_the_eighteen_entries_and_the_library_exports_them():
    declared = sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", header_text())))
    want = sorted([f"{prob}_{e}" for _, prob in FAMILIES for e in ("set_hyper", "get_hyper", "set_limits", "get_limits", "hypers_differ")] +
                  [f"{fam}_set_hyper" for fam, _ in FAMILIES])
    assert len(want) == 18 and declared == want
    assert sorted(HYPER_SYMBOLS) == want                                           # the ctypes table binds exactly these
    assert re.search(r'^#include "ctk_hip_hyper.h"', open(HEADER).read(), flags=re.M)   # a caller includes one header
    lib = _capi.load_library()
    for name in want:
        assert hasattr(lib, name), f"libctk_hip.so does not export {name}"
    assert lib.ctk_abi_version() == 6
    assert not (set(want) & set(_capi.SYMBOLS))                                    # ctk_hip.h's own list stays what it was


def test_enum_matches_the_python_table():
    body = re.search(r"enum ctk_hyper\s*\{(.*?)\}", header_text(), flags=re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"CTK_HYPER_([A-Z_]+)\s*=\s*(\d+)", body)}
    assert enum.pop("COUNT") == len(HYPERS) == 5
    assert enum == {k.upper(): v for k, v in HYPERS.items()}
    assert list(HYPERS) == ["cc_weight", "R", "LBD", "NU", "SQRTRHOINV"]
    text = open(HYPER_HEADER).read()
    assert "CTK_P_R" in text and "CTK_P_CC_WEIGHT" in text                         # the header tells them from the environment's parameters


# ---- the guard against a vacuous GPU test ------------------------------------------------------------------------------------------------------
def shows_in(own):
    """the tensors a case must show in: the one hyper_cases names for a single-value case, J for the cases that move everything"""
    return sorted({Hc.MPPI_SHOWS_IN[k] for k, _ in own}) if len(own) == 1 else ["J"]


@pytest.mark.parametrize("own", Hc.MPPI_CASES, ids=Hc.mppi_id)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_case_moves_its_tensor_by_more_than_the_gpu_bound(env, own):
    """problem 0 of the GPU test's batch keeps the defaults, problem j gets a case: with the same state, plan and draws the float32
    oracle's J (u_nom for LBD) of the case is outside the GPU bound around the defaults' on most rows, so equality with the case's handle
    cannot come from a kernel that used the defaults.  "Most rows" — more than half of the elements — is this test's own reading of "differs by
    more than the bound" (one element would satisfy the letter); a case that moves everything is held to J alone."""
    N, H, p = Hc.MPPI_SIZES[0]
    far = Hc.is_far(own)
    case, base = Hc.mppi_ref(env, own, N, H, p), Hc.mppi_ref(env, (), N, H, p, far)
    np.testing.assert_array_equal(case["s"], base["s"])
    np.testing.assert_array_equal(case["noise"], base["noise"])
    LBD = Hc.config_of(Hc.MPPI_DEFAULTS, own)["LBD"]
    for name in shows_in(own):
        tol = J_TOL if name == "J" else Hc.u_bound(min(LBD, 100.0), **U_TOL)      # the wider of the two problems' bounds
        a, b = np.asarray(case[name], np.float64), np.asarray(base[name], np.float64)
        outside = np.abs(a - b) > tol["atol"] + tol["rtol"] * np.abs(b)
        print(f"{env} {Hc.mppi_id(own)}: {name} outside the bound on {outside.mean():.2f} of the elements, largest difference {np.abs(a - b).max():.3g}")
        assert outside.mean() > 0.5, f"{env} {Hc.mppi_id(own)}: {name} differs from the defaults' by more than the bound on {outside.mean():.2f} of the elements only"
