"""CPU tests (-m "not gpu") of the per-problem parameters of a batch (include/ctk_hip.h: ctk_problem_set_param / ctk_problem_get_param /
ctk_problem_params_differ; control_toolkit_amd._capi: batch_param_args, CtkMppiBatch.set_problem_params): the symbols are declared and
bound with their argument types under names that leave the ctk_batch_* family as it was, and what needs no device is refused before the
library is asked."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
NEW = ("ctk_problem_get_param", "ctk_problem_params_differ", "ctk_problem_set_param")
NAMES = ("g", "m_cart", "m_pole", "L", "u_max", "M_fric", "J_fric", "target_position", "target_equilibrium", "dd_weight")


def test_new_symbols_are_declared_and_bound_with_argument_types():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ctk_problem_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(NEW)
    assert not any(n.startswith("ctk_batch_") for n in declared)
    assert len(set(re.findall(r"\b(ctk_batch_[a-z_0-9]+)\s*\(", src))) == 15           # the batch family itself is what it was
    lib = load_library()
    for n in NEW:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
    assert [len(SYMBOLS[n][1]) for n in NEW] == [4, 1, 5]
    assert SYMBOLS["ctk_problem_set_param"][0] is ctypes.c_int and SYMBOLS["ctk_problem_params_differ"][0] is ctypes.c_int
    assert lib.ctk_abi_version() == 6                       # additive: the ABI version stays


def test_library_refuses_null_batches():
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    v = ctypes.c_float(1.0)
    assert lib.ctk_problem_set_param(None, 0, None, 0, ctypes.byref(v)) == 1
    assert lib.ctk_problem_get_param(None, 0, 0, ctypes.byref(v)) == 1
    assert lib.ctk_problem_params_differ(None) == 0


def test_parameter_arguments_are_checked_without_a_device(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import batch_param_args

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    B = 6
    pid, ids, n, v = batch_param_args(NAMES, B, "target_position", np.linspace(-0.1, 0.1, B))
    assert pid == 7 and ids is None and n == B and v.dtype == np.float32 and v.shape == (B,) and v.flags.c_contiguous
    pid, ids, n, v = batch_param_args(NAMES, B, "L", 0.25)                                # a scalar reaches every listed problem
    assert pid == 3 and ids is None and n == B and np.array_equal(v, np.full(B, 0.25, np.float32))
    pid, ids, n, v = batch_param_args(NAMES, B, "dd_weight", [500.0, 700.0], ids=[1, 4])
    assert pid == 9 and ids.dtype == np.int32 and list(ids) == [1, 4] and n == 2 and list(v) == [500.0, 700.0]
    pid, ids, n, v = batch_param_args(NAMES, B, "dd_weight", 650, ids=[0, 2, 5])
    assert n == 3 and list(v) == [650.0] * 3
    # an unknown name
    with pytest.raises(ValueError, match=r"unknown parameter 'target_x'"):
        batch_param_args(NAMES, B, "target_x", 0.1)
    with pytest.raises(ValueError, match=r"unknown parameter 3"):
        batch_param_args(NAMES, B, 3, 0.1)
    # the shape of values against ids
    with pytest.raises(ValueError, match=r"one value per listed problem \(6\)"):
        batch_param_args(NAMES, B, "L", np.zeros(5))
    with pytest.raises(ValueError, match=r"one value per listed problem \(2\)"):
        batch_param_args(NAMES, B, "L", np.zeros(B), ids=[0, 1])
    with pytest.raises(ValueError, match=r"one value per listed problem \(6\)"):
        batch_param_args(NAMES, B, "L", np.zeros((B, 1)))
    with pytest.raises(ValueError, match=r"one value per listed problem \(3\)"):
        batch_param_args(NAMES, B, "L", [], ids=[0, 1, 2])
    # ids that are not strictly ascending, or outside the batch
    for bad in ([2, 1], [1, 1], [0, 3, 2]):
        with pytest.raises(ValueError, match="strictly ascending"):
            batch_param_args(NAMES, B, "L", np.zeros(len(bad)), ids=bad)
    with pytest.raises(ValueError, match=r"0 \.\. 5"):
        batch_param_args(NAMES, B, "L", [0.2, 0.2], ids=[0, 6])
    with pytest.raises(ValueError, match="non-empty"):
        batch_param_args(NAMES, B, "L", [], ids=[])
    # a value that is not finite
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            batch_param_args(NAMES, B, "L", bad)
        vals = np.full(B, 0.2)
        vals[4] = bad
        with pytest.raises(ValueError, match=r"finite.*problem 4"):
            batch_param_args(NAMES, B, "L", vals)
    with pytest.raises(ValueError, match="finite"):
        batch_param_args(NAMES, B, "L", 1e39)                                           # overflows fp32, which is what the table holds
    with pytest.raises(ValueError, match="number"):
        batch_param_args(NAMES, B, "L", "long")


def test_batch_methods_exist():
    from control_toolkit_amd._capi import CtkMppiBatch
    for m in ("set_problem_params", "get_problem_param", "get_problem_params", "params_differ"):
        assert callable(getattr(CtkMppiBatch, m))
