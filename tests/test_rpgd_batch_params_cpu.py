"""CPU tests (-m "not gpu") of the per-problem parameters of an RPGD batch (include/ctk_hip.h: ctk_rpgd_problem_set_param /
ctk_rpgd_problem_get_param / ctk_rpgd_problem_params_differ; control_toolkit_amd._capi: CtkRpgdBatch.set_problem_params): the symbols are
declared and bound with their argument types under names that leave the ctk_rpgd_batch_* family as it was, and the library refuses NULL
batches without a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
NEW = ("ctk_rpgd_problem_get_param", "ctk_rpgd_problem_params_differ", "ctk_rpgd_problem_set_param")


def test_new_symbols_are_declared_and_bound_with_argument_types():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ctk_rpgd_problem_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(NEW)                                                      # exactly the three
    lib = load_library()
    for n in NEW:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
        assert res is ctypes.c_int
    assert [len(SYMBOLS[n][1]) for n in NEW] == [4, 1, 5]
    # the CEM and MPPI trios' argument types, one for one
    for n in NEW:
        assert SYMBOLS[n] == SYMBOLS[n.replace("ctk_rpgd_problem_", "ctk_cem_problem_")] == SYMBOLS[n.replace("ctk_rpgd_problem_", "ctk_problem_")], n
    assert lib.ctk_abi_version() == 6                       # additive: the ABI version stays


def test_library_refuses_null_batches():
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    v = ctypes.c_float(1.0)
    assert lib.ctk_rpgd_problem_set_param(None, 0, None, 0, ctypes.byref(v)) == 1
    assert lib.ctk_rpgd_problem_get_param(None, 0, 0, ctypes.byref(v)) == 1 and v.value == 1.0
    assert lib.ctk_rpgd_problem_params_differ(None) == 0


def test_batch_methods_exist():
    from control_toolkit_amd._capi import CtkCemBatch, CtkRpgdBatch
    for m in ("set_problem_params", "get_problem_param", "get_problem_params", "params_differ"):
        assert callable(getattr(CtkRpgdBatch, m))
        assert getattr(CtkRpgdBatch, m).__doc__ == getattr(CtkCemBatch, m).__doc__, m      # the CEM batch's wording
