"""CPU tests (-m "not gpu") of the per-problem hyper-parameters and input limits of the CEM and RPGD batches
(include/ctk_hip_family_hyper.h, FamilyHypers(batch)): the header against the Python tables and the library's exports, the pure argument
checker, the way in (the view's constructor and nothing else), and the guard that keeps tests/test_gpu_family_hypers.py from being
vacuous — every case of family_hyper_cases moves the tensor it shows in by more than the bound the suite's GPU tests compare that tensor
with (tests/test_gpu_hyper.py, restated below because importing a GPU test module here would load the device helpers), so a kernel that
used the defaults could not equal the handle created with the case."""
import os
import re
import subprocess

import numpy as np
import pytest

from control_toolkit_amd import _capi
from control_toolkit_amd._capi import CEM_HYPERS, FAMILY_HYPER_SYMBOLS, RPGD_HYPERS, FamilyHypers, family_hyper_args
import family_hyper_cases as Fc
import hyper_cases as Hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
FAMILY_HEADER = os.path.join(ROOT, "include", "ctk_hip_family_hyper.h")
FAMILIES = (("ctk_cem_batch", "ctk_cem_problem"), ("ctk_rpgd_batch", "ctk_rpgd_problem"))
CEM_TOL = dict(rtol=1e-4, atol=1e-5)            # test_gpu_hyper.CEM_TOL: U_NOM and STD
PLAN_TOL = dict(rtol=2e-5, atol=2e-5)           # the template kernels' plans (test_gpu_hyper.check_rpgd, tuned = False)


# ---- the header -----------------------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(FAMILY_HEADER).read(), flags=re.S)


def test_header_declares_the_twelve_entries_and_the_library_exports_them():
    declared = sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", header_text())))
    want = sorted([f"{prob}_{e}" for _, prob in FAMILIES for e in ("set_hyper", "get_hyper", "set_limits", "get_limits", "hypers_differ")] +
                  [f"{fam}_set_hyper" for fam, _ in FAMILIES])
    assert len(want) == 12 and declared == want
    assert sorted(FAMILY_HYPER_SYMBOLS) == want                                    # the ctypes table binds exactly these
    assert len(re.findall(r'^#include "ctk_hip_family_hyper.h"', open(HEADER).read(), flags=re.M)) == 1   # a caller includes one header
    lib = _capi.load_library()
    for name in want:
        assert hasattr(lib, name), f"libctk_hip.so does not export {name}"
    assert lib.ctk_abi_version() == 6
    assert not (set(want) & (set(_capi.SYMBOLS) | set(_capi.HYPER_SYMBOLS)))       # the other headers' lists stay what they were


def test_header_compiles_as_c(tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cc is not None, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "ctk_hip.h"\nint use(ctk_cem_batch* b, ctk_rpgd_batch* r) {\n'
                   "    float v = 2.0f, lo = -1.0f, hi = 1.0f;\n"
                   "    return ctk_cem_problem_set_hyper(b, 0, 0, CTK_CEM_HYPER_BEST_K, &v) + ctk_cem_batch_set_hyper(b, CTK_CEM_HYPER_OUTER_IT, v) +\n"
                   "           ctk_rpgd_problem_set_limits(r, 0, 0, &lo, &hi) + ctk_rpgd_problem_hypers_differ(r) + CTK_RPGD_HYPER_COUNT;\n}\n")
    done = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def enum_of(name, prefix):
    body = re.search(r"enum %s\s*\{(.*?)\}" % name, header_text(), flags=re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(prefix + r"([A-Z_0-9]+)\s*=\s*(\d+)", body)}


def test_enums_match_the_python_tables():
    cem, rpgd = enum_of("ctk_cem_hyper", "CTK_CEM_HYPER_"), enum_of("ctk_rpgd_hyper", "CTK_RPGD_HYPER_")
    assert cem.pop("COUNT") == len(CEM_HYPERS) == 4 and rpgd.pop("COUNT") == len(RPGD_HYPERS) == 11
    assert cem == {k[4:].upper(): v for k, v in CEM_HYPERS.items()}                 # cem_best_k -> BEST_K
    assert rpgd == {k.upper(): v for k, v in RPGD_HYPERS.items()}
    assert set(CEM_HYPERS) == set(Fc.CEM_NAMES)
    assert tuple(RPGD_HYPERS) == Fc.RPGD_NAMES
    import control_toolkit_amd
    for name in ("CEM_HYPERS", "RPGD_HYPERS", "FAMILY_HYPER_SYMBOLS", "FamilyHypers", "family_hyper_args"):
        assert getattr(control_toolkit_amd, name) is getattr(_capi, name) and name in control_toolkit_amd.__all__


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------
def test_checker_accepts_scalars_and_one_value_per_listed_problem():
    hid, idv, n, vals = family_hyper_args("cem", 4, "cem_best_k", 8, num_rollouts=64)
    assert (hid, idv, n) == (CEM_HYPERS["cem_best_k"], None, 4) and vals.dtype == np.float32 and vals.tolist() == [8.0] * 4
    hid, idv, n, vals = family_hyper_args("rpgd", 4, "learning_rate", [0.2, 0.01], ids=[1, 3])
    assert hid == RPGD_HYPERS["learning_rate"] and idv.tolist() == [1, 3] and idv.dtype == np.int32 and n == 2 and vals.tolist() == [np.float32(0.2), np.float32(0.01)]
    for name in CEM_HYPERS:
        assert family_hyper_args("cem", 2, name, 1.0)[0] == CEM_HYPERS[name]
    for name in RPGD_HYPERS:
        assert family_hyper_args("rpgd", 2, name, 1.0)[0] == RPGD_HYPERS[name]
    assert family_hyper_args("rpgd", 2, "outer_its", 0)[3].tolist() == [0.0, 0.0]            # outer_its may be 0, as at creation
    assert family_hyper_args("cem", 2, "cem_stdev_min", -1.0)[3].tolist() == [-1.0, -1.0]    # creation has no rule for the deviations
    assert family_hyper_args("cem", 1, "cem_best_k", 64.0, num_rollouts=64)[3].tolist() == [64.0]


def test_checker_accepts_limits_as_scalars_rows_and_tables():
    hid, idv, n, (lo, hi) = family_hyper_args("cem", 3, "limits", (-0.2, 0.4), Cn=2)
    assert hid is None and idv is None and n == 3 and lo.shape == hi.shape == (3, 2) and lo.dtype == np.float32
    _, _, _, (lo, hi) = family_hyper_args("rpgd", 3, "limits", ([-0.2, -0.3], [0.35, 0.15]), Cn=2)
    assert lo.tolist() == [[np.float32(-0.2), np.float32(-0.3)]] * 3 and hi[2].tolist() == [np.float32(0.35), np.float32(0.15)]
    _, idv, n, (lo, hi) = family_hyper_args("cem", 3, "limits", ([[-1.0], [0.0]], 0.5), ids=[0, 2], Cn=1)
    assert idv.tolist() == [0, 2] and n == 2 and lo.tolist() == [[-1.0], [0.0]] and hi.tolist() == [[0.5], [0.5]]


@pytest.mark.parametrize("args,kw,text", [
    (("mppi", 4, "LBD", 1.0), {}, "family is 'cem' or 'rpgd'"),
    (("cem", 4, "learning_rate", 1.0), {}, "unknown hyper-parameter 'learning_rate'"),       # the other family's
    (("rpgd", 4, "cem_best_k", 1.0), {}, "unknown hyper-parameter"),
    (("rpgd", 4, "shift_previous", 1.0), {}, "unknown hyper-parameter"),                     # shared: it changes the launch structure
    (("rpgd", 4, "opt_keep_k", 4), {}, "unknown hyper-parameter"),
    (("cem", 4, "warmup_iterations", 4), {}, "unknown hyper-parameter"),
    (("cem", 4, "target_position", 1.0), {}, "unknown hyper-parameter"),                     # an environment parameter is not a hyper-parameter
    (("cem", 4, "cem_stdev_min", [1.0, 2.0]), {}, r"one value per listed problem \(4\)"),
    (("cem", 4, "cem_stdev_min", [1.0, 2.0, 3.0]), {"ids": [0, 2]}, r"one value per listed problem \(2\)"),
    (("cem", 4, "cem_stdev_min", "much"), {}, "must be a number"),
    (("cem", 4, "cem_stdev_min", 1.0), {"ids": [0, 4]}, r"ids must lie in 0 \.\. 3"),
    (("cem", 4, "cem_stdev_min", 1.0), {"ids": [2, 1]}, "strictly ascending"),
    (("rpgd", 4, "adam_beta_1", [0.9, float("nan"), 0.9, 0.9]), {}, "finite in fp32.*problem 1"),
    (("rpgd", 4, "gradmax_clip", [1.0, float("inf")]), {"ids": [0, 3]}, "finite in fp32.*problem 3"),
    (("rpgd", 4, "sample_mean", 1e39), {}, "finite in fp32.*problem 0"),
    (("cem", 4, "cem_best_k", [2, 2, 2.5, 2]), {}, "'cem_best_k' must be integral.*problem 2"),
    (("cem", 4, "cem_best_k", 0), {}, "'cem_best_k' must be >= 1.*problem 0"),
    (("cem", 4, "cem_best_k", [8, 65]), {"ids": [1, 3], "num_rollouts": 64}, r"'cem_best_k' must be <= num_rollouts \(64\).*problem 3"),
    (("cem", 4, "cem_outer_it", 0), {}, "'cem_outer_it' must be >= 1"),
    (("cem", 4, "cem_outer_it", 1.5), {}, "'cem_outer_it' must be integral"),
    (("rpgd", 4, "outer_its", -1), {}, "'outer_its' must be >= 0"),
    (("rpgd", 4, "outer_its", 0.25), {}, "'outer_its' must be integral"),
    (("rpgd", 4, "resamp_per", 0), {}, "'resamp_per' must be >= 1"),
    (("rpgd", 4, "resamp_per", [1, 2.5]), {"ids": [0, 2]}, "'resamp_per' must be integral.*problem 2"),
    (("cem", 4, "limits", 1.0), {}, r"pair \(low, high\)"),
    (("cem", 4, "limits", ([0.0, 0.0], 1.0)), {"Cn": 1}, "low must be a scalar"),
    (("rpgd", 4, "limits", (0.0, float("nan"))), {}, "high must be finite in fp32.*problem 0, input 0"),
    (("rpgd", 4, "limits", ([[0.0, 0.2], [0.0, 0.6]], 0.5)), {"ids": [1, 2], "Cn": 2}, "low must be <= high.*problem 2, input 1"),
    (("cem", 4, "limits", (0.0, 1.0)), {"ids": [7]}, "ids must lie in"),
])
def test_checker_refuses(args, kw, text):
    with pytest.raises(ValueError, match=text):
        family_hyper_args(*args, **kw)


# ---- the way in -------------------------------------------------------------------------------------------------------------------------------
class FakeLib:
    """records the entry a call asks the library for"""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        self.asked.append(name)
        return lambda *a: 0


@pytest.mark.parametrize("cls,family,prefixes", [(_capi.CtkCemBatch, "cem", FAMILIES[0]), (_capi.CtkRpgdBatch, "rpgd", FAMILIES[1])])
def test_the_view_forwards_to_its_family(cls, family, prefixes):
    b = cls.__new__(cls)                                            # no device: the forwarding needs no handle
    b._lib, b._h, b.B, b.C, b.N = FakeLib(), None, 3, 1, 64
    b._check = lambda rc: None
    view = FamilyHypers(b)
    assert view.family == family and view.names is (CEM_HYPERS if family == "cem" else RPGD_HYPERS)
    name = "cem_best_k" if family == "cem" else "resamp_per"
    view.set_problem_hypers(name, [2, 3], ids=[0, 2])
    view.set_hyper(name, 4)
    view.get_problem_hyper(name, 1)
    view.set_problem_limits(-0.5, 0.5)
    view.get_problem_limits(2)
    view.hypers_differ()
    batch, prob = prefixes
    assert b._lib.asked == [f"{prob}_set_hyper", f"{batch}_set_hyper", f"{prob}_get_hyper", f"{prob}_set_limits", f"{prob}_get_limits", f"{prob}_hypers_differ"]
    with pytest.raises(ValueError, match="unknown hyper-parameter"):
        view.set_problem_hypers("LBD", 1.0)
    with pytest.raises(ValueError, match="unknown hyper-parameter"):
        view.get_problem_hyper("LBD", 0)
    assert FamilyHypers.CALLS == _capi.BatchHypers.CALLS and all(callable(getattr(FamilyHypers, n)) for n in FamilyHypers.CALLS)


def test_the_constructor_is_the_only_way_in():
    for cls in (_capi.CtkCemBatch, _capi.CtkRpgdBatch):
        assert not hasattr(cls, "hypers")
        b = cls.__new__(cls)
        assert not any(hasattr(b, n) for n in FamilyHypers.CALLS), cls.__name__
    for cls in (_capi.CtkMppiBatch, _capi.CtkMppiMlpBatch, _capi.CtkMppiGruBatch, _capi.CtkEngine):
        with pytest.raises(TypeError, match="CtkCemBatch or a CtkRpgdBatch"):
            FamilyHypers(cls.__new__(cls))
    with pytest.raises(TypeError):
        FamilyHypers(None)
    assert "FamilyHypers(batch)" in _capi.BatchHypers.__doc__ and "have no such view" not in _capi.BatchHypers.__doc__


# ---- the guard against a vacuous GPU test ------------------------------------------------------------------------------------------------------
def outside(case, base, rtol, atol):
    a, b = np.asarray(case, np.float64), np.asarray(base, np.float64)
    return np.abs(a - b) > atol + rtol * np.abs(b)


@pytest.mark.parametrize("size", Hc.CEM_SIZES, ids=lambda s: "N%d-H%d" % s)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_cem_case_moves_std_by_more_than_the_gpu_bound(env, size):
    """problem 0 of the GPU test's batch keeps the defaults, problem j gets a case: with the same state and draws the float32 oracle's STD
    after the step (U_NOM as well for the limits, whose middle refills its tail) is outside the GPU bound around the defaults' on more than
    half of the elements — this test's reading of "moves by more than the bound", as test_batch_hypers_cpu.py's"""
    N, H = size
    base = Hc.cem_ref(env, (), N, H)
    cases = Fc.cem_cases(N)
    assert [own for own in cases if len(own) == 1 and own[0][0] == "cem_best_k"] == [(("cem_best_k", k),) for k in (2, 32, 64, N)]
    assert {own[0][1] for own in cases if own[0][0] == "cem_outer_it"} == {1, 4} and all(c in cases for c in Hc.CEM_CASES)
    for own in cases:
        case = Hc.cem_ref(env, own, N, H)
        np.testing.assert_array_equal(case["s"], base["s"])
        share = outside(case["std"], base["std"], **CEM_TOL).mean()
        print(f"{env} N{N} {Hc.cem_id(own)}: STD outside the bound on {share:.2f} of the elements, largest difference {np.abs(case['std'] - base['std']).max():.3g}")
        assert share > 0.5, f"{env} N{N} {Hc.cem_id(own)}: STD differs from the defaults' by more than the bound on {share:.2f} of the elements only"
    assert all(dict(own).get("cem_best_k", 1) <= N for own in cases)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_every_rpgd_case_moves_its_tensor_by_more_than_the_gpu_bound(env):
    """the same for RPGD: the tensor family_hyper_cases.rpgd_shows_in names (the reset's population for the sampling range and the limits,
    the descended plans or a moment after the second step, the warm-started population where the resampling period differs), between the
    oracle's run of the batch's defaults and of the case; the moments at the bounds test_gpu_hyper.check_rpgd holds them to"""
    names = set()
    for own in Fc.RPGD_CASES:
        far = Fc.rpgd_far(own)
        base, case = Fc.rpgd_run(env, (), far), Fc.rpgd_run(env, own, far)
        np.testing.assert_array_equal(case["s"], base["s"])
        np.testing.assert_array_equal(case["reset_draws"], base["reset_draws"])
        t, tensor = Fc.rpgd_shows_in(own)
        a, b = (case[tensor], base[tensor]) if t < 0 else (case["steps"][t][tensor], base["steps"][t][tensor])
        tol = (dict(rtol=2e-3, atol=2e-4 * float(np.abs(b).max())) if tensor == "m" else dict(rtol=4e-3, atol=4e-4 * float(np.abs(b).max())) if tensor == "v"
               else PLAN_TOL)
        share = outside(a, b, **tol).mean()
        print(f"{env} {Hc.rpgd_id(own)}: {tensor} of step {t} outside the bound on {share:.2f} of the elements")
        assert share > 0.5, f"{env} {Hc.rpgd_id(own)}: {tensor} of step {t} differs from the defaults' by more than the bound on {share:.2f} of the elements only"
        names.update(k for k, _ in own)
    assert {("outer_its", 0), ("outer_its", 5), ("resamp_per", 1), ("resamp_per", 3), ("uniform_dist_min", -0.4), ("uniform_dist_max", 0.7)} <= {o[0] for o in Fc.RPGD_CASES}
    # the two names no case moves are read only by the NORMAL sampling map, which is shared: test_gpu_family_hypers.py gives them a batch of their own
    assert set(Fc.RPGD_NAMES) - names == {"sample_stdev", "sample_mean"}
