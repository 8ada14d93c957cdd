"""CPU tests (-m "not gpu") of the closed loops of the CEM and RPGD batches on the device (BatchClosedLoop(cem_batch) /
BatchClosedLoop(rpgd_batch); include/ctk_hip_loop.h: the ctk_cem_batch_ and ctk_rpgd_batch_ forms of ctk_batch_run, ctk_batch_episodes
and the plant and noise entries): every new entry point is declared, bound with the argument types of the ctk_batch_ form and exported;
the header compiles as C; the Python side checks its arguments BEFORE the library is touched, with the messages of the MPPI batches;
the classes keep their method sets; and the counter rules of a segment's step records, restated on the host in family_loop_cases.py,
give the hand-written sequences below."""
import os
import re
import subprocess

import numpy as np
import pytest

import family_loop_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip_loop.h")
FAMILIES = ("ctk_cem_batch", "ctk_rpgd_batch")


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", src)))


# ---- 1. symbols and headers ---------------------------------------------------------------------------------------------------------------
def test_every_new_symbol_is_declared_bound_and_exported():
    from control_toolkit_amd._capi import load_library, EPISODE_SYMBOLS, LOOP_SYMBOLS, RUN_SYMBOLS, SYMBOLS
    want = sorted(f"{fam}_{e}" for fam in FAMILIES for e in F.ENTRIES)
    assert len(F.ENTRIES) == len(set(F.ENTRIES)) == 14 and len(want) == 28
    assert declared(HEADER) == want == sorted(LOOP_SYMBOLS)
    assert not set(LOOP_SYMBOLS) & (set(SYMBOLS) | set(RUN_SYMBOLS) | set(EPISODE_SYMBOLS))
    text = open(os.path.join(ROOT, "include", "ctk_hip.h")).read()
    assert len(re.findall(r'^#include "ctk_hip_loop.h"', text, flags=re.M)) == 1
    src = open(HEADER).read()
    for fam in FAMILIES:                                     # each declaration cites the entry it mirrors
        for e in F.ENTRIES:
            assert re.search(rf"\b{fam}_{e}\([^;]*;\s*/\*\s*ctk_batch_{e}\s*\*/", src, flags=re.S), f"{fam}_{e} does not cite ctk_batch_{e}"
    lib = load_library()
    assert lib.ctk_abi_version() == 6                        # additive
    mppi = dict(RUN_SYMBOLS, **EPISODE_SYMBOLS)
    for fam in FAMILIES:
        for e in F.ENTRIES:
            res, args = LOOP_SYMBOLS[f"{fam}_{e}"]
            fn = getattr(lib, f"{fam}_{e}")                  # AttributeError: not exported
            assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, (fam, e)
            want_res, want_args = mppi[f"ctk_batch_{e}"]
            assert res == want_res and list(args[1:]) == list(want_args[1:]) and len(args) == len(want_args), (fam, e)
    # NULL handles answer like the other entries'
    for fam in FAMILIES:
        f = lambda e: getattr(lib, f"{fam}_{e}")                                            # noqa: E731
        assert f("run")(None, 0, None, None, None, 1, 0, None, None, None) == 1
        assert f("episodes")(None, 0, None, None, None, None, 1, 0, None, None, None, None, None) == 1
        assert f("plant_step")(None, 0, None, None, None, 0, None) == 1
        assert f("plant_step_noisy")(None, 0, None, None, None, None, 0, None, None, None) == 1
        assert f("plant_set_param")(None, 0, None, 0, None) == 1 and f("plant_get_param")(None, 0, 0, None) == 1
        assert f("plant_clear_params")(None) == 1
        assert f("plant_set_noise")(None, 0, None, 0, None) == 1 and f("plant_get_noise")(None, 0, 0, None) == 1
        assert f("plant_clear_noise")(None) == 1 and f("plant_set_noise_seed")(None, 0, None, None) == 1
        assert f("plant_get_noise_seed")(None, 0, None) == 1 and f("plant_noise_get_position")(None, 0, None) == 1
        assert f("plant_noise_set_position")(None, 0, 0) == 1


def test_the_header_compiles_as_c(tmp_path):
    for first in ("ctk_hip.h", "ctk_hip_loop.h"):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\nint main(void) {{ return ctk_cem_batch_run(0, 0, 0, 0, 0, 1, 0, 0, 0, 0) + ctk_rpgd_batch_plant_clear_noise(0) + '
                     'ctk_rpgd_batch_episodes(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0) > 99; }\n')
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")], check=True)


# ---- 2. the Python side -------------------------------------------------------------------------------------------------------------------
def test_the_constructor_is_the_way_in_and_the_classes_keep_their_methods():
    from control_toolkit_amd._capi import BatchClosedLoop, CtkCemBatch, CtkRpgdBatch
    assert not hasattr(CtkCemBatch, "closed_loop") and not hasattr(CtkRpgdBatch, "closed_loop")
    for cls in (CtkCemBatch, CtkRpgdBatch):
        assert not [m for m in ("run", "episodes", "plant_step", "plant_step_noisy", "set_noise") if hasattr(cls, m)]
    assert CtkCemBatch._BATCH == "ctk_cem_batch" and CtkRpgdBatch._BATCH == "ctk_rpgd_batch"
    assert "BatchClosedLoop(cem_batch)" in BatchClosedLoop.__doc__ and "BatchClosedLoop(rpgd_batch)" in BatchClosedLoop.__doc__
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "BatchClosedLoop(cem_batch)" in text and "BatchClosedLoop(rpgd_batch)" in text and "ctk_hip_loop.h" in text


@pytest.mark.parametrize("prefix", FAMILIES)
def test_arguments_are_checked_before_the_library_is_touched(prefix):
    from control_toolkit_amd._capi import BatchClosedLoop

    class NoLibrary:                                          # stands in for a batch: any touch of the library or a buffer raises
        B, S, C = 3, 4, 1
        _BATCH = prefix
        param_names = ("g", "m_cart", "m_pole")

        def __getattr__(self, name):
            raise AssertionError(f"the batch's {name} was touched before the arguments were checked")

    loop = BatchClosedLoop(NoLibrary())
    S0, U = np.zeros((3, 4), np.float32), np.zeros((3, 1), np.float32)
    for call in (lambda s, n, **kw: loop.run(s, n, **kw), lambda s, n, **kw: loop.episodes(s, n, **kw)):
        for bad in (np.zeros((3, 5)), np.zeros((2, 4)), np.zeros(4), np.zeros((3, 4, 1))):
            with pytest.raises(ValueError, match=r"states must have shape \(3, 4\)"):
                call(bad, 6)
        with pytest.raises(ValueError, match=r"states must have shape \(2, 4\)"):
            call(S0, 6, ids=[0, 2])
        with pytest.raises(ValueError, match=r"u_prev must have shape \(3, 1\)"):
            call(S0, 6, u_prev=np.zeros((3, 2)))
        for bad in ([3], [-1, 0], [0, 3]):
            with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
                call(S0[:len(bad)], 6, ids=bad)
        with pytest.raises(ValueError, match="strictly ascending"):
            call(S0[:2], 6, ids=[1, 0])
        for bad in (0, -1, 2.5, None, True):
            with pytest.raises(ValueError, match="at least one step"):
                call(S0, bad)
        for bad in (0, -2, 1.5, False):
            with pytest.raises(ValueError, match="plant_substeps must be an integer >= 1 or None"):
                call(S0, 6, plant_substeps=bad)
    for samples in (np.zeros((3, 70, 3, 1), np.float32), 0x7F0000001000):
        with pytest.raises(NotImplementedError, match="device Philox only"):
            loop.run(S0, 6, samples=samples)
    with pytest.raises(ValueError, match=r"Y0 must have shape \(3, 4\)"):
        loop.episodes(S0, 6, Y0=np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"S must have shape \(3, 4\)"):
        loop.plant_step(np.zeros((3, 3)), U)
    with pytest.raises(ValueError, match=r"U must have shape \(3, 1\)"):
        loop.plant_step(S0, None)
    with pytest.raises(ValueError, match=r"U_prev must have shape \(3, 1\)"):
        loop.plant_step_noisy(S0, U, None)
    with pytest.raises(ValueError, match="unknown parameter 'mass'"):
        loop.set_plant_params("mass", 1.0)
    with pytest.raises(ValueError, match="one value per listed problem"):
        loop.set_plant_params("m_pole", [0.1, 0.2])
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="process noise: a standard deviation is finite and >= 0"):
            loop.set_noise(process=bad)
    with pytest.raises(ValueError, match="seeds must have one entry per listed problem"):
        loop.set_noise_seeds(None)


# ---- 3. the cases and the counter rules ---------------------------------------------------------------------------------------------------
def test_cases_are_what_the_issue_names():
    K = F.K
    assert F.CEM_CASES == ("one_workgroup", "quad2d", "hover")
    assert F.RPGD_CASES == ("cartpole_small", "cartpole_partial", "cartpole_full_wave", "quad2d", "hover")
    assert (K.B, K.B_SPLIT, K.STEPS, K.STEPS_SEGMENTS, K.SPLIT_PER_LAUNCH, K.SEGMENT_STEPS) == (3, 5, 6, 10, 2, 4)
    want = {"one_workgroup": ("CartPole", 64, 8, 8, 2), "quad2d": ("Quad2D", 128, 20, 20, 2), "hover": ("Hover", 96, 16, 12, 2)}
    for case in F.CEM_CASES:
        kw = F.batch_kwargs("cem", case)
        assert (kw["environment"], kw["num_rollouts"], kw["mpc_horizon"], kw["cem_best_k"], kw["cem_outer_it"]) == want[case]
        assert kw["environment"] == F.environment("cem", case) and kw["dt"] == K.DT
        assert (kw.get("warmup"), kw.get("warmup_iterations")) == ((True, 3) if case == "one_workgroup" else (None, None))
    kw = F.batch_kwargs("rpgd", "cartpole_small")
    assert (kw["num_rollouts"], kw["mpc_horizon"], kw["period_interpolation_inducing_points"], kw["opt_keep_k"], kw["outer_its"], kw["resamp_per"],
            kw["warmup"], kw["warmup_iterations"]) == (16, 12, 5, 4, 2, 2, True, 3)
    kw = F.batch_kwargs("rpgd", "cartpole_partial")
    assert (kw["resamp_per"], kw["shift_previous"]) == (1, 2)
    assert F.batch_kwargs("rpgd", "cartpole_full_wave")["resamp_per"] == 3
    for case in F.RPGD_CASES:
        kw = F.batch_kwargs("rpgd", case)
        assert kw["environment"] == F.environment("rpgd", case) and kw["dt"] == K.DT
        assert -(-K.STEPS // kw["resamp_per"]) >= 2          # a run of 6 steps resamples at least twice


def test_cem_counters_over_six_steps():
    rule = dict(warmup=True, warmup_iterations=3, cem_outer_it=2)
    # a fresh problem: the warm-up step, then cem_outer_it; the tags are consecutive from 1
    assert F.cem_counters(0, 1, 6, **rule) == ([(3, 1), (2, 4), (2, 6), (2, 8), (2, 10), (2, 12)], 14)
    # a problem that has stepped: no warm-up
    assert F.cem_counters(4, 11, 6, **rule) == ([(2, 11), (2, 13), (2, 15), (2, 17), (2, 19), (2, 21)], 23)
    # without cfg.warmup the first step is an ordinary one
    assert F.cem_counters(0, 1, 6, warmup=False, warmup_iterations=3, cem_outer_it=2)[0][0] == (2, 1)
    # one wrap: the step whose tags would pass 2^32 restarts at 1 (tag 0 is never used), applied in order, step by step
    top = 2 ** 32
    got, after = F.cem_counters(0, top - 6, 6, **rule)
    assert got == [(3, top - 6), (2, top - 3), (2, 1), (2, 3), (2, 5), (2, 7)] and after == 9
    got, after = F.cem_counters(7, top - 2, 6, **rule)      # a step that would end exactly at 2^32 restarts too: its sum is 0
    assert got == [(2, 1), (2, 3), (2, 5), (2, 7), (2, 9), (2, 11)] and after == 13
    assert all(tag != 0 for _, tag in got)


def test_rpgd_counters_over_six_steps():
    rule = dict(warmup=True, warmup_iterations=3, outer_its=2)
    # (iters, t0, resample): the first step after a reset runs the warm-up count; t0 sums the earlier steps' iterations
    assert F.rpgd_counters(0, 0, 6, resamp_per=2, **rule) == [(3, 0, 1), (2, 3, 0), (2, 5, 1), (2, 7, 0), (2, 9, 1), (2, 11, 0)]
    assert F.rpgd_counters(0, 0, 6, resamp_per=3, **rule) == [(3, 0, 1), (2, 3, 0), (2, 5, 0), (2, 7, 1), (2, 9, 0), (2, 11, 0)]
    assert F.rpgd_counters(0, 0, 6, resamp_per=1, **rule) == [(3, 0, 1), (2, 3, 1), (2, 5, 1), (2, 7, 1), (2, 9, 1), (2, 11, 1)]
    # a problem that has stepped 3 times (7 Adam iterations): no warm-up, the resampling phase continues
    assert F.rpgd_counters(3, 7, 6, resamp_per=2, **rule) == [(2, 7, 0), (2, 9, 1), (2, 11, 0), (2, 13, 1), (2, 15, 0), (2, 17, 1)]
    # without cfg.warmup the first step runs outer_its
    assert F.rpgd_counters(0, 0, 2, resamp_per=2, warmup=False, warmup_iterations=3, outer_its=2) == [(2, 0, 1), (2, 2, 0)]
