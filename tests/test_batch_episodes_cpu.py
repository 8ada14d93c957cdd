"""CPU tests (-m "not gpu") of the stochastic closed loop on the device (BatchClosedLoop.episodes / plant_step_noisy / the noise settings;
include/ctk_hip_episode.h: ctk_batch_plant_*noise*, ctk_batch_plant_step_noisy, ctk_batch_episodes and the ctk_mlp_batch_ forms): every
new entry point is declared, bound with argument types and exported; the Python side checks shapes, ids, counts and sigma values BEFORE
the library is touched; guards on the inputs and references of test_gpu_batch_episodes.py, and the two bounds that are measured here
(batch_episode_cases.py: DRAW_BOUND, COST_ATOL).  That the float32 oracle's TRANSITION uses at most a tenth of TRAJ_TOL on these start
states is shown by test_batch_run_cpu.py::test_the_oracle_step_uses_a_small_part_of_the_bound and not repeated."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_episode_cases as E
import batch_run_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip_episode.h")
ENTRIES = ["plant_set_noise", "plant_get_noise", "plant_clear_noise", "plant_set_noise_seed", "plant_get_noise_seed", "plant_noise_get_position",
           "plant_noise_set_position", "plant_step_noisy", "episodes"]
METHODS = ["set_noise", "get_noise", "clear_noise", "set_noise_seeds", "get_noise_seeds", "noise_position", "set_noise_position",
           "plant_step_noisy", "episodes"]


def declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", src)))


# ---- 1. symbols and headers ---------------------------------------------------------------------------------------------------------------
def test_every_new_symbol_is_declared_bound_and_exported():
    from control_toolkit_amd._capi import load_library, EPISODE_SYMBOLS, RUN_SYMBOLS, SYMBOLS
    want = sorted(f"{fam}_{e}" for fam in ("ctk_batch", "ctk_mlp_batch") for e in ENTRIES)
    assert declared(HEADER) == want == sorted(EPISODE_SYMBOLS)
    assert not set(EPISODE_SYMBOLS) & (set(SYMBOLS) | set(RUN_SYMBOLS))
    text = open(os.path.join(ROOT, "include", "ctk_hip.h")).read()
    assert len(re.findall(r'^#include "ctk_hip_episode.h"', text, flags=re.M)) == 1
    src = open(HEADER).read()
    for n in want:                                           # each declaration cites what it replaces
        assert re.search(rf"\b{n}\([^;]*;\s*/\*[^\n]*(replaces:|ctk_batch_)", src, flags=re.S), f"{n} does not cite what it replaces"
    lib = load_library()
    assert lib.ctk_abi_version() == 6
    for n in want:
        res, args = EPISODE_SYMBOLS[n]
        fn = getattr(lib, n)                                 # AttributeError: not exported
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
    for e in ENTRIES:                                        # the MLP family forwards under its own names, same signatures
        assert EPISODE_SYMBOLS["ctk_mlp_batch_" + e] == EPISODE_SYMBOLS["ctk_batch_" + e]
    assert len(EPISODE_SYMBOLS["ctk_batch_episodes"][1]) == 13 and len(EPISODE_SYMBOLS["ctk_batch_plant_step_noisy"][1]) == 10
    # NULL handles answer like the other entries'
    for fam in ("ctk_batch", "ctk_mlp_batch"):
        f = lambda e: getattr(lib, f"{fam}_{e}")                                            # noqa: E731
        assert f("episodes")(None, 0, None, None, None, None, 1, 0, None, None, None, None, None) == 1
        assert f("plant_step_noisy")(None, 0, None, None, None, None, 0, None, None, None) == 1
        assert f("plant_set_noise")(None, 0, None, 0, None) == 1 and f("plant_get_noise")(None, 0, 0, None) == 1
        assert f("plant_clear_noise")(None) == 1 and f("plant_set_noise_seed")(None, 0, None, None) == 1
        assert f("plant_get_noise_seed")(None, 0, None) == 1 and f("plant_noise_get_position")(None, 0, None) == 1
        assert f("plant_noise_set_position")(None, 0, 0) == 1


def test_the_header_compiles_as_c(tmp_path):
    for first in ("ctk_hip.h", "ctk_hip_episode.h"):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\nint main(void) {{ return ctk_batch_episodes(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0) + '
                     'ctk_mlp_batch_plant_clear_noise(0) + ctk_batch_run(0, 0, 0, 0, 0, 1, 0, 0, 0, 0) > 99; }\n')
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")], check=True)


def test_the_class_has_the_methods_and_the_package_the_tuple():
    import control_toolkit_amd
    from control_toolkit_amd._capi import BatchClosedLoop, Episodes
    assert control_toolkit_amd.Episodes is Episodes and "Episodes" in control_toolkit_amd.__all__
    assert Episodes._fields == ("states", "observations", "inputs", "costs")
    for m in METHODS:
        assert callable(getattr(BatchClosedLoop, m)), m


# ---- 2. argument checks -------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched():
    from control_toolkit_amd._capi import BatchClosedLoop, batch_episode_args, batch_noise_args

    class NoLibrary:                                          # stands in for a batch: any touch of the library or a buffer raises
        B, S, C = 3, 4, 1
        param_names = ("g", "m_cart", "m_pole")

        def __getattr__(self, name):
            raise AssertionError(f"the batch's {name} was touched before the arguments were checked")

    loop = BatchClosedLoop(NoLibrary())
    S0, U = np.zeros((3, 4), np.float32), np.zeros((3, 1), np.float32)
    for bad in (np.zeros((3, 5)), np.zeros((2, 4)), np.zeros(4), np.zeros((3, 4, 1))):
        with pytest.raises(ValueError, match=r"states must have shape \(3, 4\)"):
            loop.episodes(bad, 6)
        with pytest.raises(ValueError, match=r"Y0 must have shape \(3, 4\)"):
            loop.episodes(S0, 6, Y0=bad)
    with pytest.raises(ValueError, match=r"Y0 must have shape \(2, 4\)"):
        loop.episodes(S0[:2], 6, ids=[0, 2], Y0=S0)
    with pytest.raises(ValueError, match=r"u_prev must have shape \(3, 1\)"):
        loop.episodes(S0, 6, u_prev=np.zeros((3, 2)))
    for bad in ([3], [-1, 0], [0, 3]):
        with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
            loop.episodes(S0[:len(bad)], 6, ids=bad)
        with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
            loop.set_noise(process=0.1, ids=bad)
        with pytest.raises(ValueError, match="ids must lie in 0 .. 2"):
            loop.set_noise_seeds([1] * len(bad), ids=bad)
    with pytest.raises(ValueError, match="strictly ascending"):
        loop.episodes(S0[:2], 6, ids=[1, 0])
    with pytest.raises(ValueError, match="strictly ascending"):
        loop.plant_step_noisy(S0[:2], U[:2], U[:2], ids=[1, 0])
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="at least one step"):
            loop.episodes(S0, bad)
    for bad in (0, -2, 1.5, False):
        with pytest.raises(ValueError, match="plant_substeps must be an integer >= 1 or None"):
            loop.episodes(S0, 6, plant_substeps=bad)
        with pytest.raises(ValueError, match="plant_substeps must be an integer >= 1 or None"):
            loop.plant_step_noisy(S0, U, U, plant_substeps=bad)
    # the sigmas: shapes and values, either kind; a good first argument does not reach the library when the second is bad
    for kind in ("process", "measurement"):
        for bad in (np.zeros((3, 5)), np.zeros((2, 4)), np.zeros(3), np.zeros((3, 4, 1)), np.zeros((1, 4))):
            with pytest.raises(ValueError, match=rf"{kind} noise must be a scalar, \(4,\) or \(3, 4\)"):
                loop.set_noise(**{kind: bad})
        for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), 1e39, [0.1, 0.1, -0.0001, 0.1], "x"):
            with pytest.raises(ValueError, match=f"{kind} noise"):
                loop.set_noise(**{kind: bad})
    with pytest.raises(ValueError, match="measurement noise: a standard deviation is finite and >= 0, got nan for problem 2, state 1"):
        loop.set_noise(process=0.01, measurement=[[0, 0, 0, 0], [0, float("nan"), 0, 0]], ids=[0, 2])
    with pytest.raises(ValueError, match=r"seeds must have one entry per"):
        loop.set_noise_seeds([1, 2])
    with pytest.raises(ValueError, match=r"seeds must have one entry per"):
        loop.set_noise_seeds(None)
    # plant_step_noisy: S, U and U_prev, the last one required
    with pytest.raises(ValueError, match=r"S must have shape \(3, 4\)"):
        loop.plant_step_noisy(np.zeros((3, 3)), U, U)
    with pytest.raises(ValueError, match=r"U must have shape \(3, 1\)"):
        loop.plant_step_noisy(S0, np.zeros((3, 2)), U)
    with pytest.raises(ValueError, match=r"U must have shape \(3, 1\)"):
        loop.plant_step_noisy(S0, None, U)
    with pytest.raises(ValueError, match=r"U_prev must have shape \(3, 1\)"):
        loop.plant_step_noisy(S0, U, None)
    with pytest.raises(ValueError, match=r"U_prev must have shape \(3, 1\)"):
        loop.plant_step_noisy(S0, U, np.zeros((2, 1)))
    assert batch_episode_args(3, 4, 1, S0, 6) == (None, 3, 0)
    assert batch_episode_args(3, 4, 1, S0[:1], np.int64(2), ids=[1], plant_substeps=4, observations=S0[:1])[1:] == (1, 4)
    idv, n, sg = batch_noise_args(3, 4, [0.0, 0.1, 0.2, 0.3], ids=[0, 2])
    assert list(idv) == [0, 2] and n == 2 and sg.dtype == np.float32 and sg.shape == (2, 4) and sg.flags.c_contiguous
    np.testing.assert_array_equal(sg, np.tile(np.array([0.0, 0.1, 0.2, 0.3], np.float32), (2, 1)))
    assert batch_noise_args(3, 4, 0.5)[2].shape == (3, 4)


def test_cases_are_what_the_issue_names():
    assert E.PLANT_STREAM == 0x504C4E54
    src = open(os.path.join(ROOT, "control_toolkit_amd", "csrc", "ctk_launch.h")).read()
    assert len(re.findall(r"0x504C4E54", src)) == 1 and "CTK_PLANT_STREAM = 0x504C4E54u" in src      # defined once in the product
    assert not set(E.noise_seeds(K.B_SPLIT)) & set(K.seeds(K.B_SPLIT)) and len(set(E.noise_seeds(K.B_SPLIT))) == K.B_SPLIT
    for env in K.ENVS:
        w, v = E.sigmas(env, K.B_SPLIT)
        S = K.CASES[env][4].S
        assert w.shape == v.shape == (K.B_SPLIT, S) and w.dtype == v.dtype == np.float32
        assert not w[0].any() and not v[0].any() and not w[3].any() and not v[3].any()          # problem 0: all zero
        assert not v[1].any() and (w[1] == 0).sum() == 1 and w[1, 1] == 0                       # problem 1: process only, one component zero
        assert (w[2] > 0).all() and (v[2] > 0).all()                                            # problem 2: both kinds ...
        assert len(set(w[2])) == S and len(set(v[2])) == S and not set(w[2]) & set(v[2])        # ... distinct per kind and component
        both = np.concatenate([w[w > 0], v[v > 0]])
        assert 5e-3 <= both.min() and both.max() <= 3e-2                                        # about 1e-2 in state units


# ---- 3. input guards ----------------------------------------------------------------------------------------------------------------------
def test_the_oracles_draws_use_a_quarter_of_the_draw_bound():
    """DRAW_BOUND is 4 x the float32 device_noise's worst deviation from normal_f64 on the cases' words, by construction; here: it is
    positive, of the size test_gpu_device_rng.py measured (~3.4e-7 x 4), and every single word is within a quarter of it."""
    bound = E.draw_bound()
    print(f"draw bound {bound:.3e}")
    assert 2e-7 < bound <= 2e-6                               # never above the inherited bound of test_gpu_device_rng.py
    for seed in E.noise_seeds(K.B_SPLIT):
        for pos in (0, 1, 7, E.MAX_POS):
            for S in (4, 6, 7):
                assert np.abs(E.expected_noise(seed, pos, S).astype(np.float64) - E.noise_f64(seed, pos, S)).max() <= bound / 4


def cost_rows(env):
    """(own, s, u, u_prev) over the case start states of 5 problems (with the per-problem plant override) and 300 uniform inputs"""
    name, vals = K.override_values(env, K.B_SPLIT)
    s = K.start_states(env, K.B_SPLIT)
    U, UP = K.uniform_inputs(env, (300, K.B_SPLIT), seed=41), K.uniform_inputs(env, (300, K.B_SPLIT), seed=42)
    for p in range(K.B_SPLIT):
        for k in range(300):
            yield {name: vals[p]}, s[p], U[k, p], UP[k, p]


@pytest.mark.parametrize("env", K.ENVS)
def test_the_cost_bound_is_four_times_the_oracles_own_error(env):
    """Measures what COST_ATOL states: the float32 oracle's worst absolute deviation from the same cost in float64 over the case start
    states and 300 uniform inputs, x 4; and the guard: against the whole bound (atol + rtol |c|) the oracle uses at most a quarter.
    Every reference is finite and its largest term is not the only non-zero one."""
    worst_abs, worst_used = 0.0, 0.0
    for own, s, u, up in cost_rows(env):
        got = float(E.stage_cost_oracle(env, own, s, u, up))
        want, terms = E.stage_cost_f64(env, own, s, u, up)
        assert np.isfinite(got) and np.isfinite(want)
        assert sum(t != 0.0 for t in terms) >= 2 and max(terms) < want
        worst_abs = max(worst_abs, abs(got - want))
        worst_used = max(worst_used, abs(got - want) / float(E.cost_bound(env, want)))
    print(f"{env}: the float32 cost deviates from float64 by at most {worst_abs:.3e} (x 4 = {4 * worst_abs:.3e}; stated {E.COST_ATOL[env]:.3e}), "
          f"{100 * worst_used:.1f} % of the bound")
    assert 4 * worst_abs <= E.COST_ATOL[env] <= 4 * worst_abs * 1.1      # the stated atol IS the measurement (rounded up, at most 10 %)
    assert worst_used <= 0.25


def test_the_cost_reference_sees_the_previous_input_and_the_overrides():
    for env in K.ENVS:
        name, vals = K.override_values(env, K.B)
        s, u, up = K.start_states(env, 1)[0], K.uniform_inputs(env, (), seed=1), K.uniform_inputs(env, (), seed=2)
        base = E.stage_cost_oracle(env, None, s, u, up)
        assert E.stage_cost_oracle(env, None, s, u, u) != base                       # the stale u_prev = u_k is another number
        assert E.stage_cost_oracle(env, {"ccrc_weight": 5.0}, s, u, up) != base       # a cost weight override
        tgt = "target_position" if env == "CartPole" else "target_x"
        assert E.stage_cost_oracle(env, {tgt: 0.3}, s, u, up) != base
        np.testing.assert_allclose(base, E.stage_cost_f64(env, None, s, u, up)[0], rtol=1e-5)


# ---- 4. expected_noise --------------------------------------------------------------------------------------------------------------------
def test_expected_noise_tells_positions_seeds_and_halves_apart():
    a, b = E.noise_seeds(2)
    for S in (4, 6, 7):
        n = E.expected_noise(a, 3, S)
        assert n.shape == (2 * S,) and n.dtype == np.float32 and np.isfinite(n).all()
        np.testing.assert_array_equal(n, E.expected_noise(a, 3, S))
        assert not np.array_equal(n, E.expected_noise(a, 4, S)) and not np.array_equal(n, E.expected_noise(b, 3, S))
        assert not np.array_equal(n[:S], n[S:]) and len(set(n.tolist())) == 2 * S
        # the draws are device_noise's: stream PLANT, call = position, row 0
        from oracle import ctk_oracle as O
        np.testing.assert_array_equal(n, O.device_noise(a, 0x504C4E54, 3, 0, 1, 2 * S, "normal")[0])
        assert not np.array_equal(n, O.device_noise(a, 0, 3, 0, 1, 2 * S, "normal")[0])
