"""-m gpu: per-problem hyper-parameters and input limits of the CEM and RPGD batches (include/ctk_hip_family_hyper.h, FamilyHypers(batch);
kernels ctk_cem_batch_hp<ENV, TRAJ>, ctk_g_rpgd_batch_hp<ENV>).

The contract under test: problem p of a batch behaves BIT FOR BIT like CtkEngine("cem", "ODE", seed=seeds[p], ...) /
CtkEngine("rpgd", "ODE", generic_kernels=True, seed=seeds[p], ...) created with p's values and given the same calls; a change between two
steps makes the problem equal to a FRESH such handle that received the problem's state vector and Philox position; reset keeps the values
and refills from them.  Every comparison against handles and between batches is assert_array_equal: there is no tolerance in this file.
That equality with the case's handle cannot come from a kernel that used the defaults is test_family_hypers_cpu.py's guard; the tests
here also give every problem ONE seed and one set of draws, so that a problem differs from the default problem through its values alone,
and assert that it does.  Sizes: hyper_cases.CEM_SIZES (two workgroups per problem, the second ragged or full) and RPGD_N / RPGD_H /
RPGD_P; cases: family_hyper_cases.py."""
import ctypes

import numpy as np
import pytest

import batch_episode_cases as E
import family_hyper_cases as Fc
import hyper_cases as Hc
import large_angle_cases as L
from control_toolkit_amd import BatchClosedLoop, CtkCemBatch, CtkEngine, CtkRpgdBatch, FamilyHypers
from control_toolkit_amd._capi import CEM_HYPERS, RPGD_HYPERS
from test_gpu_batch_episodes import same_episodes
from test_gpu_batch_params import OWN
from test_gpu_family_loop import episode_loop, run_loop
from test_gpu_hyper import lim, rpgd_cfg, set_params
from test_gpu_large_angles import ENV_ID

pytestmark = pytest.mark.gpu

DT = Hc.DT
ERR_INVALID = 1                                          # CTK_ERR_INVALID_ARGUMENT
SEED = 11                                                # every problem's: the problems differ through their values alone
WARMUP_ITS = 3                                           # the first CEM step of a problem (shared), beside cem_outer_it 1, 2 and 4
CEM_BUFFERS = ("U_NOM", "STD", "J", "Q", "BEST_IDX")
RPGD_BUFFERS = ("PLAN", "ADAM_M", "ADAM_V", "AGES", "J", "U_NOM", "Q", "AGES_LOGGED", "BEST_IDX")
RPGD_K = int(max(int(Hc.RPGD_N * Hc.RPGD_DEFAULTS["opt_keep_k_ratio"]), 1))


def close_all(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def give(batch, env, q, own):
    """problem q of the batch gets the case's values through the per-problem entries"""
    view = FamilyHypers(batch)
    for name, value in own:
        if name == "limits":
            view.set_problem_limits(*Hc.limits_of(env, own), ids=[q])
        else:
            view.set_problem_hypers(name, value, ids=[q])


def compare(batch, handles, buffers, tag, who=None):
    for q in (range(batch.B) if who is None else who):
        h = handles[q]
        for name in buffers:
            np.testing.assert_array_equal(batch.read(name, q), h.read(name), err_msg=f"{tag}: {name} of problem {q}")
        np.testing.assert_array_equal(batch.get_state(q), h.get_state(), err_msg=f"{tag}: state vector of problem {q}")
        assert batch.rng_position(q) == h.rng_position(), f"{tag}: Philox position of problem {q}"


def differs_from_problem_0(batch, names, tag):
    base = [batch.read(n, 0) for n in names]
    for q in range(1, batch.B):
        assert not all(np.array_equal(batch.read(n, q), x) for n, x in zip(names, base)), f"{tag}: problem {q} equals the default problem"


# ---- CEM: a batch created with the DEFAULTS whose problem q then gets cases[q], and the handles created with cases[q] -----------------------------
def cem_kw(size, materialize, **over):
    N, H = size
    return dict(dict(num_rollouts=N, mpc_horizon=H, dt=DT, materialize_trajectories=materialize, warmup=True, warmup_iterations=WARMUP_ITS), **over)


def cem_handle(env, own, size, materialize, seed=SEED, **over):
    lo, hi = Hc.limits_of(env, own)
    h = CtkEngine("cem", "ODE", environment=env, seed=seed, action_low=lim(lo), action_high=lim(hi), **Fc.cem_values(own), **cem_kw(size, materialize, **over))
    set_params(h, L.env_params(env))
    return h


def cem_batch(env, B, size, materialize, seeds=None, **over):
    lo, hi = L.LIMITS[env]
    b = CtkCemBatch(B, seeds=[SEED] * B if seeds is None else seeds, environment=env, action_low=lim(lo), action_high=lim(hi), **Hc.CEM_DEFAULTS,
                    **cem_kw(size, materialize, **over))
    set_params(b, L.env_params(env))
    return b


def make_cem(env, size, materialize, cases, **over):
    batch = cem_batch(env, len(cases), size, materialize, **over)
    for q, own in enumerate(cases):
        give(batch, env, q, own)
    batch.reset()                                        # the mean and deviation of every problem from ITS limits and initial deviation
    return batch, [cem_handle(env, own, size, materialize, **over) for own in cases]


def cem_its(batch, q):
    return batch.samples_needed(q) // (batch.N * batch.H * batch.C)


def cem_step_both(batch, handles, S, tag, ids=None, noise=None):
    """one step of the listed problems on both sides, u bit for bit.  noise [its_max, N, H, C]: host draws, the same for every problem (each
    takes the iterations it runs) — the listed problems are then stepped in groups of equal iteration counts, as the library demands"""
    who = list(range(batch.B)) if ids is None else list(ids)
    groups = [who] if noise is None else [[q for q in who if cem_its(batch, q) == n] for n in sorted({cem_its(batch, q) for q in who})]
    for g in groups:
        block = None if noise is None else noise[:cem_its(batch, g[0])]
        u = batch.step(S[g], None if block is None else np.stack([block] * len(g)), ids=None if g == list(range(batch.B)) else g)
        for j, q in enumerate(g):
            np.testing.assert_array_equal(u[j], handles[q].step(S[q], block), err_msg=f"{tag}: u of problem {q}")


# ---- RPGD ----------------------------------------------------------------------------------------------------------------------------------------
RPGD_SIZES = dict(num_rollouts=Hc.RPGD_N, mpc_horizon=Hc.RPGD_H, period_interpolation_inducing_points=Hc.RPGD_P, dt=DT)


def rpgd_handle(env, own, base=Fc.RPGD_BASE, seed=SEED):
    lo, hi = Hc.limits_of(env, own)
    h = CtkEngine("rpgd", "ODE", environment=env, seed=seed, generic_kernels=True, action_low=lim(lo), action_high=lim(hi),
                  **rpgd_cfg(tuple(base) + tuple(own), RPGD_K), **RPGD_SIZES)
    set_params(h, L.env_params(env))
    return h


def rpgd_batch(env, B, base=Fc.RPGD_BASE, seeds=None):
    lo, hi = L.LIMITS[env]
    b = CtkRpgdBatch(B, seeds=[SEED] * B if seeds is None else seeds, environment=env, action_low=lim(lo), action_high=lim(hi), **rpgd_cfg(tuple(base), RPGD_K),
                     **RPGD_SIZES)
    set_params(b, L.env_params(env))
    return b


def rpgd_reset_both(batch, handles, draws=None, ids=None):
    """draws [N, P, C] for every listed problem alike, or None: the device Philox, every problem at its own position"""
    who = list(range(batch.B)) if ids is None else list(ids)
    batch.reset(None if draws is None else np.stack([draws] * len(who)), ids=ids)
    for q in who:
        handles[q].reset(draws)


def make_rpgd(env, cases, base=Fc.RPGD_BASE, draws=None):
    batch = rpgd_batch(env, len(cases), base)
    for q, own in enumerate(cases):
        give(batch, env, q, own)
    handles = [rpgd_handle(env, own, base) for own in cases]
    rpgd_reset_both(batch, handles, draws)
    return batch, handles


def rpgd_step_both(batch, handles, S, tag, ids=None, rng=None):
    """one step of the listed problems on both sides; rng: host draws — one [N - k, P, C] block, the same for every listed problem that
    resamples at this step"""
    who = list(range(batch.B)) if ids is None else list(ids)
    need = [batch.samples_needed(q) for q in who]
    for q, n in zip(who, need):
        assert n == handles[q].samples_needed(), f"{tag}: samples_needed of problem {q}"
    block, samples = None, None
    if rng is not None and any(need):
        block = rng.random(max(need), dtype=np.float32)
        samples = np.concatenate([block for n in need if n])
    u = batch.step(S[who], samples, ids=ids)
    for j, q in enumerate(who):
        np.testing.assert_array_equal(u[j], handles[q].step(S[q], block if need[j] else None), err_msg=f"{tag}: u of problem {q}")


def rpgd_states(env, cases):
    return np.stack([Hc.rpgd_state_of(env, (), far=Fc.rpgd_far(own)) for own in cases])


# ---- 1. every case in ONE batch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "philox"])
@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("size", Hc.CEM_SIZES, ids=lambda s: "N%d-H%d" % s)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_all_cases_in_one_batch(env, size, materialize, source):
    """problem 0 keeps the defaults, problem j has case j - 1; three steps: the warm-up step (3 iterations for every problem) and two short
    ones (1, 2 or 4 iterations by the problem's cem_outer_it)"""
    N, H = size
    cases = [()] + Fc.cem_cases(N)
    batch, handles = make_cem(env, size, materialize, cases)
    view, log = FamilyHypers(batch), "true" if materialize else "false"
    assert view.hypers_differ() == 1 and batch.params_differ() == 0
    assert batch.dominant_kernel() == f"ctk_cem_batch_hp<{ENV_ID[env]}, {log}>", batch.dominant_kernel()
    for q, own in enumerate(cases):
        for name in CEM_HYPERS:
            assert view.get_problem_hyper(name, q) == np.float32(Fc.cem_values(own)[name]), (q, name)
        lo, hi = view.get_problem_limits(q)
        np.testing.assert_array_equal(lo, Hc.limits_of(env, own)[0]); np.testing.assert_array_equal(hi, Hc.limits_of(env, own)[1])
        assert batch.read("BEST_IDX", q).shape == (Fc.cem_values(own)["cem_best_k"],)
    compare(batch, handles, ("U_NOM", "STD"), f"{env} N{N} after the reset")
    S = np.stack([Hc.STATE[env]] * len(cases))
    rng = np.random.default_rng(N + 3)
    want_its = [[WARMUP_ITS] * len(cases)] + [[Fc.cem_values(own)["cem_outer_it"] for own in cases]] * 2
    buffers = CEM_BUFFERS + (("TRAJ",) if materialize else ())
    for t in range(3):
        assert [cem_its(batch, q) for q in range(len(cases))] == want_its[t]
        noise = rng.standard_normal((4, N, H, batch.C)).astype(np.float32) if source == "host" else None
        tag = f"{env} N{N} log={log} {source} step {t}"
        cem_step_both(batch, handles, S, tag, noise=noise)
        compare(batch, handles, buffers, tag)
        if t >= 1:                                       # (cem_outer_it cannot show in the warm-up step, whose length is shared)
            differs_from_problem_0(batch, ("STD", "U_NOM", "BEST_IDX"), tag)
    assert batch.dominant_kernel() == f"ctk_cem_batch_hp<{ENV_ID[env]}, {log}>"
    close_all(batch, handles)


@pytest.mark.parametrize("source", ["host", "philox"])
@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_all_cases_in_one_batch(env, source):
    """problem 0 keeps the batch's defaults, problem j has case j - 1; reset and three steps: every problem resamples at the first, the
    problem with resamp_per 1 at the second, all but the one with resamp_per 3 at the third"""
    cases = [()] + Fc.RPGD_CASES
    rng = np.random.default_rng(5)
    C, Pn = L.LIMITS[env][0].size, 5
    batch, handles = make_rpgd(env, cases, draws=rng.random((Hc.RPGD_N, Pn, C), dtype=np.float32) if source == "host" else None)
    view = FamilyHypers(batch)
    assert view.hypers_differ() == 1 and batch.dominant_kernel() == f"ctk_g_rpgd_batch_hp<{ENV_ID[env]}>", batch.dominant_kernel()
    for q, own in enumerate(cases):
        for name in RPGD_HYPERS:
            assert view.get_problem_hyper(name, q) == np.float32(Fc.rpgd_values(own)[name]), (q, name)
    compare(batch, handles, ("PLAN", "AGES"), f"{env} after the reset")
    S = rpgd_states(env, cases)
    resampled, differed = [], set()
    shown = ("PLAN", "ADAM_M", "ADAM_V", "AGES")
    for t in range(3):
        resampled.append([batch.samples_needed(q) > 0 for q in range(len(cases))])
        tag = f"{env} {source} step {t}"
        rpgd_step_both(batch, handles, S, tag, rng=rng if source == "host" else None)
        compare(batch, handles, RPGD_BUFFERS, tag)
        base = [batch.read(n, 0) for n in shown]
        differed |= {q for q in range(1, len(cases)) if not all(np.array_equal(batch.read(n, q), x) for n, x in zip(shown, base))}
    per = [Fc.rpgd_values(own)["resamp_per"] for own in cases]
    assert resampled == [[t % p == 0 for p in per] for t in range(3)] and not all(resampled[1]) and any(resampled[1]) and not all(resampled[2])
    # every non-default problem differs from the default one after some step (rows descend independently of one another, so a problem
    # whose keepers are the default problem's can hold the default problem's state again after a later resampling)
    assert differed == set(range(1, len(cases))), f"{env}: problems {sorted(set(range(1, len(cases))) - differed)} never differed from the default problem"
    close_all(batch, handles)


# ---- 2. subsets and launch splitting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_subsets_and_split_launches(env, monkeypatch):
    """five problems at two per launch: ids [1, 3] (one launch whose record j is not problem j), then the rest, then all five as three
    launches, the second and third of which read their elements from an offset behind the records"""
    size = Hc.CEM_SIZES[0]
    cases = [(), (("cem_best_k", 2),), (("cem_outer_it", 4),), Hc.CEM_ALL, (("cem_best_k", 64), ("cem_stdev_min", 0.4))]
    monkeypatch.setenv("CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH", "2")
    batch, handles = make_cem(env, size, False, cases)
    monkeypatch.delenv("CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    S = np.stack([Hc.STATE[env] * (1.0 + 0.05 * q) for q in range(5)]).astype(np.float32)
    for t, ids in enumerate([[1, 3], [0, 2, 4], None, [1, 3, 4], None]):
        cem_step_both(batch, handles, S, f"{env} split launches, call {t}", ids=ids)
        compare(batch, handles, CEM_BUFFERS, f"{env} split launches, call {t}")
    close_all(batch, handles)


NORMAL = (("SAMPLING_DISTRIBUTION", "normal"),)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_subsets_and_the_normal_sampling_constants(env):
    """a batch that samples from a normal distribution, where sample_mean and sample_stdev are read: ids [1, 3], the rest, then all"""
    cases = [(), (("sample_mean", 0.3),), (("sample_stdev", 0.8), ("resamp_per", 1)), (("sample_mean", -0.2), ("learning_rate", 0.2)), (("limits", "asym"), ("outer_its", 5))]
    batch, handles = make_rpgd(env, cases, base=NORMAL)
    compare(batch, handles, ("PLAN", "AGES"), f"{env} normal, after the reset")
    differs_from_problem_0(batch, ("PLAN",), f"{env} normal, after the reset")
    S = np.stack([Hc.STATE[env] * (1.0 + 0.05 * q) for q in range(5)]).astype(np.float32)
    for t, ids in enumerate([[1, 3], [0, 2, 4], None, [1, 3], None]):
        rpgd_step_both(batch, handles, S, f"{env} normal, call {t}", ids=ids)
        compare(batch, handles, RPGD_BUFFERS, f"{env} normal, call {t}")
    close_all(batch, handles)


WHOLE = (("sample_whole_control_space", True),)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_limits_are_the_sampling_range_of_a_whole_space_batch(env):
    """the library's default sampling, uniform over the whole control space: a problem's own limits are then its sampling range, at the
    reset and for the fresh rows of a resampling step"""
    cases = [(), (("limits", "asym"),), (("limits", "asym"), ("resamp_per", 1)), (("learning_rate", 0.2),)]
    for draws in (None, np.random.default_rng(9).random((Hc.RPGD_N, 5, L.LIMITS[env][0].size), dtype=np.float32)):
        source = "philox" if draws is None else "host"
        batch, handles = make_rpgd(env, cases, base=WHOLE, draws=draws)
        assert batch.dominant_kernel() == f"ctk_g_rpgd_batch_hp<{ENV_ID[env]}>"
        compare(batch, handles, ("PLAN", "AGES"), f"{env} whole space {source}, after the reset")
        lo, hi = Hc.ASYM[env]
        for q in (1, 2):                                 # spread over ITS limits: inside them, and reaching their outer thirds
            plan = batch.read("PLAN", q)
            assert (plan >= lo - np.float32(1e-6)).all() and (plan <= hi + np.float32(1e-6)).all()
            assert (plan.min(axis=(0, 1)) < lo + (hi - lo) / 3).all() and (plan.max(axis=(0, 1)) > hi - (hi - lo) / 3).all()
        assert not np.array_equal(batch.read("PLAN", 1), batch.read("PLAN", 0))
        S = np.stack([Hc.STATE[env]] * len(cases))
        rng = np.random.default_rng(10)
        for t in range(3):                               # every problem resamples at steps 0 and 2, problem 2 at step 1 as well
            rpgd_step_both(batch, handles, S, f"{env} whole space {source} step {t}", rng=None if draws is None else rng)
            compare(batch, handles, RPGD_BUFFERS, f"{env} whole space {source} step {t}")
        close_all(batch, handles)


# ---- 3. together with per-problem plant and cost parameters, in both call orders -----------------------------------------------------------------
def personalise(batch, handles, env, rng):
    own = {name: rng.uniform(a, b, batch.B).astype(np.float32) for name, a, b in OWN[env]}
    for name, vals in own.items():
        for q in range(batch.B):
            handles[q].set_param(name, float(vals[q]))
    return lambda: [batch.set_problem_params(name, vals) for name, vals in own.items()]


@pytest.mark.parametrize("order", ["params_first", "hypers_first"])
@pytest.mark.parametrize("family", ["cem", "rpgd"])
@pytest.mark.parametrize("env", Hc.ENVS)
def test_with_per_problem_parameters(env, family, order):
    rng = np.random.default_rng(7)
    if family == "cem":
        cases = [(), Hc.CEM_ALL, (("cem_best_k", 64),), (("cem_outer_it", 1), ("cem_stdev_min", 0.4))]
        batch = cem_batch(env, len(cases), Hc.CEM_SIZES[0], True)
        handles = [cem_handle(env, own, Hc.CEM_SIZES[0], True) for own in cases]
    else:
        cases = [(), (("learning_rate", 0.2), ("adam_beta_1", 0.7)), (("outer_its", 5), ("limits", "asym")), (("resamp_per", 1), ("uniform_dist_min", -0.4))]
        batch = rpgd_batch(env, len(cases))
        handles = [rpgd_handle(env, own) for own in cases]
    params = personalise(batch, handles, env, rng)

    def hypers():
        for q, own in enumerate(cases):
            give(batch, env, q, own)

    for call in ((params, hypers) if order == "params_first" else (hypers, params)):
        call()
    assert batch.params_differ() == 1 and FamilyHypers(batch).hypers_differ() == 1
    want = f"ctk_cem_batch_hp<{ENV_ID[env]}, true>" if family == "cem" else f"ctk_g_rpgd_batch_hp<{ENV_ID[env]}>"
    assert batch.dominant_kernel() == want, batch.dominant_kernel()
    S = np.stack([Hc.STATE[env] * (1.0 + 0.05 * q) for q in range(len(cases))]).astype(np.float32)
    if family == "cem":
        batch.reset()
    else:
        rpgd_reset_both(batch, handles)
    for t in range(3):
        tag = f"{env} {family} {order} step {t}"
        if family == "cem":
            cem_step_both(batch, handles, S, tag)
            compare(batch, handles, CEM_BUFFERS + ("TRAJ",), tag)
        else:
            rpgd_step_both(batch, handles, S, tag)
            compare(batch, handles, RPGD_BUFFERS, tag)
    differs_from_problem_0(batch, ("J",), f"{env} {family} {order}")
    close_all(batch, handles)


# ---- 4. a change between two steps -------------------------------------------------------------------------------------------------------------------
def fresh(make, batch, q, is_rpgd=False):
    """a new handle with the problem's values that receives problem q's state vector and Philox position"""
    h = make()
    if is_rpgd:
        h.reset()
    h.set_state(batch.get_state(q))
    h.set_rng_position(batch.rng_position(q))
    return h


@pytest.mark.parametrize("env", Hc.ENVS)
def test_cem_change_between_steps(env):
    size, B = Hc.CEM_SIZES[0], 4
    seeds = [31 + q for q in range(B)]
    batch = cem_batch(env, B, size, False, seeds=seeds)
    view = FamilyHypers(batch)
    owns = [() for _ in range(B)]
    handles = [cem_handle(env, (), size, False, seed=seeds[q]) for q in range(B)]
    S = np.stack([Hc.STATE[env] * (1.0 + 0.1 * q) for q in range(B)]).astype(np.float32)
    for t in range(2):
        cem_step_both(batch, handles, S, f"{env} shared form, step {t}")
    assert batch.dominant_kernel() == f"ctk_cem_batch<{ENV_ID[env]}, false>" and view.hypers_differ() == 0
    # problem 1: a new cem_best_k; problem 2: a clamp that binds and limits that cut its current mean
    view.set_problem_hypers("cem_best_k", 2, ids=[1])
    view.set_problem_hypers("cem_stdev_min", 0.4, ids=[2])
    lo, hi = Hc.ASYM[env]
    view.set_problem_limits(lo, hi, ids=[2])
    owns[1], owns[2] = (("cem_best_k", 2),), (("cem_stdev_min", 0.4), ("limits", "asym"))
    assert batch.dominant_kernel() == f"ctk_cem_batch_hp<{ENV_ID[env]}, false>" and view.hypers_differ() == 1
    for q in (1, 2):
        handles[q].close()
        handles[q] = fresh(lambda: cem_handle(env, owns[q], size, False, seed=seeds[q]), batch, q)      # problems 0 and 3 keep their old handles
    for t in range(2):
        assert [cem_its(batch, q) for q in range(B)] == [2] * B          # the step count travelled with the state: no second warm-up
        cem_step_both(batch, handles, S, f"{env} after the change, step {t}")
        compare(batch, handles, CEM_BUFFERS, f"{env} after the change, step {t}")
    assert batch.read("BEST_IDX", 1).shape == (2,) and float(batch.read("STD", 2).min()) >= np.float32(0.4)
    mean2 = batch.read("U_NOM", 2)
    assert (mean2 >= lo).all() and (mean2 <= hi).all()
    # the whole batch at once, on an id subset afterwards
    view.set_hyper("cem_outer_it", 4)
    assert view.get_problem_hypers("cem_outer_it").tolist() == [4.0] * B and view.get_problem_hypers("cem_best_k").tolist() == [16.0, 2.0, 16.0, 16.0]
    for q in range(B):
        owns[q] = owns[q] + (("cem_outer_it", 4),)
        handles[q].close()
        handles[q] = fresh(lambda: cem_handle(env, owns[q], size, False, seed=seeds[q]), batch, q)
    for t in range(2):
        cem_step_both(batch, handles, S, f"{env} after set_hyper, step {t}", ids=None if t == 0 else [1, 3])
        compare(batch, handles, CEM_BUFFERS, f"{env} after set_hyper, step {t}")
    close_all(batch, handles)


@pytest.mark.parametrize("env", Hc.ENVS)
def test_rpgd_change_between_steps(env):
    """learning_rate and both betas after step 2: problem 1 gets a pair that needs a NEW bias-correction table, problem 2 then the same pair
    (the table exists), problem 3 another new one; the Adam step number keeps counting, so the tables are read at t = 7 and on"""
    B = 4
    seeds = [31 + q for q in range(B)]
    batch = rpgd_batch(env, B, seeds=seeds)
    view = FamilyHypers(batch)
    owns = [() for _ in range(B)]
    handles = [rpgd_handle(env, (), seed=seeds[q]) for q in range(B)]
    rpgd_reset_both(batch, handles)
    S = np.stack([Hc.STATE[env] * (1.0 + 0.1 * q) for q in range(B)]).astype(np.float32)
    for t in range(2):
        rpgd_step_both(batch, handles, S, f"{env} shared form, step {t}")
    assert batch.dominant_kernel() == f"ctk_g_rpgd_batch<{ENV_ID[env]}>" and view.hypers_differ() == 0
    view.set_problem_hypers("adam_beta_1", 0.7, ids=[1])
    view.set_problem_hypers("learning_rate", 0.2, ids=[1])
    view.set_problem_hypers("adam_beta_1", 0.7, ids=[2])
    view.set_problem_hypers("adam_beta_2", [0.9], ids=[3])
    owns[1], owns[2], owns[3] = (("adam_beta_1", 0.7), ("learning_rate", 0.2)), (("adam_beta_1", 0.7),), (("adam_beta_2", 0.9),)
    assert batch.dominant_kernel() == f"ctk_g_rpgd_batch_hp<{ENV_ID[env]}>" and view.hypers_differ() == 1
    adam_before = [batch.get_state(q)[-2] for q in range(B)]
    assert adam_before == [6.0] * B                      # two steps of outer_its 3
    for q in (1, 2, 3):
        handles[q].close()
        handles[q] = fresh(lambda: rpgd_handle(env, owns[q], seed=seeds[q]), batch, q, True)
    for t in range(3):
        rpgd_step_both(batch, handles, S, f"{env} after the change, step {t}")
        compare(batch, handles, RPGD_BUFFERS, f"{env} after the change, step {t}")
    assert [batch.get_state(q)[-2] for q in range(B)] == [15.0] * B
    # a pair goes out of use and its table is taken by the next new pair; problem 2 keeps reading the pair it shares
    view.set_problem_hypers("adam_beta_1", 0.8, ids=[1])
    view.set_hyper("outer_its", 2)
    owns[1] = (("adam_beta_1", 0.8), ("learning_rate", 0.2))
    for q in range(B):
        owns[q] = owns[q] + (("outer_its", 2),)
        handles[q].close()
        handles[q] = fresh(lambda: rpgd_handle(env, owns[q], seed=seeds[q]), batch, q, True)
    for t in range(2):
        rpgd_step_both(batch, handles, S, f"{env} after the second change, step {t}", ids=None if t == 0 else [1, 2])
        compare(batch, handles, RPGD_BUFFERS, f"{env} after the second change, step {t}")
    # ONE call that brings a pair whose table exists but is named by no problem at that moment (0.7, after problem 2 left it) AND a new
    # pair: the new pair's table must not be written over the one the call's other problem is about to name
    view.set_problem_hypers("adam_beta_1", 0.6, ids=[2])
    view.set_problem_hypers("adam_beta_1", [0.7, 0.5], ids=[0, 2])
    assert view.get_problem_hypers("adam_beta_1").tolist() == [np.float32(0.7), np.float32(0.8), np.float32(0.5), np.float32(0.9)]
    owns[0], owns[2] = (("adam_beta_1", 0.7), ("outer_its", 2)), (("adam_beta_1", 0.5), ("outer_its", 2))
    for q in (0, 2):
        handles[q].close()
        handles[q] = fresh(lambda: rpgd_handle(env, owns[q], seed=seeds[q]), batch, q, True)
    for t in range(2):
        rpgd_step_both(batch, handles, S, f"{env} after the third change, step {t}")
        compare(batch, handles, RPGD_BUFFERS, f"{env} after the third change, step {t}")
    close_all(batch, handles)


# ---- 5. reset of a subset after changed limits and initial deviation / sampling range ----------------------------------------------------------------
@pytest.mark.parametrize("env", Hc.ENVS)
def test_reset_refills_from_the_problems_values(env):
    size, B = Hc.CEM_SIZES[0], 3
    batch = cem_batch(env, B, size, False)
    handles = [cem_handle(env, (), size, False) for q in range(B)]
    S = np.stack([Hc.STATE[env]] * B)
    cem_step_both(batch, handles, S, f"{env} cem before")
    own = (("cem_initial_action_stdev", 1.3), ("limits", "asym"))
    for q in (1, 2):
        give(batch, env, q, own)
    batch.reset(ids=[1, 2])
    for q in (1, 2):
        handles[q].close()
        handles[q] = cem_handle(env, own, size, False)
        handles[q].set_rng_position(batch.rng_position(q))       # a reset keeps the position
    compare(batch, handles, ("U_NOM", "STD"), f"{env} cem after the reset")
    mid = 0.5 * (Hc.ASYM[env][0] + Hc.ASYM[env][1])
    np.testing.assert_array_equal(batch.read("U_NOM", 1)[0, -1], mid)
    assert (batch.read("STD", 2) == np.float32(1.3)).all() and (batch.read("STD", 0) != np.float32(1.3)).all()
    assert [cem_its(batch, q) for q in range(B)] == [2, WARMUP_ITS, WARMUP_ITS]
    cem_step_both(batch, handles, S, f"{env} cem after the reset")
    compare(batch, handles, CEM_BUFFERS, f"{env} cem after the reset and a step")
    close_all(batch, handles)
    # RPGD: the draws of the device Philox mapped with the problem's range and clipped to its limits
    batch = rpgd_batch(env, B)
    handles = [rpgd_handle(env, ()) for q in range(B)]
    rpgd_reset_both(batch, handles)
    S = np.stack([Hc.STATE[env]] * B)
    rpgd_step_both(batch, handles, S, f"{env} rpgd before")
    own = (("uniform_dist_min", -0.4), ("uniform_dist_max", 0.7), ("limits", "asym"))
    for q in (1, 2):
        give(batch, env, q, own)
        handles[q].close()
        handles[q] = rpgd_handle(env, own)
        handles[q].set_rng_position(batch.rng_position(q))
    rpgd_reset_both(batch, handles, ids=[1, 2])
    for q in (1, 2):                                     # (the state vector holds u, which a reset keeps and a new handle does not have)
        for name in ("PLAN", "ADAM_M", "ADAM_V", "AGES"):
            np.testing.assert_array_equal(batch.read(name, q), handles[q].read(name), err_msg=f"{env} rpgd after the reset: {name} of problem {q}")
        assert batch.rng_position(q) == handles[q].rng_position()
    plan = batch.read("PLAN", 1)
    ulp = np.float32(1e-6)                               # (a plan is interpolated between two clipped inducing points: a rounding of room)
    assert (plan >= np.maximum(Hc.ASYM[env][0], np.float32(-0.4)) - ulp).all() and (plan <= np.minimum(Hc.ASYM[env][1], np.float32(0.7)) + ulp).all()
    assert not np.array_equal(plan, batch.read("PLAN", 0))
    for q in (1, 2):                                     # the problem's last output, which the reset kept
        handles[q].set_state(batch.get_state(q))
    rpgd_step_both(batch, handles, S, f"{env} rpgd after the reset")
    compare(batch, handles, RPGD_BUFFERS, f"{env} rpgd after the reset and a step")
    close_all(batch, handles)


# ---- 6. the closed loops on the device: records computed ahead, with per-problem iteration counts and resampling periods ---------------------------
@pytest.mark.parametrize("family", ["cem", "rpgd"])
@pytest.mark.parametrize("env", Hc.ENVS)
def test_closed_loops_are_the_host_loops(env, family):
    steps, B = 6, 4
    if family == "cem":
        cases = [(), (("cem_outer_it", 1), ("cem_best_k", 2)), (("cem_outer_it", 4),), Hc.CEM_ALL + (("cem_outer_it", 1),)]
    else:
        cases = [(), (("outer_its", 5), ("resamp_per", 1)), (("outer_its", 0), ("resamp_per", 3)), (("learning_rate", 0.2), ("limits", "asym"), ("resamp_per", 4))]
    twins = []
    for _ in range(2):
        b = cem_batch(env, B, Hc.CEM_SIZES[0], False, seeds=[21 + q for q in range(B)]) if family == "cem" else rpgd_batch(env, B, seeds=[21 + q for q in range(B)])
        for q, own in enumerate(cases):
            give(b, env, q, own)
        b.reset()
        w, v = E.sigmas(env, B)
        BatchClosedLoop(b).set_noise(process=w, measurement=v)
        BatchClosedLoop(b).set_noise_seeds(E.noise_seeds(B))
        twins.append(b)
    a, b = twins
    S0 = np.stack([Hc.STATE[env] * (1.0 + 0.1 * q) for q in range(B)]).astype(np.float32)
    tag = f"{env} {family}"
    states, inputs = BatchClosedLoop(a).run(S0, steps)
    want_states, want_inputs = run_loop(b, S0, steps)
    np.testing.assert_array_equal(states, want_states, err_msg=f"{tag}: run, states")
    np.testing.assert_array_equal(inputs, want_inputs, err_msg=f"{tag}: run, inputs")
    assert np.isfinite(inputs).all()
    buffers = {"cem": CEM_BUFFERS[:-1], "rpgd": RPGD_BUFFERS[:-1]}[family]

    def same(tag):
        for q in range(B):
            for name in buffers + ("BEST_IDX",):
                np.testing.assert_array_equal(a.read(name, q), b.read(name, q), err_msg=f"{tag}: {name} of problem {q}")
            np.testing.assert_array_equal(a.get_state(q), b.get_state(q), err_msg=f"{tag}: state vector of problem {q}")
            assert a.rng_position(q) == b.rng_position(q), f"{tag}: Philox position of problem {q}"

    same(f"{tag} after the run")
    ids = [0, 1, 3]
    got, want = BatchClosedLoop(a).episodes(states[ids, -1], steps, ids=ids), episode_loop(b, states[ids, -1], steps, ids=ids)
    same_episodes(got, want, f"{tag}: episodes")
    same(f"{tag} after the episodes")
    np.testing.assert_array_equal(a.step(S0), b.step(S0))
    same(f"{tag} one more step")
    assert not np.array_equal(inputs[0], inputs[1])
    close_all(a, b)


# ---- 7. a batch that calls no setter launches what it always launched -------------------------------------------------------------------------------
@pytest.mark.parametrize("env", Hc.ENVS)
def test_untouched_batches_report_the_old_kernels(env):
    eid = ENV_ID[env]
    for materialize in (False, True):
        b = cem_batch(env, 2, Hc.CEM_SIZES[0], materialize)
        view, log = FamilyHypers(b), "true" if materialize else "false"
        assert view.hypers_differ() == 0 and b.dominant_kernel() == f"ctk_cem_batch<{eid}, {log}>"
        assert view.get_problem_hypers("cem_best_k").tolist() == [16.0, 16.0]
        b.step(np.stack([Hc.STATE[env]] * 2))
        assert b.dominant_kernel() == f"ctk_cem_batch<{eid}, {log}>"
        b.set_problem_params(OWN[env][0][0], [0.1, 0.2])
        assert view.hypers_differ() == 0 and b.dominant_kernel() == f"ctk_cem_batch_pp<{eid}, {log}>"
        b.step(np.stack([Hc.STATE[env]] * 2))
        view.set_hyper("cem_stdev_min", 0.02)
        assert view.hypers_differ() == 1 and b.params_differ() == 1 and b.dominant_kernel() == f"ctk_cem_batch_hp<{eid}, {log}>"
        b.close()
    b = rpgd_batch(env, 2)
    view = FamilyHypers(b)
    b.reset()
    assert view.hypers_differ() == 0 and b.dominant_kernel() == f"ctk_g_rpgd_batch<{eid}>"
    b.step(np.stack([Hc.STATE[env]] * 2))
    b.set_problem_params(OWN[env][0][0], [0.1, 0.2])
    assert view.hypers_differ() == 0 and b.dominant_kernel() == f"ctk_g_rpgd_batch_pp<{eid}>"
    view.set_problem_limits(-0.5, 0.5, ids=[1])
    assert view.hypers_differ() == 1 and b.dominant_kernel() == f"ctk_g_rpgd_batch_hp<{eid}>"
    b.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def snapshot(batch, names):
    view = FamilyHypers(batch)
    return ([view.get_problem_hypers(n).tolist() for n in names], [[x.tolist() for x in view.get_problem_limits(q)] for q in range(batch.B)],
            [batch.get_state(q).tolist() for q in range(batch.B)], [batch.rng_position(q) for q in range(batch.B)], view.hypers_differ(), batch.dominant_kernel())


@pytest.mark.parametrize("family", ["cem", "rpgd"])
@pytest.mark.parametrize("env", Hc.ENVS)
def test_refusals_change_nothing(env, family):
    B = 3
    if family == "cem":
        batch, names, prefix, count, intname = cem_batch(env, B, Hc.CEM_SIZES[0], False), CEM_HYPERS, ("ctk_cem_batch", "ctk_cem_problem"), 4, "cem_best_k"
    else:
        batch, names, prefix, count, intname = rpgd_batch(env, B), RPGD_HYPERS, ("ctk_rpgd_batch", "ctk_rpgd_problem"), 11, "resamp_per"
        batch.reset()
    view = FamilyHypers(batch)
    for touched in (False, True):
        if touched:
            view.set_problem_hypers(intname, 2, ids=[1])
        batch.step(np.stack([Hc.STATE[env]] * B))
        before = snapshot(batch, names)
        lib, h, C = batch._lib, batch._h, batch.C
        fam, prob = prefix
        f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        ids_bad, ids_desc, ids_ok = (ctypes.c_int32 * 2)(0, B), (ctypes.c_int32 * 2)(2, 1), (ctypes.c_int32 * 2)(0, 2)
        nan, inf = (ctypes.c_float * 3)(1.0, float("nan"), 1.0), (ctypes.c_float * 3)(float("inf"), 1.0, 1.0)
        lo_ok, hi_ok = (ctypes.c_float * (3 * C))(*[-0.5] * (3 * C)), (ctypes.c_float * (3 * C))(*[0.5] * (3 * C))
        hi_low = (ctypes.c_float * (3 * C))(*([0.5] * (3 * C - 1) + [-0.6]))
        hi_nan = (ctypes.c_float * (3 * C))(*([0.5] * (3 * C - 1) + [float("nan")]))
        frac = (ctypes.c_float * 3)(2.0, 2.5, 2.0)
        small = (ctypes.c_float * 3)(1.0, 0.0 if family == "cem" else -1.0, 1.0)
        set_hyper, set_limits, set_all = getattr(lib, f"{prob}_set_hyper"), getattr(lib, f"{prob}_set_limits"), getattr(lib, f"{fam}_set_hyper")
        calls = [
            (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ids_bad, 0, f3), "outside"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ids_desc, 0, f3), "strictly ascending"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, count, f3), "unknown hyper-parameter"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, -1, f3), "unknown hyper-parameter"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, 0, None), "NULL values"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, 1, nan), "finite"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, 2, inf), "finite"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, names[intname], frac), "integral"),
            (f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, names[intname], small), "needs"),
            (f"{fam}_set_hyper", lambda: set_all(h, count, 1.0), "unknown hyper-parameter"),
            (f"{fam}_set_hyper", lambda: set_all(h, 1, float("nan")), "finite"),
            (f"{fam}_set_hyper", lambda: set_all(h, names[intname], 1.5), "integral"),
            (f"{prob}_set_limits", lambda: set_limits(h, 2, ids_bad, lo_ok, hi_ok), "outside"),
            (f"{prob}_set_limits", lambda: set_limits(h, 0, None, None, hi_ok), "NULL limits"),
            (f"{prob}_set_limits", lambda: set_limits(h, 0, None, lo_ok, None), "NULL limits"),
            (f"{prob}_set_limits", lambda: set_limits(h, 0, None, lo_ok, hi_low), "action_low must be <= action_high"),
            (f"{prob}_set_limits", lambda: set_limits(h, 0, None, lo_ok, hi_nan), "a limit is finite"),
        ]
        if family == "cem":
            big = (ctypes.c_float * 3)(1.0, 1.0, float(batch.N + 1))
            calls.append((f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, names["cem_best_k"], big), "cem_best_k <= num_rollouts"))
            calls.append((f"{prob}_set_hyper", lambda: set_hyper(h, 2, ids_ok, names["cem_outer_it"], small), "cem_outer_it >= 1"))
        else:
            zero = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
            calls.append((f"{prob}_set_hyper", lambda: set_hyper(h, 0, None, names["resamp_per"], zero), "resamp_per >= 1"))
        for entry, call, text in calls:
            assert call() == ERR_INVALID, (entry, text)
            msg = batch._b.last_error(h).decode()
            assert msg.startswith(entry + ":") and text in msg, (entry, text, msg)
            assert snapshot(batch, names) == before, (entry, text)
        # the getters refuse quietly
        out = ctypes.c_float()
        assert getattr(lib, f"{prob}_get_hyper")(h, B, 0, ctypes.byref(out)) == ERR_INVALID and getattr(lib, f"{prob}_get_hyper")(h, 0, count, ctypes.byref(out)) == ERR_INVALID
        assert getattr(lib, f"{prob}_get_limits")(h, 0, None, None) == ERR_INVALID and getattr(lib, f"{prob}_hypers_differ")(None) == 0
        with pytest.raises(ValueError, match="integral"):
            view.set_problem_hypers(intname, 1.5)
        assert snapshot(batch, names) == before
        batch.step(np.stack([Hc.STATE[env]] * B))        # ... and nothing was left half done: the batch goes on stepping
    if family == "cem":                                   # caller-supplied samples with mixed per-problem iteration counts are refused as a warm-up mix is
        view.set_problem_hypers("cem_outer_it", 4, ids=[2])
        state = snapshot(batch, names)
        with pytest.raises(ValueError, match=r"0: 2, 1: 2, 2: 4.*separate calls"):
            batch.step(np.stack([Hc.STATE[env]] * B), np.zeros((B, 2, batch.N, batch.H, batch.C), np.float32))
        assert snapshot(batch, names) == state
    batch.close()
