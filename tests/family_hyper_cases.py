"""The per-problem hyper-parameters of the CEM and RPGD batches (include/ctk_hip_family_hyper.h) moved away from a batch's defaults, shared by
test_family_hypers_cpu.py (which guards the cases) and test_gpu_family_hypers.py (which gives every case to one problem of a batch).  A
plain module, not a conftest.

A case is hyper_cases' kind of tuple ((name, value), ...) with "limits": "asym" for hyper_cases.ASYM[env].  The cases are
hyper_cases.CEM_CASES and RPGD_CASES restricted to the names a problem can have of its own (a case that names a shared field —
shift_previous, SAMPLING_DISTRIBUTION, sample_whole_control_space — is left out), plus single cases for the counts and the uniform range.

Two choices that the guard (test_family_hypers_cpu.py) forced, both by choosing another value or state and neither by loosening it:
  * cem_best_k = 16 IS hyper_cases.CEM_DEFAULTS' value, so it cannot move anything: 32 stands in its place (2, 32, 64 and N).
  * uniform_dist_min / uniform_dist_max are read only with sample_whole_control_space off, which is shared: the RPGD batch of these tests
    is created with it off (RPGD_BASE), and every reference below is the oracle's run of RPGD_BASE + the case.
resamp_per shows only where count % resamp_per differs from count % 2: at the second step for 1, at the THIRD for 3 — hyper_cases.rpgd_ref
has two steps, so rpgd_run below is that function with a third step and draws for every step (the oracle takes them where it resamples).

The reference builders are cached and their results are left unchanged by every test."""
import functools

import numpy as np

from oracle import ctk_oracle as O
import hyper_cases as Hc
import large_angle_cases as L

f32 = np.float32

CEM_NAMES = ("cem_best_k", "cem_initial_action_stdev", "cem_stdev_min", "cem_outer_it")
RPGD_NAMES = ("learning_rate", "adam_beta_1", "adam_beta_2", "adam_epsilon", "gradmax_clip", "sample_stdev", "sample_mean", "uniform_dist_min",
              "uniform_dist_max", "outer_its", "resamp_per")
# the keyword of CtkEngine / CtkRpgdBatch where it is not the hyper-parameter's name
ENGINE_KW = {"uniform_dist_min": "sample_min", "uniform_dist_max": "sample_max"}


def restricted(cases, names):
    return [own for own in cases if all(k in names or k == "limits" for k, _ in own)]


# ---- CEM ------------------------------------------------------------------------------------------------------------------------------------
def cem_new(N):
    """the single cases this feature adds, at population N"""
    return [(("cem_best_k", k),) for k in (2, 32, 64, N)] + [(("cem_outer_it", 1),), (("cem_outer_it", 4),)]


def cem_cases(N):
    return restricted(Hc.CEM_CASES, CEM_NAMES) + cem_new(N)


def cem_values(own):
    """the four hyper-parameters of a case"""
    return Hc.config_of(Hc.CEM_DEFAULTS, own)


# ---- RPGD -----------------------------------------------------------------------------------------------------------------------------------
RPGD_BASE = (("sample_whole_control_space", False),)
RPGD_NEW = [(("outer_its", 0),), (("outer_its", 5),), (("resamp_per", 1),), (("resamp_per", 3),), (("uniform_dist_min", -0.4),), (("uniform_dist_max", 0.7),)]
RPGD_CASES = restricted(Hc.RPGD_CASES, RPGD_NAMES) + [(("limits", "asym"),)] + RPGD_NEW
RPGD_STEPS = 3


def rpgd_far(own):
    """the clip that never binds starts where the defaults' clip binds on every row (hyper_cases.RPGD_CLIP_NEVER)"""
    return own == Hc.RPGD_CLIP_NEVER


def rpgd_values(own):
    return Hc.config_of(Hc.RPGD_DEFAULTS, RPGD_BASE + tuple(own))


# (name of the case's first hyper-parameter) -> (step, tensor) it must show in: the step's index in rpgd_run, -1 for the reset
RPGD_SHOWS_IN = {"learning_rate": (1, "descended"), "adam_epsilon": (1, "descended"), "outer_its": (1, "descended"), "adam_beta_1": (1, "m"),
                 "gradmax_clip": (1, "m"), "adam_beta_2": (1, "v"), "uniform_dist_min": (-1, "Q_init"), "uniform_dist_max": (-1, "Q_init"),
                 "limits": (-1, "Q_init")}


def rpgd_shows_in(own):
    (name, value), = own
    if name == "resamp_per":
        return (1, "Q") if value == 1 else (2, "Q")
    return RPGD_SHOWS_IN[name]


@functools.lru_cache(maxsize=None)
def rpgd_run(env, own, far=False, seed=Hc.RPGD_SEED):
    """hyper_cases.rpgd_ref of RPGD_BASE + own with RPGD_STEPS steps: the reset, then every step from the previous one's state, with
    resampling draws offered at every step"""
    full = RPGD_BASE + tuple(own)
    o = Hc.rpgd_oracle(env, full)
    C, Pn = o.C, O.num_inducing_points(Hc.RPGD_H, Hc.RPGD_P)
    rng = np.random.default_rng(seed)
    d0 = rng.random((Hc.RPGD_N, Pn, C), dtype=f32)
    draws = [rng.random((Hc.RPGD_N - o.k, Pn, C), dtype=f32) for _ in range(RPGD_STEPS)]
    o.optimizer_reset(d0)
    o.u = O._u_out(np.full(C, Hc.U_PREV, f32))
    s, steps = Hc.rpgd_state_of(env, (), far), []
    Q_init = o.Q.copy()
    for t in range(RPGD_STEPS):
        resamples = o.count % o.resamp_per == 0
        u = np.asarray(o.step(s, draws[t]), f32).reshape(-1)
        steps.append(dict(u=u, J=o.J, descended=o.Q_before_warmstart, Q=o.Q.copy(), m=o.opt.m.copy(), v=o.opt.v.copy(), ages=o.trajectory_ages.copy(),
                          resampled=resamples))
    return dict(s=s, reset_draws=d0, draws=draws, Q_init=Q_init, steps=steps, k=o.k)


def limits_of(env, own):
    return Hc.limits_of(env, own)
