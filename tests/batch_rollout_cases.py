"""The cases of the batch rollout (BatchRollout.rollout; include/ctk_hip_rollout.h), stated once for test_batch_rollout_cpu.py (which
guards the inputs) and test_gpu_batch_rollout.py (which feeds them to every batch family).  A plain module, not a conftest.

Shapes: the smallest at which the kernels can still go wrong.  N 70 / H 7 with M in {1, 37, 70}: one partial workgroup, a full one and a
partial one (the one-wave and four-wave kernels own 64 rows per workgroup), and for the GRU's 16-row tiles three and five workgroups;
N 128 / H 12 with M 128: two full workgroups, eight GRU tiles.  B 3 or 5 problems; ids None, a permuted subset, a single problem.
Plans: uniform in the input limits from a fixed NumPy seed, plus ONE row outside the limits — plans are taken as given and not clipped,
so the twin must agree there too.  Per problem: the inertial parameter scaled 0.8 / 1.0 / 1.3 and a target parameter of its own."""
import numpy as np

from oracle import ctk_oracle as O
import large_angle_cases as L

f32 = np.float32
DT = 0.02
SHAPES = [(70, 7, 1), (70, 7, 37), (70, 7, 70), (128, 12, 128)]        # (N, H, M)
INERTIAL = {"CartPole": "m_pole", "Quad2D": "inertia", "Hover": "inertia"}
TARGET = {"CartPole": "target_position", "Quad2D": "target_x", "Hover": "target_x"}
SCALES = (0.8, 1.0, 1.3, 0.8, 1.3)                                     # problem p: SCALES[p]
TARGETS = (0.15, -0.1, 0.05, 0.3, -0.25)
LIMITS = {"CartPole": ([-1.0], [1.0]), "Quad2D": ([-1.0, -0.8], [1.0, 0.9]), "Hover": ([-1.0, -0.7, -0.9], [1.0, 0.8, 0.6])}
OUTSIDE = 1.4                                                          # the row outside the limits: every input at OUTSIDE * high
IDS = {3: [None, [2, 0], [1]], 5: [None, [4, 1, 3], [2]]}              # by batch size: all, a permuted subset, a single problem


def own_params(env, p):
    """the (name, value) pairs problem p's controller differs from L.env_params(env) by"""
    base = L.env_params(env)
    return ((INERTIAL[env], float(f32(getattr(base, INERTIAL[env]) * SCALES[p]))), (TARGET[env], float(f32(TARGETS[p]))))


def params_of(env, p, extra=()):
    return L.params_with(env, own_params(env, p) + tuple(extra))


def states(env, n, seed=11):
    """[n, S]: the large-angle file's base state with the angle and its rate moved per row, so that no two rows start alike"""
    rng = np.random.default_rng(seed)
    s = np.stack([L.base_state(env, 0.4 + 0.3 * j, -0.7 + 0.2 * j) for j in range(n)]).astype(f32)
    return (s + f32(0.05) * rng.standard_normal(s.shape)).astype(f32)


def plans(env, n, M, H, seed=5):
    """[n, M, H, C]: uniform in the limits; the last row of problem 0 lies outside them"""
    lo, hi = (np.asarray(a, f32) for a in LIMITS[env])
    q = np.random.default_rng(seed).uniform(lo, hi, (n, M, H, lo.size)).astype(f32)
    q[0, M - 1] = f32(OUTSIDE) * hi
    return q


def u_prev(env, n, seed=3):
    lo, hi = (np.asarray(a, f32) for a in LIMITS[env])
    return np.random.default_rng(seed).uniform(lo, hi, (n, lo.size)).astype(f32)


def oracle_rollout(env, p, s, Q, up, kind="ODE", weights=None, hidden=None, substeps=1, extra=()):
    """(traj [M, H + 1, S], J [M]) of O.Predictor(...).predict_core + cost.get_trajectory_cost with problem p's parameters"""
    pars = params_of(env, p, extra)
    kw = dict(dt=DT, env=pars, intermediate_steps=substeps)
    if kind != "ODE":
        kw["weights"] = weights
    pred = O.Predictor(kind, **kw)
    if hidden is not None:
        pred.hidden = np.asarray(hidden, f32).reshape(2, -1).copy()
    traj = pred.predict_core(np.tile(np.asarray(s, f32), (Q.shape[0], 1)), Q)
    return traj, O.Cost(pars).get_trajectory_cost(traj, Q, np.asarray(up, f32))
