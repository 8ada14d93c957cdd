"""Sizes, start states and plant overrides of the closed-loop-on-the-device tests (CtkMppiBatch.closed_loop: run / plant_step), shared by
test_batch_run_cpu.py (which guards the inputs) and test_gpu_batch_run.py (which runs them).  A plain module, not a conftest.

The sizes are the smallest at which the batch kernels still take their usual paths: CartPole N 70 / H 7 / period 3 is `cartpole_small`
of test_gpu_mppi_batch.py (two workgroups per problem, the second one partly filled, interpolated inputs), Quad2D 128 / 12 / 5 and
Hover 128 / 12 / 1 cover 2 and 3 control inputs with and without interpolation.  B = 3, or 5 where a split into launches is wanted;
runs are 6 steps, or 10 where segments are wanted."""
import numpy as np

from oracle import ctk_oracle as O

f32 = np.float32
DT = 0.02
B, B_SPLIT = 3, 5
STEPS, STEPS_SEGMENTS = 6, 10
SPLIT_PER_LAUNCH, SEGMENT_STEPS = 2, 4          # 5 problems as 2 + 2 + 1 launches; 10 steps as 4 + 4 + 2
SUBSTEPS = (1, 2, 4)                            # at dt 0.02 the library's and the oracle's sub-step lengths are the same float32 at these counts
# the project's trajectory bound (tests/test_gpu_mppi.py: traj of the reference-recorded fixtures)
TRAJ_TOL = dict(rtol=1e-4, atol=2e-5)

# environment -> (N, H, period, extra engine keywords, the oracle's parameters, the inertial parameter the overrides scale)
CASES = {
    "CartPole": (70, 7, 3, {}, O.EnvParams, "m_pole"),
    "Quad2D": (128, 12, 5, {"action_low": [-1.0, -1.0], "action_high": [1.0, 1.0]}, O.Quad2DParams, "mass"),
    "Hover": (128, 12, 1, {}, O.HoverParams, "mass"),
}
ENVS = tuple(CASES)
SCALES = (0.8, 1.0, 1.3)                        # problem p's plant: the inertial parameter times SCALES[p % 3]
# the MLP batch: B 2, a 5-8-12-4 network per problem, the analytic CartPole as the plant
MLP = dict(B=2, N=64, H=8, hidden=(8, 12))


def batch_kwargs(env, materialize=False):
    N, H, period, extra, _, _ = CASES[env]
    return dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=DT, period_interpolation_inducing_points=period,
                materialize_trajectories=materialize, **extra)


def seeds(n):
    return [7 + q for q in range(n)]


def start_states(env, n, seed=0):
    """first_states of tests/test_gpu_mppi_batch.py: uniform in +-0.4, CartPole's pendulum hanging away from the target"""
    S = CASES[env][4].S
    s = np.random.default_rng(1000 + seed).uniform(-0.4, 0.4, (n, S)).astype(f32)
    if S == 4:
        s[:, 2] += 2.6
    return s


def limits(env):
    C = CASES[env][4].C
    return -np.ones(C, f32), np.ones(C, f32)


def uniform_inputs(env, shape, seed):
    """inputs drawn uniformly inside the limits, shape + (C,)"""
    lo, hi = limits(env)
    return np.random.default_rng(seed).uniform(lo, hi, tuple(shape) + (lo.size,)).astype(f32)


def override_values(env, n):
    """(parameter name, [n] values as float32): the default of the inertial parameter scaled per problem"""
    name = CASES[env][5]
    base = getattr(CASES[env][4](), name)
    return name, np.array([base * SCALES[p % len(SCALES)] for p in range(n)], f32)


def plant_oracle(env, substeps=1, **own):
    """the oracle's one-step plant with the parameters `own` replaced (as the float32 the library holds)"""
    pars = CASES[env][4](**{k: float(f32(v)) for k, v in own.items()})
    return O.Predictor("ODE", dt=DT, intermediate_steps=substeps, env=pars)


def oracle_step(env, S, U, substeps=1, own=None):
    """row p of S [n, S], U [n, C] through problem p's plant: own = None (the defaults) or {name: [n] values}"""
    S, U = np.asarray(S, f32), np.asarray(U, f32)
    if not own:
        return plant_oracle(env, substeps).step(S, U)
    return np.concatenate([plant_oracle(env, substeps, **{k: v[p] for k, v in own.items()}).step(S[p:p + 1], U[p:p + 1]) for p in range(S.shape[0])])
