"""Noise settings, references and bounds of the stochastic closed-loop tests (BatchClosedLoop.episodes / plant_step_noisy, kernel
ctk_batch_plant_noisy<ENV>), shared by test_batch_episodes_cpu.py (which guards the inputs and measures the bounds) and
test_gpu_batch_episodes.py (which runs them).  A plain module, not a conftest.  Sizes, start states, overrides and the one-step plant
oracle are batch_run_cases.py's: CartPole N 70 / H 7 / period 3, Quad2D 128 / 12 / 5, Hover 128 / 12 / 1, B 3 (5 where a split is wanted),
6 steps (10 where segments are wanted), the MLP batch B 2, N 64 / H 8, network 5-8-12-4.

Per-problem sigmas (problem p takes pattern p % 3): 0 all zero; 1 process noise only, with one component zero; 2 both kinds, with
different magnitudes for the two kinds and per component, so that a swap of the process and measurement columns shows.  About 1e-2 in
state units.

Bounds.  None is invented here:
  transition   the project's TRAJ_TOL (rtol 1e-4 / atol 2e-5) + sigma_w * DRAW_BOUND
  observation  sigma_v * DRAW_BOUND + 2^-23 |y| (one rounding of the sum; the compiler may fuse the multiply-add)
  DRAW_BOUND   the rule of test_gpu_device_rng.py: 4 x the float32 oracle's own worst deviation from philox_cases.normal_f64, on the
               words these cases use (the noise seeds, positions 0 .. MAX_POS, 2 S columns for S = 4, 6, 7); computed here
  cost         rtol J_RTOL (3e-5), atol COST_ATOL[env] = 4 x the float32 oracle's worst absolute deviation from the same cost in float64
               over the case start states and 300 uniform inputs: measured by test_batch_episodes_cpu.py and stated here."""
import functools

import numpy as np

import batch_run_cases as K
import philox_cases as PC
from oracle import ctk_oracle as O

f32 = np.float32
PLANT_STREAM = 0x504C4E54                   # csrc/ctk_launch.h: CTK_PLANT_STREAM
MAX_POS = 48                                # the tests keep every noise position below this
TRAJ_TOL = K.TRAJ_TOL
J_RTOL = PC.J_RTOL
# measured by test_batch_episodes_cpu.py::test_the_cost_bound_is_four_times_the_oracles_own_error (worst |float32 - float64| over the case
# start states of 5 problems x 300 uniform inputs and previous inputs: CartPole 3.58e-3 at costs of some 1e4, Quad2D 3.74e-4, Hover 4.45e-5), x 4
COST_ATOL = {"CartPole": 1.44e-2, "Quad2D": 1.5e-3, "Hover": 1.78e-4}


def noise_seeds(n):
    """distinct from the controller seeds (batch_run_cases.seeds: 7 + q); the high word is not zero"""
    return [((0xA11CE5ED + q) << 32) | (0x0BAD5EED + 17 * q) for q in range(n)]


def sigmas(env, n):
    """(process [n, S], measurement [n, S]) as float32"""
    S = K.CASES[env][4].S
    i = np.arange(S)
    w, v = np.zeros((n, S), f32), np.zeros((n, S), f32)
    for p in range(n):
        if p % 3 == 1:
            w[p] = 1.0e-2 * (1.0 + 0.25 * i)
            w[p, 1] = 0.0
        elif p % 3 == 2:
            w[p] = 0.8e-2 * (1.0 + 0.3 * i)
            v[p] = 2.1e-2 * (1.0 - 0.07 * i)
    return w, v


def expected_noise(seed, pos, S):
    """the normal draws [2 S] of one transition: columns [0, S) process, [S, 2 S) measurement"""
    return O.device_noise(int(seed), PLANT_STREAM, int(pos), 0, 1, 2 * S, "normal")[0]


def noise_f64(seed, pos, S):
    return PC.normal_f64(int(seed), PLANT_STREAM, int(pos), 0, 1, 2 * S)[0]


@functools.lru_cache(maxsize=None)
def draw_bound():
    """4 x the float32 oracle's worst deviation from the float64 transform on the words of these cases"""
    own = 0.0
    for seed in noise_seeds(K.B_SPLIT):
        for pos in range(MAX_POS + 1):
            for S in (4, 6, 7):
                own = max(own, float(np.abs(expected_noise(seed, pos, S).astype(np.float64) - noise_f64(seed, pos, S)).max()))
    return 4.0 * own


def env_pars(env, own=None):
    """the oracle's parameters with `own` = {name: value} replaced (as the float32 the library holds)"""
    return K.CASES[env][4](**{k: float(f32(v)) for k, v in (own or {}).items()})


def stage_cost_oracle(env, own, s, u, u_prev):
    """the float32 oracle's stage cost of ONE row: s [S], u [C], u_prev [C]; own = None or {name: value}"""
    pars = env_pars(env, own)
    c = O.Cost(pars, dt=K.DT).get_stage_cost(np.asarray(s, f32).reshape(1, 1, pars.S), np.asarray(u, f32).reshape(1, 1, pars.C),
                                            np.asarray(u_prev, f32).reshape(pars.C))
    return f32(np.asarray(c).reshape(-1)[0])


def stage_cost_f64(env, own, s, u, u_prev):
    """(cost, its terms) of the same row with the oracle's float32 constants and float64 arithmetic"""
    e = env_pars(env, own)
    k = {n: float(v) for n, v in O.derived_constants(e, K.DT, 1).items()}
    g = lambda name: float(f32(getattr(e, name)))                                         # noqa: E731
    s, u, up = (np.asarray(x, f32).astype(np.float64).reshape(-1) for x in (s, u, u_prev))
    cc, ccrc = k["ccR"] * float(u @ u), g("ccrc_weight") * float((u - up) @ (u - up))
    if env == "CartPole":
        dxn, omc = (s[0] - g("target_position")) * k["inv_xs"], 1.0 - np.cos(s[2])
        terms = [g("dd_weight") * dxn * dxn, k["ep_c"] * omc * omc, g("ekp_weight") * s[3] * s[3], cc, ccrc]
    else:
        ty = g("target_z") if env == "Quad2D" else g("target_y")
        dx, dy = s[0] - g("target_x"), s[2] - ty
        vel = g("vel_weight") * (s[1] * s[1] + s[3] * s[3]) + g("angvel_weight") * s[5] * s[5]
        if env == "Hover":
            vel += g("wheel_weight") * s[6] * s[6]
        terms = [k["pos_c"] * (dx * dx + dy * dy), g("ang_weight") * (1.0 - np.cos(s[4])), vel, cc, ccrc]
    return float(sum(terms)), [float(t) for t in terms]


def cost_bound(env, want):
    return COST_ATOL[env] + J_RTOL * np.abs(np.asarray(want, np.float64))
