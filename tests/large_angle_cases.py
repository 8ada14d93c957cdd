"""Start states with a large pole / body / craft angle, shared by test_large_angles_cpu.py (which guards them) and
test_gpu_large_angles.py (which feeds them to every analytic rollout kernel).  A plain module, not a conftest.

The rollout kernels evaluate sin / cos with ctk_sincosf_fast (csrc/ctk_device.h: no range check, documented for
|x| <= CTK_SINCOS_FAST_LIMIT = 32768) and run the horizon again with the checked ctk_sincosf where a wave or workgroup saw a larger
angle.  The cases sit on both sides of that limit:

 * IN_RANGE   the fast path alone, at reduction quotients n ~ +-16 000 and ~ +-20 000 (every other test of the suite has |n| <= 2);
 * JUST_OUT   the second pass is taken; the fast formula is still right there (error 7e-8 up to 2.6e5), so these cases show that the
              second pass is CORRECT, not that it ran;
 * FAR_OUT    the fast formula is wrong by O(1): the only cases that fail when a range check is missing or without effect;
 * CROSSING   (theta0, omega0, H): the angle passes the limit inside the horizon, so that amax first trips at a chosen step.

Smaller angles (3e2 .. 2e4) are left out on purpose: there single-ulp flips of theta between two associations of the same fp32
arithmetic are frequent and move J by up to 1e-4 relative (measured in test_large_angles_cpu.py's docstring), which says nothing about
a kernel.  The module also builds the inputs of the GPU file and the oracle's results for them (mppi_ref, cem_ref), once."""
import functools

import numpy as np

from oracle import ctk_oracle as O

f32 = np.float32
LIMIT = f32(32768.0)
BELOW, ABOVE = float(np.nextafter(LIMIT, f32(0))), float(np.nextafter(LIMIT, f32(np.inf)))

# the first four stay inside the range for the whole horizon in every environment (fast path alone); +-32767.5 and +-BELOW start inside
# and, where the pole or body picks up speed, leave it some steps later.  (+-300.5, 3.0) and (+-300.5, 0.7) were measured too and are NOT
# used: at 300 rad one float32 spacing is 3e-5, a quarter of the rows have a near-tie in some angle update (near_ties() below), the oracle's
# own float64-step form then differs from it in 1 - 2 rows of 256 (J by up to 4.7e-5 relative), and so did the four-wave MPPI kernel
# (2 spacings in 7 of 2100 angles, J and every other tensor inside their bounds).  +-25000.5 takes their place.
IN_RANGE = [(32760.5, 0.7), (-32760.5, -0.7), (25000.5, 0.7), (-25000.5, -0.7), (32767.5, 0.7), (-32767.5, -0.7), (BELOW, 0.0), (-BELOW, 0.0)]
JUST_OUT = [(32768.5, 0.7), (ABOVE, 0.0), (-40000.25, 0.7)]
FAR_OUT = [(float(f32(1e9)), 0.7), (float(f32(-3e8)), -2.0)]

# (theta0, omega0, H, step): `step` = the first h in 0 .. H whose angle traj[:, h, angle] is out of range in ANY row (h = H is the terminal
# state: no sin / cos of the dynamics is taken there, only the terminal cost's), for the inputs draws_for(env, 128, H).  Found by a
# search in theta0 that keeps 0.02 rad (5 ulp) between the limit and the angles either side of it, so that an ulp in the inputs does not
# move the step; test_large_angles_cpu.py recomputes every one.  With other inputs or other N the crossing lies elsewhere in the horizon.
# 15 and 16 lie either side of the S1 = 16 split of the four-wave kernels' horizon.
CROSSING = {
    "CartPole": [(32767.72, 5.0, 4, 3), (32766.48, 5.0, 20, 15), (32766.44, 5.0, 20, 16), (-32766.33, -5.0, 20, 15), (32767.59, 5.0, 4, 4)],
    "Quad2D": [(32767.71, 5.0, 4, 3), (32765.97, 5.0, 20, 15), (32765.82, 5.0, 20, 16), (-32765.71, -5.0, 20, 15), (32767.58, 5.0, 4, 4)],
    "Hover": [(32767.75, 5.0, 4, 3), (32766.53, 5.0, 20, 15), (32766.43, 5.0, 20, 16), (-32766.55, -5.0, 20, 15), (32767.65, 5.0, 4, 4)],
}

# CartPole, H = 6 (the throughput kernels' test): in range at the start, out of it from step 1 or 2 on
SHORT_CROSSING = [(32767.9, 5.0), (-32767.9, -5.0)]

ANGLE = {"CartPole": 2, "Quad2D": 4, "Hover": 4}
_BASE = {"CartPole": [0.1, -0.2, 0.0, 0.0], "Quad2D": [0.3, -0.2, 0.7, 0.1, 0.0, 0.0], "Hover": [0.2, -0.1, -0.3, 0.15, 0.0, 0.0, 0.5]}
LIMITS = {"CartPole": (np.array([-1.0], f32), np.array([1.0], f32)),
          "Quad2D": (np.array([-1.0, -0.8], f32), np.array([1.0, 0.9], f32)),
          "Hover": (np.array([-1.0, -0.7, -0.5], f32), np.array([0.9, 1.0, 0.5], f32))}
ENVS = ("CartPole", "Quad2D", "Hover")


def env_params(env):
    """the plant + cost parameters of every test of the two files (a terminal cost, so that the terminal angle's cos counts)"""
    if env == "CartPole":
        return O.EnvParams(terminal_weight=0.3)
    if env == "Quad2D":
        return O.Quad2DParams(terminal_weight=0.4, target_x=0.1)
    return O.HoverParams(terminal_weight=0.35, target_x=0.2)


def base_state(env, theta0=0.0, omega0=0.0):
    s = np.array(_BASE[env], f32)
    s[ANGLE[env]], s[ANGLE[env] + 1] = theta0, omega0
    return s


class StepF64(O.Predictor):
    """the oracle's predictor with every step's arithmetic in float64 on the float32 state, rounded back (by the parent's own cast):
    stands in for "another association of the same fp32 arithmetic" — what a kernel may differ from the oracle by"""
    def step(self, s, q):
        return super().step(np.asarray(s, np.float64), q)


def first_out_of_range_step(traj, angle_index):
    """first h of traj [N, H+1, S] at which any row's |angle| exceeds the fast sin/cos limit; None if none does"""
    out = np.nonzero((np.abs(traj[:, :, angle_index]) > LIMIT).any(axis=0))[0]
    return int(out[0]) if out.size else None


def normals_for(env, N, H, seed=None):
    """standard-normal draws [N, H, C]; the rows of a smaller N are the first rows of a larger one (N <= 128)"""
    C = LIMITS[env][0].size
    return np.random.default_rng(PLAIN_SEED[env] if seed is None else seed).standard_normal((128, H, C)).astype(f32)[:N].copy()


def draws_for(env, N, H, seed=None):
    """the control inputs of the CPU checks and of the crossing search: clip(0.5 N(0, 1)) to the environment's limits [N, H, C] — what
    CEM's first iteration forms from normals_for() (mean 0, stdev 0.5), what MPPI forms from mppi_noise_for() and what rollout() is given"""
    lo, hi = LIMITS[env]
    return np.clip(f32(0.5) * normals_for(env, N, H, seed), lo, hi).astype(f32)


def mppi_noise_for(env, N, H, seed, stdev):
    """draws [N, H, C] for an MPPI step with period 1 from a zero plan whose inputs clip(stdev * noise) equal draws_for() to an ulp"""
    return (f32(0.5) * normals_for(env, N, H, seed) / f32(stdev)).astype(f32)


def all_cases(env):
    """[(name, theta0, omega0, H)]: every state the GPU file feeds `env`'s kernels"""
    out = [(f"{kind}{i}", th, om, 20) for kind, lst in (("in", IN_RANGE), ("just", JUST_OUT), ("far", FAR_OUT)) for i, (th, om) in enumerate(lst)]
    out += [(f"cross{step}_{i}", th, om, H) for i, (th, om, H, step) in enumerate(CROSSING[env])]
    return out + ([(f"short{i}", th, om, 6) for i, (th, om) in enumerate(SHORT_CROSSING)] if env == "CartPole" else [])


# what the single-gradient and descent tests start from: one state of each kind
GRAD_CASES = [IN_RANGE[0], JUST_OUT[2], FAR_OUT[0]]


def near_ties(traj, angle_index, dt=0.02, substeps=1, omega_ulps=16.0):
    """rows of traj [N, H+1, S] in which some angle update theta' = theta + dt * omega lands so close to a float32 rounding boundary that
    another association of the same arithmetic (a fused multiply-add; omega off by up to `omega_ulps` spacings) could round it the other
    way.  One spacing of theta near 32768 is 2e-3 - 4e-3 rad, which moves J by ~1e-4 relative: such a row says nothing about a kernel, so
    the inputs are chosen (seeds, below) to have none.  (With Euler sub-steps pass the trajectory of the sub-steps.)"""
    th, om = traj[:, :-1, angle_index].astype(np.float64), traj[:, :-1, angle_index + 1].astype(np.float64)
    nxt = traj[:, 1:, angle_index]
    h = float(f32(dt / substeps))
    exact = th + h * om
    half_up = 0.5 * (np.nextafter(nxt, f32(np.inf)).astype(np.float64) - nxt)
    half_dn = 0.5 * (nxt - np.nextafter(nxt, f32(-np.inf)).astype(np.float64))
    margin = np.minimum(nxt + half_up - exact, exact - (nxt - half_dn))
    delta = np.spacing(np.abs(h * om).astype(f32)).astype(np.float64) + h * omega_ulps * np.spacing(np.abs(om).astype(f32)).astype(np.float64)
    return np.nonzero((margin <= delta).any(axis=1))[0]


# Seeds of the draws.  They are CHOSEN (tests/test_large_angles_cpu.py checks the choice): with them no angle update of any row of any case
# is a near-tie (near_ties() above), so that a kernel's other association of the same arithmetic cannot round an angle the other way.
PLAIN_SEED = {"CartPole": 23, "Quad2D": 1, "Hover": 4}      # normals_for / draws_for: rollout(), MPPI with period 1, CEM's first iteration
# ("mppi" | "cem", env, N, H) -> seed: MPPI with period > 1, CEM's second iteration
OTHER_SEED = {("mppi", "CartPole", 100, 20): 1, ("mppi", "CartPole", 100, 4): 0, ("cem", "CartPole", 128, 20): 4, ("cem", "CartPole", 100, 20): 22,
              ("cem", "CartPole", 128, 4): 0, ("mppi", "Quad2D", 100, 20): 1, ("mppi", "Quad2D", 100, 4): 0, ("cem", "Quad2D", 128, 20): 4,
              ("cem", "Quad2D", 100, 20): 1, ("cem", "Quad2D", 128, 4): 0, ("mppi", "Hover", 100, 20): 1, ("mppi", "Hover", 100, 4): 0,
              ("cem", "Hover", 128, 20): 7, ("cem", "Hover", 100, 20): 1, ("cem", "Hover", 128, 4): 0, ("mppi", "CartPole", 32832, 6): 0}


# ---- the inputs of the GPU file and the oracle's results for them (computed once, shared, left unchanged) -----------------------------
MPPI_CONFIGS = [(128, 20, 1), (100, 20, 5), (128, 4, 1), (100, 4, 5)]      # (N, H, period)
CEM_SIZES = [(128, 20), (100, 20), (128, 4)]
CEM_K, CEM_ITS = 16, 2
TP_N, TP_H = 32768 + 64, 6
TP_STATES = [IN_RANGE[0], IN_RANGE[1]] + SHORT_CROSSING + JUST_OUT + FAR_OUT


def params_with(env, own):
    """the environment's parameters with the (name, value) pairs of `own` replaced (a batch problem's own parameters)"""
    pars = env_params(env)
    for n, v in own:
        setattr(pars, n, float(np.float32(v)))
    return pars


def cases(env, H):
    """[(name, theta0, omega0, crossing step or None)] of horizon H"""
    out = []
    for name, th, om, Hc in all_cases(env):
        if Hc == H:
            step = int(name[5:].split("_")[0]) if name.startswith("cross") else None
            out.append((name, th, om, step))
    return out


@functools.lru_cache(maxsize=None)
def mppi_ref(env, N, H, p, th, om, own=(), isteps=1, predictor=O.Predictor):
    """one oracle MPPI step from a zero plan and u_prev = 0 (shared by every form that runs this case; left unchanged)"""
    pars = params_with(env, own)
    lo, hi = LIMITS[env]
    o = O.MPPI(predictor("ODE", dt=0.02, env=pars, intermediate_steps=isteps), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H,
               period_interpolation_inducing_points=p)
    o.u_nom = np.zeros_like(o.u_nom)
    rows = min(N, 128)              # the throughput sizes repeat 128 distinct rows: few distinct trajectories, every row still compared
    if p == 1:                      # inputs = draws_for(env, N, H) to an ulp: the crossings lie where CROSSING says
        noise = mppi_noise_for(env, rows, H, PLAIN_SEED[env], o.stdev)
    else:
        noise = np.random.default_rng(OTHER_SEED[("mppi", env, N, H)]).standard_normal((rows, o.P, o.C)).astype(np.float32)
    noise = np.ascontiguousarray(np.tile(noise, (-(-N // rows), 1, 1))[:N])
    s = base_state(env, th, om)
    u = np.asarray(o.step(s, noise), np.float32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.u_run, traj=o.rollout_trajectories, u_nom=o.u_nom)


@functools.lru_cache(maxsize=None)
def cem_ref(env, N, H, th, om, own=(), predictor=O.Predictor):
    pars = params_with(env, own)
    lo, hi = LIMITS[env]
    o = O.CEM(predictor("ODE", dt=0.02, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=CEM_ITS, cem_best_k=CEM_K)
    # the first iteration's plans: clip(0.5 (lo + hi) + 0.5 * normals_for(env, N, H, 0)), draws_for() where the limits are symmetric
    noise = np.stack([normals_for(env, N, H), np.random.default_rng(OTHER_SEED[("cem", env, N, H)]).standard_normal((N, H, o.C)).astype(np.float32)])
    s = base_state(env, th, om)
    u = np.asarray(o.step(s, noise), np.float32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.Q, traj=o.rollout_trajectories, mu=o.dist_mue, std=o.stdev)


