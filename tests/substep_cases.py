"""Euler sub-steps (intermediate_steps > 1) and time steps other than 0.02, shared by test_substeps_cpu.py (which guards the inputs) and
test_gpu_substeps.py (which feeds them to every analytic rollout kernel).  A plain module, not a conftest.

Every analytic kernel has code of its own for sub-steps: CartPole's four-wave and affine kernels leave their fast path altogether
(Env<0>::fast_ok) and run the checked recurrence with a loop i = 1 .. isteps - 1; Quad2D and Hover loop inside the fast path and track
the largest angle again for every sub-step.  A kernel that gets the count or the length of the sub-steps wrong returns plausible numbers
for another plant, so the cases below are compared with the float32 oracle (oracle/ctk_oracle.py: _ode_step / _quad_step / _hover_step),
fed the same draws as the large-angle file's (large_angle_cases.normals_for, mppi_noise_for, PLAIN_SEED, OTHER_SEED).

CONFIGS   (dt, intermediate_steps).  3 sub-steps catch "one sub-step too many / too few" where 2 might not; 0.03 / 3 is not exact in
          binary, so it exercises the double -> float32 derivation of the sub-step length; (0.005, 1) is another dt on the fast path.
          The handle's dt is a float32 in the C ABI, so a kernel integrates at f32(f64(f32(dt)) / k), the oracle at f32(dt / k): the pairs
          are chosen so that the two are the same float32 (kernel_substep / oracle_substep; test_substeps_cpu.py asserts it).  They
          differ by one ulp at (0.02, 3), (0.02, 5), (0.005, 3) and (0.01, 3), which is why those are not here.
STATES    three ordinary ones and two large ones (large_angle_cases.IN_RANGE[0], FAR_OUT[0]).  On Quad2D and Hover the large ones put
          the sub-step loop inside the fast path (25000.5 .. 32760.5 rad) and inside the second pass (1e9 rad); on CartPole every
          sub-step run is the checked path already.  test_substeps_cpu.py decides which large states are kept (DROPPED below).
SIZES     (N, H, period): two full tiles and a ragged population, H = 4 below and H = 20 across the four-wave kernels' S1 = 16 split.

The reference builders are cached and their results are left unchanged by every test."""
import functools

import numpy as np

from oracle import ctk_oracle as O
import large_angle_cases as L

f32 = np.float32
CONFIGS = [(0.02, 2), (0.03, 3), (0.005, 1)]
CONFIG_IDS = ["dt0.02-k2", "dt0.03-k3", "dt0.005-k1"]
COMPOSITIONS = [(0.02, 2, 10, 0.01, 20), (0.02, 4, 5, 0.005, 20)]       # (dt_a, k, H_a, dt_b, H_b): (dt_a, k) against (dt_a / k, 1) on repeated inputs
ORDINARY = [(0.4, -0.7), (-2.9, 1.5), (3.1, 0.0)]
LARGE = [L.IN_RANGE[0], L.FAR_OUT[0]]
SIZES = [(128, 20, 1), (100, 20, 5), (128, 4, 1)]                       # MPPI (N, H, period)
CEM_SIZES = [(128, 20), (100, 20)]
CEM_K, CEM_ITS = L.CEM_K, L.CEM_ITS
ROLLOUT_SIZES = [(128, 20), (100, 20), (128, 4)]                        # random action and plain rollout()
TP_CONFIGS = [(0.005, 1), (0.03, 3)]                                    # the throughput kernels: (0.02, 2) is test_gpu_large_angles.py's
GMM_ENVS = ("CartPole", "Quad2D")                                       # the environments test_gpu_large_angles.py runs ctk_affine_rollout_mix on
RANDOM_SEED = 11                                                        # the uniform draws of the random-action step (+ N + H)
GMM_SEED = 5                                                            # normals and component uniforms of the CEM-GMM step, as the large-angle file's
ROLLOUT_GAIN = f32(1.5)                                                 # plain rollout(): plans 1.5 N(0, 1), a good share beyond every limit

# (environment, large state) that test_substeps_cpu.py's guards refuse (an angle bit or a near-tie between the oracle and SubstepF64, or
# a gap in J above a tenth of the GPU bound) are listed here and fed to no kernel; see that file's docstring for the measurements.
DROPPED = set()

# Seeds of the draws where the large-angle file's own (PLAIN_SEED, OTHER_SEED) or this module's defaults leave a near-tie in some angle
# update of a SUB-step at 32760.5 rad (test_substeps_cpu.py names the row): (kind, environment, N, H, dt, k) -> seed, chosen there.
SEEDS = {("mppi", "CartPole", 100, 20, 0.03, 3): 2, ("rollout", "CartPole", 128, 20, 0.03, 3): 1, ("gmm", "CartPole", 128, 20, 0.005, 1): 1,
         ("random", "Quad2D", 128, 20, 0.03, 3): 2, ("cem", "Hover", 100, 20, 0.02, 2): 2, ("mppi", "Hover", 128, 20, 0.03, 3): 1,
         ("cem", "CartPole", 128, 20, 0.02, 2, (("target_position", 0.05),)): 1}

# The batch tests: one state per problem, ordinary and large ones in one launch; with per-problem parameters problem q has its own target
# (the values of test_gpu_large_angles.py's batch tests).
BATCH_OWN = {"CartPole": ("target_position", [0.0, 0.05, -0.04, 0.08]), "Quad2D": ("target_x", [0.1, 0.3, -0.2, 0.25]),
             "Hover": ("target_x", [0.2, -0.1, 0.35, 0.05])}
MPPI_BATCH_SIZES = [(128, 20, 1), (100, 20, 5)]
CEM_BATCH_SIZE = (128, 20)


def batch_states(env, B):
    """[(theta0, omega0, is_large)], one per problem: B = 4 ordinary, large, ordinary, large; B = 3 ordinary, large, large (the large ones that
    the guards keep; an ordinary state takes the place of a dropped one)"""
    want = [ORDINARY[0], LARGE[0], ORDINARY[1], LARGE[1]] if B == 4 else [ORDINARY[0], LARGE[0], LARGE[1]]
    return [(ORDINARY[2][0], ORDINARY[2][1], False) if (env, st) in DROPPED else (st[0], st[1], st in LARGE) for st in want]


def batch_own(env, B, per_problem):
    name, vals = BATCH_OWN[env]
    return [((name, vals[q]),) if per_problem else () for q in range(B)]


def batch_sets(env):
    """[(label, dt, k, theta0, omega0, is_large, builder(predictor=...))]: what the PER-PROBLEM batch tests add to input_sets (the shared
    form's problems are cases of input_sets)"""
    out = []
    for dt, k in CONFIGS:
        for n, h, p in MPPI_BATCH_SIZES:
            for (th, om, large), own in zip(batch_states(env, 4), batch_own(env, 4, True)):
                out.append((f"mppi batch_pp N{n} H{h} p{p} dt{dt} k{k} {own}", dt, k, th, om, large, functools.partial(mppi_ref, env, n, h, p, th, om, dt, k, own)))
        n, h = CEM_BATCH_SIZE
        for (th, om, large), own in zip(batch_states(env, 3), batch_own(env, 3, True)):
            out.append((f"cem batch_pp N{n} H{h} dt{dt} k{k} {own}", dt, k, th, om, large, functools.partial(cem_ref, env, n, h, th, om, dt, k, own)))
    return out


def seed_for(kind, env, N, H, dt, k, default, own=()):
    """a batch problem with parameters of its own may name a seed of its own: (kind, environment, N, H, dt, k, own)"""
    return SEEDS.get((kind, env, N, H, dt, k, own), SEEDS.get((kind, env, N, H, dt, k), default))


def kernel_substep(dt, k):
    """the sub-step length a handle derives: dt crosses the C ABI as a float32, the library divides in double and rounds once"""
    return f32(np.float64(f32(dt)) / k)


def oracle_substep(dt, k):
    return f32(dt / k)


def states(env, large=True):
    """[(name, theta0, omega0, is_large)] fed to `env`'s kernels"""
    out = [(f"ord{i}", th, om, False) for i, (th, om) in enumerate(ORDINARY)]
    if large:
        out += [(f"large{i}", th, om, True) for i, (th, om) in enumerate(LARGE) if (env, (th, om)) not in DROPPED]
    return out


class SubstepF64(O.Predictor):
    """the oracle's predictor with every SUB-step's arithmetic in float64 on the float32 state, rounded to float32 after every sub-step:
    "another association of the same fp32 arithmetic" for a kernel that rounds after each sub-step.  (large_angle_cases.StepF64 rounds
    once per MPC step: with sub-steps at large angles that is another computation, not another association.)"""
    def step(self, s, q):
        one = L.StepF64(self.kind, dt=float(oracle_substep(self.dt, self.intermediate_steps)), intermediate_steps=1, env=self.env)
        for _ in range(self.intermediate_steps):
            s = one.step(np.asarray(s, np.float32), q)
        return s


def sub_trajectory(env, s, Q, dt, k, own=()):
    """[N, k H + 1, S]: the states after every SUB-step, by rolling the one-sub-step predictor at dt / k with each input repeated k times
    (legitimate where f32((dt / k) / 1) == f32(dt / k), which test_substeps_cpu.py asserts)"""
    pred = O.Predictor("ODE", dt=dt / k, env=L.params_with(env, own), intermediate_steps=1)
    return pred.predict_core(np.tile(s, (Q.shape[0], 1)), np.repeat(Q, k, axis=1))


def _models(env, dt, k, own, predictor):
    pars = L.params_with(env, own)
    return pars, predictor("ODE", dt=dt, env=pars, intermediate_steps=k), O.Cost(pars, dt=dt)


@functools.lru_cache(maxsize=None)
def mppi_ref(env, N, H, p, th, om, dt, isteps, own=(), predictor=O.Predictor):
    """one oracle MPPI step from a zero plan and u_prev = 0: large_angle_cases.mppi_ref with a time step"""
    pars, pred, cost = _models(env, dt, isteps, own, predictor)
    lo, hi = L.LIMITS[env]
    o = O.MPPI(pred, cost, lo, hi, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
    o.u_nom = np.zeros_like(o.u_nom)
    rows = min(N, 128)
    if p == 1:
        noise = L.mppi_noise_for(env, rows, H, seed_for("mppi", env, N, H, dt, isteps, L.PLAIN_SEED[env], own), o.stdev)
    else:
        noise = np.random.default_rng(seed_for("mppi", env, N, H, dt, isteps, L.OTHER_SEED[("mppi", env, N, H)], own)).standard_normal((rows, o.P, o.C)).astype(np.float32)
    noise = np.ascontiguousarray(np.tile(noise, (-(-N // rows), 1, 1))[:N])
    s = L.base_state(env, th, om)
    u = np.asarray(o.step(s, noise), np.float32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.u_run, traj=o.rollout_trajectories, u_nom=o.u_nom)


@functools.lru_cache(maxsize=None)
def cem_ref(env, N, H, th, om, dt, isteps, own=(), predictor=O.Predictor):
    pars, pred, cost = _models(env, dt, isteps, own, predictor)
    lo, hi = L.LIMITS[env]
    o = O.CEM(pred, cost, lo, hi, num_rollouts=N, mpc_horizon=H, cem_outer_it=CEM_ITS, cem_best_k=CEM_K)
    noise = np.stack([L.normals_for(env, N, H), np.random.default_rng(seed_for("cem", env, N, H, dt, isteps, L.OTHER_SEED[("cem", env, N, H)], own)).standard_normal((N, H, o.C)).astype(np.float32)])
    s = L.base_state(env, th, om)
    u = np.asarray(o.step(s, noise), np.float32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.Q, traj=o.rollout_trajectories, mu=o.dist_mue, std=o.stdev)


@functools.lru_cache(maxsize=None)
def random_ref(env, N, H, th, om, dt, isteps, predictor=O.Predictor, own=()):
    """one oracle random-action step: uniform plans between the limits, the arg-min's first input"""
    pars, pred, cost = _models(env, dt, isteps, own, predictor)
    lo, hi = L.LIMITS[env]
    o = O.RandomAction(pred, cost, lo, hi, num_rollouts=N, mpc_horizon=H)
    u01 = np.random.default_rng(seed_for("random", env, N, H, dt, isteps, RANDOM_SEED + N + H)).random((N, H, lo.size), dtype=np.float32)
    s = L.base_state(env, th, om)
    u = np.asarray(o.step(s, u01), np.float32).reshape(-1)
    return dict(s=s, u01=u01, u=u, J=o.J, Q=o.Q, traj=o.rollout_trajectories, best_idx=int(o.best_idx))


@functools.lru_cache(maxsize=None)
def rollout_ref(env, N, H, th, om, dt, isteps, predictor=O.Predictor, own=()):
    """plain rollouts of plans that nobody clips (ROLLOUT_GAIN * normals_for), u_prev = 0.1"""
    pars, pred, cost = _models(env, dt, isteps, own, predictor)
    Q = (ROLLOUT_GAIN * L.normals_for(env, N, H, seed_for("rollout", env, N, H, dt, isteps, None))).astype(np.float32)
    up = np.full(pars.C, 0.1, np.float32)
    s = L.base_state(env, th, om)
    traj = pred.predict_core(np.tile(s, (N, 1)), Q)
    return dict(s=s, Q=Q, u_prev=up, traj=traj, J=cost.get_trajectory_cost(traj, Q, up))


def composition_plans(env, N, Ha):
    """the plans of the composition check (each input is then repeated k times for the handle at dt / k)"""
    return L.draws_for(env, N, Ha, seed_for("compose", env, N, Ha, None, None, None))


def gmm_draws(env, N, H, dt, k):
    rng = np.random.default_rng(seed_for("gmm", env, N, H, dt, k, GMM_SEED))
    return rng.standard_normal((1, N, H, L.LIMITS[env][0].size)).astype(np.float32), rng.random((1, N), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def gmm_ref(env, N, H, K, th, om, dt, isteps, predictor=O.Predictor, own=()):
    """one outer iteration of CEM-GMM from the initial mixture (tests/gmm_oracle.py), as the large-angle file runs it"""
    from gmm_oracle import CEMGMM
    pars, pred, cost = _models(env, dt, isteps, own, predictor)
    lo, hi = L.LIMITS[env]
    o = CEMGMM(pred, cost, *((float(lo[0]), float(hi[0])) if lo.size == 1 else (lo, hi)), num_rollouts=N, mpc_horizon=H, cem_outer_it=1, cem_best_k=K)
    normals, uniforms = gmm_draws(env, N, H, dt, isteps)
    s = L.base_state(env, th, om)
    u = np.asarray(o.step(s, normals, uniforms), np.float32).reshape(-1)
    return dict(s=s, normals=normals, uniforms=uniforms, u=u, J=o.J, Q=o.Q, traj=o.rollout_trajectories)


def _swap(ref, dt, k):
    """ref(..., theta0, omega0, dt, k, predictor=...) as a function that ends in (theta0, omega0, predictor=...)"""
    def call(*args, predictor=O.Predictor):
        return ref(*args, dt, k, predictor=predictor)
    return call


def input_sets(env):
    """every (label, H, dt, k, with large states, builder) of the GPU file for `env`; builder(theta0, omega0, predictor=...) -> results
    with keys s, Q, J, traj"""
    sets = []
    for dt, k in CONFIGS:
        c = f"dt{dt} k{k}"
        sets += [(f"mppi N{n} H{h} p{p} {c}", h, dt, k, True, functools.partial(_swap(mppi_ref, dt, k), env, n, h, p)) for n, h, p in SIZES]
        sets += [(f"cem N{n} H{h} {c}", h, dt, k, True, functools.partial(_swap(cem_ref, dt, k), env, n, h)) for n, h in CEM_SIZES]
        sets += [(f"random N{n} H{h} {c}", h, dt, k, True, functools.partial(_swap(random_ref, dt, k), env, n, h)) for n, h in ROLLOUT_SIZES]
        sets += [(f"rollout N{n} H{h} {c}", h, dt, k, True, functools.partial(_swap(rollout_ref, dt, k), env, n, h)) for n, h in ROLLOUT_SIZES]
        if env in GMM_ENVS:
            sets.append((f"gmm N128 H20 {c}", 20, dt, k, True, functools.partial(_swap(gmm_ref, dt, k), env, 128, 20, 16)))
    if env == "CartPole":
        for dt, k in TP_CONFIGS:
            sets += [(f"throughput p{p} dt{dt} k{k}", L.TP_H, dt, k, False, functools.partial(_swap(mppi_ref, dt, k), env, L.TP_N, L.TP_H, p)) for p in (1, 2)]
    return sets
