"""The optimizers' own hyper-parameters (the fields of ctk_config) moved away from their defaults, shared by test_hyper_cases_cpu.py (which
guards the cases) and test_gpu_hyper.py (which feeds them to the kernels).  A plain module, not a conftest.

The rest of the suite runs MPPI at cc_weight = R = 1, LBD 100, NU 1000, SQRTRHOINV 0.03, Adam at 0.9 / 0.999 / 1e-8 with a clip that never
binds, CEM between symmetric limits with a clamp that rarely binds.  The library pre-combines these values (mppi_constants -> MppiK, the
Adam constants) and the oracle repeats the combinations, so this module states the optimizer arithmetic a THIRD time:

OptimF64   float64, from the PRIMARY hyper-parameters alone (rounded to float32 first, as they cross the C ABI): the MPPI correction cost
           and soft-min update with the clip, CEM's refit / clamp / shift / tail refill, clip_by_norm, both Adam rules (the in-repo torch
           rule of the reference and the published Keras rule), the two sampling maps and the warm start (plans shifted by shift_previous,
           moments by ONE step).  No pre-combined constant of mppi_constants, of the Adam constants or of the oracle is used or named.
           The plant's cost is param_cases.PlantF64's.

FIXTURES   the names of the reference recordings at these values (tests/golden/make_golden.py: record_hyper_cases).

MPPI_SINGLE / CEM_SINGLE / RPGD_SINGLE   one case ((name, value), ...) per hyper-parameter; *_ALL moves every one at once.  "limits": "asym"
           stands for ASYM[env].  The states are near the target (STATE), where the correction cost is a visible share of J: at the
           suite's usual CartPole state (angle 2.6, J ~ 1.8e4) a kernel that ignored cc_weight, R or NU altogether stays within two bounds.

The reference builders are cached and their results are left unchanged by every test."""
import functools

import numpy as np

from oracle import ctk_oracle as O
import large_angle_cases as L
import param_cases as P

f32 = np.float32
ENVS = L.ENVS
DT = P.DT

# ---- the reference recordings ---------------------------------------------------------------------------------------------------------
MPPI_FIXTURES = [f"{h}_{e}" for h in ("hyper_all", "hyper_saturated") for e in ("cartpole", "cartpole_mlp", "quad2d", "hover")]
RPGD_FIXTURES = ["hyper_normal_cartpole", "hyper_normal_cartpole_mlp", "hyper_normal_quad2d", "hyper_uniform_cartpole", "hyper_uniform_quad2d"]
RPGD_KEEP_ALL_FIXTURE = "hyper_keep_all"                    # opt_keep_k_ratio 1.0: k = N, no fresh rows on a resampling step
CEM_FIXTURES = ["hyper_cartpole", "hyper_hover"]
RANDOM_FIXTURES = ["hyper_cartpole", "hyper_hover"]
CEM_NAIVE_GRAD_FIXTURES = ["hyper_cartpole", "hyper_quad2d"]

# ---- limits and states ------------------------------------------------------------------------------------------------------------------
# (tighter than the recordings' [-0.3, 0.9]: with MPPI's default stdev of 0.21 and a period of 5 most rollouts must touch a limit for the
# case to show in J)
ASYM = {"CartPole": (np.array([-0.15], f32), np.array([0.4], f32)),
        "Quad2D": (np.array([-0.2, -0.3], f32), np.array([0.35, 0.15], f32)),
        "Hover": (np.array([-0.25, -0.1, -0.3], f32), np.array([0.15, 0.3, 0.2], f32))}
# near the target: J 5 .. 100, so that the correction cost is a visible share of it
STATE = {"CartPole": np.array([0.02, -0.05, 0.05, 0.1], f32), "Quad2D": np.array([0.16, -0.1, 0.94, 0.08, 0.1, -0.2], f32),
         "Hover": np.array([0.26, -0.08, -0.14, 0.06, 0.15, -0.1, 0.4], f32)}
# LBD shows in the update only where the costs spread over about LBD or more: the LBD cases start further out (J spread of hundreds)
STATE_LBD = {"CartPole": np.array([0.06, -0.12, 0.15, 0.3], f32), "Quad2D": np.array([0.7, -0.3, 0.4, 0.3, 0.3, -0.4], f32),
             "Hover": np.array([1.1, -0.3, 0.7, 0.3, 0.5, -0.3, 0.4], f32)}
# (the same states serve RPGD's clip that never binds: every fresh plan's gradient there is longer than the defaults' clip of 5, so the
# defaults clip every row and the case clips none)
U_PREV = 0.05


def is_far(own):
    return bool(own) and all(k == "LBD" for k, _ in own)


def state_of(env, own=(), far=False):
    return (STATE_LBD if far or is_far(own) else STATE)[env].copy()


def limits_of(env, own=()):
    return ASYM[env] if dict(own).get("limits") == "asym" else L.LIMITS[env]


def config_of(defaults, own):
    """the keyword arguments of a case: the defaults with the case's values, without the limits"""
    return dict(defaults, **{k: v for k, v in own if k != "limits"})


def case_id(own, everything):
    return "ALL" if own == everything else "defaults" if own == () else ",".join(f"{k}={v}" for k, v in own)


def plan0(env, H):
    """the plan every MPPI case starts from: smooth, non-zero (so that R u delta_u counts) and inside every set of limits"""
    C = L.LIMITS[env][0].size
    h, c = np.arange(H, dtype=np.float64)[:, None], np.arange(C, dtype=np.float64)[None, :]
    return (0.12 * np.cos(0.4 * h + 0.9 * c) + 0.05).astype(f32)


# ---- MPPI -----------------------------------------------------------------------------------------------------------------------------------
MPPI_DEFAULTS = dict(cc_weight=1.0, R=1.0, LBD=100.0, NU=1000.0, SQRTRHOINV=0.03)
MPPI_SINGLE = [(("cc_weight", 0.37),), (("R", 2.3),), (("NU", 2.0),), (("NU", 0.5),), (("LBD", 10.0),), (("LBD", 1000.0),), (("SQRTRHOINV", 0.2),),
               (("limits", "asym"),)]
MPPI_ALL = (("cc_weight", 0.37), ("R", 2.3), ("LBD", 30.0), ("NU", 2.0), ("SQRTRHOINV", 0.08), ("limits", "asym"))
MPPI_SATURATED = (("cc_weight", 0.37), ("R", 2.3), ("LBD", 30.0), ("NU", 2.0), ("SQRTRHOINV", 0.2), ("limits", "asym"))
MPPI_CASES = MPPI_SINGLE + [MPPI_ALL, MPPI_SATURATED]
MPPI_SIZES = [(64, 20, 5), (128, 20, 1)]                # (N, H, period): (H - 1) % 5 != 0; two tiles at period 1
NET_SIZE = (48, 15, 4)
TWO_TILE_SIZE = (4128, 10, 4)                           # 258 full tiles: the smallest N at which the template's split MLP rollout puts two tiles in a workgroup
# the tensor a single-value case is compared in
MPPI_SHOWS_IN = {"cc_weight": "J", "R": "J", "NU": "J", "SQRTRHOINV": "J", "limits": "J", "LBD": "u_nom"}


def mppi_id(own):
    return "saturated" if own == MPPI_SATURATED else case_id(own, MPPI_ALL)


def u_bound(LBD, rtol=1e-4, atol=2e-5):
    """the suite's u / U_NOM bound (test_gpu_mppi.U_TOL by default) assumes LBD = 100: the soft-min turns a cost error dJ into a relative
    weight error dJ / LBD.  Below 100 it scales by 100 / LBD; at and above 100 it is unchanged."""
    k = max(1.0, 100.0 / float(LBD))
    return dict(rtol=rtol * k, atol=atol * k)


def mppi_oracle(env, own, N, H, p, predictor=None):
    pars = L.env_params(env)
    lo, hi = limits_of(env, own)
    pred = predictor if predictor is not None else O.Predictor("ODE", dt=DT, env=pars)
    return O.MPPI(pred, O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, **config_of(MPPI_DEFAULTS, own))


def mppi_noise(env, N, H, p):
    C = L.LIMITS[env][0].size
    return np.random.default_rng(1000 * N + 10 * H + p).standard_normal((N, O.num_inducing_points(H, p), C)).astype(f32)


@functools.lru_cache(maxsize=None)
def mppi_ref(env, own, N, H, p, far=False):
    """one oracle MPPI step of a case from its state (state_of: STATE[env]; STATE_LBD[env] for the LBD cases and where `far`), plan0 and
    u_prev = U_PREV"""
    o = mppi_oracle(env, own, N, H, p)
    return _mppi_step(o, env, own, N, H, p, far)


def _mppi_step(o, env, own, N, H, p, far=False):
    C = o.C
    start = np.clip(plan0(env, H), o.low, o.high).astype(f32)
    o.u_nom = start[None].copy()
    o.u = O._u_out(np.full(C, U_PREV, f32))
    noise, s = mppi_noise(env, N, H, p), state_of(env, own, far)
    u = np.asarray(o.step(s, noise), f32).reshape(-1)
    return dict(s=s, noise=noise, plan0=start, u_prev=np.full(C, U_PREV, f32), u=u, J=o.J, Q=o.u_run, traj=o.rollout_trajectories, u_nom=o.u_nom,
                delta_u=o.delta_u)


@functools.lru_cache(maxsize=None)
def net_mppi_ref(env, kind, own, hidden=(32, 32), size=NET_SIZE):
    """the same step through a network predictor (zero hidden state)"""
    N, H, p = size
    pars = L.env_params(env)
    if kind == "MLP" and hidden != (32, 32):
        w = O.mlp_default_weights(9, pars.S + pars.C, pars.S, hidden)
        pred = O.Predictor("MLP", dt=DT, env=pars, weights=w, hidden_sizes=hidden)
    else:
        w = P.net_weights(env, kind)
        pred = O.Predictor(kind, dt=DT, env=pars, weights=w)
    r = _mppi_step(mppi_oracle(env, own, N, H, p, pred), env, own, N, H, p)
    r["weights"] = w
    return r


# ---- CEM ------------------------------------------------------------------------------------------------------------------------------------
CEM_DEFAULTS = dict(cem_outer_it=2, cem_best_k=16, cem_initial_action_stdev=0.5, cem_stdev_min=0.01)
CEM_SINGLE = [(("cem_stdev_min", 0.4), ("cem_best_k", 2)), (("cem_initial_action_stdev", 1.3),), (("limits", "asym"),)]
CEM_ALL = (("cem_stdev_min", 0.4), ("cem_best_k", 2), ("cem_initial_action_stdev", 1.3), ("limits", "asym"))
CEM_CASES = CEM_SINGLE + [CEM_ALL]
CEM_SIZES = [(100, 20), (128, 20)]


def cem_id(own):
    return case_id(own, CEM_ALL)


@functools.lru_cache(maxsize=None)
def cem_ref(env, own, N, H, variant=0):
    """one oracle CEM step from STATE[env].  variant 1 / 2: the same draws with the rollouts in reverse order / with the other sign (the
    problems of a batch)"""
    pars = L.env_params(env)
    lo, hi = limits_of(env, own)
    kw = config_of(CEM_DEFAULTS, own)
    o = O.CEM(O.Predictor("ODE", dt=DT, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, **kw)
    C = o.C
    noise = np.random.default_rng(77 + N).standard_normal((kw["cem_outer_it"], N, H, C)).astype(f32)
    noise = (noise, noise[:, ::-1].copy(), -noise)[variant]
    s = STATE[env].copy()
    u = np.asarray(o.step(s, noise), f32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.Q, traj=o.rollout_trajectories, mu=o.dist_mue, std=o.stdev, best=o.best_idx, kw=kw, lo=lo, hi=hi)


# ---- RPGD -----------------------------------------------------------------------------------------------------------------------------------
RPGD_DEFAULTS = dict(outer_its=3, resamp_per=2, shift_previous=1, opt_keep_k_ratio=0.25, SAMPLING_DISTRIBUTION="uniform", sample_whole_control_space=True,
                     sample_stdev=0.5, sample_mean=0.0, uniform_dist_min=-1.0, uniform_dist_max=1.0, learning_rate=0.05, gradmax_clip=5.0,
                     adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-8)
RPGD_N, RPGD_H, RPGD_P = 32, 20, 5
RPGD_SINGLE = [(("learning_rate", 0.2),), (("adam_beta_1", 0.7),), (("adam_beta_2", 0.9),), (("adam_epsilon", 1e-2),),
               (("gradmax_clip", 0.05),), (("gradmax_clip", 1e9),),
               (("shift_previous", 0),), (("shift_previous", 2),), (("shift_previous", RPGD_H - 1),),
               (("SAMPLING_DISTRIBUTION", "normal"), ("sample_mean", 0.3), ("sample_stdev", 0.8)),
               (("sample_whole_control_space", False), ("uniform_dist_min", -0.6), ("uniform_dist_max", 0.2), ("limits", "asym"))]
RPGD_ALL = (("learning_rate", 0.2), ("adam_beta_1", 0.7), ("adam_beta_2", 0.9), ("adam_epsilon", 1e-3), ("gradmax_clip", 0.05), ("shift_previous", 2),
            ("SAMPLING_DISTRIBUTION", "normal"), ("sample_mean", 0.3), ("sample_stdev", 0.8), ("limits", "asym"))
RPGD_CASES = RPGD_SINGLE + [RPGD_ALL]
RPGD_CLIP_NEVER = (("gradmax_clip", 1e9),)               # starts from STATE_LBD, where the defaults' clip binds on every row
# the tensors a single-value case must show in (after the first step, which resamples, or the second, which does not)
ADAM_NAMES = ("learning_rate", "adam_beta_1", "adam_beta_2", "adam_epsilon", "gradmax_clip")


def rpgd_id(own):
    return case_id(own, RPGD_ALL)


RPGD_NET_N = 48                                          # CartPole's MLP: more than one workgroup's worth of plans, the one-launch (persistent) descent


def rpgd_oracle(env, own, adam_rule="torch", predictor=None, N=RPGD_N, H=RPGD_H, p=RPGD_P):
    pars = L.env_params(env)
    lo, hi = limits_of(env, own)
    pred = predictor if predictor is not None else O.Predictor("ODE", dt=DT, env=pars)
    return O.RPGD(pred, O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, adam_rule=adam_rule,
                  **config_of(RPGD_DEFAULTS, own))


RPGD_SEED = 31


def rpgd_draws(env, own, N=RPGD_N, H=RPGD_H, p=RPGD_P, seed=RPGD_SEED):
    """(reset draws [N, P, C], resampling draws [N - k, P, C]): standard normal or U[0, 1), as the case samples"""
    C, Pn = L.LIMITS[env][0].size, O.num_inducing_points(H, p)
    rng = np.random.default_rng(seed)
    k = int(max(int(N * config_of(RPGD_DEFAULTS, own)["opt_keep_k_ratio"]), 1))
    if config_of(RPGD_DEFAULTS, own)["SAMPLING_DISTRIBUTION"] == "normal":
        return rng.standard_normal((N, Pn, C)).astype(f32), rng.standard_normal((N - k, Pn, C)).astype(f32)
    return rng.random((N, Pn, C), dtype=f32), rng.random((N - k, Pn, C), dtype=f32)


def rpgd_state_of(env, own=(), far=False):
    return (STATE_LBD if far or own == RPGD_CLIP_NEVER else STATE)[env].copy()


@functools.lru_cache(maxsize=None)
def rpgd_ref(env, own, adam_rule="torch", kind="ODE", far=False, seed=RPGD_SEED):
    """two oracle steps from rpgd_state_of (STATE[env]; STATE_LBD[env] for the clip that never binds and where `far`): the first resamples
    (count 0), the second does not (resamp_per 2).  Per step: the descended
    population, J, the best rows, and the state after the warm start (plans, moments, ages, u).  The second step starts from the first's
    own state.  `seed`: of the draws (the problems of a batch).  kind "MLP" / "GRU": through param_cases.net_weights' network (zero hidden state), RPGD_NET_N plans."""
    N = RPGD_N if kind == "ODE" else RPGD_NET_N
    pred = None if kind == "ODE" else O.Predictor(kind, dt=DT, env=L.env_params(env), weights=P.net_weights(env, kind))
    o = rpgd_oracle(env, own, adam_rule, pred, N)
    d0, d1 = rpgd_draws(env, own, N, seed=seed)
    o.optimizer_reset(d0)
    o.u = O._u_out(np.full(o.C, U_PREV, f32))
    s, steps = rpgd_state_of(env, own, far), []
    for t in range(2):
        before = dict(Q=o.Q.copy(), m=None if o.opt.m is None else o.opt.m.copy(), v=None if o.opt.v is None else o.opt.v.copy(),
                      ages=o.trajectory_ages.copy(), u=np.asarray(o.u, f32).reshape(-1).copy(), adam_step=o.opt.step_count, count=o.count)
        u = np.asarray(o.step(s, d1 if t == 0 else None), f32).reshape(-1)
        steps.append(dict(before=before, u=u, J=o.J, descended=o.Q_before_warmstart, best=o.best_idx, Q=o.Q.copy(), m=o.opt.m.copy(), v=o.opt.v.copy(),
                          ages=o.trajectory_ages.copy(), u_nom=o.u_nom.copy(), adam_step=o.opt.step_count, count=o.count))
    return dict(s=s, reset_draws=d0, resample_draws=d1, Q_init=steps[0]["before"]["Q"], steps=steps, k=o.k, lo=o.low, hi=o.high, N=N,
                weights=None if kind == "ODE" else pred.weights)


# ---- CEM-GMM ----------------------------------------------------------------------------------------------------------------------------------
GMM_ENVS = ("CartPole", "Quad2D")
GMM_KW = dict(cem_outer_it=2, cem_best_k=16, cem_initial_action_stdev=1.3, cem_stdev_min=0.2)
GMM_SEED = {"CartPole": 5, "Quad2D": 5}                   # of the draws: the restatement's own cluster labels have no near-tie (asserted)


@functools.lru_cache(maxsize=None)
def gmm_ref(env, N=128, H=20):
    """one step of the CEM-GMM restatement between ASYM[env]: a saturating initial deviation and a clamp that binds on the mixture's deviations"""
    from gmm_oracle import CEMGMM
    pars = L.env_params(env)
    lo, hi = ASYM[env]
    o = CEMGMM(O.Predictor("ODE", dt=DT, env=pars), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H, **GMM_KW)
    rng = np.random.default_rng(GMM_SEED[env])
    normals = rng.standard_normal((GMM_KW["cem_outer_it"], N, H, o.C)).astype(f32)
    uniforms = rng.random((GMM_KW["cem_outer_it"], N), dtype=f32)
    s = STATE[env].copy()
    u = np.asarray(o.step(s, normals, uniforms), f32).reshape(-1)
    return dict(s=s, normals=normals, uniforms=uniforms, u=u, Q=o.Q, J=o.J, mu=o.dist_mue, std=o.stdev, probs=o.probs, best=o.best_idx, labels=o.labels,
                min_margin=o.min_margin, min_cost_gap=o.min_cost_gap, lo=lo, hi=hi)


# ---- the float64 statement --------------------------------------------------------------------------------------------------------------------
def _r(x):
    """a hyper-parameter as it crosses the C ABI: a float32"""
    return float(f32(x))


class OptimF64:
    """see the module's docstring.  numpy float64 throughout; inputs are the float32 arrays of a step (draws, plans, gradients, costs)."""

    # -- interpolation: the reference's matrix, applied in float64 --
    @staticmethod
    def interpolate(y, H, period):
        M = O.interpolation_matrix(H, period, y.shape[2]).astype(np.float64)                  # [P, H, C]
        return np.einsum("npc,phc->nhc", np.asarray(y, np.float64), M)

    # -- MPPI --
    @staticmethod
    def mppi_perturbation(noise, SQRTRHOINV, dt, H, period):
        """delta_u [N, H, C]: draws times SQRTRHOINV / sqrt(dt), interpolated"""
        return OptimF64.interpolate(np.asarray(noise, np.float64) * (_r(SQRTRHOINV) / np.sqrt(_r(dt))), H, period)

    @staticmethod
    def mppi_inputs(plan, delta_u, lo, hi):
        """(the plan shifted by one step repeating its last input [1, H, C], the clipped inputs of every rollout [N, H, C])"""
        plan = np.asarray(plan, np.float64).reshape(1, *np.shape(plan)[-2:])
        shifted = np.concatenate([plan[:, 1:], plan[:, -1:]], 1)
        return shifted, np.clip(shifted + delta_u, np.asarray(lo, np.float64), np.asarray(hi, np.float64))

    @staticmethod
    def mppi_correction(u, delta_u, cc_weight, R, NU):
        """[N]: cc_weight * sum over the horizon and the inputs of  (1 - 1 / NU) / 2 * R * delta_u^2  +  R * u * delta_u  +  R / 2 * u^2,
        u the CLIPPED input and delta_u the UNCLIPPED perturbation"""
        cc, R, NU = _r(cc_weight), _r(R), _r(NU)
        return cc * ((1.0 - 1.0 / NU) / 2.0 * R * delta_u ** 2 + R * u * delta_u + R / 2.0 * u ** 2).sum(axis=(1, 2))

    @staticmethod
    def mppi_update(shifted, J, delta_u, LBD, lo, hi):
        """[1, H, C]: clip(shifted plan + sum_n w_n delta_u_n / sum_n w_n), w_n = exp(-(J_n - min J) / LBD)"""
        J = np.asarray(J, np.float64)
        w = np.exp(-(J - J.min()) / _r(LBD))
        return np.clip(shifted + np.einsum("n,nhc->hc", w, delta_u)[None] / w.sum(), np.asarray(lo, np.float64), np.asarray(hi, np.float64))

    @staticmethod
    def mppi_step(env, pars, cfg, lo, hi, H, period, plan, u_prev, noise, traj, dt=DT):
        """(J [N], u_nom [1, H, C], Q [N, H, C]) of one step; the plant's cost is PlantF64's on the given (float32) trajectories"""
        du = OptimF64.mppi_perturbation(noise, cfg["SQRTRHOINV"], dt, H, period)
        shifted, Q = OptimF64.mppi_inputs(plan, du, lo, hi)
        plant = P.PlantF64(env, pars, dt)
        J = plant.trajectory_cost(np.asarray(traj, np.float64), Q, u_prev).numpy() + OptimF64.mppi_correction(Q, du, cfg["cc_weight"], cfg["R"], cfg["NU"])
        return J, OptimF64.mppi_update(shifted, J, du, cfg["LBD"], lo, hi), Q

    # -- CEM --
    @staticmethod
    def cem_finish(elite, stdev_min, initial_stdev, lo, hi, stdev_max=1.0e8):
        """(mean [1, H, C], stdev [1, H, C]) after a step: the elites' mean and population standard deviation, the deviation clamped to
        [stdev_min, stdev_max], both shifted by one step; the mean's tail is refilled with the MIDDLE of the limits, the deviation's with the
        initial one"""
        e = np.asarray(elite, np.float64)
        mu = e.mean(axis=0, keepdims=True)
        sd = np.clip(np.sqrt(((e - mu) ** 2).mean(axis=0, keepdims=True)), _r(stdev_min), stdev_max)
        mid = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2.0
        C = e.shape[2]
        return (np.concatenate([mu[:, 1:], np.broadcast_to(mid, (C,)).reshape(1, 1, C)], 1),
                np.concatenate([sd[:, 1:], np.full((1, 1, C), _r(initial_stdev))], 1))

    # -- the gradient family --
    @staticmethod
    def clip_by_norm(g, clip):
        """every rollout's gradient [H, C] scaled down to norm `clip` where it is longer"""
        g = np.asarray(g, np.float64)
        norm = np.sqrt((g ** 2).sum(axis=(1, 2), keepdims=True))
        return g * (_r(clip) / np.maximum(norm, _r(clip)))

    @staticmethod
    def adam_torch(g, var, m, v, t, lr, b1, b2, eps):
        """the reference's in-repo rule, iteration t (1-based): bias-corrected moments, epsilon OUTSIDE the corrected root"""
        lr, b1, b2, eps = float(lr), float(b1), float(b2), float(eps)
        m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
        v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g ** 2
        return np.asarray(var, np.float64) - lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps), m, v

    @staticmethod
    def adam_keras(g, var, m, v, t, lr, b1, b2, eps):
        """the published Keras rule: the corrections folded into the step size, epsilon beside the UNCORRECTED root"""
        lr, b1, b2, eps = float(lr), float(b1), float(b2), float(eps)
        m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
        v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g ** 2
        return np.asarray(var, np.float64) - lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) * m / (np.sqrt(v) + eps), m, v

    @staticmethod
    def descent_iteration(rule, g, Q, m, v, t, kw, lo, hi):
        """one iteration of the descent: clip the gradient's norm, one Adam step, clip to the limits"""
        fn = OptimF64.adam_keras if rule == "keras" else OptimF64.adam_torch
        Qn, m, v = fn(OptimF64.clip_by_norm(g, kw["gradmax_clip"]), Q, m, v, t, kw["learning_rate"], kw["adam_beta_1"], kw["adam_beta_2"], kw["adam_epsilon"])
        return np.clip(Qn, np.asarray(lo, np.float64), np.asarray(hi, np.float64)), m, v

    @staticmethod
    def sample(draws, kw, lo, hi, H, period):
        """fresh plans [n, H, C] from draws [n, P, C]: normal draws times sample_stdev plus sample_mean, or U[0, 1) draws mapped onto
        [min, max) (the limits when sample_whole_control_space), clipped to the limits, interpolated"""
        d = np.asarray(draws, np.float64)
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        if kw["SAMPLING_DISTRIBUTION"] == "normal":
            y = d * _r(kw["sample_stdev"]) + _r(kw["sample_mean"])
        else:
            a, b = (lo, hi) if kw["sample_whole_control_space"] else (_r(kw["uniform_dist_min"]), _r(kw["uniform_dist_max"]))
            y = d * (b - a) + a
        return OptimF64.interpolate(np.clip(y, lo, hi), H, period)

    @staticmethod
    def warm_start(Q, m, v, ages, best, fresh, shift_previous):
        """(plans, m, v, ages) of the next step.  Plans are shifted by shift_previous steps repeating the last input; the moments by ONE step,
        zero-filled; `fresh` [N - k, H, C] (a resampling step) replaces all but the k best rows, which move to the end in order of cost,
        with zero moments and age 0; every age then grows by one."""
        Q, m, v, ages = (np.asarray(a, np.float64) for a in (Q, m, v, ages))
        sp = int(shift_previous)
        Qs = np.concatenate([Q[:, sp:], np.repeat(Q[:, -1:], sp, axis=1)], 1)
        z = np.zeros_like(m[:, :1])
        ms, vs = np.concatenate([m[:, 1:], z], 1), np.concatenate([v[:, 1:], z], 1)
        if fresh is not None:
            n = fresh.shape[0]
            Qs = np.concatenate([np.asarray(fresh, np.float64), Qs[best]], 0)
            ms, vs = (np.concatenate([np.zeros((n,) + a.shape[1:]), a[best]], 0) for a in (ms, vs))
            ages = np.concatenate([np.zeros(n), ages[best]])
        return Qs, ms, vs, ages + 1.0
