"""Every plant and cost parameter moved away from its default, shared by test_param_cases_cpu.py (which guards the cases) and
test_gpu_params.py (which feeds them to every kernel).  A plain module, not a conftest.

Every kernel consumes float32 constants that the library derives from the environment's primary parameters (csrc/ctk_common.h:
derive_constants, csrc/ctk_env.h: Env<ENV>::derive, the batches' per-problem derivation), and oracle/ctk_oracle.py repeats those
derivations "by the same expressions".  A wrong expression shared by the two is invisible to a comparison of the two, so this module
states the plants and costs a THIRD time:

PlantF64   one predictor step, the stage cost, the terminal cost and the trajectory cost (mean over H + 1) in float64, written from the
           PRIMARY parameters alone: masses, lengths, thrusts and weights appear as themselves, in the textbook form of each plant, and no
           derived constant of the library or of the oracle is used or named.  The parameters are rounded to float32 first, as they cross
           the C ABI.  Two forms: rollout() runs free in float64 (for autograd), rollout(rounded=True) steps the float32 state in float64
           and rounds after every step (what large_angle_cases.StepF64 does with the oracle's own expressions), for comparison with the
           float32 oracle.

CASES[env] one case ((name, value),) per parameter: the library default x 1.37 (not a power of two, so a missing or doubled factor shows), 0.07
           where the default is 0, and -1 as a second value of CartPole's target_equilibrium.  Some parameters take a larger value:
           test_param_cases_cpu.py's sensitivity guard decides (OVERRIDES below).  ALL[env] moves every parameter at once, cc_weight != R.

"Without the perturbation" means large_angle_cases.env_params(env): the defaults plus a terminal weight and a target, so that the terminal
cost and the target count in every case.  State, plans and draws are the large-angle file's: substep_cases.ORDINARY[0], draws_for,
normals_for and their seeds.  The reference builders are cached and their results are left unchanged by every test."""
import functools

import numpy as np

from oracle import ctk_oracle as O
import large_angle_cases as L
import substep_cases as S

f32 = np.float32
ENVS = L.ENVS
STATE = S.ORDINARY[0]                                   # (theta0, omega0) of every case
SIZES = [(100, 20, 5), (128, 20, 1)]                    # MPPI (N, H, period)
CEM_SIZES = [(100, 20), (128, 20)]
ROLLOUT_SIZES = [(100, 20), (128, 20)]
NET_SIZE = (48, 15)                                     # the network predictors' (N, H)
FACTOR = 1.37
FROM_ZERO = 0.07
DT = 0.02

# Seeds of the draws where the large-angle file's own leave a case unusable: (kind, environment, N, H, own) -> seed.  None is needed.
SEEDS = {}

# the first parameters of each environment enter the dynamics, the rest the cost alone
N_DYNAMICS = {"CartPole": 7, "Quad2D": 7, "Hover": 9}

# (environment, name) -> value, where default x 1.37 does not meet the sensitivity guard (test_param_cases_cpu.py) on EVERY set of plans.
#  * The weights of the input terms (cc_weight, R, ccrc_weight): MPPI's plans with period 5 are small and smooth (stdev 0.5, five
#    inducing points), so x 1.37 moves J by 0.06 - 8 bounds there (the other sets: 3 - 1400); the values below move it by 25 or more.
#    cc_weight and R get different values, so that their two cases are two cases.
#  * Hover's wheel: its speed stays below ~2 rad/s from the base state's 0.5, so wheel_friction x 1.37 and wheel_weight x 1.37 stay
#    below 20 bounds on most rows; vel_weight x 1.37 meets the guard on 65 rows of 128, which is too close to call.
OVERRIDES = {("CartPole", "cc_weight"): 41.0, ("CartPole", "R"): 43.0, ("CartPole", "ccrc_weight"): 190.0,
             ("Quad2D", "cc_weight"): 4.1, ("Quad2D", "R"): 4.3, ("Quad2D", "ccrc_weight"): 20.6,
             ("Hover", "cc_weight"): 2.3, ("Hover", "R"): 2.45, ("Hover", "ccrc_weight"): 7.7,
             ("Hover", "wheel_friction"): 0.05 * 12.0, ("Hover", "wheel_weight"): 0.02 * 29.0, ("Hover", "vel_weight"): 6.0 * 1.61}

# (environment, case) -> (theta0, omega0) where the state of every other case makes a case ill-conditioned.  With target_equilibrium = -1
# the angle term is negative; from (0.4, -0.7) one of rollout()'s plans ends at J = 4.6 as a difference of terms of ~3000, where the float32
# oracle and PlantF64 differ by 0.19 of the GPU bound (guard: 0.1).  From (0.2, -0.3) the smallest |J| is 128 and the gap 0.02.
STATE_FOR = {("CartPole", (("target_equilibrium", -1.0),)): (0.2, -0.3)}


def defaults(env):
    return O.ENVIRONMENTS[env]()


def param_names(env):
    return tuple(defaults(env).param_names())


def is_dynamics(env, name):
    return param_names(env).index(name) < N_DYNAMICS[env]


def value_for(env, name):
    d = float(getattr(defaults(env), name))
    return float(f32(OVERRIDES.get((env, name), d * FACTOR if d != 0.0 else FROM_ZERO)))


def _single(env):
    out = [((n, value_for(env, n)),) for n in param_names(env)]
    if env == "CartPole":
        out.append((("target_equilibrium", -1.0),))
    return out


def _all(env):
    """every parameter away from its default at once: its single case's value (OVERRIDES included, so that the tests which run ALL alone
    see the input weights and the wheel as well) times a factor that differs from name to name (0.87 .. 1.17), cc_weight != R"""
    return tuple((n, float(f32(value_for(env, n) * (0.87 + 0.05 * (i % 7))))) for i, n in enumerate(param_names(env)))


SINGLE = {env: _single(env) for env in ENVS}
ALL = {env: _all(env) for env in ENVS}
CASES = {env: SINGLE[env] + [ALL[env]] for env in ENVS}


# the library's defaults, written as a case (params_with() starts from env_params(), which sets a terminal weight and a target)
DEFAULTS = {env: tuple((n, float(getattr(defaults(env), n))) for n in param_names(env)
                       if float(getattr(defaults(env), n)) != float(getattr(L.env_params(env), n))) for env in ENVS}


def case_id(env, own):
    return "ALL" if own == ALL[env] else "defaults" if own == DEFAULTS[env] else "base" if own == () else f"{own[0][0]}={own[0][1]:.6g}"


def cost_cases(env):
    """the cases a network predictor sees: single cost parameters, and ALL"""
    return [own for own in CASES[env] if own == ALL[env] or not is_dynamics(env, own[0][0])]


def params_with(env, own):
    return L.params_with(env, own)


def state_of(env, own=()):
    """(theta0, omega0) of a case"""
    return STATE_FOR.get((env, own), STATE)


def base_state(env, own=()):
    return L.base_state(env, *state_of(env, own))


# ---- the float64 statement ------------------------------------------------------------------------------------------------------------
class PlantF64:
    """see the module's docstring.  States [N, S], inputs [N, C], torch float64 throughout (numpy arrays are accepted and converted)."""

    def __init__(self, env, params, dt=DT):
        import torch
        self.torch, self.env = torch, env
        self.S, self.C = params.S, params.C
        self.dt = float(f32(dt))                                           # the handle's dt is a float32 in the C ABI
        for n in params.param_names():
            setattr(self, n, float(f32(getattr(params, n))))               # the primary parameters, as they cross the ABI

    def T(self, a):
        t = self.torch
        return a if isinstance(a, t.Tensor) else t.tensor(np.asarray(a, np.float64))

    # -- dynamics: explicit Euler, every derivative taken at the old state --
    def derivative(self, s, u):
        t = self.torch
        if self.env == "CartPole":
            # cart of mass m_cart on a track with viscous friction M_fric, uniform pole of mass m_pole and HALF length L on a joint with
            # friction J_fric, force u_max * u on the cart (the classic cart-pole equations with both friction terms)
            x, v, th, om = s.unbind(1)
            F = self.u_max * u[:, 0]
            m_total = self.m_cart + self.m_pole
            sn, cs = t.sin(th), t.cos(th)
            push = (F + self.m_pole * self.L * om ** 2 * sn - self.M_fric * v) / m_total
            thdd = (self.g * sn - cs * push - self.J_fric * om / (self.m_pole * self.L)) / (self.L * (4.0 / 3.0 - self.m_pole * cs ** 2 / m_total))
            xdd = (F + self.m_pole * self.L * (om ** 2 * sn - thdd * cs) - self.M_fric * v) / m_total
            return t.stack([v, xdd, om, thdd], 1)
        if self.env == "Quad2D":
            # two rotors at distance arm from the centre, each of thrust (mass g / 2) (1 + thrust_gain u_i); drag on the velocities
            x, vx, z, vz, th, om = s.unbind(1)
            T1 = 0.5 * self.mass * self.g * (1.0 + self.thrust_gain * u[:, 0])
            T2 = 0.5 * self.mass * self.g * (1.0 + self.thrust_gain * u[:, 1])
            lift = (T1 + T2) / self.mass
            ax = -lift * t.sin(th) - self.drag_lin * vx
            az = lift * t.cos(th) - self.g - self.drag_lin * vz
            al = self.arm * (T1 - T2) / self.inertia - self.drag_ang * om
            return t.stack([vx, ax, vz, az, om, al], 1)
        # hovercraft: main thruster along the body axis, lateral thruster across it, a reaction wheel whose torque reacts on the body
        x, vx, y, vy, th, om, w = s.unbind(1)
        main, side, torque = self.thrust_max * u[:, 0], self.lateral_max * u[:, 1], self.torque_max * u[:, 2]
        sn, cs = t.sin(th), t.cos(th)
        ax = (main * cs - side * sn) / self.mass - self.drag_lin * vx
        ay = (main * sn + side * cs) / self.mass - self.drag_lin * vy
        al = -torque / self.inertia - self.drag_ang * om
        aw = torque / self.wheel_inertia - self.wheel_friction * w
        return t.stack([vx, ax, vy, ay, om, al, aw], 1)

    def step(self, s, u):
        s, u = self.T(s), self.T(u)
        return s + self.dt * self.derivative(s, u)

    def rollout(self, s0, Q, rounded=False):
        """[N, H + 1, S] from s0 [S] or [N, S] and plans Q [N, H, C]; rounded: the state is rounded to float32 after every step"""
        t = self.torch
        Q = self.T(Q)
        s = self.T(np.asarray(s0, np.float64)) if not isinstance(s0, t.Tensor) else s0
        if s.dim() == 1:
            s = s.unsqueeze(0).repeat(Q.shape[0], 1)
        out = [s]
        for h in range(Q.shape[1]):
            s = self.step(s, Q[:, h, :])
            if rounded:
                s = s.to(t.float32).to(t.float64)
            out.append(s)
        return t.stack(out, 1)

    # -- cost --
    def state_cost(self, s):
        """the part that the terminal cost weighs: distance to the target and attitude"""
        t = self.torch
        if self.env == "CartPole":
            # the reference's cost template: target_equilibrium * 0.25 * (1 - cos(angle)) ** 2, weighed by ep_weight
            dd = self.dd_weight * ((s[..., 0] - self.target_position) / self.x_scale) ** 2
            ep = self.ep_weight * self.target_equilibrium * 0.25 * (1.0 - t.cos(s[..., 2])) ** 2
            return dd + ep
        second = self.target_z if self.env == "Quad2D" else self.target_y
        dist2 = ((s[..., 0] - self.target_x) / self.pos_scale) ** 2 + ((s[..., 2] - second) / self.pos_scale) ** 2
        return self.pos_weight * dist2 + self.ang_weight * (1.0 - t.cos(s[..., 4]))

    def stage_cost(self, s, u, u_before):
        """s [N, H, S], u [N, H, C], u_before [N, H, C] = the input applied one step earlier"""
        if self.env == "CartPole":
            motion = self.ekp_weight * s[..., 3] ** 2
        else:
            motion = self.vel_weight * (s[..., 1] ** 2 + s[..., 3] ** 2) + self.angvel_weight * s[..., 5] ** 2
            if self.env == "Hover":
                motion = motion + self.wheel_weight * s[..., 6] ** 2
        effort = self.cc_weight * self.R * (u ** 2).sum(-1) + self.ccrc_weight * ((u - u_before) ** 2).sum(-1)
        return self.state_cost(s) + motion + effort

    def terminal_cost(self, s):
        return self.terminal_weight * self.state_cost(s)

    def trajectory_cost(self, traj, Q, u_prev):
        """[N]: the mean over the H stage costs and the terminal cost"""
        t = self.torch
        traj, Q = self.T(traj), self.T(Q)
        first = self.T(np.asarray(u_prev, np.float64).reshape(1, 1, self.C)).expand(Q.shape[0], 1, self.C)
        before = t.cat([first, Q[:, :-1, :]], 1)
        stage = self.stage_cost(traj[:, :-1, :], Q, before)
        return (stage.sum(1) + self.terminal_cost(traj[:, -1, :])) / (Q.shape[1] + 1)


def plant_check(env, own, s, Q, u_prev):
    """(TRAJ, J) of the stepwise-rounded float64 statement for the plans Q from state s, as numpy float64"""
    plant = PlantF64(env, params_with(env, own))
    traj = plant.rollout(np.asarray(s, f32), np.asarray(Q, f32), rounded=True)
    return traj.numpy(), plant.trajectory_cost(traj, np.asarray(Q, f32), np.asarray(u_prev, f32)).numpy()


# ---- network steps in torch float64 (the cost-parameter cases of the network predictors) -----------------------------------------------
def net_weights(env, kind, seed=1):
    Sn, Cn = defaults(env).S, defaults(env).C
    return O.mlp_default_weights(seed, Sn + Cn, Sn) if kind == "MLP" else O.gru_default_weights(seed, Sn + Cn, Sn)


def net_rollout(env, kind, weights, s0, Q, torch):
    """[N, H + 1, S] float64: the MLP (tanh, tanh, linear) or the two-layer GRU from a zero hidden state, written out"""
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    Sn, Cn = defaults(env).S, defaults(env).C
    N, H = Q.shape[0], Q.shape[1]
    s = T(s0).unsqueeze(0).repeat(N, 1)
    out = [s]
    if kind == "MLP":
        W1, b1, W2, b2, W3, b3 = (T(a) for a in O.mlp_unpack(weights, Sn + Cn, Sn))
        for h in range(H):
            s = torch.tanh(torch.tanh(torch.cat([s, Q[:, h, :]], 1) @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
            out.append(s)
        return torch.stack(out, 1)
    layers, Wo, bo = O.gru_unpack(weights, Sn + Cn, Sn)
    hid = [torch.zeros((N, O.GRU_H), dtype=torch.float64) for _ in range(2)]
    for h in range(H):
        x, new = torch.cat([s, Q[:, h, :]], 1), []
        for (Wi, Wh, bi, bh), hp in zip(layers, hid):
            gi, gh = x @ T(Wi).T + T(bi), hp @ T(Wh).T + T(bh)
            G = O.GRU_H
            r, z = torch.sigmoid(gi[:, :G] + gh[:, :G]), torch.sigmoid(gi[:, G:2 * G] + gh[:, G:2 * G])
            x = (1 - z) * torch.tanh(gi[:, 2 * G:] + r * gh[:, 2 * G:]) + z * hp
            new.append(x)
        hid = new
        s = x @ T(Wo).T + T(bo)
        out.append(s)
    return torch.stack(out, 1)


def grad_inputs(env, N=64, H=20, own=()):
    """(s, Q0 [N, H, C] uniform between the limits, u_prev): what the single-gradient tests start from"""
    lo, hi = L.LIMITS[env]
    Q0 = (lo + (hi - lo) * np.random.default_rng(3).random((N, H, lo.size), dtype=f32)).astype(f32)
    return base_state(env, own), Q0, np.full(lo.size, 0.05, f32)


@functools.lru_cache(maxsize=None)
def grad_ref(env, kind, own, N=64, H=20):
    """(J [N], dJ/dQ [N, H, C]) in float64 by autograd through PlantF64 (kind "ODE") or through the network step above with PlantF64's
    cost (kind "MLP" / "GRU", weights net_weights(env, kind)), free-running, for grad_inputs(env, N, H)"""
    import torch
    s, Q0, up = grad_inputs(env, N, H, own)
    plant = PlantF64(env, params_with(env, own))
    Q = torch.tensor(Q0.astype(np.float64), requires_grad=True)
    traj = plant.rollout(s, Q) if kind == "ODE" else net_rollout(env, kind, net_weights(env, kind), s, Q, torch)
    J = plant.trajectory_cost(traj, Q, up)
    J.sum().backward()
    return J.detach().numpy(), Q.grad.numpy()


# ---- the float32 oracle's results (computed once, shared, left unchanged) ---------------------------------------------------------------
def mppi_ref(env, N, H, p, own=(), predictor=O.Predictor):
    return L.mppi_ref(env, N, H, p, *state_of(env, own), own, 1, predictor)


def cem_ref(env, N, H, own=(), predictor=O.Predictor):
    return L.cem_ref(env, N, H, *state_of(env, own), own, predictor)


def random_ref(env, N, H, own=(), predictor=O.Predictor):
    return S.random_ref(env, N, H, *state_of(env, own), DT, 1, predictor, own)


def rollout_ref(env, N, H, own=(), predictor=O.Predictor):
    return S.rollout_ref(env, N, H, *state_of(env, own), DT, 1, predictor, own)


def gmm_ref(env, own=(), predictor=O.Predictor):
    return S.gmm_ref(env, 128, 20, 16, *state_of(env, own), DT, 1, predictor, own)


@functools.lru_cache(maxsize=None)
def net_mppi_ref(env, kind, own=()):
    """one oracle MPPI step of a network predictor from a zero plan, zero hidden state and u_prev = 0"""
    N, H = NET_SIZE
    pars = params_with(env, own)
    lo, hi = L.LIMITS[env]
    o = O.MPPI(O.Predictor(kind, dt=DT, env=pars, weights=net_weights(env, kind)), O.Cost(pars), lo, hi, num_rollouts=N, mpc_horizon=H,
               period_interpolation_inducing_points=1)
    o.u_nom = np.zeros_like(o.u_nom)
    noise = L.mppi_noise_for(env, N, H, L.PLAIN_SEED[env], o.stdev)
    s = base_state(env, own)
    u = np.asarray(o.step(s, noise), f32).reshape(-1)
    return dict(s=s, noise=noise, u=u, J=o.J, Q=o.u_run, traj=o.rollout_trajectories, u_nom=o.u_nom)


@functools.lru_cache(maxsize=None)
def oracle_grad(env, kind, own, N=64, H=20):
    """(J, dJ/dQ) of the float32 oracle's hand-written reverse mode for grad_inputs(env, N, H)"""
    s, Q0, up = grad_inputs(env, N, H, own)
    pars = params_with(env, own)
    pred = O.Predictor(kind, dt=DT, env=pars, weights=None if kind == "ODE" else net_weights(env, kind))
    J, _, g = O.rollout_cost_and_grad(pred, O.Cost(pars), np.tile(s, (N, 1)), Q0, up)
    return J, g


def inputs_of(env, own):
    """[(label, s, Q, u_prev, oracle TRAJ)] of a case: the plans the GPU file rolls out for it, for the CPU guards"""
    out = []
    for N, H, p in SIZES:
        r = mppi_ref(env, N, H, p, own)
        out.append((f"mppi N{N} H{H} p{p}", r["s"], r["Q"], np.zeros(r["Q"].shape[2], f32), r["traj"]))
    for N, H in CEM_SIZES:
        r = cem_ref(env, N, H, own)
        out.append((f"cem N{N} H{H}", r["s"], r["Q"], np.zeros(r["Q"].shape[2], f32), r["traj"]))
    for N, H in ROLLOUT_SIZES:
        r = rollout_ref(env, N, H, own)
        out.append((f"rollout N{N} H{H}", r["s"], r["Q"], r["u_prev"], r["traj"]))
        r = random_ref(env, N, H, own)
        out.append((f"random N{N} H{H}", r["s"], r["Q"], np.zeros(r["Q"].shape[2], f32), r["traj"]))
    return out
