"""NumPy restatement of the reference's Optimizers/optimizer_cem_gmm_tf.py (CEM with a two-component Gaussian-mixture
sampling distribution), in the style of oracle.ctk_oracle.CEM.  fp32 throughout.

State in the reference's layout: dist_mue / stdev [H,C,2] (components_distribution.mean() / .stddev()), probs [2].
Draw convention (include/ctk_hip.h, block comment above ctk_step): per outer iteration N*H*C standard normals [N,H,C] and
N uniforms in [0,1); rollout n takes component 0 iff uniform[n] < probs[0].  The mixture's Categorical has a scalar batch
shape, so MixtureSameFamily.sample([N]) draws ONE component per rollout and the whole [H,C] plan comes from it (:59)."""
import numpy as np

from oracle.ctk_oracle import Predictor, Cost, argsort_total_order, _limits, _u_out, device_noise, f32   # noqa: F401

UNIFORM_STREAM = 0x40000000   # + outer iteration: Philox stream of the component draws (csrc/ctk_launch.h: CTK_GMM_UNIFORM_STREAM)


class CEMGMM:
    def __init__(self, predictor, cost, low=-1.0, high=1.0, *, num_rollouts, mpc_horizon, cem_outer_it=3,
                 cem_initial_action_stdev=0.5, cem_stdev_min=0.01, cem_best_k=40):
        if cem_best_k < 2:
            raise ValueError("CEM-GMM needs cem_best_k >= 2: with one elite the second cluster is empty (NaN in the reference)")
        self.predictor, self.cost = predictor, cost
        self.N, self.H = num_rollouts, mpc_horizon
        self.S, self.C = predictor.S, predictor.C
        self.low, self.high = _limits(low, high, self.C)
        self.cem_outer_it, self.K = cem_outer_it, cem_best_k
        self.init_std, self.std_min = f32(cem_initial_action_stdev), f32(cem_stdev_min)
        self.u = _u_out(np.zeros(self.C, np.float32))     # Optimizers/__init__.py:35
        self.count = 0
        self.min_margin = np.inf                          # smallest |d0-d1| / (d0+d1) any label was decided by
        self.min_cost_gap = np.inf                        # smallest relative gap between the costs that decide the seeds and the elite set
        self.optimizer_reset()

    def optimizer_reset(self):
        # :131-137 (self.u is not touched)
        mue = ((self.low + self.high) * f32(0.5) * np.ones((self.H, self.C), np.float32)).astype(np.float32)
        std = (self.init_std * np.ones((self.H, self.C), np.float32)).astype(np.float32)
        self.dist_mue = np.stack(2 * [mue], axis=-1)
        self.stdev = np.stack(2 * [std], axis=-1)
        self.probs = np.array([0.5, 0.5], np.float32)
        self.count = 0

    def sample(self, normals, uniforms):
        # :59-60
        comp = np.where(np.asarray(uniforms, np.float32) < self.probs[0], 0, 1)
        mue = np.moveaxis(self.dist_mue, -1, 0)[comp]     # [N,H,C]
        std = np.moveaxis(self.stdev, -1, 0)[comp]
        Q = (mue + np.asarray(normals, np.float32) * std).astype(np.float32)
        return np.clip(Q, self.low, self.high).astype(np.float32), comp

    def update_distribution(self, s_t, normals, uniforms):
        # :57-95
        Q, comp = self.sample(normals, uniforms)
        traj = self.predictor.predict_core(s_t, Q)
        J = self.cost.get_trajectory_cost(traj, Q, np.asarray(self.u, np.float32).reshape(self.C))
        best = argsort_total_order(J)[: self.K]           # :69-71
        elite = Q[best]
        srt = np.sort(J)[: self.K + 1].astype(np.float64)                  # seeds: ranks 0 | 1 | 2; elite set: ranks K-1 | K
        pairs = [(0, 1), (1, 2)][: self.K - 1] + ([(self.K - 1, self.K)] if self.K < self.N else [])
        self.min_cost_gap = min([self.min_cost_gap] + [(srt[b] - srt[a]) / abs(srt[a]) for a, b in pairs])
        # :74-76: 2-norm over (H, C) of every other elite to elite 0 and to elite 1; argmin (a tie goes to elite 0)
        rest = elite[2:]
        d = np.stack([np.sqrt(np.sum(((rest - elite[k]) ** 2).reshape(len(rest), self.H * self.C), axis=1, dtype=np.float32)) for k in (0, 1)], axis=1)
        sel = np.argmin(d, axis=1) if len(rest) else np.zeros(0, np.int64)
        if len(rest):
            self.min_margin = min(self.min_margin, float(np.min(np.abs(d[:, 0] - d[:, 1]) / (d[:, 0] + d[:, 1]))))
        c1 = np.concatenate([elite[0:1], rest[sel == 0]], axis=0)       # :77-78
        c2 = np.concatenate([elite[1:2], rest[sel == 1]], axis=0)
        p = f32(f32(len(c1)) / f32(self.K))                                # :79-80
        self.probs = np.array([p, f32(1.0) - p], np.float32)

        def fit(c):
            m = np.mean(c, axis=0, dtype=np.float32)
            sd = np.sqrt(np.mean((c - m) ** 2, axis=0, dtype=np.float32)).astype(np.float32)     # tf.math.reduce_std: ddof 0
            return m, np.clip(sd, self.std_min, f32(1.0e4)).astype(np.float32)                   # :88-89, inside every iteration
        (m1, s1), (m2, s2) = fit(c1), fit(c2)
        self.dist_mue = np.stack([m1, m2], axis=-1)
        self.stdev = np.stack([s1, s2], axis=-1)
        self.labels = np.concatenate([[0, 1], sel]).astype(np.int64)
        return Q, elite, J, traj, best, comp

    def step(self, s, normals, uniforms):
        """normals [cem_outer_it, N, H, C], uniforms [cem_outer_it, N]"""
        s_t = np.tile(np.asarray(s, np.float32).reshape(1, self.S), (self.N, 1))
        assert normals.shape[0] == self.cem_outer_it and uniforms.shape == (self.cem_outer_it, self.N)
        for it in range(self.cem_outer_it):               # :106-107 (no warm-up)
            Q, elite, J, traj, best, comp = self.update_distribution(s_t, normals[it], uniforms[it])
        self.u = _u_out(elite[0, 0, :])                   # :110
        # :113-120: shift along H repeating the last row; probs are kept
        self.dist_mue = np.concatenate([self.dist_mue[1:], self.dist_mue[-1:]], axis=0)
        self.stdev = np.concatenate([self.stdev[1:], self.stdev[-1:]], axis=0)
        self.Q, self.J, self.rollout_trajectories, self.best_idx, self.comp = Q, J, traj, best, comp
        self.count += 1
        return np.array(self.u, np.float32)

    # ---- the engine's layouts ----------------------------------------------------------------------------------------
    def state(self) -> np.ndarray:
        """ctk_get_state of a CEM-GMM handle: mu[2,H,C] | std[2,H,C] | probs[2] | u[C] | count"""
        u = np.broadcast_to(np.asarray(self.u, np.float32).reshape(-1), (self.C,))
        return np.concatenate([np.moveaxis(self.dist_mue, -1, 0).reshape(-1), np.moveaxis(self.stdev, -1, 0).reshape(-1),
                               self.probs, u, [np.float32(self.count)]]).astype(np.float32)


def pack_draws(normals, uniforms) -> np.ndarray:
    """[its,N,H,C] normals and [its,N] uniforms -> the flat layout of one ctk_step: per iteration the normals, then the uniforms"""
    its = uniforms.shape[0]
    return np.concatenate([np.asarray(normals, np.float32).reshape(its, -1), np.asarray(uniforms, np.float32)], axis=1).reshape(-1)


def device_draws(seed, call, its, N, HC):
    """what a CTK_LOC_NONE step of a CEM-GMM handle draws: normals on Philox stream `it`, the uniform of row n = word 0 of
    block (n, 0, call, UNIFORM_STREAM + it)"""
    normals = np.stack([device_noise(seed, it, call, 0, N, HC, "normal") for it in range(its)])
    uniforms = np.stack([device_noise(seed, UNIFORM_STREAM + it, call, 0, N, 1, "uniform")[:, 0] for it in range(its)])
    return normals, uniforms
