"""optimizer_cem_gmm_hip — drop-in for reference Optimizers/optimizer_cem_gmm_tf.py (ctor keys :16-33,
step :98-129, optimizer_reset :131-137) running on libctk_hip.so: CEM whose sampling distribution is a mixture of
two diagonal Gaussians.  Every rollout draws its whole plan from ONE component (the mixture's Categorical has a scalar
batch shape); the elites are split into two clusters seeded by the best two, and each cluster is refitted."""
from typing import Tuple

import numpy as np

from . import template_optimizer, logging_kwargs
from ..computation_library import HipLibrary


def pack_gmm_draws(normals, uniforms) -> np.ndarray:
    """The layout one ctk_step of a CEM-GMM handle consumes (include/ctk_hip.h, block comment above ctk_step): per outer
    iteration N*H*C standard normals (row-major [N,H,C]) followed by N uniforms in [0,1).
    normals [its,N,H,C], uniforms [its,N] -> flat [its * (N*H*C + N)]."""
    normals = np.asarray(normals, np.float32)
    uniforms = np.asarray(uniforms, np.float32)
    its, n = uniforms.shape
    return np.concatenate([normals.reshape(its, -1), uniforms.reshape(its, n)], axis=1).reshape(-1)


def gmm_samples_needed(cem_outer_it: int, num_rollouts: int, mpc_horizon: int, num_control_inputs: int) -> int:
    """ctk_samples_needed of a CEM-GMM handle"""
    return cem_outer_it * (num_rollouts * mpc_horizon * num_control_inputs + num_rollouts)


class optimizer_cem_gmm_hip(template_optimizer):
    supported_computation_libraries = (HipLibrary,)
    engine_name = "cem_gmm"

    def __init__(self, predictor, cost_function, control_limits: "Tuple[np.ndarray, np.ndarray]",
                 computation_library, seed, mpc_horizon: int, cem_outer_it: int, cem_initial_action_stdev: float,
                 num_rollouts: int, cem_stdev_min: float, cem_best_k: int, optimizer_logging: bool,
                 calculate_optimal_trajectory: bool = False, **kwargs):
        super().__init__(predictor=predictor, cost_function=cost_function, control_limits=control_limits,
                         optimizer_logging=optimizer_logging, seed=seed, num_rollouts=num_rollouts,
                         mpc_horizon=mpc_horizon, computation_library=computation_library,
                         calculate_optimal_trajectory=calculate_optimal_trajectory,
                         rng_mode=kwargs.get("rng_mode", "device"), device=kwargs.get("device", 0), **logging_kwargs(kwargs))
        self.cem_outer_it = cem_outer_it
        self.cem_initial_action_stdev = cem_initial_action_stdev
        self.cem_stdev_min = cem_stdev_min
        self.cem_best_k = cem_best_k

    def configure(self, num_states: int, num_control_inputs: int, dt: float = None, predictor_specification=None, **kwargs):
        super().configure(num_states=num_states, num_control_inputs=num_control_inputs, default_configure=False)
        if dt is None:
            raise ValueError("optimizer_cem_gmm_hip.configure needs dt")
        self._build_engine(dt, predictor_specification, cem_outer_it=self.cem_outer_it, cem_best_k=self.cem_best_k,
                           cem_initial_action_stdev=self.cem_initial_action_stdev, cem_stdev_min=self.cem_stdev_min)
        self.optimizer_reset()

    def _step_draws(self):
        """None (on-device Philox) or the packed host draws of one step: sampling_dist.sample([N]) per outer iteration (:59)"""
        its, N = self.cem_outer_it, self.num_rollouts
        normals = self._draws("normal", [its, N, self.mpc_horizon, self.num_control_inputs])
        if normals is None:
            return None
        return pack_gmm_draws(normals, self._draws("uniform", [its, N]))

    def step(self, s: np.ndarray, time=None):
        if self.optimizer_logging:
            self.logging_values = {"s_logged": np.asarray(s).copy()}   # :100
        s = self._prepare_state(s)
        self._sync_parameters()
        self._publish_u(self.engine.step(s, self._step_draws(), u_prev=self._u_prev()))
        if self.optimizer_logging:
            self._fill_logging(s, self.u)   # :124-127
        return self.u

    # [H,C,2]: the layout of the reference's sampling_dist.components_distribution.mean() / .stddev()
    @property
    def dist_mue(self):
        return np.ascontiguousarray(np.moveaxis(self.engine.read("MIX_MU"), 0, -1))

    @property
    def stdev(self):
        return np.ascontiguousarray(np.moveaxis(self.engine.read("MIX_STD"), 0, -1))

    @property
    def mixture_probs(self):
        return self.engine.read("MIX_PROB")

    def optimizer_reset(self):
        self.engine.reset()   # :131-137; self.u is not touched there
