#!/usr/bin/env python3
"""Record tests/golden/cem_gmm_*.npz by EXECUTING the unmodified reference module Optimizers/optimizer_cem_gmm_tf.py through the
reference's own controller_mpc, the way make_golden.py runs the other TF-only optimizers: `import tensorflow as tf` resolves to
standins/tensorflow, `tensorflow_probability.python.distributions` to standins/tensorflow_probability (see its README for what
such a recording pins).  The `tf.*` names that module uses and standins/tensorflow lacks are attached below, at run time.

Per closed-loop step the fixture holds: s, u_prev, the raw draws of every outer iteration (normals [its,N,H,C], uniforms [its,N]),
Q and J of the last iteration, u, and dist_mue / stdev [H,C,2] / probs [2] after the shift.

Usage (build container only):  python tests/golden/make_golden_gmm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import O  # noqa: E402


def attach_tf_names():
    """tf.* names of optimizer_cem_gmm_tf.py:74-92 on torch tensors, after TensorFlow's documented definitions"""
    import tensorflow as tf
    tf.newaxis = None
    tf.norm = lambda x, axis=None: torch.sqrt(torch.sum(x * x, dim=tuple(axis) if axis is not None else None))   # 2-norm over `axis`
    tf.transpose = lambda x, perm: x.permute(*perm)
    tf.argmin = lambda x, axis=0: torch.argmin(x, dim=axis)        # first minimum: a tie goes to the lower index
    tf.stack = lambda values, axis=0: torch.stack(list(values), dim=axis)
    tf.shape = lambda x: tuple(x.shape)
    tf.cast = lambda x, dtype: torch.as_tensor(x, dtype=dtype)


def main():
    out_dir = HERE
    mg.setup_workdir()
    attach_tf_names()
    import tensorflow_probability.python.distributions as tfpd
    dt = 0.02
    env = O.EnvParams(terminal_weight=0.5)
    mlp_w = O.mlp_default_weights(0)
    qenv = O.Quad2DParams(terminal_weight=0.4, target_x=0.1)
    mg.inject_constants(env, dt, mlp_w)

    import Control_Toolkit.Controllers.controller_mpc as cm
    import SI_Toolkit.Predictors.predictor_wrapper as pw

    def quad_state(seed):
        r = np.random.default_rng(seed)
        return np.array([r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5), r.uniform(0.6, 1.4), r.uniform(-0.5, 0.5),
                         r.uniform(-0.5, 0.5), r.uniform(-1, 1)], np.float32)

    envs = {
        "CartPole": dict(env=env, low=np.array([-1.0], np.float32), high=np.array([1.0], np.float32), C=1, state=mg.initial_state,
                         inject=lambda: mg.inject_constants(env, dt, mlp_w),
                         common=dict(env_params=env.as_array(), env_param_names=np.array(O.PARAM_NAMES), dt=np.float32(dt))),
        "Quad2D": dict(env=qenv, low=np.array([-1.0, -0.8], np.float32), high=np.array([1.0, 0.9], np.float32), C=2, state=quad_state,
                       inject=lambda: mg.inject_quad(qenv, dt),
                       common=dict(env_params=qenv.as_array(), env_param_names=np.array(O.QUAD2D_PARAM_NAMES), dt=np.float32(dt))),
    }
    cases = {
        "default": dict(env="CartPole", N=200, H=40, K=40, its=3, steps=4, seed=71),      # config_optimizers.yml:15-22 (cem-gmm-tf)
        "quad2d":  dict(env="Quad2D", N=128, H=20, K=20, its=3, steps=4, seed=72),
    }
    mg.set_computation_library("tensorflow")
    try:
        for name, c in cases.items():
            e = envs[c["env"]]
            e["inject"]()
            pw.ENVIRONMENT = c["env"]
            cfg = dict(seed=1, mpc_horizon=c["H"], cem_outer_it=c["its"], num_rollouts=c["N"], cem_stdev_min=0.01,
                       cem_initial_action_stdev=0.5, cem_best_k=c["K"], mpc_timestep=dt)
            cm.config_optimizers["cem-gmm-tf"] = dict(cfg)
            tfpd.seed(c["seed"])
            ctrl = cm.controller_mpc(c["env"], (e["low"], e["high"]), {})
            ctrl.controller_logging = True
            ctrl.configure(optimizer_name="cem-gmm-tf", predictor_specification="ODE")
            opt = ctrl.optimizer
            assert type(opt).__name__ == "optimizer_cem_gmm_tf" and ctrl.lib.lib == "TF" and opt.optimizer_logging

            def dist():
                sd = opt.sampling_dist
                return (sd.components_distribution.mean().numpy().copy(), sd.components_distribution.stddev().numpy().copy(),
                        sd.mixture_distribution.probs.numpy().copy())
            d = dict(e["common"], low=e["low"], high=e["high"], predictor=np.array("ODE"), environment=np.array(c["env"]),
                     **{k: (np.float32(v) if isinstance(v, float) else np.array(v)) for k, v in cfg.items()})
            d["dist_mue_init"], d["stdev_init"], d["probs_init"] = dist()
            plant = O.Predictor(kind="ODE", dt=dt, env=e["env"])
            s = e["state"](c["seed"])
            for t in range(c["steps"]):
                ndraw = len(tfpd.DRAW_LOG)
                u_prev = np.broadcast_to(np.asarray(opt.u, np.float32).reshape(-1), (e["C"],)).copy()
                u = ctrl.step(s.copy())
                lv = opt.logging_values
                draws = tfpd.DRAW_LOG[ndraw:]
                assert len(draws) == c["its"]                       # one sampling_dist.sample per outer iteration (:59)
                d[f"s_{t}"] = s.copy(); d[f"u_prev_{t}"] = u_prev
                d[f"normals_{t}"] = np.stack([z for z, _ in draws])
                d[f"uniforms_{t}"] = np.stack([u01 for _, u01 in draws])
                d[f"u_{t}"] = np.asarray(u, np.float32).reshape(-1)
                d[f"dist_mue_{t}"], d[f"stdev_{t}"], d[f"probs_{t}"] = dist()
                d[f"J_{t}"] = np.asarray(lv["J_logged"]).copy()
                d[f"Q_{t}"] = np.asarray(lv["Q_logged"]).copy()
                s = mg.plant_step(plant, s, u)
            d["steps"] = np.int32(c["steps"])
            mg.save_fixture(os.path.join(out_dir, f"cem_gmm_{name}.npz"), **d)
            print(f"cem_gmm_{name}: recorded {c['steps']} steps, probs {d['probs_' + str(c['steps'] - 1)]}")
    finally:
        mg.set_computation_library("pytorch")
        pw.ENVIRONMENT = "CartPole"


if __name__ == "__main__":
    main()
