"""-m gpu: a handle's life — buffers that grow (the staging of host draws, the temporary trajectories of ctk_rollout), the step log's
rings enabled, resized and released, ctk_destroy and a second ctk_create — leaves no trace in what the handle computes.  The engine
counterpart of the batch families' test_state_survives_destroy_and_create_after_buffers_grew.

Two twin handles `a` and `ref` do the same work; `a` is then closed, created again and given its state and Philox position back, and
one step with the in-kernel sampler on both must agree bit for bit: u, get_state() and every buffer ctk_read allows for the optimizer.
(Two never-destroyed twins agree bit for bit for every optimizer here — the assertions "twins, ..." below say so at every stage —, so
no optimizer is reduced to the state round trip alone.)"""
import numpy as np
import pytest

from control_toolkit_amd import CtkEngine
from control_toolkit_amd._capi import BUFFERS, CtkError

pytestmark = pytest.mark.gpu

S0 = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
# ODE predictor, CartPole; per optimizer the smallest configuration of its own test file with more than one rollout:
# test_gpu_mppi.py, test_gpu_cem_random.py, test_gpu_cem_gmm.py, test_gpu_variants.py, test_gpu_rpgd.py
CONFIGS = {
    "mppi": dict(num_rollouts=70, mpc_horizon=7, period_interpolation_inducing_points=3),
    "cem": dict(num_rollouts=100, mpc_horizon=5, cem_outer_it=2, cem_best_k=1),
    "cem_gmm": dict(num_rollouts=96, mpc_horizon=16, cem_outer_it=3, cem_best_k=2, cem_initial_action_stdev=0.5, cem_stdev_min=0.01),
    "cem_naive_grad": dict(num_rollouts=256, mpc_horizon=12, cem_outer_it=3, cem_best_k=32, cem_initial_action_stdev=0.5, cem_stdev_min=0.1,
                           learning_rate=0.1, gradmax_clip=10.0),
    "cem_grad_bharadhwaj": dict(num_rollouts=32, mpc_horizon=50, cem_outer_it=2, cem_best_k=8, cem_initial_action_stdev=2.0, cem_stdev_min=1e-6,
                                learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-8, gradmax_clip=5.0),
    "random_action": dict(num_rollouts=32, mpc_horizon=10),
    "rpgd": dict(num_rollouts=64, mpc_horizon=7, period_interpolation_inducing_points=3, outer_its=5, resamp_per=2, shift_previous=1,
                 opt_keep_k=16, sampling_distribution=0, sample_min=-1.0, sample_max=1.0, learning_rate=0.05, gradmax_clip=5.0),
    "gradient": dict(num_rollouts=100, mpc_horizon=8, outer_its=1, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-7,
                     gradmax_clip=5.0),
}
NEEDS_RESET = ("rpgd", "gradient")
UNIFORM_DRAWS = ("random_action", "rpgd", "gradient")


def make(opt):
    return CtkEngine(opt, "ODE", dt=0.02, seed=21, **CONFIGS[opt])      # materialize_trajectories stays off: ctk_rollout takes temporaries


def host_draws(e, opt, rng):
    """the draws of one step in the layout ctk_step consumes (ctk_samples_needed floats), or None where the step takes none"""
    n = e.samples_needed()
    if n == 0:
        return None
    if opt == "cem_gmm":       # per iteration the normals, then one uniform per rollout
        its = CONFIGS[opt]["cem_outer_it"]
        per = n // its - e.N
        return np.concatenate([np.concatenate([rng.standard_normal(per), rng.random(e.N)]) for _ in range(its)]).astype(np.float32)
    return (rng.random(n) if opt in UNIFORM_DRAWS else rng.standard_normal(n)).astype(np.float32)


def readable(e):
    """every buffer ctk_read allows for this handle"""
    out = {}
    for name in BUFFERS:
        try:
            out[name] = e.read(name)
        except (ValueError, CtkError):
            pass
    return out


def plans_of(e):
    return np.random.default_rng(8).uniform(-1.0, 1.0, (e.N, e.H, 1)).astype(np.float32)


def drive(e, opt):
    """the work before the destroy; everything it returns must agree between the twins"""
    rng = np.random.default_rng(3)
    got = []
    if opt in NEEDS_RESET:
        e.reset(rng.random(e.samples_needed_reset(), dtype=np.float32))
    for n in (1, e.N):                                  # the temporary trajectories, and a staging buffer that grows
        traj, J = e.rollout(S0, plans_of(e)[:n], want_traj=True)
        got += [traj, J]
    got.append(e.step(S0, host_draws(e, opt, rng)))
    e.log_enable(2)
    got += [e.step(S0), e.step(S0)]
    assert e.log_count() == 2
    got.append(e.log_read("J", 0, 2))
    e.log_enable(5)                                     # the rings are released and allocated again, then released for good
    got.append(e.step(S0))
    e.log_enable(0)
    return got


def equal(tag, got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{tag}, result {i}")


@pytest.mark.parametrize("opt", list(CONFIGS))
def test_state_survives_destroy_and_create_after_buffers_grew(opt):
    a, ref = make(opt), make(opt)
    equal(f"{opt}: twins, before the destroy", drive(a, opt), drive(ref, opt))
    state, pos = a.get_state(), a.rng_position()
    np.testing.assert_array_equal(state, ref.get_state(), err_msg=f"{opt}: twins, state")
    assert pos == ref.rng_position() and pos > 0
    a.close()
    a = make(opt)
    # ctk_read's Q of an MPPI handle that does not materialise is no output of its step: it holds the plans of the last ctk_rollout
    # (measured: a fresh handle reads zeros there, its twin the rollout's plans).  So that EVERY readable buffer can be compared, the
    # handle created again is given that last rollout too; its state and Philox position come from set_state / set_rng_position alone.
    a.rollout(S0, plans_of(a), want_traj=True)
    a.set_state(state)
    np.testing.assert_array_equal(a.get_state(), state, err_msg=f"{opt}: get_state after set_state")
    a.set_rng_position(pos)
    tag = f"{opt}: created again against its never-destroyed twin"
    np.testing.assert_array_equal(a.step(S0), ref.step(S0), err_msg=f"{tag}, u")
    np.testing.assert_array_equal(a.get_state(), ref.get_state(), err_msg=f"{tag}, state")
    assert a.rng_position() == ref.rng_position()
    bufs_a, bufs_ref = readable(a), readable(ref)
    assert set(bufs_a) == set(bufs_ref) and {"Q", "J"} <= set(bufs_a)
    for name in bufs_a:
        np.testing.assert_array_equal(bufs_a[name], bufs_ref[name], err_msg=f"{tag}, {name}")
    a.close(); ref.close()
