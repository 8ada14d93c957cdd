"""-m gpu: the publish of a launched step without a release fence (ctk_device.h: publish_u_launched / publish_u_vec_launched).

When step() returns the host has read {u, seq}, the error words and (C > 1) the vector behind them out of the pinned slot — stored
relaxed, with no write-back of the device's caches in front of them.  Everything else a step leaves is reached through API entries
ordered on the handle's stream.  So, over closed loops of 100 steps and after EVERY step:

  * the u that step() returned equals, bit for bit, the device copy read back through the API: U_NOM[0] for MPPI and RPGD (u is the
    plan's first entry), Q[BEST_IDX[0]][0] for CEM and random-action (u is the cheapest row's first input); for two control inputs
    both components;
  * the error word stays clear: step() raises CtkError the moment ctk_api.hip:finish_step finds it set, so a loop that runs through
    is that assertion (and every u is finite);
  * in the MPPI sample-buffer cases the buffer is refilled in place, on another stream, the moment step() returns.

Shapes: the smallest at which each path exists — one block; two blocks, the second partial; 128 records (two lane batches of the early
merge); 128 records of 22 words (the wide tail: late publish from the final update); the headline once; the vector publish of two
control inputs; CEM's, random-action's and RPGD's finishes; the network kernels' tail."""
import numpy as np
import pytest

from oracle import ctk_oracle as O   # the default MLP weights only

pytestmark = pytest.mark.gpu

STEPS = 100


def advance(s, u):
    """a closed loop: the next state depends on the input this step produced"""
    d = np.zeros_like(s)
    d[0] = s[1]; d[1] = u.ravel()[0]; d[2] = s[3]; d[3] = -np.sin(s[2])
    return (s + np.float32(0.02) * d).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def check_u(e, u, t, how):
    assert np.isfinite(u).all(), (t, u)
    if how == "plan":
        dev = e.read("U_NOM").reshape(e.H, e.C)[0]
    else:
        dev = e.read("Q")[int(e.read("BEST_IDX")[0]), 0, :]
    assert u.shape == (e.C,) and dev.shape == (e.C,)
    np.testing.assert_array_equal(bits(u), bits(dev), err_msg=f"step {t}: returned u {u} != device copy {dev}")


MPPI_BUFFER_CASES = [
    dict(N=64, H=1),                       # one block
    dict(N=100, H=7),                      # two blocks, one partial
    dict(N=8192, H=10),                    # 128 records: two lane batches of the early merge
    dict(N=8192, H=20),                    # 128 records of 22 words: the wide tail, late publish
    dict(N=1024, H=50),                    # the headline
    dict(N=128, H=5, env="Quad2D"),        # two control inputs: the vector publish
]


@pytest.mark.parametrize("case", MPPI_BUFFER_CASES, ids=lambda c: f"{c.get('env', 'CartPole')}_N{c['N']}_H{c['H']}")
def test_mppi_returned_u_is_the_device_copy_after_every_step_with_the_buffer_refilled_in_place(case):
    import torch
    from control_toolkit_amd import CtkEngine
    e = CtkEngine("mppi", "ODE", environment=case.get("env", "CartPole"), num_rollouts=case["N"], mpc_horizon=case["H"], dt=0.02,
                  period_interpolation_inducing_points=1, seed=7)
    try:
        g = torch.Generator(device="cuda"); g.manual_seed(5)
        buf = torch.randn((e.samples_needed(),), generator=g, device="cuda")
        torch.cuda.synchronize()
        s = np.array([0.05, -0.1, 2.8, 0.4, 0.02, -0.03][:e.S], np.float32)
        for t in range(STEPS):
            u = e.step(s, buf.data_ptr())
            buf.normal_(generator=g)           # the moment step() returns: new draws into the SAME buffer, on torch's stream
            check_u(e, u, t, "plan")
            torch.cuda.synchronize()
            s = advance(s, u)
    finally:
        e.close()


def test_cem_returned_u_is_the_best_rows_first_input_after_every_step():
    from control_toolkit_amd import CtkEngine
    e = CtkEngine("cem", "ODE", num_rollouts=256, mpc_horizon=5, dt=0.02, cem_outer_it=3, cem_best_k=16, seed=3)
    try:
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        for t in range(STEPS):
            u = e.step(s)
            check_u(e, u, t, "best")
            s = advance(s, u)
    finally:
        e.close()


def test_random_action_returned_u_is_the_best_rows_first_input_after_every_step():
    from control_toolkit_amd import CtkEngine
    e = CtkEngine("random_action", "ODE", num_rollouts=64, mpc_horizon=5, dt=0.02, seed=3)
    try:
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        for t in range(STEPS):
            u = e.step(s)
            check_u(e, u, t, "best")
            s = advance(s, u)
    finally:
        e.close()


def test_rpgd_returned_u_is_the_best_plans_first_entry_after_every_step():
    from control_toolkit_amd import CtkEngine
    e = CtkEngine("rpgd", "ODE", num_rollouts=32, mpc_horizon=5, dt=0.02, period_interpolation_inducing_points=1, outer_its=2, resamp_per=3,
                  opt_keep_k=8, seed=11)
    try:
        e.reset()
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        for t in range(STEPS):
            u = e.step(s)
            check_u(e, u, t, "plan")
            s = advance(s, u)
    finally:
        e.close()


def test_mppi_mlp_returned_u_is_the_device_copy_after_every_step():
    from control_toolkit_amd import CtkEngine
    e = CtkEngine("mppi", "MLP", num_rollouts=64, mpc_horizon=5, dt=0.02, period_interpolation_inducing_points=1, seed=7)
    try:
        e.set_predictor_weights(O.mlp_default_weights(0))
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        for t in range(STEPS):
            u = e.step(s)
            check_u(e, u, t, "plan")
            s = advance(s, u)
    finally:
        e.close()
