"""-m gpu: CtkMppiBatch (ctk_batch_*, kernel ctk_mppi_batch<ENV, LOG>) — B independent MPPI problems stepped by one launch.

The contract under test: problem p of a batch behaves BIT FOR BIT like a CtkEngine("mppi", "ODE", seed=seeds[p]) created from the same
configuration that received the same calls.  Every comparison against single handles is assert_array_equal; the only tolerances in this
file are the existing ones of the reference-recorded fixture (tests/test_gpu_mppi.py: J rtol 1e-5, u / u_nom rtol 1e-5 / atol 1e-5,
u_run 1e-6 / 1e-6, traj rtol 1e-4 / atol 2e-5), applied to a problem that replays that fixture INSIDE a batch."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkError
from helpers import load, env_from
from gpu_helpers import ENV_NAMES
from margins import close

pytestmark = pytest.mark.gpu

# name -> (environment, N, H, period, extra engine keywords, the oracle's plant parameters)
CONFIGS = {
    "cartpole_cfg2": ("CartPole", 1024, 50, 1, {}, O.EnvParams),
    "cartpole_interp": ("CartPole", 1000, 35, 10, {}, O.EnvParams),
    "cartpole_small": ("CartPole", 70, 7, 3, {}, O.EnvParams),
    "cartpole_generic": ("CartPole", 256, 20, 5, {"generic_kernels": True}, O.EnvParams),
    "quad2d": ("Quad2D", 256, 20, 5, {"action_low": [-1.0, -1.0], "action_high": [1.0, 1.0]}, O.Quad2DParams),
    "hover": ("Hover", 128, 12, 1, {}, O.HoverParams),
}
SOURCES = [("philox", True), ("host", False), ("devptr", True), ("philox", False), ("host", True), ("devptr", False)]   # (draws, u_prev given)
STEPS = 5


def make(config, B, materialize, seeds=None, **kw):
    """(batch, B single handles with seeds[p], the plant)"""
    env, N, H, p, extra, params = CONFIGS[config]
    seeds = [7 + q for q in range(B)] if seeds is None else seeds
    common = dict(num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, environment=env,
                  materialize_trajectories=materialize, **extra, **kw)
    batch = CtkMppiBatch(B, seeds=seeds, **common)
    handles = [CtkEngine("mppi", "ODE", seed=seeds[q], **common) for q in range(B)]
    return batch, handles, O.Predictor("ODE", dt=0.02, env=params())


def first_states(rng, B, S):
    s = rng.uniform(-0.4, 0.4, (B, S)).astype(np.float32)
    if S == 4:
        s[:, 2] += 2.6          # CartPole: the pendulum hangs away from the target
    return s


def draws_for(source, rng, n, batch):
    """(what the batch is given, what handle row j is given, keep-alive)"""
    if source == "philox":
        return None, [None] * n, None
    arr = rng.standard_normal((n, batch.N, batch.samples_needed() // (batch.N * batch.C), batch.C)).astype(np.float32)
    if source == "host":
        return arr, [arr[j] for j in range(n)], None
    import torch
    t = torch.from_numpy(arr).to("cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), [t.data_ptr() + 4 * j * arr[0].size for j in range(n)], t


def compare(batch, handles, problems, materialize, tag):
    for q in problems:
        h = handles[q]
        np.testing.assert_array_equal(batch.read("U_NOM", q), h.read("U_NOM"), err_msg=f"{tag}: U_NOM of problem {q}")
        np.testing.assert_array_equal(batch.read("J", q), h.read("J"), err_msg=f"{tag}: J of problem {q}")
        np.testing.assert_array_equal(batch.get_state(q), h.get_state(), err_msg=f"{tag}: state vector of problem {q}")
        assert batch.rng_position(q) == h.rng_position(), f"{tag}: Philox position of problem {q}"
        if materialize:
            np.testing.assert_array_equal(batch.read("Q", q), h.read("Q"), err_msg=f"{tag}: Q of problem {q}")
            np.testing.assert_array_equal(batch.read("TRAJ", q), h.read("TRAJ"), err_msg=f"{tag}: TRAJ of problem {q}")


def close_all(batch, handles):
    batch.close()
    for h in handles:
        h.close()


# ---- 1. batch == single handles, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("B", [1, 3, 16, 40])
def test_batch_equals_single_handles(B, config, materialize):
    """every sample source with u_prev given and None, one after another on the SAME objects (the contract holds for any interleaving):
    STEPS closed-loop steps each, the plant being the oracle's Predictor.step with every problem's own output fed back"""
    batch, handles, plant = make(config, B, materialize)
    rng = np.random.default_rng(B * 131 + len(config))
    s = first_states(rng, B, batch.S)
    for source, given in SOURCES:
        for t in range(STEPS):
            up = rng.uniform(-1.0, 1.0, (B, batch.C)).astype(np.float32) if given else None
            bs, hs, keep = draws_for(source, rng, B, batch)
            u = batch.step(s, bs, u_prev=up)
            uh = np.stack([handles[q].step(s[q], hs[q], u_prev=None if up is None else up[q]) for q in range(B)])
            np.testing.assert_array_equal(u, uh, err_msg=f"{config} B={B} {source} u_prev={'given' if given else 'None'} step {t}: u")
            s = plant.step(s, u).astype(np.float32)
            del keep
        compare(batch, handles, range(B), materialize, f"{config} B={B} after {source}/{'given' if given else 'None'}")
    close_all(batch, handles)


@pytest.mark.parametrize("config", ["cartpole_cfg2", "cartpole_small"])
def test_split_into_launches_gives_the_same_bits(config, monkeypatch):
    """B = 40 with CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH = 16 runs as three launches (16 + 16 + 8) and gives the bits of one launch"""
    B = 40
    one, handles, plant = make(config, B, True)
    monkeypatch.setenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH", "16")
    split = CtkMppiBatch(B, seeds=[7 + q for q in range(B)], num_rollouts=one.N, mpc_horizon=one.H, dt=0.02, materialize_trajectories=True,
                         period_interpolation_inducing_points=CONFIGS[config][3], environment=CONFIGS[config][0])
    monkeypatch.delenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    rng = np.random.default_rng(40)
    s = first_states(rng, B, one.S)
    for t in range(STEPS):
        u1, u2 = one.step(s), split.step(s)
        uh = np.stack([handles[q].step(s[q]) for q in range(B)])
        np.testing.assert_array_equal(u1, u2)
        np.testing.assert_array_equal(u1, uh)
        s = plant.step(s, u1).astype(np.float32)
    compare(one, handles, range(B), True, "one launch")
    compare(split, handles, range(B), True, "three launches")
    # an id list longer than the cap is split as well
    ids = list(range(1, 40, 2))
    u2 = split.step(s[ids], ids=ids)
    uh = np.stack([handles[q].step(s[q]) for q in ids])
    np.testing.assert_array_equal(u2, uh)
    compare(split, handles, ids, True, "subset over two launches")
    split.close()
    close_all(one, handles)


# ---- 2. subset steps, resets, state round trip --------------------------------------------------------------------------------------------
def snapshot(batch, q):
    return dict(U_NOM=batch.read("U_NOM", q), J=batch.read("J", q), Q=batch.read("Q", q), TRAJ=batch.read("TRAJ", q),
                state=batch.get_state(q), rng=batch.rng_position(q))


def assert_unchanged(batch, q, snap, tag):
    now = snapshot(batch, q)
    for k, v in snap.items():
        np.testing.assert_array_equal(now[k], v, err_msg=f"{tag}: {k} of untouched problem {q} changed")


def test_subset_steps_and_resets():
    B = 8
    batch, handles, plant = make("cartpole_interp", B, True)
    rng = np.random.default_rng(8)
    s = first_states(rng, B, batch.S)
    for t in range(2):                                   # two whole-batch steps first: every problem has a plan and a Philox position of its own
        u = batch.step(s)
        np.testing.assert_array_equal(u, np.stack([handles[q].step(s[q]) for q in range(B)]))
        s = plant.step(s, u).astype(np.float32)
    ids = [1, 4, 5]
    rest = [q for q in range(B) if q not in ids]
    snaps = {q: snapshot(batch, q) for q in rest}
    for t in range(3):
        u = batch.step(s[ids], ids=ids)
        np.testing.assert_array_equal(u, np.stack([handles[q].step(s[q]) for q in ids]))
        s[ids] = plant.step(s[ids], u).astype(np.float32)
    for q in rest:
        assert_unchanged(batch, q, snaps[q], "subset step")
    compare(batch, handles, range(B), True, "after subset steps")
    # reset of one problem = ctk_reset of its handle; nobody else moves
    snaps = {q: snapshot(batch, q) for q in range(B) if q != 4}
    batch.reset([4])
    handles[4].reset()
    for q in snaps:
        assert_unchanged(batch, q, snaps[q], "reset([4])")
    compare(batch, handles, [4], True, "after reset([4])")
    for t in range(2):
        up = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
        u = batch.step(s, u_prev=up)
        np.testing.assert_array_equal(u, np.stack([handles[q].step(s[q], u_prev=up[q]) for q in range(B)]))
        s = plant.step(s, u).astype(np.float32)
    compare(batch, handles, range(B), True, "after the reset and two more steps")
    # get_state / set_state / set_rng_position: a batch restored into a FRESH batch continues bit for bit
    fresh = CtkMppiBatch(B, seeds=[7 + q for q in range(B)], num_rollouts=batch.N, mpc_horizon=batch.H, dt=0.02,
                         period_interpolation_inducing_points=CONFIGS["cartpole_interp"][3], materialize_trajectories=True)
    for q in range(B):
        fresh.set_state(q, batch.get_state(q))
        fresh.set_rng_position(q, batch.rng_position(q))
        np.testing.assert_array_equal(fresh.get_state(q), batch.get_state(q))
    for t in range(3):
        u = batch.step(s)
        np.testing.assert_array_equal(fresh.step(s), u)
        s = plant.step(s, u).astype(np.float32)
    for q in range(B):
        for k, v in snapshot(batch, q).items():
            np.testing.assert_array_equal(snapshot(fresh, q)[k], v, err_msg=f"restored batch: {k} of problem {q}")
    fresh.close()
    close_all(batch, handles)


# ---- 3. the reference-recorded fixture inside a batch -------------------------------------------------------------------------------------
J_RTOL = 1e-5                                   # tests/test_gpu_mppi.py: the bounds of the reference-recorded fixtures
GOLDEN_U_TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("materialize", [True, False])
def test_reference_fixture_inside_a_batch(materialize):
    """B = 5; problem 2 replays mppi_cfg2_ode (the loop of test_mppi_matches_reference_golden, re-pinned with set_state) while the other
    four problems run other states and draws in the same launches"""
    d = load("mppi_cfg2_ode.npz")
    B, me = 5, 2
    N, H = int(d["num_rollouts"]), int(d["mpc_horizon"])
    batch = CtkMppiBatch(B, seeds=[11, 12, 13, 14, 15], num_rollouts=N, mpc_horizon=H, dt=float(d["dt"]),
                         action_low=float(d["low"][0]), action_high=float(d["high"][0]),
                         period_interpolation_inducing_points=int(d["period_interpolation_inducing_points"]),
                         materialize_trajectories=materialize, cc_weight=float(d["cc_weight"]), R=float(d["R"]), LBD=float(d["LBD"]),
                         NU=float(d["NU"]), SQRTRHOINV=float(d["SQRTRHOINV"]))
    env = env_from(d)
    for n in ENV_NAMES:
        batch.set_param(n, float(getattr(env, n)))
    assert batch.dominant_kernel() == f"ctk_mppi_batch<0, {'true' if materialize else 'false'}>"
    np.testing.assert_array_equal(batch.read("U_NOM", me), d["u_nom_init"])
    rng = np.random.default_rng(52)
    P = batch.samples_needed() // N
    for t in range(int(d["steps"])):
        s = first_states(rng, B, 4)
        s[me] = d[f"s_{t}"]
        noise = rng.standard_normal((B, N, P, 1)).astype(np.float32)
        noise[me] = np.asarray(d[f"noise_{t}"], np.float32).reshape(N, P, 1)
        up = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
        up[me, 0] = d[f"u_prev_{t}"]
        u = batch.step(s, noise, u_prev=up)
        tag = f"batch5[2]=mppi_cfg2_ode[materialize={materialize}] step {t}"
        if materialize:
            close(tag, "u_run", batch.read("Q", me), d[f"u_run_{t}"], rtol=1e-6, atol=1e-6)
        close(tag, "J", batch.read("J", me), d[f"J_{t}"], rtol=J_RTOL)
        close(tag, "u_nom", batch.read("U_NOM", me), d[f"u_nom_{t}"], **GOLDEN_U_TOL)
        close(tag, "u", u[me], d[f"u_{t}"], **GOLDEN_U_TOL)
        if materialize and f"traj_{t}" in d.files:
            close(tag, "traj", batch.read("TRAJ", me), d[f"traj_{t}"], rtol=1e-4, atol=2e-5)
        assert np.all(np.isfinite(u))
        # re-pin to the reference's own warm-start state so every step is checked in isolation
        batch.set_state(me, np.concatenate([d[f"u_nom_{t}"].reshape(H), d[f"u_{t}"].reshape(1)]))
    batch.close()


# ---- 4. set_param reaches every problem -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,name", [("cartpole_interp", "target_position"), ("quad2d", "target_x")])
def test_set_param_reaches_every_problem(config, name):
    B = 3
    batch, handles, plant = make(config, B, True)
    rng = np.random.default_rng(3)
    s = first_states(rng, B, batch.S)
    u0 = batch.step(s)
    np.testing.assert_array_equal(u0, np.stack([handles[q].step(s[q]) for q in range(B)]))
    batch.set_param(name, 0.3)
    assert batch.get_param(name) == np.float32(0.3)
    for h in handles:
        h.set_param(name, 0.3)
    J_before = batch.read_all("J")
    for t in range(2):
        u = batch.step(s)
        np.testing.assert_array_equal(u, np.stack([handles[q].step(s[q]) for q in range(B)]))
    compare(batch, handles, range(B), True, f"{name} = 0.3")
    assert batch.read_all("J").shape == (B, batch.N) and not np.array_equal(batch.read_all("J"), J_before)    # the parameter is in the cost
    close_all(batch, handles)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages():
    kw = dict(num_rollouts=256, mpc_horizon=20, dt=0.02)
    with pytest.raises(NotImplementedError, match="MPPI controllers only"):
        CtkMppiBatch(4, optimizer="cem", **kw)
    with pytest.raises(NotImplementedError, match=r"analytic \(ODE\) predictor only"):
        CtkMppiBatch(4, predictor="MLP", **kw)
    with pytest.raises(NotImplementedError, match=r"num_rollouts 4096, mpc_horizon 50, 50 inducing points x 1 inputs = 64 block records of 52 words.*narrow in-launch hand-off"):
        CtkMppiBatch(4, num_rollouts=4096, mpc_horizon=50, dt=0.02)
    with pytest.raises(NotImplementedError, match="throughput"):
        CtkMppiBatch(2, num_rollouts=32768, mpc_horizon=10, dt=0.02)
    with pytest.raises(ValueError, match="at least one problem"):
        CtkMppiBatch(0, **kw)
    # the library says the same when it is asked directly (a caller of the C ABI)
    import ctypes
    from control_toolkit_amd import _capi
    lib = _capi.load_library()
    for field, value, pat in (("optimizer", 1, b"MPPI controllers only (cfg.optimizer == 1)"), ("predictor", 1, b"(ODE) predictor only (cfg.predictor == 1)")):
        cfg = _capi._make_config("mppi", "ODE", 0, "CartPole", 1, action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=1, seed=0, device=0,
                                 intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=4, num_control_inputs=1,
                                 generic_kernels=False, **kw)
        setattr(cfg, field, value)
        out = ctypes.c_void_p()
        assert lib.ctk_batch_create(ctypes.byref(cfg), 4, None, ctypes.byref(out)) == 2 and not out.value
        assert pat in lib.ctk_batch_last_error(None)
    b = CtkMppiBatch(4, **kw)
    s = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="strictly ascending"):
        b.step(s[:2], ids=[2, 1])
    with pytest.raises(ValueError, match="strictly ascending"):
        b.reset(ids=[1, 1])
    with pytest.raises(ValueError, match=r"0 \.\. 3"):
        b.step(s[:1], ids=[4])
    with pytest.raises(ValueError, match=r"consumes 4 x 5120 draws"):
        b.step(s, np.zeros((4, 256, 19, 1), np.float32))
    with pytest.raises(ValueError, match=r"consumes 2 x 5120 draws"):
        b.step(s[:2], np.zeros((4, 256, 20, 1), np.float32), ids=[0, 3])
    with pytest.raises(ValueError, match="states must have shape"):
        b.step(s[:3])
    # ... and the C ABI refuses bad id lists itself
    ids = (ctypes.c_int32 * 2)(2, 1)
    assert lib.ctk_batch_step(b._h, 2, ids, s.ctypes.data, None, None, 0, None) == 1
    assert b"strictly ascending" in lib.ctk_batch_last_error(b._h)
    ids = (ctypes.c_int32 * 1)(4)
    assert lib.ctk_batch_reset(b._h, 1, ids) == 1
    with pytest.raises(CtkError, match="not materialised"):
        b.read("TRAJ", 0)
    u = b.step(s)                                     # the refusals left the batch usable
    assert u.shape == (4, 1) and np.all(np.isfinite(u))
    b.close()


# ---- 6. kernel names -----------------------------------------------------------------------------------------------------------------------------
def test_dominant_kernel_names():
    b = CtkMppiBatch(2, num_rollouts=1024, mpc_horizon=50, dt=0.02)
    assert b.dominant_kernel() == "ctk_mppi_batch<0, false>"
    b.close()
    b = CtkMppiBatch(2, num_rollouts=64, mpc_horizon=10, dt=0.02, environment="Quad2D", materialize_trajectories=True)
    assert b.dominant_kernel() == "ctk_mppi_batch<1, true>"
    b.close()
    e = CtkEngine("mppi", "ODE", num_rollouts=1024, mpc_horizon=50, dt=0.02)        # the single handle's name is what it was
    assert e.dominant_kernel() == "ctk_mppi_rollout<0, 0, false, false>"
    e.step(np.zeros(4, np.float32))
    assert e.dominant_kernel() == "ctk_mppi_rollout<0, 0, false, false>"
    e.close()


# ---- 7. what a batch allocates: buffers that grow, destroy, create again --------------------------------------------------------------------------
def test_state_survives_destroy_and_create_after_buffers_grew():
    """The staging buffer grows (host draws for one problem, then for all), the run buffer grows (a run of 2 steps, of 5, episodes of 3);
    then every problem's state is read, the batch destroyed, created again from the same seeds and given the states and Philox positions
    back: its next step, by the in-kernel sampler, equals bit for bit that of a batch that took the same steps and was never destroyed."""
    env, N, H, p, extra, _ = CONFIGS["cartpole_small"]
    kw = dict(seeds=[7, 8, 9], num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, environment=env, **extra)
    rng = np.random.default_rng(41)
    s, s_next = first_states(rng, 3, 4), first_states(rng, 3, 4)

    def used(batch):
        draws = np.random.default_rng(42).standard_normal((3, N, batch.samples_needed() // (N * batch.C), batch.C)).astype(np.float32)
        batch.step(s[1:2], draws[:1], ids=[1])
        batch.step(s, draws)
        for steps in (2, 5):
            batch.closed_loop.run(s, steps)
        batch.closed_loop.episodes(s, 3)
        return batch

    a, ref = used(CtkMppiBatch(3, **kw)), used(CtkMppiBatch(3, **kw))
    saved = [(a.get_state(q), a.rng_position(q)) for q in range(3)]
    a.close()
    a = CtkMppiBatch(3, **kw)
    for q, (state, position) in enumerate(saved):
        np.testing.assert_array_equal(state, ref.get_state(q))
        a.set_state(q, state)
        a.set_rng_position(q, position)
    np.testing.assert_array_equal(a.step(s_next), ref.step(s_next))
    for q in range(3):
        for name in ("U_NOM", "J"):
            np.testing.assert_array_equal(a.read(name, q), ref.read(name, q), err_msg=f"{name} of problem {q}")
        np.testing.assert_array_equal(a.get_state(q), ref.get_state(q), err_msg=f"state vector of problem {q}")
        assert a.rng_position(q) == ref.rng_position(q)
    a.close()
    ref.close()
