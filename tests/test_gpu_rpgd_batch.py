"""-m gpu: CtkRpgdBatch (ctk_rpgd_batch_*, kernel ctk_g_rpgd_batch<ENV>) — B independent RPGD problems stepped by one launch.

The contract under test: problem p of a batch behaves BIT FOR BIT like a CtkEngine("rpgd", "ODE", seed=seeds[p], generic_kernels=True)
created from the same configuration that received the same calls.  Every comparison against single handles is assert_array_equal; the
only tolerances in this file are those of the reference-golden tests of the handles (test_gpu_rpgd / test_gpu_env / test_gpu_hover), whose
bodies are RUN (not restated) on a problem that replays a reference-recorded fixture INSIDE a batch."""
import numpy as np
import pytest

from control_toolkit_amd import CtkEngine, CtkError, CtkRpgdBatch
import test_gpu_rpgd
import test_gpu_env
import test_gpu_hover

pytestmark = pytest.mark.gpu


def tape_in_scratch_horizon(env):
    """the smallest multiple of 8 whose state tape does not fit in LDS beside the plans and gradients (ctk_g_rpgd_descent_lds' rule), with
    the check that the next smaller multiple fits"""
    H = 8
    while CtkRpgdBatch.descent_lds(env, H)[1]:
        H += 8
    assert H > 8 and CtkRpgdBatch.descent_lds(env, H - 8)[1] and not CtkRpgdBatch.descent_lds(env, H)[1]
    return H


def cfg(env, N, H, p, K, its, resamp_per, **kw):
    return dict(environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, opt_keep_k=K, outer_its=its,
                resamp_per=resamp_per, **kw)


# the smallest sizes at which each branch of the kernel is taken
CONFIGS = {
    "cartpole_small": lambda: cfg("CartPole", 16, 12, 5, 4, 2, 2, sampling_distribution=0, sample_whole_control_space=1),
    "cartpole_partial": lambda: cfg("CartPole", 40, 7, 3, 10, 3, 1, sampling_distribution=1, shift_previous=2, sample_whole_control_space=0,
                                    sample_min=-0.6, sample_max=0.7, sample_stdev=0.4, sample_mean=0.1),
    "cartpole_full_wave": lambda: cfg("CartPole", 64, 20, 1, 16, 2, 3, sample_whole_control_space=1),
    "quad2d": lambda: cfg("Quad2D", 32, 10, 5, 8, 3, 2, action_low=[-1.0, -0.8], action_high=[1.0, 0.9], sample_whole_control_space=1),   # limits as test_gpu_env.py
    "hover": lambda: cfg("Hover", 24, 8, 4, 6, 2, 2, sample_whole_control_space=1),
    "hover_tape_in_scratch": lambda: cfg("Hover", 16, tape_in_scratch_horizon("Hover"), 8, 4, 2, 2, sample_whole_control_space=1),   # the per-problem scratch stride
}
BUFFERS = ("Q", "J", "U_NOM", "PLAN", "ADAM_M", "ADAM_V", "AGES", "AGES_LOGGED", "BEST_IDX")
PARAMS = {"CartPole": (("dd_weight", 450.0), ("m_pole", 0.11)), "Quad2D": (("pos_weight", 310.0), ("mass", 0.62)),
          "Hover": (("ang_weight", 95.0), ("drag_lin", 0.41))}       # one cost weight and one plant parameter per environment


def make(config, B, seeds=None, handles_for=None, **kw):
    """(batch, {p: the single handle of problem p})"""
    seeds = [11 + 3 * q for q in range(B)] if seeds is None else seeds
    common = dict(CONFIGS[config]() if isinstance(config, str) else config)
    common.update(kw)
    batch = CtkRpgdBatch(B, seeds=seeds, **common)
    handles = {q: CtkEngine("rpgd", "ODE", seed=seeds[q], generic_kernels=True, **common) for q in (range(B) if handles_for is None else handles_for)}
    return batch, handles


def states(rng, n, S):
    s = rng.uniform(-0.4, 0.4, (n, S)).astype(np.float32)
    if S == 4:
        s[:, 2] += 2.6          # CartPole: the pendulum hangs away from the target
    return s


def draw_block(rng, batch, rows):
    """[rows, P, C] raw draws of the batch's sampling distribution"""
    P = batch.samples_needed_reset() // (batch.N * batch.C)
    shape = (rows, P, batch.C)
    return (rng.uniform(0.0, 1.0, shape) if int(batch.cfg.sampling_distribution) == 0 else rng.standard_normal(shape)).astype(np.float32)


def reset_both(batch, handles, rng, host, ids=None):
    ids = list(range(len(batch))) if ids is None else ids
    blocks = [draw_block(rng, batch, batch.N) for _ in ids] if host else None
    batch.reset(None if blocks is None else np.stack(blocks), ids=ids)
    for j, q in enumerate(ids):
        if q in handles:
            handles[q].reset(None if blocks is None else blocks[j])


def step_both(batch, handles, rng, s, host, up=None, ids=None, tag=""):
    """one step of the listed problems on both sides; host draws in the concatenated form (a block for exactly the problems that draw)"""
    ids = list(range(len(batch))) if ids is None else ids
    blocks = {q: draw_block(rng, batch, batch.N - batch.K) for q in ids if batch.samples_needed(q)} if host else {}
    for q, blk in blocks.items():
        assert blk.size == batch.samples_needed(q)
    cat = np.concatenate([blocks[q].ravel() for q in ids if q in blocks]) if blocks else (np.zeros(0, np.float32) if host else None)
    u = batch.step(s, cat, u_prev=up, ids=ids)
    assert u.shape == (len(ids), batch.C) and np.all(np.isfinite(u))
    for j, q in enumerate(ids):
        if q in handles:
            uh = handles[q].step(s[j], blocks.get(q), u_prev=None if up is None else up[j])
            np.testing.assert_array_equal(u[j], uh, err_msg=f"{tag}: u of problem {q}")
    return u


def compare(batch, handles, problems, tag):
    for q in problems:
        h = handles[q]
        for name in BUFFERS:
            got = batch.read(name, q)
            np.testing.assert_array_equal(got, h.read(name).reshape(got.shape), err_msg=f"{tag}: {name} of problem {q}")
        np.testing.assert_array_equal(batch.get_state(q), h.get_state(), err_msg=f"{tag}: state vector of problem {q}")
        assert batch.rng_position(q) == h.rng_position(), f"{tag}: Philox position of problem {q}"
        assert batch.samples_needed(q) == h.samples_needed(), f"{tag}: samples_needed of problem {q}"


def snapshot(batch, q):
    return [batch.read(name, q) for name in BUFFERS] + [batch.get_state(q), np.array([batch.rng_position(q), batch.samples_needed(q)])]


def assert_untouched(batch, q, before, tag):
    for a, b in zip(before, snapshot(batch, q)):
        np.testing.assert_array_equal(a, b, err_msg=f"{tag}: problem {q} was not listed")


def close_all(batch, handles):
    batch.close()
    for h in handles.values():
        h.close()


# ---- 1. batch == single handles, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["philox", "host"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("B", [1, 3, 5])
def test_batch_equals_single_handles(B, config, source):
    """after a reset, 2 * resamp_per + 1 steps (resampling and plain steps both ways round) from states that differ per problem and per
    step, u_prev alternating between given and None"""
    batch, handles = make(config, B)
    host = source == "host"
    rng = np.random.default_rng(B * 131 + len(config))
    if config == "hover_tape_in_scratch":
        assert not CtkRpgdBatch.descent_lds("Hover", batch.H)[1] and CtkRpgdBatch.descent_lds("Hover", batch.H - 8)[1]
    reset_both(batch, handles, rng, host)
    compare(batch, handles, range(B), f"{config} B={B} {source} after the reset")
    for t in range(2 * int(batch.cfg.resamp_per) + 1):
        up = rng.uniform(-1.0, 1.0, (B, batch.C)).astype(np.float32) if t % 2 == 0 else None
        step_both(batch, handles, rng, states(rng, B, batch.S), host, up, tag=f"{config} B={B} {source} step {t}")
        compare(batch, handles, range(B), f"{config} B={B} {source} after step {t}")
    close_all(batch, handles)


def test_more_problems_than_compute_units():
    """B = 300 workgroups in one launch, more than the chip has compute units: nothing waits for anything"""
    B, watched = 300, (0, 137, 299)
    batch, handles = make("cartpole_small", B, handles_for=watched)
    rng = np.random.default_rng(5)
    reset_both(batch, handles, rng, False)
    for t in range(2):
        u = step_both(batch, handles, rng, states(rng, B, batch.S), False, tag=f"B=300 step {t}")
        assert np.all(np.isfinite(u)) and np.all(u >= -1.0) and np.all(u <= 1.0)
    compare(batch, handles, watched, "B=300")
    close_all(batch, handles)


def test_device_pointer_samples_with_per_problem_offsets():
    """the third sample source: ONE device buffer holding the concatenated blocks (reset: [n, N, P, C]; step: a block for exactly the
    problems that draw, so a problem's block starts where the drawing problems before it end), the handles reading their own block
    through a device pointer as well"""
    import torch
    B = 4
    batch, handles = make("quad2d", B)
    rng = np.random.default_rng(31)
    blocks = [draw_block(rng, batch, batch.N) for _ in range(B)]
    t = torch.from_numpy(np.stack(blocks)).to("cuda")
    torch.cuda.synchronize()
    batch.reset(t.data_ptr())
    for q in range(B):
        handles[q].reset(t.data_ptr() + 4 * q * blocks[0].size, 2)              # CTK_LOC_DEVICE
    compare(batch, handles, range(B), "device-pointer reset")
    step_both(batch, handles, rng, states(rng, B, batch.S), False, tag="all in step")        # counts 1: nobody draws next
    reset_both(batch, handles, rng, False, ids=[1, 3])                                       # counts 1, 0, 1, 0: problems 1 and 3 draw
    for it in range(3):
        ids = [0, 1, 3] if it == 1 else list(range(B))
        drawing = [q for q in ids if batch.samples_needed(q)]
        blocks = {q: draw_block(rng, batch, batch.N - batch.K) for q in drawing}
        cat = np.concatenate([blocks[q].ravel() for q in drawing]) if drawing else np.zeros(1, np.float32)
        t = torch.from_numpy(cat).to("cuda")
        torch.cuda.synchronize()
        offs = dict(zip(drawing, np.cumsum([0] + [blocks[q].size for q in drawing])[:-1]))
        s = states(rng, len(ids), batch.S)
        u = batch.step(s, t.data_ptr(), ids=ids)
        for j, q in enumerate(ids):
            uh = handles[q].step(s[j], t.data_ptr() + 4 * int(offs[q]) if q in offs else None)
            np.testing.assert_array_equal(u[j], uh, err_msg=f"device-pointer step {it}: u of problem {q}")
        compare(batch, handles, range(B), f"device-pointer step {it}")
        if it == 0:
            assert drawing == [1, 3]                          # problem 3's block lies behind problem 1's, not at 3 blocks' distance
    close_all(batch, handles)


def test_mixed_iteration_counts_and_resampling_in_one_launch():
    """subset resets put a warm-up step (5 iterations, resampling), a resampling step and a plain step (2 iterations each) at different
    Adam step numbers into ONE launch; host draws in the concatenated form; a wrong total is refused and changes nothing"""
    B = 3
    batch, handles = make("cartpole_small", B, warmup=1, warmup_iterations=5)
    rng = np.random.default_rng(17)
    reset_both(batch, handles, rng, True)
    step_both(batch, handles, rng, states(rng, B, 4), True, tag="first step")                    # counts 1, 1, 1
    reset_both(batch, handles, rng, True, ids=[1])
    step_both(batch, handles, rng, states(rng, B, 4), True, tag="second step")                   # counts 2, 1, 2
    reset_both(batch, handles, rng, False, ids=[2])                                              # counts 2, 1, 0
    per = (batch.N - batch.K) * (batch.samples_needed_reset() // batch.N)
    assert [batch.samples_needed(q) for q in range(B)] == [per, 0, per]                          # resampling, plain, warm-up + resampling
    assert [int(batch.get_state(q)[-2]) for q in range(B)] == [7, 5, 0]                          # Adam step numbers differ as well
    before = [snapshot(batch, q) for q in range(B)]
    s = states(rng, B, 4)
    for wrong in (per, 3 * per, 2 * per + 1):
        with pytest.raises(ValueError, match=rf"{wrong} samples given, the listed problems need {2 * per}\b"):
            batch.step(s, np.zeros(wrong, np.float32))
    for q in range(B):
        assert_untouched(batch, q, before[q], "after the refused steps")
    compare(batch, handles, range(B), "after the refused steps")
    step_both(batch, handles, rng, s, True, tag="mixed launch")
    assert [int(batch.get_state(q)[-2]) for q in range(B)] == [9, 7, 5]
    compare(batch, handles, range(B), "after the mixed launch")
    step_both(batch, handles, rng, states(rng, B, 4), False, up=rng.uniform(-1, 1, (B, 1)).astype(np.float32), tag="mixed launch, Philox")
    compare(batch, handles, range(B), "after the second mixed launch")
    close_all(batch, handles)


def test_subset_steps_resets_and_set_state():
    B = 4
    batch, handles = make("quad2d", B)
    rng = np.random.default_rng(23)
    S = batch.S
    reset_both(batch, handles, rng, False, ids=[0, 1, 2])                                        # problem 3 stays as created
    with pytest.raises(CtkError, match=r"problem 3 was never reset"):
        batch.step(states(rng, B, S))
    with pytest.raises(CtkError, match=r"problem 3 was never reset"):
        batch.step(states(rng, 2, S), ids=[1, 3])
    compare(batch, handles, [0, 1, 2], "nothing was launched")
    step_both(batch, handles, rng, states(rng, 3, S), False, ids=[0, 1, 2], tag="three of four")
    compare(batch, handles, [0, 1, 2], "three of four")
    before = snapshot(batch, 1)
    step_both(batch, handles, rng, states(rng, 2, S), True, ids=[0, 2], up=rng.uniform(-0.8, 0.8, (2, batch.C)).astype(np.float32), tag="subset")
    assert_untouched(batch, 1, before, "subset step")
    reset_both(batch, handles, rng, True, ids=[3])
    assert_untouched(batch, 1, before, "subset reset")
    step_both(batch, handles, rng, states(rng, 2, S), False, ids=[1, 3], tag="late starter")
    compare(batch, handles, range(B), "late starter")
    st = handles[0].get_state()                                                                  # a handle's state continues inside the batch
    batch.set_state(2, st)
    handles[2].set_state(st)
    before = snapshot(batch, 3)
    reset_both(batch, handles, rng, False, ids=[0])
    assert_untouched(batch, 3, before, "reset of another problem")
    batch.set_rng_position(1, 1000)
    handles[1].set_rng_position(1000)
    for t in range(3):
        step_both(batch, handles, rng, states(rng, B, S), t == 1, tag=f"whole batch {t}")
        compare(batch, handles, range(B), f"whole batch {t}")
    close_all(batch, handles)


@pytest.mark.parametrize("config", ["cartpole_small", "quad2d", "hover"])
def test_set_param_reaches_every_problem(config):
    B = 3
    batch, handles = make(config, B)
    rng = np.random.default_rng(29)
    reset_both(batch, handles, rng, False)
    step_both(batch, handles, rng, states(rng, B, batch.S), False, tag="defaults")
    ref = batch.read_all("J")
    for name, value in PARAMS[batch.environment]:
        batch.set_param(name, value)
        assert batch.get_param(name) == np.float32(value)
        for h in handles.values():
            h.set_param(name, value)
        step_both(batch, handles, rng, states(rng, B, batch.S), False, tag=f"{name} set")
        compare(batch, handles, range(B), f"{name} set")
    assert not np.array_equal(ref, batch.read_all("J"))
    close_all(batch, handles)


# ---- the reference-recorded fixtures inside a batch ---------------------------------------------------------------------------------------
class ProblemAsEngine:
    """Problem `me` of a batch behind the CtkEngine calls the handles' reference-golden tests make, with a single handle that receives
    the same calls beside it: every step and every read asserts the two bit-equal, the neighbours run other seeds, states and draws in
    the same launches."""

    def __init__(self, batch, me, handle, rng):
        self.batch, self.me, self.handle, self.rng = batch, me, handle, rng
        self.S, self.C = batch.S, batch.C

    def set_param(self, name, value):
        self.batch.set_param(name, value)
        self.handle.set_param(name, value)

    def reset(self, draws):
        blocks = [draw_block(self.rng, self.batch, self.batch.N) for _ in range(len(self.batch))]
        blocks[self.me] = np.asarray(draws, np.float32).reshape(blocks[self.me].shape)
        self.batch.reset(np.stack(blocks))
        self.handle.reset(draws)

    def samples_needed(self):
        assert self.batch.samples_needed(self.me) == self.handle.samples_needed()
        return self.batch.samples_needed(self.me)

    def read(self, name):
        got, want = self.batch.read(name, self.me), self.handle.read(name)
        np.testing.assert_array_equal(got, want.reshape(got.shape), err_msg=f"{name} of problem {self.me} against its handle")
        return want

    def step(self, s, samples, u_prev=None):
        B, me = len(self.batch), self.me
        S = states(self.rng, B, self.S)
        S[me] = s
        blocks = []
        for q in range(B):                                   # every problem that draws gets a block; the fixture's goes to `me`
            if self.batch.samples_needed(q):
                blocks.append(np.asarray(samples, np.float32).ravel() if q == me else draw_block(self.rng, self.batch, self.batch.N - self.batch.K).ravel())
        up = self.rng.uniform(-0.5, 0.5, (B, self.C)).astype(np.float32)
        up[me] = np.asarray(u_prev, np.float32).reshape(-1)
        u = self.batch.step(S, np.concatenate(blocks) if blocks else None, u_prev=up)
        uh = self.handle.step(s, samples, u_prev=u_prev)
        np.testing.assert_array_equal(u[me], uh)
        assert np.all(np.isfinite(u))
        np.testing.assert_array_equal(self.batch.get_state(me), self.handle.get_state())
        assert self.batch.rng_position(me) == self.handle.rng_position()
        return uh

    def set_state(self, st):
        self.batch.set_state(self.me, st)
        self.handle.set_state(st)

    def close(self):
        self.batch.close()
        self.handle.close()


def strict_close(actual, desired, rtol, atol, **_):
    """the handles' Hover test allows a few outliers; a problem of a batch gets none"""
    np.testing.assert_allclose(actual, desired, rtol=rtol, atol=atol)


@pytest.mark.parametrize("fixture", ["rpgd_ode_small", "rpgd_ode_normal", "rpgd_quad2d", "rpgd_hover_ode"])
def test_reference_fixture_inside_a_batch(monkeypatch, fixture):
    """the fixture's draws, states and set_state sequence fed to problem 1 of B = 3 by the body of the handle's own reference-golden test
    (its tolerances, nothing restated, no outlier allowance): bit-equal to a template handle, and within the reference's tolerances"""
    made = []

    def engine(opt, pred, **kw):
        assert opt == "rpgd" and pred == "ODE"
        handle = CtkEngine(opt, pred, generic_kernels=True, **kw)
        batch = CtkRpgdBatch(3, seeds=[41, int(kw.get("seed", 0)), 43], **kw)
        made.append(batch.dominant_kernel())
        return ProblemAsEngine(batch, 1, handle, np.random.default_rng(37))

    case = fixture[len("rpgd_"):]
    if case in ("ode_small", "ode_normal"):
        import gpu_helpers
        monkeypatch.setattr(gpu_helpers, "CtkEngine", engine)
        test_gpu_rpgd.test_rpgd_matches_reference_golden(case)
    elif case == "quad2d":
        monkeypatch.setattr(test_gpu_env, "CtkEngine", engine)
        test_gpu_env.test_quad2d_rpgd_matches_reference_golden(case)
    else:
        monkeypatch.setattr(test_gpu_hover, "CtkEngine", engine)
        monkeypatch.setattr(test_gpu_hover, "assert_close_mostly", strict_close)
        test_gpu_hover.test_hover_rpgd_matches_reference_golden(case)
    assert len(made) == 1 and made[0].startswith("ctk_g_rpgd_batch<")


def test_dominant_kernel_names():
    for config, env_id in (("cartpole_small", 0), ("quad2d", 1), ("hover", 2)):
        batch, handles = make(config, 2, handles_for=[0])
        assert batch.dominant_kernel() == f"ctk_g_rpgd_batch<{env_id}>"
        assert handles[0].dominant_kernel() == f"ctk_g_rpgd_descent<{env_id}>"          # the handle the contract refers to
        close_all(batch, handles)


# ---- what a batch allocates: a staging buffer that grows, destroy, create again ------------------------------------------------------------------
def test_state_survives_destroy_and_create_after_buffers_grew():
    """The staging buffer grows (host draws for one problem, then for all); then every problem's state is read, the batch destroyed,
    created again from the same seeds and given the states and Philox positions back: its next step, by the in-kernel sampler, equals
    bit for bit that of a batch that took the same steps and was never destroyed."""
    kw = dict(seeds=[11, 14, 17], **CONFIGS["cartpole_small"]())
    rng = np.random.default_rng(47)
    s, s_next = states(rng, 3, 4), states(rng, 3, 4)

    def used(batch):
        draws = np.random.default_rng(48)
        batch.reset()
        for ids in ([1], [0, 1, 2]):
            blocks = [draw_block(draws, batch, batch.N - batch.K).ravel() for q in ids if batch.samples_needed(q)]
            assert blocks                                   # the step after a reset resamples: there are draws to stage
            batch.step(s[ids], np.concatenate(blocks), ids=ids)
        return batch

    a, ref = used(CtkRpgdBatch(3, **kw)), used(CtkRpgdBatch(3, **kw))
    saved = [(a.get_state(q), a.rng_position(q)) for q in range(3)]
    a.close()
    a = CtkRpgdBatch(3, **kw)
    for q, (state, position) in enumerate(saved):
        np.testing.assert_array_equal(state, ref.get_state(q))
        a.set_state(q, state)                               # marks the problem reset
        a.set_rng_position(q, position)
    np.testing.assert_array_equal(a.step(s_next), ref.step(s_next))
    for q in range(3):
        for name in BUFFERS:
            np.testing.assert_array_equal(a.read(name, q), ref.read(name, q), err_msg=f"{name} of problem {q}")
        np.testing.assert_array_equal(a.get_state(q), ref.get_state(q), err_msg=f"state vector of problem {q}")
        assert a.rng_position(q) == ref.rng_position(q)
    a.close()
    ref.close()
