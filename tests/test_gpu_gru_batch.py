"""-m gpu: CtkMppiGruBatch (ctk_gru_batch_* / ctk_gru_problem_*, kernels ctk_mppi_batch_gru<LOG, FORM> / ctk_mppi_batch_gru_pp<LOG, FORM> and
ctk_gru_advance_batch) — B independent MPPI problems whose plant model is a GRU with a carried hidden state, stepped by one rollout launch
and one hidden-state launch, every problem with a network and a hidden state of its own.

The contract under test: problem p of a batch behaves BIT FOR BIT like a CtkEngine("mppi", "GRU", seed=seeds[p]) created from the same
configuration that received the same calls — set_predictor_weights, set_param, step, reset, set_state, predictor_get_hidden /
predictor_set_hidden — the carried hidden state after every step included.  Every comparison against single handles and between batches is
assert_array_equal; the only tolerances in this file are those tests/test_gpu_gru.py applies to a single handle against the oracle
(TRAJ_TOL, U_TOL, J rtol 1e-4 / atol 2e-3, hidden state rtol 1e-4 / atol 2e-5), applied to two problems INSIDE a batch."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiGruBatch, CtkError
from control_toolkit_amd._capi import gru_batch_fit, gru_weight_count
from gpu_helpers import apply_env
from test_gpu_gru import TRAJ_TOL, U_TOL

pytestmark = pytest.mark.gpu

# (N, H, period): one workgroup | five workgroups, the last one partial | 64 records of 32 words = 2 048, the last narrow tail | 64 x 33: the
# first wide one | cfg2, the headline size: 64 x 52 | 128 records, interpolated
SMALL = [(16, 5, 2), (70, 12, 5)]
LARGE = [(1024, 30, 1), (1024, 31, 1), (1024, 50, 1), (2048, 40, 10)]
SOURCES = [("philox", True), ("host", False), ("devptr", True), ("philox", False), ("host", True), ("devptr", False)]   # (draws, u_prev given)
STEPS = 5
LIMIT = 32768.0                                         # CTK_SINCOS_FAST_LIMIT: beyond it a rollout takes the checked cosine
PLANT = O.Predictor("ODE", dt=0.02, env=O.EnvParams())
_W = {}


def weights(seed, hidden=(32, 32)):
    """one network, computed once: O.gru_default_weights(seed), or for narrower widths draws of the same scale in the raw layout"""
    key = (seed, hidden)
    if key not in _W:
        if hidden == (32, 32):
            _W[key] = O.gru_default_weights(seed)
        else:
            _W[key] = (0.3 * np.random.default_rng(seed).standard_normal(gru_weight_count(4, 1, hidden))).astype(np.float32)
        _W[key].setflags(write=False)
    return _W[key]


def make(size, B, materialize, weight_seeds="own", hidden=None, **kw):
    """(batch, B single handles with seeds[p]); weight_seeds: "own" = seed 100 + p per problem, None = no weights yet"""
    N, H, p = size
    seeds = [7 + q for q in range(B)]
    common = dict(num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=materialize, **kw)
    batch = CtkMppiGruBatch(B, seeds=seeds, **({} if hidden is None else {"predictor_hidden": hidden}), **common)
    handles = [CtkEngine("mppi", "GRU", seed=seeds[q], **common) for q in range(B)]
    if weight_seeds == "own":
        hid = (32, 32) if hidden is None else hidden
        batch.set_problem_weights(np.stack([weights(100 + q, hid) for q in range(B)]))
        for q in range(B):
            handles[q].set_predictor_weights(weights(100 + q, hid), hidden=hid)
    return batch, handles


def first_states(rng, B):
    s = rng.uniform(-0.4, 0.4, (B, 4)).astype(np.float32)
    s[:, 2] += 2.6          # the pendulum hangs away from the target
    return s


def draws_for(source, rng, n, batch):
    """(what the batch is given, what handle row j is given, keep-alive)"""
    if source == "philox":
        return None, [None] * n, None
    arr = rng.standard_normal((n, batch.N, batch.samples_needed() // batch.N, 1)).astype(np.float32)
    if source == "host":
        return arr, [arr[j] for j in range(n)], None
    import torch
    t = torch.from_numpy(arr).to("cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), [t.data_ptr() + 4 * j * arr[0].size for j in range(n)], t


def hidden_of(handles, problems):
    return np.stack([handles[q].predictor_get_hidden() for q in problems])


def compare(batch, handles, problems, materialize, tag):
    problems = list(problems)
    np.testing.assert_array_equal(batch.get_hidden(problems), hidden_of(handles, problems), err_msg=f"{tag}: hidden states")
    for q in problems:
        h = handles[q]
        np.testing.assert_array_equal(batch.read("U_NOM", q), h.read("U_NOM"), err_msg=f"{tag}: U_NOM of problem {q}")
        np.testing.assert_array_equal(batch.read("J", q), h.read("J"), err_msg=f"{tag}: J of problem {q}")
        np.testing.assert_array_equal(batch.get_state(q), h.get_state(), err_msg=f"{tag}: state vector of problem {q}")
        assert batch.rng_position(q) == h.rng_position(), f"{tag}: Philox position of problem {q}"
        if materialize:
            np.testing.assert_array_equal(batch.read("Q", q), h.read("Q"), err_msg=f"{tag}: Q of problem {q}")
            np.testing.assert_array_equal(batch.read("TRAJ", q), h.read("TRAJ"), err_msg=f"{tag}: TRAJ of problem {q}")


def step_both(batch, handles, s, ids=None, up=None):
    """one step of the listed problems on both sides (device Philox); asserts u bit for bit and returns it"""
    idl = list(range(len(handles))) if ids is None else list(ids)
    u = batch.step(s[idl] if ids is not None else s, u_prev=up, ids=ids)
    uh = np.stack([handles[q].step(s[q], u_prev=None if up is None else up[j]) for j, q in enumerate(idl)])
    np.testing.assert_array_equal(u, uh)
    return u


def close_all(batch, handles):
    batch.close()
    for h in handles:
        h.close()


def snapshot(batch, q):
    return dict(U_NOM=batch.read("U_NOM", q), J=batch.read("J", q), Q=batch.read("Q", q), TRAJ=batch.read("TRAJ", q),
                state=batch.get_state(q), rng=batch.rng_position(q), hidden=batch.get_hidden([q]))


def assert_unchanged(batch, q, snap, tag):
    now = snapshot(batch, q)
    for k, v in snap.items():
        np.testing.assert_array_equal(now[k], v, err_msg=f"{tag}: {k} of untouched problem {q} changed")


def kernel_names(size, materialize, per_problem=False):
    """(the batch's kernel, the kernel of a handle of that size): the same form — from the fit, which tests/test_gru_batch_cpu.py pins"""
    log = "true" if materialize else "false"
    wide = gru_batch_fit(*size)[3]
    return (f"ctk_mppi_batch_gru{'_pp' if per_problem else ''}<{log}, {1 if wide else 0}>",
            f"ctk_mppi_rollout<0, 2, {log}, false, 1>" if wide else f"ctk_mppi_rollout<0, 2, {log}, false>")


# ---- 1. batch == single handles, bit for bit, every problem with its own network and hidden state ---------------------------------------
CASES = [(B, size) for size in SMALL for B in (1, 3, 16)] + [(3, size) for size in LARGE]


@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("B,size", CASES)
def test_batch_equals_single_handles(B, size, materialize):
    """every sample source with u_prev given and None, one after another on the SAME objects: STEPS closed-loop steps each on the oracle's
    plant with every problem's own output fed back; everything compared after every step"""
    batch, handles = make(size, B, materialize)
    assert batch.weight_count() == O.gru_num_weights() and all(batch.have_weights(q) for q in range(B))
    want_batch, want_handle = kernel_names(size, materialize)
    assert batch.dominant_kernel() == want_batch
    rng = np.random.default_rng(B * 131 + size[0])
    s = first_states(rng, B)
    for source, given in SOURCES:
        for t in range(STEPS):
            up = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32) if given else None
            bs, hs, keep = draws_for(source, rng, B, batch)
            u = batch.step(s, bs, u_prev=up)
            uh = np.stack([handles[q].step(s[q], hs[q], u_prev=None if up is None else up[q]) for q in range(B)])
            tag = f"{size} B={B} {source} u_prev={'given' if given else 'None'} step {t}"
            np.testing.assert_array_equal(u, uh, err_msg=f"{tag}: u")
            compare(batch, handles, range(B), materialize, tag)
            s = PLANT.step(s, u).astype(np.float32)
            del keep
    assert batch.get_hidden().any()                        # the carried states did move
    assert handles[0].dominant_kernel() == want_handle     # the form compared with
    close_all(batch, handles)


# ---- 2. split into launches: the advance is issued once per record ------------------------------------------------------------------------
def test_split_into_launches_gives_the_same_bits(monkeypatch):
    """B = 5 with CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH = 2 runs as three rollout launches (2 + 2 + 1) and one advance, and gives the bits of
    one launch; an id list longer than the cap as well"""
    B, size = 5, (70, 12, 5)
    one, handles = make(size, B, True)
    monkeypatch.setenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH", "2")
    split = CtkMppiGruBatch(B, seeds=[7 + q for q in range(B)], num_rollouts=size[0], mpc_horizon=size[1], dt=0.02, materialize_trajectories=True,
                            period_interpolation_inducing_points=size[2])
    monkeypatch.delenv("CTK_BATCH_MAX_PROBLEMS_PER_LAUNCH")
    split.set_problem_weights(np.stack([weights(100 + q) for q in range(B)]))
    s = first_states(np.random.default_rng(40), B)
    for t in range(STEPS):
        u1 = step_both(one, handles, s)
        np.testing.assert_array_equal(split.step(s), u1)
        compare(split, handles, range(B), True, f"three launches, step {t}")
        s = PLANT.step(s, u1).astype(np.float32)
    compare(one, handles, range(B), True, "one launch")
    ids = [0, 2, 3]
    u2 = split.step(s[ids], ids=ids)
    np.testing.assert_array_equal(u2, np.stack([handles[q].step(s[q]) for q in ids]))
    compare(split, handles, range(B), True, "subset over two launches")      # the unlisted problems' hidden states stayed
    split.close()
    close_all(one, handles)


# ---- 3. subset steps and resets -----------------------------------------------------------------------------------------------------------
def test_subset_steps_and_resets():
    B, size = 6, (70, 12, 5)
    batch, handles = make(size, B, True)
    rng = np.random.default_rng(8)
    s = first_states(rng, B)
    for t in range(2):
        s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    ids = [1, 4, 5]
    rest = [q for q in range(B) if q not in ids]
    snaps = {q: snapshot(batch, q) for q in rest}
    for t in range(3):
        u = step_both(batch, handles, s, ids=ids)
        s[ids] = PLANT.step(s[ids], u).astype(np.float32)
    for q in rest:
        assert_unchanged(batch, q, snaps[q], "subset step")          # hidden state, plan, outputs and Philox position
    compare(batch, handles, range(B), True, "after subset steps")
    snaps = {q: snapshot(batch, q) for q in range(B)}
    batch.reset([4])
    handles[4].reset()
    for q in snaps:
        if q != 4:
            assert_unchanged(batch, q, snaps[q], "reset([4])")
    np.testing.assert_array_equal(batch.get_hidden([4]), snaps[4]["hidden"])     # ctk_reset leaves a handle's hidden state alone
    compare(batch, handles, [4], True, "after reset([4])")
    batch.set_rng_position(2, 17); handles[2].set_rng_position(17)
    batch.set_state(1, snaps[1]["state"]); handles[1].set_state(snaps[1]["state"])
    np.testing.assert_array_equal(batch.get_hidden([1]), snaps[1]["hidden"])     # ... and so does ctk_set_state
    for t in range(2):
        up = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
        s = PLANT.step(s, step_both(batch, handles, s, up=up)).astype(np.float32)
    compare(batch, handles, range(B), True, "after the reset and two more steps")
    close_all(batch, handles)


# ---- 4. no weight or hidden-state call touches another problem's hidden state --------------------------------------------------------------
def test_hidden_state_isolation():
    B, size = 3, (70, 12, 5)
    batch, handles = make(size, B, True)
    rng = np.random.default_rng(4)
    s = first_states(rng, B)
    for t in range(2):
        s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    before = batch.get_hidden()
    assert before.any(axis=(1, 2)).all()
    batch.set_problem_weights(np.stack([weights(200), weights(202)]), ids=[0, 2])
    handles[0].set_predictor_weights(weights(200)); handles[2].set_predictor_weights(weights(202))
    after = batch.get_hidden()
    np.testing.assert_array_equal(after[1], before[1], err_msg="set_problem_weights([0, 2]) moved problem 1's hidden state")
    assert not after[0].any() and not after[2].any()
    compare(batch, handles, range(B), True, "after new networks for problems 0 and 2")
    s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    compare(batch, handles, range(B), True, "the step after them")
    # set_hidden on a subset, then zeros for all
    before = batch.get_hidden()
    hid = rng.uniform(-0.9, 0.9, (2, 2, 32)).astype(np.float32)
    batch.set_hidden(hid, ids=[1, 2])
    handles[1].predictor_set_hidden(hid[0]); handles[2].predictor_set_hidden(hid[1])
    after = batch.get_hidden()
    np.testing.assert_array_equal(after[0], before[0], err_msg="set_hidden([1, 2]) moved problem 0's hidden state")
    np.testing.assert_array_equal(after[1:], hid)
    s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    compare(batch, handles, range(B), True, "the step after set_hidden([1, 2])")
    batch.set_hidden(None, ids=[0])
    handles[0].predictor_set_hidden(None)
    assert not batch.get_hidden([0]).any()
    compare(batch, handles, range(B), True, "set_hidden(None, [0])")
    batch.set_hidden(None)
    for h in handles:
        h.predictor_set_hidden(None)
    assert not batch.get_hidden().any()
    s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    compare(batch, handles, range(B), True, "the step after set_hidden(None)")
    batch.set_weights(weights(5))                          # one network for all: every hidden state is zero again
    for h in handles:
        h.set_predictor_weights(weights(5))
    assert not batch.get_hidden().any()
    step_both(batch, handles, s)
    compare(batch, handles, range(B), True, "shared network")
    close_all(batch, handles)


# ---- 5. the choice between the unchecked and the checked cosine, per problem and per step, inside one launch ---------------------------
def test_cosine_decision_per_problem_inside_one_launch():
    """problem 0 is ordinary, problem 1 is given an angle beyond the unchecked cosine's range, problem 2 a caller-set hidden state large
    enough for net_out_bound * hidden_scale to exceed it, problem 3 both: each equals its handle, which decides per step on the host"""
    B, size = 4, (70, 12, 5)
    batch, handles = make(size, B, True)
    s = first_states(np.random.default_rng(5), B)
    s[1, 2] += 40000.0
    s[3, 2] -= 50000.0
    big = np.zeros((2, 2, 32), np.float32)
    big[:, 1, :4] = 1.0e5                                  # max |h| = 1e5: with any output row's |W_o| sum above 0.33 the bound is past 32 768
    batch.set_hidden(big, ids=[2, 3])
    handles[2].predictor_set_hidden(big[0]); handles[3].predictor_set_hidden(big[1])
    for t in range(3):
        u = step_both(batch, handles, s)
        compare(batch, handles, range(B), True, f"mixed cosine decisions, step {t}")
        s[0] = PLANT.step(s[0:1], u[0:1]).astype(np.float32)[0]
    # a zero hidden state resets hidden_scale, as a handle's entry does: problem 2 is ordinary again
    batch.set_hidden(None, ids=[2]); handles[2].predictor_set_hidden(None)
    step_both(batch, handles, s)
    compare(batch, handles, range(B), True, "after set_hidden(None, [2])")
    close_all(batch, handles)


def crossing_start():
    """a start state from which the ORACLE's plant carries the angle across LIMIT within 4 steps whatever the input in [-1, 1]"""
    s0 = np.array([0.0, 0.0, LIMIT - 0.25, 10.0], np.float32)
    for u in (-1.0, 0.0, 1.0):
        s, crossed = s0[None].copy(), None
        for k in range(4):
            s = PLANT.step(s, np.full((1, 1), u, np.float32)).astype(np.float32)
            if crossed is None and abs(s[0, 2]) > LIMIT:
                crossed = k + 1
        assert crossed is not None and crossed >= 2, (u, crossed)          # not at once: the run starts on the unchecked side
    return s0


def test_cosine_decision_inside_a_run():
    """the plant carries problem 1's angle across the limit in mid-run, where the state of the next step exists on the device only: the run
    equals the loop of step and plant_step, and handles stepped on the realised states"""
    B, size, steps = 3, (70, 12, 5), 6
    a, handles = make(size, B, True)
    b, _unused = make(size, B, True)
    for h in _unused:
        h.close()
    S0 = first_states(np.random.default_rng(6), B)
    S0[1] = crossing_start()
    states, inputs = a.closed_loop.run(S0, steps)
    th = np.abs(states[1, :, 2])
    assert th[0] <= LIMIT and th[1] <= LIMIT and (th[:5] > LIMIT).any(), th
    S = S0.copy()
    for k in range(steps):
        u = b.step(S)
        uh = np.stack([handles[q].step(S[q]) for q in range(B)])
        np.testing.assert_array_equal(u, uh, err_msg=f"step {k}")
        np.testing.assert_array_equal(inputs[:, k], u, err_msg=f"run, step {k}")
        S = b.closed_loop.plant_step(S, u)
        np.testing.assert_array_equal(states[:, k + 1], S, err_msg=f"run, state {k + 1}")
    compare(a, handles, range(B), True, "after the run")
    compare(b, handles, range(B), True, "after the loop")
    a.close()
    close_all(b, handles)


# ---- 6. one shared narrow network, per-problem parameters ----------------------------------------------------------------------------------
def test_shared_narrow_network_and_per_problem_parameters():
    B, hid, size = 4, (8, 20), (70, 12, 5)
    batch, handles = make(size, B, True, weight_seeds=None, hidden=hid)
    assert batch.weight_count() == gru_weight_count(4, 1, hid) == handles[0].predictor_weight_count(hid)
    assert not any(batch.have_weights(q) for q in range(B))
    batch.set_weights(weights(5, hid))
    for h in handles:
        h.set_predictor_weights(weights(5, hid), hidden=hid)
    assert all(batch.have_weights(q) for q in range(B))
    s = first_states(np.random.default_rng(2), B)
    for t in range(2):
        s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    compare(batch, handles, range(B), True, "shared 8-20 network")
    hid_now = batch.get_hidden()
    assert hid_now[:, 0, :8].any() and not hid_now[:, 0, 8:].any() and not hid_now[:, 1, 20:].any()      # the embedded units stay at zero
    batch.set_param("target_position", 0.3)
    for h in handles:
        h.set_param("target_position", 0.3)
    assert batch.params_differ() == 0 and batch.dominant_kernel() == kernel_names(size, True)[0]
    step_both(batch, handles, s)
    ids, vals = [0, 3], [-0.4, 0.7]
    batch.set_problem_params("target_position", vals, ids=ids)
    for q, v in zip(ids, vals):
        handles[q].set_param("target_position", v)
    assert batch.params_differ() == 1 and batch.dominant_kernel() == kernel_names(size, True, per_problem=True)[0]
    J1 = batch.read_all("J")
    for t in range(2):
        s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
        compare(batch, handles, range(B), True, "target_position per problem")
    assert not np.array_equal(batch.read_all("J")[ids], J1[ids])
    with pytest.raises(ValueError, match="weights"):
        batch.set_weights(weights(1))                     # a 32-32 network into a batch of 8-20 ones
    close_all(batch, handles)


@pytest.mark.parametrize("size", [(1024, 50, 1)])
def test_per_problem_parameters_in_the_wide_form(size):
    B = 3
    batch, handles = make(size, B, False)
    vals = [-0.4, 0.1, 0.7]
    batch.set_problem_params("target_position", vals)
    for q, v in enumerate(vals):
        handles[q].set_param("target_position", v)
    assert batch.dominant_kernel() == "ctk_mppi_batch_gru_pp<false, 1>"
    s = first_states(np.random.default_rng(12), B)
    for t in range(2):
        s = PLANT.step(s, step_both(batch, handles, s)).astype(np.float32)
    compare(batch, handles, range(B), False, "wide form, per-problem constants")
    close_all(batch, handles)


# ---- 7. closed loop ------------------------------------------------------------------------------------------------------------------------
def loop(batch, S0, steps):
    n = S0.shape[0]
    states, inputs = np.empty((n, steps + 1, 4), np.float32), np.empty((n, steps, 1), np.float32)
    states[:, 0] = S0
    for k in range(steps):
        inputs[:, k] = batch.step(states[:, k])
        states[:, k + 1] = batch.closed_loop.plant_step(states[:, k], inputs[:, k])
    return states, inputs


def test_run_is_the_loop_and_the_handles():
    B, size, steps = 3, (70, 12, 5), 6
    a, handles = make(size, B, True)
    b, extra = make(size, B, True)
    for h in extra:
        h.close()
    S0 = first_states(np.random.default_rng(70), B)
    states, inputs = a.closed_loop.run(S0, steps)
    np.testing.assert_array_equal(states[:, 0], S0)
    ls, li = loop(b, S0, steps)
    np.testing.assert_array_equal(inputs, li)
    np.testing.assert_array_equal(states, ls)
    for k in range(steps):                                 # three handles given what the controllers of the run were given
        uh = np.stack([handles[q].step(states[q, k]) for q in range(B)])
        np.testing.assert_array_equal(inputs[:, k], uh, err_msg=f"handles, step {k}")
        np.testing.assert_allclose(states[:, k + 1], PLANT.step(states[:, k], inputs[:, k]), rtol=1e-4, atol=2e-5)   # the plant is the analytic CartPole
    compare(a, handles, range(B), True, "after the run")
    compare(b, handles, range(B), True, "after the loop")
    # a subset run moves the listed problems alone, hidden states included
    snap = snapshot(a, 1)
    ids = [0, 2]
    got = a.closed_loop.run(S0[ids], 2, ids=ids)
    for k in range(2):
        np.testing.assert_array_equal(got[1][:, k], np.stack([handles[q].step(got[0][j, k]) for j, q in enumerate(ids)]))
    assert_unchanged(a, 1, snap, "subset run")
    compare(a, handles, range(B), True, "after the subset run")
    a.close()
    close_all(b, handles)


def test_episodes_are_the_noisy_loop():
    B, size, steps = 3, (70, 12, 5), 5
    a, ha = make(size, B, True)
    b, hb = make(size, B, True)
    for h in hb:
        h.close()
    for x in (a, b):
        x.closed_loop.set_noise(process=[0.0, 0.02, 0.0, 0.05], measurement=[0.01, 0.0, 0.03, 0.0])
    rng = np.random.default_rng(71)
    S0 = first_states(rng, B)
    up = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
    ep = a.closed_loop.episodes(S0, steps, u_prev=up)
    S, Y, U_prev = S0.copy(), S0.copy(), up
    for k in range(steps):
        U = b.step(Y, u_prev=up if k == 0 else None)
        np.testing.assert_array_equal(ep.inputs[:, k], U, err_msg=f"episode input {k}")
        np.testing.assert_array_equal(U, np.stack([ha[q].step(Y[q], u_prev=up[q] if k == 0 else None) for q in range(B)]))   # the handles see the observations
        S, Y, c = b.closed_loop.plant_step_noisy(S, U, U_prev)
        np.testing.assert_array_equal(ep.states[:, k + 1], S)
        np.testing.assert_array_equal(ep.observations[:, k + 1], Y)
        np.testing.assert_array_equal(ep.costs[:, k], c)
        U_prev = U
    assert not np.array_equal(ep.states, ep.observations)
    compare(a, ha, range(B), True, "after the episodes")
    compare(b, ha, range(B), True, "after the noisy loop")
    # with every sigma 0 an episode gives the states and inputs of a run
    for x in (a, b):
        x.closed_loop.clear_noise()
    ep0 = a.closed_loop.episodes(S0, 3)
    r = b.closed_loop.run(S0, 3)
    np.testing.assert_array_equal(ep0.states, r[0])
    np.testing.assert_array_equal(ep0.inputs, r[1])
    np.testing.assert_array_equal(ep0.observations, ep0.states)
    np.testing.assert_array_equal(a.get_hidden(), b.get_hidden())
    a.close()
    close_all(b, ha)


# ---- 8. a step without weights moves nothing ------------------------------------------------------------------------------------------------
def test_step_without_weights_moves_nothing():
    B = 4
    batch, handles = make((70, 12, 5), B, True, weight_seeds=None)
    s = first_states(np.random.default_rng(9), B)
    batch.set_problem_weights(np.stack([weights(100), weights(101)]), ids=[0, 1])
    for q in (0, 1):
        handles[q].set_predictor_weights(weights(100 + q))
    assert [batch.have_weights(q) for q in range(B)] == [True, True, False, False]
    hid = np.random.default_rng(10).uniform(-0.5, 0.5, (B, 2, 32)).astype(np.float32)
    batch.set_hidden(hid)                                  # (a hidden state may be set before the weights, as a handle's)
    for q in range(B):
        handles[q].predictor_set_hidden(hid[q])
    step_both(batch, handles, s, ids=[0, 1])
    snaps = {q: snapshot(batch, q) for q in range(B)}
    with pytest.raises(CtkError, match=r"\[ctk 5\] ctk_gru_batch_step: no network weights for problem\(s\) 2, 3 "):
        batch.step(s)
    with pytest.raises(CtkError, match=r"problem\(s\) 2 "):
        batch.step(s[[1, 2]], ids=[1, 2])
    with pytest.raises(CtkError, match=r"ctk_gru_batch_run: no network weights for problem\(s\) 2, 3 "):
        batch.closed_loop.run(s, 2)
    for q in range(B):
        assert_unchanged(batch, q, snaps[q], "refused step")          # plan, outputs, Philox position and hidden state
    step_both(batch, handles, s, ids=[0, 1])              # the refusals left the batch usable, and in step with the handles
    compare(batch, handles, [0, 1], True, "after the refused steps")
    np.testing.assert_array_equal(batch.get_hidden([2, 3]), hid[2:])
    close_all(batch, handles)


# ---- 9. two problems of the headline size against the oracle --------------------------------------------------------------------------------
def test_two_headline_problems_match_the_oracle():
    """the loop of tests/test_gpu_gru.py::test_mppi_gru_matches_oracle for (1024, 50, 1), with its tolerances, on both problems of a batch"""
    N, H, p, B = 1024, 50, 1, 2
    env = O.EnvParams(terminal_weight=0.25)
    ws = [O.gru_default_weights(1), O.gru_default_weights(2)]
    preds = [O.Predictor("GRU", dt=0.02, env=env, weights=w) for w in ws]
    os_ = [O.MPPI(pr, O.Cost(env), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p) for pr in preds]
    batch = CtkMppiGruBatch(B, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=True)
    apply_env(batch, env)
    batch.set_problem_weights(np.stack(ws))
    rng = np.random.default_rng(N)
    s = np.array([[0.1, -0.2, 2.5, 0.7], [-0.3, 0.1, 2.9, -0.4]], np.float32)
    for t in range(2):
        noise = rng.standard_normal((B, N, os_[0].P, 1)).astype(np.float32)
        uo = np.array([os_[q].step(s[q], noise[q]) for q in range(B)], np.float32).reshape(B, 1)
        ug = batch.step(s, noise)
        hid = batch.get_hidden()
        for q in range(B):
            np.testing.assert_allclose(batch.read("TRAJ", q), os_[q].rollout_trajectories, **TRAJ_TOL)
            np.testing.assert_allclose(batch.read("J", q), os_[q].J, rtol=1e-4, atol=2e-3)
            np.testing.assert_allclose(batch.read("U_NOM", q), os_[q].u_nom, **U_TOL)
            np.testing.assert_allclose(ug[q], uo[q], **U_TOL)
            np.testing.assert_allclose(hid[q], preds[q].hidden, rtol=1e-4, atol=2e-5)
            batch.set_state(q, np.concatenate([os_[q].u_nom.reshape(H), uo[q]]))     # keep both sides on the oracle's plan
        batch.set_hidden(np.stack([pr.hidden for pr in preds]))
        s = (s + np.float32(0.05) * rng.standard_normal((B, 4))).astype(np.float32)
    batch.close()


# ---- 10. state survives destroy and create ---------------------------------------------------------------------------------------------------
def test_state_survives_destroy_and_create():
    """state vector, Philox position and hidden state of every problem out of one batch and into a new one (which gets the networks anew:
    they are not state): its next steps equal those of a batch that was never destroyed"""
    N, H, p = SMALL[1]
    kw = dict(seeds=[7, 8, 9], num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=True)
    w = np.stack([weights(100 + q) for q in range(3)])
    rng = np.random.default_rng(43)
    s, s_next = first_states(rng, 3), first_states(rng, 3)

    def used(batch):
        batch.set_problem_weights(w)
        batch.step(s[1:2], ids=[1])
        batch.step(s)
        batch.closed_loop.run(s, 3)
        batch.closed_loop.episodes(s, 2)
        return batch

    a, ref = used(CtkMppiGruBatch(3, **kw)), used(CtkMppiGruBatch(3, **kw))
    saved = [(a.get_state(q), a.rng_position(q)) for q in range(3)]
    hid = a.get_hidden()
    np.testing.assert_array_equal(hid, ref.get_hidden())
    assert a.get_state(0).size == H + 1                    # neither weights nor hidden state are in the state vector
    a.close()
    a = CtkMppiGruBatch(3, **kw)
    a.set_problem_weights(w)
    a.set_hidden(hid)
    for q, (state, position) in enumerate(saved):
        a.set_state(q, state)
        a.set_rng_position(q, position)
    for t in range(2):
        u = ref.step(s_next)
        np.testing.assert_array_equal(a.step(s_next), u)
        s_next = PLANT.step(s_next, u).astype(np.float32)
    for q in range(3):
        for k, v in snapshot(ref, q).items():
            np.testing.assert_array_equal(snapshot(a, q)[k], v, err_msg=f"restored batch: {k} of problem {q}")
    a.close()
    ref.close()
