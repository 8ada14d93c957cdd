"""-m gpu: per-problem plant and cost parameters of a CtkRpgdBatch (ctk_rpgd_problem_set_param, kernel ctk_g_rpgd_batch_pp<ENV>).

The contract under test extends test_gpu_rpgd_batch.py's: problem p of a batch behaves BIT FOR BIT like a CtkEngine("rpgd", "ODE",
seed=seeds[p], generic_kernels=True) created from the same configuration that received the same calls, and set_param is one of those
calls - batch.set_problem_params(name, values, ids) is handles[q].set_param(name, values[j]) for every listed q, batch.set_param(name, v)
is set_param(name, v) on every handle.  Every comparison against single handles is assert_array_equal (u, Q, J, U_NOM, PLAN, ADAM_M,
ADAM_V, AGES, AGES_LOGGED, BEST_IDX, the state vector, the Philox position: test_gpu_rpgd_batch.compare); the only tolerances in this file
are those of the handles' reference-golden tests, whose bodies are RUN (not restated) on a problem of a batch in the per-problem form.
The sizes are test_gpu_rpgd_batch.CONFIGS: the smallest at which each branch of the kernel is taken."""
import ctypes
import os

import numpy as np
import pytest

from control_toolkit_amd import CtkEngine, CtkRpgdBatch
import test_gpu_rpgd
import test_gpu_env
from test_gpu_rpgd_batch import CONFIGS, PARAMS, ProblemAsEngine, close_all, compare, make, reset_both, states, step_both

pytestmark = pytest.mark.gpu

TARGET = {"CartPole": ("target_position", -0.15, 0.15), "Quad2D": ("target_x", -0.5, 0.5), "Hover": ("target_x", -0.5, 0.5)}


def own_of(environment):
    """the parameters every problem gets a value of its own for: the target, and PARAMS' cost weight and plant parameter drawn from
    within 20 % of the value test_gpu_rpgd_batch.py gives the whole batch"""
    return (TARGET[environment],) + tuple((name, 0.8 * value, 1.2 * value) for name, value in PARAMS[environment])


def set_own(batch, handles, rng, name, lo, hi, ids=None):
    """one value of `name` per listed problem, drawn from [lo, hi): to the batch in one call, to each handle through set_param"""
    who = list(range(batch.B)) if ids is None else list(ids)
    vals = rng.uniform(lo, hi, len(who)).astype(np.float32)
    batch.set_problem_params(name, vals, ids=ids)
    for j, q in enumerate(who):
        if q in handles:
            handles[q].set_param(name, float(vals[j]))
            assert batch.get_problem_param(name, q) == vals[j] == np.float32(handles[q].get_param(name))
    return vals


def personalise(batch, handles, rng, ids=None):
    """a target, a plant parameter and a cost weight of its own for every listed problem"""
    for name, lo, hi in own_of(batch.environment):
        set_own(batch, handles, rng, name, lo, hi, ids)


def pp_name(batch):
    return f"ctk_g_rpgd_batch_pp<{batch.cfg.environment}>"


def shared_name(batch):
    return f"ctk_g_rpgd_batch<{batch.cfg.environment}>"


def tables_of(batch):
    return {n: batch.get_problem_params(n) for n in batch.param_names}


def assert_tables(batch, tables, handles, tag):
    for n in batch.param_names:
        np.testing.assert_array_equal(batch.get_problem_params(n), tables[n], err_msg=f"{tag}: {n}")
        for q, h in handles.items():
            assert batch.get_problem_param(n, q) == np.float32(h.get_param(n)), f"{tag}: {n} of problem {q}"


# ---- 1. batch == single handles that have parameters of their own, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("source", ["philox", "host"])
@pytest.mark.parametrize("config", ["cartpole_small", "cartpole_partial", "quad2d", "hover", "hover_tape_in_scratch"])
def test_batch_equals_handles_with_their_own_parameters(config, source):
    """before the first step every problem gets its own target, one plant parameter and one cost weight; then max(4, 2 * resamp_per)
    steps, so that resampling and plain steps both occur (resamp_per 1: every step resamples), u_prev alternating between given and None"""
    B = 3
    batch, handles = make(config, B)
    host = source == "host"
    rng = np.random.default_rng(139 + len(config))
    assert batch.params_differ() == 0 and batch.dominant_kernel() == shared_name(batch)
    reset_both(batch, handles, rng, host)
    personalise(batch, handles, rng)
    assert batch.params_differ() == 1 and batch.dominant_kernel() == pp_name(batch)
    resampled = set()
    for t in range(max(4, 2 * int(batch.cfg.resamp_per))):
        resampled.add(batch.samples_needed(0) > 0)
        up = rng.uniform(-1.0, 1.0, (B, batch.C)).astype(np.float32) if t % 2 == 0 else None
        step_both(batch, handles, rng, states(rng, B, batch.S), host, up, tag=f"{config} {source} step {t}")
        compare(batch, handles, range(B), f"{config} {source} after step {t}")
    assert resampled == ({True} if int(batch.cfg.resamp_per) == 1 else {True, False})
    close_all(batch, handles)


# ---- 2. a new target array before every step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["cartpole_small", "quad2d"])
def test_per_step_targets(config):
    """all problems on even steps, a strict subset of ids on odd steps, mirrored on the handles; every step steps every problem"""
    B = 4
    batch, handles = make(config, B)
    rng = np.random.default_rng(16)
    reset_both(batch, handles, rng, False)
    personalise(batch, handles, rng)
    for t in range(5):
        set_own(batch, handles, rng, *TARGET[batch.environment], ids=None if t % 2 == 0 else [1, 3])
        step_both(batch, handles, rng, states(rng, B, batch.S), t == 3, tag=f"{config} per-step targets, step {t}")
        compare(batch, handles, range(B), f"{config} per-step targets, step {t}")
    close_all(batch, handles)


# ---- 3. launch order is not problem id ----------------------------------------------------------------------------------------------------
def test_launch_order_is_not_problem_id():
    """B = 5 stepped as ids [1, 3, 4] (record j is not problem j), then [0, 2], then all; between the steps parameters change on
    problems that the next step does not step, which pick the change up when they are next stepped.  Constants indexed by problem id
    where the launch order is required (or the reverse), or derived only for problems that are dirty AND stepped in the same call but
    never copied for the clean ones, fail here."""
    B, config = 5, "quad2d"
    batch, handles = make(config, B)
    rng = np.random.default_rng(40)
    S = batch.S
    reset_both(batch, handles, rng, False)
    personalise(batch, handles, rng)
    for rnd in range(2):
        step_both(batch, handles, rng, states(rng, 3, S), rnd == 1, ids=[1, 3, 4], tag=f"round {rnd}: [1, 3, 4]")
        compare(batch, handles, range(B), f"round {rnd}: after [1, 3, 4]")
        personalise(batch, handles, rng, ids=[3, 4])                     # set now, not stepped by the next step, stepped by the one after
        set_own(batch, handles, rng, "target_z", 0.7, 1.3, ids=[0])      # set now, stepped by the next step
        step_both(batch, handles, rng, states(rng, 2, S), False, ids=[0, 2], tag=f"round {rnd}: [0, 2]")
        compare(batch, handles, range(B), f"round {rnd}: after [0, 2]")
        set_own(batch, handles, rng, "mass", 0.5, 0.7, ids=[2])
        step_both(batch, handles, rng, states(rng, B, S), False, up=rng.uniform(-0.8, 0.8, (B, batch.C)).astype(np.float32), tag=f"round {rnd}: all")
        compare(batch, handles, range(B), f"round {rnd}: after all")
    # a problem whose parameter changes twice before it is stepped keeps the last value
    set_own(batch, handles, rng, "mass", 0.5, 0.7, ids=[0, 2])
    step_both(batch, handles, rng, states(rng, 3, S), False, ids=[1, 3, 4], tag="twice: [1, 3, 4]")
    set_own(batch, handles, rng, "mass", 0.5, 0.7, ids=[0])
    step_both(batch, handles, rng, states(rng, 3, S), False, ids=[0, 2, 4], tag="twice: [0, 2, 4]")
    compare(batch, handles, range(B), "after parameters set on problems that were stepped later")
    close_all(batch, handles)


# ---- 4. mixed iteration counts under different parameters ------------------------------------------------------------------------------
def test_mixed_iteration_counts_under_different_parameters():
    """subset resets put a warm-up step (5 iterations, resampling), a resampling step and a plain step (2 iterations each) at different
    Adam step numbers into ONE launch of ids [1, 2, 3] - record j is problem j + 1 - each problem with its own parameters, changed just
    before; the whole batch follows in another order of records with nothing changed in between, so every record needs the constants
    of ITS problem again although none was re-derived"""
    B = 4
    batch, handles = make("cartpole_small", B, warmup=1, warmup_iterations=5)
    rng = np.random.default_rng(17)
    reset_both(batch, handles, rng, True)
    personalise(batch, handles, rng)
    step_both(batch, handles, rng, states(rng, B, 4), True, tag="first step")                    # counts 1, 1, 1, 1
    reset_both(batch, handles, rng, True, ids=[2])
    step_both(batch, handles, rng, states(rng, B, 4), True, tag="second step")                   # counts 2, 2, 1, 2
    tables = tables_of(batch)
    reset_both(batch, handles, rng, False, ids=[3])                                              # counts 2, 2, 1, 0
    assert_tables(batch, tables, handles, "after reset([3])")
    set_own(batch, handles, rng, "target_position", -0.15, 0.15)
    set_own(batch, handles, rng, "m_pole", 0.09, 0.13, ids=[2, 3])
    per = (batch.N - batch.K) * (batch.samples_needed_reset() // batch.N)
    assert [batch.samples_needed(q) for q in range(B)] == [per, per, 0, per]                     # resampling, resampling, plain, warm-up + resampling
    assert [int(batch.get_state(q)[-2]) for q in range(B)] == [7, 7, 5, 0]                       # Adam step numbers differ as well
    step_both(batch, handles, rng, states(rng, 3, 4), True, ids=[1, 2, 3], tag="mixed launch")
    assert [int(batch.get_state(q)[-2]) for q in range(B)] == [7, 9, 7, 5]
    compare(batch, handles, range(B), "after the mixed launch")
    step_both(batch, handles, rng, states(rng, B, 4), False, up=rng.uniform(-1, 1, (B, 1)).astype(np.float32), tag="whole batch, Philox")
    compare(batch, handles, range(B), "after the whole batch")
    close_all(batch, handles)


# ---- 5. the two forms of the kernel compute the same ------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["cartpole_small", "quad2d", "hover"])
def test_the_two_forms_give_the_same_bits(config):
    """two batches of the same seeds: one never touched, the other with every parameter of every problem set per problem to the value
    it already has"""
    B = 3
    seeds = [21 + q for q in range(B)]
    common = CONFIGS[config]()
    shared, own = CtkRpgdBatch(B, seeds=seeds, **common), CtkRpgdBatch(B, seeds=seeds, **common)
    for name in own.param_names:
        own.set_problem_params(name, np.full(B, shared.get_param(name), np.float32))
    assert shared.params_differ() == 0 and own.params_differ() == 1
    assert shared.dominant_kernel() == shared_name(shared) and own.dominant_kernel() == pp_name(own)
    rng = np.random.default_rng(5)
    shared.reset()
    own.reset()
    for t in range(4):
        s = states(rng, B, shared.S)
        up = rng.uniform(-1.0, 1.0, (B, shared.C)).astype(np.float32) if t % 2 else None
        u = shared.step(s, u_prev=up)
        np.testing.assert_array_equal(own.step(s, u_prev=up), u)
        for q in range(B):
            for buf in ("Q", "J", "U_NOM", "PLAN", "ADAM_M", "ADAM_V", "AGES", "AGES_LOGGED", "BEST_IDX"):
                np.testing.assert_array_equal(own.read(buf, q), shared.read(buf, q), err_msg=f"{config} step {t}: {buf} of problem {q}")
            np.testing.assert_array_equal(own.get_state(q), shared.get_state(q))
            assert own.rng_position(q) == shared.rng_position(q)
    assert shared.params_differ() == 0 and shared.dominant_kernel() == shared_name(shared)
    shared.close()
    own.close()


# ---- 6. the parameters are in the result ------------------------------------------------------------------------------------------------
def test_parameters_matter():
    """problems 0 and 1: the same seed, state and draws, different target_position - different u and J, each equal to its handle;
    problem 2, untouched, equals the shared-form result.  An implementation that ignores the tables cannot pass."""
    common = CONFIGS["cartpole_small"]()
    B, seeds = 3, [9, 9, 9]
    s = np.tile(np.array([0.05, -0.1, 2.8, 0.4], np.float32), (B, 1))
    up = np.zeros((B, 1), np.float32)
    shared = CtkRpgdBatch(B, seeds=seeds, **common)
    shared.reset()
    u = shared.step(s, u_prev=up)                                 # same everything: same result
    assert u[0, 0] == u[1, 0] == u[2, 0]
    np.testing.assert_array_equal(shared.read("J", 0), shared.read("J", 1))
    fresh, handles = make("cartpole_small", B, seeds=seeds)
    reset_both(fresh, handles, None, False)
    targets = [-0.12, 0.12]
    fresh.set_problem_params("target_position", targets, ids=[0, 1])
    for q, v in enumerate(targets):
        handles[q].set_param("target_position", v)
    u2 = fresh.step(s, u_prev=up)
    uh = np.stack([handles[q].step(s[q], u_prev=up[q]) for q in range(B)])
    np.testing.assert_array_equal(u2, uh)
    compare(fresh, handles, range(B), "two targets")
    assert u2[0, 0] != u2[1, 0]
    J0, J1 = fresh.read("J", 0), fresh.read("J", 1)
    assert not np.array_equal(J0, J1) and not np.array_equal(J0, shared.read("J", 0)) and not np.array_equal(J1, shared.read("J", 0))
    assert fresh.dominant_kernel() == pp_name(fresh) and shared.dominant_kernel() == shared_name(shared)
    assert u2[2, 0] == u[2, 0]                                    # the untouched problem: what the shared form gave
    for buf in ("Q", "J", "U_NOM", "PLAN", "ADAM_M", "ADAM_V", "AGES", "BEST_IDX"):
        np.testing.assert_array_equal(fresh.read(buf, 2), shared.read(buf, 2), err_msg=buf)
    shared.close()
    close_all(fresh, handles)


# ---- 7. a whole-batch set_param after the problems diverged -------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["cartpole_small", "quad2d"])
def test_whole_batch_set_param_after_divergence(config):
    B = 4
    batch, handles = make(config, B)
    rng = np.random.default_rng(6)
    reset_both(batch, handles, rng, False)
    personalise(batch, handles, rng)
    step_both(batch, handles, rng, states(rng, B, batch.S), False, tag="diverged")
    own = own_of(batch.environment)
    (tname, _, _), other = own[0], [n for n, _, _ in own[1:]]
    before = {n: batch.get_problem_params(n) for n in other}
    batch.set_param(tname, 0.07)                                  # overwrites that name for every problem ...
    for h in handles.values():
        h.set_param(tname, 0.07)
    assert batch.get_param(tname) == np.float32(0.07)
    np.testing.assert_array_equal(batch.get_problem_params(tname), np.full(B, 0.07, np.float32))
    for n in other:                                               # ... and leaves the other names per problem
        np.testing.assert_array_equal(batch.get_problem_params(n), before[n])
        assert len(set(before[n].tolist())) == B
    assert batch.params_differ() == 1 and batch.dominant_kernel() == pp_name(batch)
    for t in range(2):
        step_both(batch, handles, rng, states(rng, B, batch.S), t == 1, tag=f"{config}: set_param({tname}) step {t}")
    compare(batch, handles, range(B), f"{config}: set_param({tname}) after divergence")
    # get_param keeps returning the last whole-batch value, whatever a problem holds
    vals = set_own(batch, handles, rng, tname, -0.1, 0.1)
    assert batch.get_param(tname) == np.float32(0.07)
    np.testing.assert_array_equal(batch.get_problem_params(tname), vals)
    step_both(batch, handles, rng, states(rng, B, batch.S), False, tag=f"{config}: per-problem {tname} again")
    compare(batch, handles, range(B), f"{config}: per-problem {tname} again")
    close_all(batch, handles)


# ---- 8. reset, set_state, set_rng_position and parameters ---------------------------------------------------------------------------------
def test_reset_set_state_and_set_rng_position_leave_the_tables_alone():
    B = 4
    batch, handles = make("quad2d", B)
    rng = np.random.default_rng(7)
    S = batch.S
    reset_both(batch, handles, rng, False)
    personalise(batch, handles, rng)
    step_both(batch, handles, rng, states(rng, B, S), False, tag="first step")
    tables = tables_of(batch)
    vector = batch.get_state(0)
    assert vector.size == batch.state_size()                      # the tables are not part of the state vector
    reset_both(batch, handles, rng, True, ids=[1, 3])
    assert_tables(batch, tables, handles, "after reset([1, 3])")
    compare(batch, handles, range(B), "after reset([1, 3])")
    step_both(batch, handles, rng, states(rng, B, S), False, tag="after the subset reset")
    st = handles[0].get_state()                                   # a handle's state continues inside the batch, under problem 2's parameters
    batch.set_state(2, st)
    handles[2].set_state(st)
    batch.set_rng_position(1, 1000)
    handles[1].set_rng_position(1000)
    assert_tables(batch, tables, handles, "after set_state and set_rng_position")
    assert batch.params_differ() == 1
    step_both(batch, handles, rng, states(rng, B, S), False, tag="after set_state")
    compare(batch, handles, range(B), "after set_state")
    reset_both(batch, handles, rng, False)
    assert_tables(batch, tables, handles, "after reset() of all")
    step_both(batch, handles, rng, states(rng, B, S), False, tag="after reset() of all")
    compare(batch, handles, range(B), "after reset() of all and one more step")
    close_all(batch, handles)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_alone():
    B = 4
    batch, handles = make("cartpole_small", B)
    rng = np.random.default_rng(4)
    reset_both(batch, handles, rng, False)
    personalise(batch, handles, rng)
    step_both(batch, handles, rng, states(rng, B, 4), False, tag="first step")
    tables = tables_of(batch)
    lib, h = batch._lib, batch._h
    vals = (ctypes.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    n_params = len(batch.param_names)

    def refused(n_ids, ids, pid, values, pattern):
        assert lib.ctk_rpgd_problem_set_param(h, n_ids, ids, pid, values) == 1
        assert pattern in lib.ctk_rpgd_batch_last_error(h), lib.ctk_rpgd_batch_last_error(h)

    refused(0, None, n_params, vals, b"ctk_rpgd_problem_set_param: unknown parameter id")          # a bad parameter id
    refused(0, None, -1, vals, b"ctk_rpgd_problem_set_param: unknown parameter id")
    refused(1, (ctypes.c_int32 * 1)(4), 3, vals, b"ctk_rpgd_problem_set_param: problem index 4 is outside 0 .. 3")   # a problem out of range
    refused(2, (ctypes.c_int32 * 2)(0, -1), 3, vals, b"ctk_rpgd_problem_set_param: problem index -1")
    refused(2, (ctypes.c_int32 * 2)(2, 1), 3, vals, b"ctk_rpgd_problem_set_param: ids must be strictly ascending")     # descending ids
    refused(2, (ctypes.c_int32 * 2)(1, 1), 3, vals, b"ctk_rpgd_problem_set_param: ids must be strictly ascending")
    refused(5, (ctypes.c_int32 * 5)(0, 1, 2, 3, 3), 3, vals, b"ctk_rpgd_problem_set_param: n_ids must be 1 .. 4")
    refused(0, None, 3, None, b"ctk_rpgd_problem_set_param: NULL values")                            # NULL values
    refused(2, (ctypes.c_int32 * 2)(0, 3), 3, None, b"ctk_rpgd_problem_set_param: NULL values")
    v = ctypes.c_float(-1.0)
    assert lib.ctk_rpgd_problem_get_param(h, 4, 3, ctypes.byref(v)) == 1 and lib.ctk_rpgd_problem_get_param(h, 0, n_params, ctypes.byref(v)) == 1
    assert lib.ctk_rpgd_problem_get_param(h, 0, 3, None) == 1 and v.value == -1.0
    # the binding refuses the same before it asks the library
    with pytest.raises(ValueError, match="unknown parameter"):
        batch.set_problem_params("target_x", 0.1)
    with pytest.raises(ValueError, match="strictly ascending"):
        batch.set_problem_params("L", [0.2, 0.2], ids=[2, 1])
    with pytest.raises(ValueError, match=r"0 \.\. 3"):
        batch.set_problem_params("L", [0.2], ids=[4])
    with pytest.raises(ValueError, match="one value per listed problem"):
        batch.set_problem_params("L", [0.2, 0.2, 0.2])
    with pytest.raises(ValueError, match="finite"):
        batch.set_problem_params("L", [0.2, np.nan, 0.2, 0.2])
    with pytest.raises(ValueError, match=r"outside 0 \.\. 3"):
        batch.get_problem_param("L", 4)
    with pytest.raises(ValueError, match="unknown parameter"):
        batch.get_problem_param("target_x", 0)
    # nothing was written: the tables read back as before and the next step is the handles'
    assert_tables(batch, tables, handles, "after the refusals")
    step_both(batch, handles, rng, states(rng, B, 4), False, tag="after the refusals")
    compare(batch, handles, range(B), "after the refusals")
    # a refusal on a batch that never had a parameter set leaves it in the shared form
    plain = CtkRpgdBatch(2, **CONFIGS["cartpole_small"]())
    assert lib.ctk_rpgd_problem_set_param(plain._h, 0, None, 99, vals) == 1
    assert lib.ctk_rpgd_problem_set_param(plain._h, 0, None, 3, None) == 1
    assert plain.params_differ() == 0 and plain.dominant_kernel() == "ctk_g_rpgd_batch<0>"
    plain.close()
    close_all(batch, handles)


# ---- 10. the reference-recorded fixtures inside a per-problem batch -----------------------------------------------------------------------
class ProblemWithOwnParameters(ProblemAsEngine):
    """test_gpu_rpgd_batch.ProblemAsEngine whose set_param reaches problem `me` alone; the neighbours keep other targets"""

    def set_param(self, name, value):
        self.batch.set_problem_params(name, float(value), ids=[self.me])
        self.handle.set_param(name, value)

    def close(self):
        tname = TARGET[self.batch.environment][0]
        assert len(set(self.batch.get_problem_params(tname).tolist())) == len(self.batch) and self.batch.params_differ() == 1
        for n in self.batch.param_names:
            assert self.batch.get_problem_param(n, self.me) == np.float32(self.handle.get_param(n)), n
        super().close()


@pytest.mark.parametrize("fixture", ["rpgd_ode_small", "rpgd_quad2d"])
def test_reference_fixture_inside_a_per_problem_batch(monkeypatch, fixture):
    """the fixture's draws, states and set_state sequence fed to problem 1 of B = 3 in the per-problem form by the body of the handle's
    own reference-golden test (its tolerances, nothing restated): the fixture's parameters are set on problem 1 alone, the neighbours
    hold other targets.  Bit-equal to a template handle, and within the reference's tolerances"""
    made = []

    def engine(opt, pred, **kw):
        assert opt == "rpgd" and pred == "ODE"
        handle = CtkEngine(opt, pred, generic_kernels=True, **kw)
        batch = CtkRpgdBatch(3, seeds=[41, int(kw.get("seed", 0)), 43], **kw)
        tname, lo, hi = TARGET[batch.environment]
        mine = batch.get_problem_param(tname, 1)
        batch.set_problem_params(tname, [mine + 0.9 * lo, mine + 0.9 * hi], ids=[0, 2])
        made.append(batch.dominant_kernel())        # the golden test closes its engine, and with it the batch
        return ProblemWithOwnParameters(batch, 1, handle, np.random.default_rng(37))

    case = fixture[len("rpgd_"):]
    if case == "ode_small":
        import gpu_helpers
        monkeypatch.setattr(gpu_helpers, "CtkEngine", engine)
        test_gpu_rpgd.test_rpgd_matches_reference_golden(case)
    else:
        monkeypatch.setattr(test_gpu_env, "CtkEngine", engine)
        test_gpu_env.test_quad2d_rpgd_matches_reference_golden(case)
    assert len(made) == 1 and made[0].startswith("ctk_g_rpgd_batch_pp<")


# ---- 11. a user environment ---------------------------------------------------------------------------------------------------------------
def test_user_environment_has_the_per_problem_form():
    """a library built with a user model (tests/envs/pendulum_env.h) carries ctk_g_rpgd_batch_pp<3>: two problems with different
    `length`, each equal to its handle"""
    from control_toolkit_amd.build_env import register_environment
    name = register_environment(os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs", "pendulum_env.h"))
    B = 2
    common = dict(environment=name, num_rollouts=16, mpc_horizon=10, dt=0.02, period_interpolation_inducing_points=5, opt_keep_k=4, outer_its=2,
                  resamp_per=2, sample_whole_control_space=1, learning_rate=0.05, gradmax_clip=5.0)
    batch, handles = make(common, B, seeds=[31, 32])
    assert batch.dominant_kernel() == "ctk_g_rpgd_batch<3>"
    rng = np.random.default_rng(31)
    reset_both(batch, handles, rng, False)
    batch.set_problem_params("length", [0.4, 0.6])
    for q, v in enumerate((0.4, 0.6)):
        handles[q].set_param("length", v)
    batch.set_param("terminal_weight", 0.4)
    for h in handles.values():
        h.set_param("terminal_weight", 0.4)
    assert batch.params_differ() == 1 and batch.dominant_kernel() == "ctk_g_rpgd_batch_pp<3>"
    for t in range(3):
        if t == 2:
            set_own(batch, handles, rng, "target_angle", -0.3, 0.3, ids=[1])
        s = rng.uniform(-0.4, 0.4, (B, 2)).astype(np.float32)
        s[:, 0] += 2.6
        step_both(batch, handles, rng, s, t == 1, tag=f"Pendulum step {t}")
        compare(batch, handles, range(B), f"Pendulum, per-problem parameters, step {t}")
    assert not np.array_equal(batch.read("J", 0), batch.read("J", 1))
    close_all(batch, handles)
