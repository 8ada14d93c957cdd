"""-m gpu: per-problem MPPI hyper-parameters and input limits of the MPPI batches (include/ctk_hip_hyper.h; kernels
ctk_mppi_batch_hp<ENV, LOG>, ctk_mppi_batch_mlp_hp<LOG>, ctk_mppi_batch_gru_hp<LOG, FORM>).

The contract under test: problem p of a batch behaves BIT FOR BIT like a CtkEngine("mppi", <predictor>, seed=seeds[p], cc_weight=..., R=...,
LBD=..., NU=..., SQRTRHOINV=..., action_low=..., action_high=...) created with p's values and given the same calls; a change between two
steps makes the problem equal to a FRESH such handle that received the problem's state vector, its Philox position and (GRU) its hidden
state.  Every comparison against handles and between batches is assert_array_equal: there is no tolerance in this file.  That equality
with the case's handle cannot come from a kernel that ignored the problem's values is test_batch_hypers_cpu.py's guard, and each test
here also asserts that the non-default problems differ from the default one."""
import ctypes

import numpy as np
import pytest

from oracle import ctk_oracle as O
from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkMppiMlpBatch, CtkMppiGruBatch
from control_toolkit_amd._capi import HYPERS, gru_batch_fit
import hyper_cases as Hc
import large_angle_cases as L
import param_cases as P
from test_gpu_hyper import set_params, lim, mppi_start
from test_gpu_large_angles import ENV_ID
from test_gpu_batch_params import OWN
from test_gpu_gru_batch import LARGE as GRU_LARGE, weights as gru_weights
from test_gpu_mlp_batch import weights as mlp_weights
from test_gpu_batch_episodes import loop as episode_loop, same_episodes

pytestmark = pytest.mark.gpu

DT = Hc.DT
ERR_INVALID = 1                                          # CTK_ERR_INVALID_ARGUMENT
BATCH = {"ODE": CtkMppiBatch, "MLP": CtkMppiMlpBatch, "GRU": CtkMppiGruBatch}
PREFIX = {"ODE": ("ctk_batch", "ctk_problem"), "MLP": ("ctk_mlp_batch", "ctk_mlp_problem"), "GRU": ("ctk_gru_batch", "ctk_gru_problem")}
# cases for the tests that need only a few problems: the defaults, everything at once, a narrow soft-min with a wide exploration
FEW = [(), Hc.MPPI_ALL, (("LBD", 10.0), ("SQRTRHOINV", 0.2)), Hc.MPPI_SATURATED]


def values_of(env, own):
    """the seven fields of a case as keyword arguments of CtkEngine"""
    lo, hi = Hc.limits_of(env, own)
    return dict(Hc.config_of(Hc.MPPI_DEFAULTS, own), action_low=lim(lo), action_high=lim(hi))


def sizes_kw(size, materialize):
    N, H, p = size
    return dict(num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p, materialize_trajectories=materialize, dt=DT)


def give_case(batch, env, q, own):
    """problem q of the batch gets the case's values through the per-problem entries"""
    for name, value in own:
        if name == "limits":
            batch.set_problem_limits(*Hc.limits_of(env, own), ids=[q])
        else:
            batch.set_problem_hypers(name, value, ids=[q])


def make_ode(env, size, materialize, cases, seeds=None, call_order=None):
    """(a batch created with the DEFAULT hyper-parameters and limits whose problem q then gets cases[q], handles created with cases[q])"""
    B = len(cases)
    seeds = [11 + q for q in range(B)] if seeds is None else seeds
    lo, hi = L.LIMITS[env]
    batch = CtkMppiBatch(B, seeds=seeds, environment=env, action_low=lim(lo), action_high=lim(hi), **sizes_kw(size, materialize))
    set_params(batch, L.env_params(env))
    handles = []
    for q, own in enumerate(cases):
        give_case(batch, env, q, own)
        h = CtkEngine("mppi", "ODE", environment=env, seed=seeds[q], **values_of(env, own), **sizes_kw(size, materialize))
        set_params(h, L.env_params(env))
        handles.append(h)
    return batch, handles


def compare(batch, handles, materialize, tag, hidden=False):
    for q, h in enumerate(handles):
        np.testing.assert_array_equal(batch.read("U_NOM", q), h.read("U_NOM"), err_msg=f"{tag}: U_NOM of problem {q}")
        np.testing.assert_array_equal(batch.read("J", q), h.read("J"), err_msg=f"{tag}: J of problem {q}")
        np.testing.assert_array_equal(batch.get_state(q), h.get_state(), err_msg=f"{tag}: state vector of problem {q}")
        assert batch.rng_position(q) == h.rng_position(), f"{tag}: Philox position of problem {q}"
        if materialize:
            np.testing.assert_array_equal(batch.read("Q", q), h.read("Q"), err_msg=f"{tag}: Q of problem {q}")
            np.testing.assert_array_equal(batch.read("TRAJ", q), h.read("TRAJ"), err_msg=f"{tag}: TRAJ of problem {q}")
        if hidden:
            np.testing.assert_array_equal(batch.get_hidden([q])[0], h.predictor_get_hidden(), err_msg=f"{tag}: hidden state of problem {q}")


def step_both(batch, handles, S, tag, ids=None, samples=None, u_prev=None):
    """one step of the listed problems on both sides; samples [n, ...] host draws or None (device Philox); asserts u bit for bit"""
    who = list(range(batch.B)) if ids is None else list(ids)
    u = np.array(batch.step(S[who], samples, u_prev=u_prev, ids=ids))
    for j, q in enumerate(who):
        uh = handles[q].step(S[q], None if samples is None else samples[j], u_prev=None if u_prev is None else u_prev[j])
        np.testing.assert_array_equal(u[j], uh, err_msg=f"{tag}: u of problem {q}")
    return u


def differs_from_problem_0(batch, tag):
    """at least one tensor of every other problem is not problem 0's: the comparisons above are not trivially true"""
    J0, U0 = batch.read("J", 0), batch.read("U_NOM", 0)
    for q in range(1, batch.B):
        assert not (np.array_equal(batch.read("J", q), J0) and np.array_equal(batch.read("U_NOM", q), U0)), f"{tag}: problem {q} equals the default problem"


def close_all(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


# ---- 1. every case of hyper_cases in ONE batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("size", Hc.MPPI_SIZES, ids=lambda s: "N%d-H%d-p%d" % s)
@pytest.mark.parametrize("env", Hc.ENVS)
def test_all_cases_in_one_batch(env, size, materialize):
    """problem 0 keeps the defaults, problem j has case j - 1 (limits included); three steps from hyper_cases' states and plan0: host
    draws with u_prev given, device Philox, device Philox on an id subset"""
    N, H, p = size
    cases = [()] + Hc.MPPI_CASES
    B = len(cases)
    log = "true" if materialize else "false"
    plain = CtkMppiBatch(1, seeds=[11], environment=env, action_low=lim(L.LIMITS[env][0]), action_high=lim(L.LIMITS[env][1]), **sizes_kw(size, materialize))
    set_params(plain, L.env_params(env))
    batch, handles = make_ode(env, size, materialize, cases)
    assert plain.hypers_differ() == 0 and batch.hypers_differ() == 1
    assert batch.dominant_kernel() == f"ctk_mppi_batch_hp<{ENV_ID[env]}, {log}>", batch.dominant_kernel()
    refs = [Hc.mppi_ref(env, own, N, H, p) for own in cases]
    for q, (own, ref) in enumerate(zip(cases, refs)):
        batch.set_state(q, mppi_start(ref))
        handles[q].set_state(mppi_start(ref))
        for name in HYPERS:
            assert batch.get_problem_hyper(name, q) == np.float32(Hc.config_of(Hc.MPPI_DEFAULTS, own)[name])
        lo, hi = batch.get_problem_limits(q)
        np.testing.assert_array_equal(lo, Hc.limits_of(env, own)[0]); np.testing.assert_array_equal(hi, Hc.limits_of(env, own)[1])
    plain.set_state(0, mppi_start(refs[0]))
    S = np.stack([r["s"] for r in refs])
    noise = np.stack([r["noise"] for r in refs])
    up = np.stack([r["u_prev"] for r in refs])
    tag = f"{env} N{N} p{p} log={log}"
    step_both(batch, handles, S, f"{tag} host draws", samples=noise, u_prev=up)
    compare(batch, handles, materialize, f"{tag} host draws")
    differs_from_problem_0(batch, tag)
    # the untouched batch launches what it always launched, and computes what the default problem of the _hp form computes
    u_plain = plain.step(S[:1], noise[:1], u_prev=up[:1])
    np.testing.assert_array_equal(u_plain[0], batch.last_u[0])
    np.testing.assert_array_equal(plain.read("J", 0), batch.read("J", 0))
    assert plain.dominant_kernel() == f"ctk_mppi_batch<{ENV_ID[env]}, {log}>" and plain.hypers_differ() == 0 and plain.params_differ() == 0
    step_both(batch, handles, S, f"{tag} device Philox")
    compare(batch, handles, materialize, f"{tag} device Philox")
    ids = [0, 2, 5, 7, B - 1]
    step_both(batch, handles, S, f"{tag} id subset", ids=ids)
    compare(batch, handles, materialize, f"{tag} id subset")
    differs_from_problem_0(batch, tag)
    assert batch.dominant_kernel() == f"ctk_mppi_batch_hp<{ENV_ID[env]}, {log}>"
    close_all(batch, handles, plain)


# ---- 2. together with per-problem plant and cost parameters ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["params_first", "hypers_first"])
@pytest.mark.parametrize("size", [(1000, 35, 10), (1024, 50, 1)], ids=["ragged-interp", "cfg2"])
def test_with_per_problem_parameters(size, order):
    """CartPole: target, one dynamics parameter and one weight per problem (test_gpu_batch_params.OWN) AND the hyper-parameters of
    FEW per problem, in both call orders; reset() then starts every problem at the middle of ITS limits, as its handle starts"""
    env, B = "CartPole", len(FEW)
    rng = np.random.default_rng(size[1])
    seeds = [11 + q for q in range(B)]
    lo, hi = L.LIMITS[env]
    batch = CtkMppiBatch(B, seeds=seeds, environment=env, action_low=lim(lo), action_high=lim(hi), **sizes_kw(size, True))
    handles = [CtkEngine("mppi", "ODE", environment=env, seed=seeds[q], **values_of(env, own), **sizes_kw(size, True)) for q, own in enumerate(FEW)]
    own_values = {name: rng.uniform(a, b, B).astype(np.float32) for name, a, b in OWN[env]}

    def params():
        for name, vals in own_values.items():
            batch.set_problem_params(name, vals)

    def hypers():
        for q, own in enumerate(FEW):
            give_case(batch, env, q, own)

    for call in ((params, hypers) if order == "params_first" else (hypers, params)):
        call()
    for name, vals in own_values.items():
        for q in range(B):
            handles[q].set_param(name, float(vals[q]))
    assert batch.params_differ() == 1 and batch.hypers_differ() == 1
    assert batch.dominant_kernel() == "ctk_mppi_batch_hp<0, true>", batch.dominant_kernel()
    batch.reset()
    S = rng.uniform(-0.2, 0.2, (B, 4)).astype(np.float32)
    for t in range(2):
        u = step_both(batch, handles, S, f"{size} {order} step {t}")
        compare(batch, handles, True, f"{size} {order} step {t}")
        S = O.Predictor("ODE", dt=DT, env=O.EnvParams()).step(S, u).astype(np.float32)
    differs_from_problem_0(batch, f"{size} {order}")
    close_all(batch, handles)


# ---- 3. a change between two steps -------------------------------------------------------------------------------------------------------------
def fresh_handle(batch, q, env, size, values, seed):
    """a new handle with `values` that receives problem q's state vector and Philox position"""
    h = CtkEngine("mppi", "ODE", environment=env, seed=seed, **values, **sizes_kw(size, False))
    set_params(h, L.env_params(env))
    h.set_state(batch.get_state(q))
    h.set_rng_position(batch.rng_position(q))
    return h


def test_change_between_steps():
    env, size, B = "CartPole", Hc.MPPI_SIZES[0], 4
    seeds = [31 + q for q in range(B)]
    lo, hi = L.LIMITS[env]
    values = [dict(Hc.MPPI_DEFAULTS, action_low=lim(lo), action_high=lim(hi)) for _ in range(B)]
    batch = CtkMppiBatch(B, seeds=seeds, environment=env, action_low=lim(lo), action_high=lim(hi), **sizes_kw(size, False))
    set_params(batch, L.env_params(env))
    handles = [fresh_handle(batch, q, env, size, values[q], seeds[q]) for q in range(B)]
    for q in range(B):
        start = np.concatenate([Hc.plan0(env, size[1]).ravel() * (1.0 + 0.3 * q), [Hc.U_PREV]]).astype(np.float32)
        batch.set_state(q, start)
        handles[q].set_state(start)
    S = np.stack([Hc.STATE_LBD[env] * (1.0 + 0.1 * q) for q in range(B)]).astype(np.float32)
    for t in range(2):
        step_both(batch, handles, S, f"shared form, step {t}")
    assert batch.dominant_kernel() == "ctk_mppi_batch<0, false>" and batch.hypers_differ() == 0
    # problems 1 and 2: a new LBD and SQRTRHOINV; problem 2: limits that cut its current plan
    batch.set_problem_hypers("LBD", [10.0, 30.0], ids=[1, 2])
    batch.set_problem_hypers("SQRTRHOINV", [0.2, 0.08], ids=[1, 2])
    plan2 = batch.read("U_NOM", 2).ravel()
    cut = (np.float32(np.quantile(plan2, 0.3)), np.float32(np.quantile(plan2, 0.7)))
    assert plan2.min() < cut[0] < cut[1] < plan2.max()
    batch.set_problem_limits(cut[0], cut[1], ids=[2])
    values[1].update(LBD=10.0, SQRTRHOINV=0.2)
    values[2].update(LBD=30.0, SQRTRHOINV=0.08, action_low=float(cut[0]), action_high=float(cut[1]))
    assert batch.dominant_kernel() == "ctk_mppi_batch_hp<0, false>" and batch.hypers_differ() == 1
    for q in (1, 2):
        handles[q].close()
        handles[q] = fresh_handle(batch, q, env, size, values[q], seeds[q])          # problems 0 and 3 keep their old handles
    for t in range(2):
        step_both(batch, handles, S, f"after the change, step {t}")
        compare(batch, handles, False, f"after the change, step {t}")
    plan2 = batch.read("U_NOM", 2)
    assert plan2.min() >= cut[0] and plan2.max() <= cut[1]
    differs_from_problem_0(batch, "after the change")
    # the whole batch at once: every problem equals a fresh handle with its other values and the new one
    batch.set_hyper("NU", 2.0)
    assert batch.get_problem_hypers("NU").tolist() == [2.0] * B and batch.get_problem_hypers("LBD").tolist() == [100.0, 10.0, 30.0, 100.0]
    for q in range(B):
        values[q].update(NU=2.0)
        handles[q].close()
        handles[q] = fresh_handle(batch, q, env, size, values[q], seeds[q])
    for t in range(2):
        step_both(batch, handles, S, f"after set_hyper, step {t}", ids=None if t == 0 else [1, 3])
        compare(batch, handles, False, f"after set_hyper, step {t}")
    # reset keeps the values: problem 2's plan restarts at the middle of ITS limits
    batch.reset(ids=[2])
    handles[2].reset()
    compare(batch, handles, False, "after reset")
    step_both(batch, handles, S, "after reset")
    compare(batch, handles, False, "after reset and a step")
    close_all(batch, handles)


# ---- 4. / 5. the network batches ---------------------------------------------------------------------------------------------------------------
def make_net(kind, size, materialize, cases, weight_of):
    env, B = "CartPole", len(cases)
    seeds = [41 + q for q in range(B)]
    lo, hi = L.LIMITS[env]
    batch = BATCH[kind](B, seeds=seeds, action_low=lim(lo), action_high=lim(hi), **sizes_kw(size, materialize))
    set_params(batch, L.env_params(env))
    batch.set_problem_weights(np.stack([weight_of(100 + q) for q in range(B)]))
    handles = []
    for q, own in enumerate(cases):
        give_case(batch, env, q, own)
        h = CtkEngine("mppi", kind, seed=seeds[q], **values_of(env, own), **sizes_kw(size, materialize))
        set_params(h, L.env_params(env))
        h.set_predictor_weights(weight_of(100 + q))
        handles.append(h)
    return batch, handles


def run_net(kind, size, materialize, steps, kernel):
    cases = [(), Hc.MPPI_ALL, Hc.MPPI_SATURATED]
    batch, handles = make_net(kind, size, materialize, cases, mlp_weights if kind == "MLP" else gru_weights)
    assert batch.dominant_kernel() == kernel, batch.dominant_kernel()
    N, H, p = size
    for q, own in enumerate(cases):
        lo, hi = Hc.limits_of("CartPole", own)
        start = np.concatenate([np.clip(Hc.plan0("CartPole", H), lo, hi).ravel(), [Hc.U_PREV]]).astype(np.float32)
        batch.set_state(q, start)
        handles[q].set_state(start)
    S = np.stack([Hc.STATE["CartPole"] * (1.0 + 0.2 * q) for q in range(len(cases))]).astype(np.float32)
    rng = np.random.default_rng(N + H)
    noise = rng.standard_normal((len(cases), N, batch.samples_needed() // N, 1)).astype(np.float32)
    tag = f"{kind} N{N} H{H} p{p}"
    for t in range(steps):
        u = step_both(batch, handles, S, f"{tag} step {t}", samples=noise if t == 0 else None)
        compare(batch, handles, materialize, f"{tag} step {t}", hidden=kind == "GRU")
        S = O.Predictor("ODE", dt=DT, env=L.env_params("CartPole")).step(S, u).astype(np.float32)
    differs_from_problem_0(batch, tag)
    close_all(batch, handles)


@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("size", [Hc.NET_SIZE, (70, 12, 5)], ids=lambda s: "N%d-H%d-p%d" % s)
def test_mlp_batch(size, materialize):
    """ctk_mppi_batch_mlp_hp<LOG>: B = 3 with a network, hyper-parameters and limits per problem against CtkEngine("mppi", "MLP") handles"""
    run_net("MLP", size, materialize, 2, f"ctk_mppi_batch_mlp_hp<{'true' if materialize else 'false'}>")


def gru_size(which):
    """(70, 12, 5), or the smallest size of test_gpu_gru_batch.LARGE that selects the narrow / the wide {value, seq} tail — the two FORMs
    ctk_mppi_batch_gru_fit can return; (size, FORM)"""
    if which == "small":
        return (70, 12, 5), int(gru_batch_fit(70, 12, 5)[3])
    wide = which == "wide"
    fitting = [s for s in sorted(GRU_LARGE, key=lambda s: s[0] * s[1]) if gru_batch_fit(*s)[0] and gru_batch_fit(*s)[3] == wide]
    assert fitting, f"no size of LARGE selects the {which} tail"
    return fitting[0], int(wide)


@pytest.mark.parametrize("materialize", [False, True])
@pytest.mark.parametrize("which", ["small", "narrow", "wide"])
def test_gru_batch(which, materialize):
    """ctk_mppi_batch_gru_hp<LOG, FORM>, all four instantiations: B = 3, two steps, the carried hidden state after every step included"""
    size, form = gru_size(which)
    assert form == (1 if which == "wide" else 0)
    run_net("GRU", size, materialize, 2, f"ctk_mppi_batch_gru_hp<{'true' if materialize else 'false'}, {form}>")


# ---- 6. closed loops on the device ---------------------------------------------------------------------------------------------------------------
def run_loop(batch, S0, steps):
    """the loop run() replaces: u = step(S); S = plant_step(S, u)"""
    n = S0.shape[0]
    states, inputs = np.empty((n, steps + 1, batch.S), np.float32), np.empty((n, steps, batch.C), np.float32)
    states[:, 0] = S0
    for k in range(steps):
        inputs[:, k] = batch.step(states[:, k])
        states[:, k + 1] = batch.closed_loop.plant_step(states[:, k], inputs[:, k])
    return states, inputs


LOOPS = [("ODE", "CartPole", Hc.MPPI_SIZES[0]), ("ODE", "Quad2D", Hc.MPPI_SIZES[0]), ("MLP", "CartPole", Hc.NET_SIZE), ("GRU", "CartPole", (70, 12, 5))]


@pytest.mark.parametrize("kind,env,size", LOOPS, ids=[f"{k}-{e}" for k, e, _ in LOOPS])
def test_closed_loops_are_the_host_loops(kind, env, size):
    """closed_loop.run and .episodes of a batch with hyper-parameters and limits per problem: bit for bit the host loop over step and
    plant_step / plant_step_noisy of an identical batch — the step driver picks the _hp form for them too"""
    cases, steps = [(), Hc.MPPI_ALL, Hc.MPPI_SATURATED], 4
    B = len(cases)

    def make():
        lo, hi = L.LIMITS[env]
        kw = dict(seeds=[51 + q for q in range(B)], action_low=lim(lo), action_high=lim(hi), **sizes_kw(size, False))
        b = BATCH[kind](B, **(dict(kw, environment=env) if kind == "ODE" else kw))
        set_params(b, L.env_params(env))
        if kind != "ODE":
            b.set_problem_weights(np.stack([(mlp_weights if kind == "MLP" else gru_weights)(100 + q) for q in range(B)]))
        for q, own in enumerate(cases):
            give_case(b, env, q, own)
        rng = np.random.default_rng(5)
        b.closed_loop.set_noise(process=rng.uniform(0.001, 0.01, (B, b.S)), measurement=rng.uniform(0.001, 0.01, (B, b.S)))
        b.closed_loop.set_noise_seeds([900 + q for q in range(B)])
        return b

    dev, host = make(), make()
    hp = dev.dominant_kernel()
    assert "_hp<" in hp, hp
    S0 = np.stack([Hc.STATE[env] * (1.0 + 0.2 * q) for q in range(B)]).astype(np.float32)
    states, inputs = dev.closed_loop.run(S0, steps)
    want_states, want_inputs = run_loop(host, S0, steps)
    np.testing.assert_array_equal(inputs, want_inputs, err_msg=f"{kind} {env} run: inputs")
    np.testing.assert_array_equal(states, want_states, err_msg=f"{kind} {env} run: states")
    assert not np.array_equal(inputs[1], inputs[0]) and not np.array_equal(inputs[2], inputs[0])
    same_episodes(dev.closed_loop.episodes(states[:, -1], steps), episode_loop(host, want_states[:, -1], steps), f"{kind} {env} episodes")
    for q in range(B):
        np.testing.assert_array_equal(dev.get_state(q), host.get_state(q), err_msg=f"{kind} {env}: state vector of problem {q}")
        assert dev.rng_position(q) == host.rng_position(q) == 2 * steps
    if kind == "GRU":
        np.testing.assert_array_equal(dev.get_hidden(), host.get_hidden())
    assert dev.dominant_kernel() == hp
    close_all(dev, host)


# ---- 7. refusals, through the library ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ODE", "MLP", "GRU"])
def test_refusals(kind):
    """every refused call returns CTK_ERR_INVALID_ARGUMENT with a message that starts with the entry's exported name and names no other
    family, changes nothing and launches nothing: the Philox positions stay and the next step still equals the handles"""
    size = Hc.MPPI_SIZES[0] if kind == "ODE" else Hc.NET_SIZE
    cases = [(), Hc.MPPI_ALL, Hc.MPPI_SATURATED]
    if kind == "ODE":
        batch, handles = make_ode("CartPole", size, False, cases)
    else:
        batch, handles = make_net(kind, size, False, cases, mlp_weights if kind == "MLP" else gru_weights)
    S = np.stack([Hc.STATE["CartPole"]] * 3).astype(np.float32)
    batch.reset()
    step_both(batch, handles, S, f"{kind} before the refusals")
    lib, h = batch._lib, batch._h
    fam, prob = PREFIX[kind]
    others = [x for pair in PREFIX.values() for x in pair if x not in (fam, prob)]
    before = ([batch.rng_position(q) for q in range(3)], [batch.get_problem_hypers(n).tolist() for n in HYPERS], [batch.get_problem_limits(q) for q in range(3)])

    def ints(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def floats(*v):
        return (ctypes.c_float * len(v))(*v)

    set_hyper, set_limits, set_all = (getattr(lib, f"{prob}_set_hyper"), getattr(lib, f"{prob}_set_limits"), getattr(lib, f"{fam}_set_hyper"))
    nan = float("nan")
    refused = [
        (f"{prob}_set_hyper", lambda: set_hyper(h, 1, ints(3), HYPERS["R"], floats(1.0)), "outside"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ints(2, 1), HYPERS["R"], floats(1.0, 1.0)), "ascending"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ints(0, 2), HYPERS["LBD"], floats(5.0, 0.0)), "LBD > 0"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ints(0, 2), HYPERS["NU"], floats(5.0, 0.0)), "NU != 0"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 2, ints(0, 1), HYPERS["cc_weight"], floats(0.5, nan)), "finite"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 1, ints(0), 5, floats(0.5)), "unknown hyper-parameter"),
        (f"{prob}_set_hyper", lambda: set_hyper(h, 1, ints(0), HYPERS["R"], None), "NULL"),
        (f"{prob}_set_limits", lambda: set_limits(h, 1, ints(-1), floats(0.0), floats(1.0)), "outside"),
        (f"{prob}_set_limits", lambda: set_limits(h, 2, ints(1, 1), floats(0.0, 0.0), floats(1.0, 1.0)), "ascending"),
        (f"{prob}_set_limits", lambda: set_limits(h, 2, ints(0, 1), floats(-0.1, 0.3), floats(0.1, 0.2)), "action_low must be <= action_high"),
        (f"{prob}_set_limits", lambda: set_limits(h, 1, ints(1), floats(nan), floats(0.2)), "finite"),
        (f"{fam}_set_hyper", lambda: set_all(h, HYPERS["LBD"], 0.0), "LBD > 0"),
        (f"{fam}_set_hyper", lambda: set_all(h, HYPERS["NU"], 0.0), "NU != 0"),
        (f"{fam}_set_hyper", lambda: set_all(h, HYPERS["SQRTRHOINV"], nan), "finite"),
    ]
    for name, call, text in refused:
        assert call() == ERR_INVALID, name
        msg = batch._b.last_error(h).decode()
        assert msg.startswith(name + ":") and text in msg, msg
        assert not any(o + "_" in msg for o in others), msg
    after = ([batch.rng_position(q) for q in range(3)], [batch.get_problem_hypers(n).tolist() for n in HYPERS], [batch.get_problem_limits(q) for q in range(3)])
    assert before[0] == after[0] and before[1] == after[1]
    for (lo0, hi0), (lo1, hi1) in zip(before[2], after[2]):
        np.testing.assert_array_equal(lo0, lo1); np.testing.assert_array_equal(hi0, hi1)
    # the Python checker refuses the same ahead of the library
    for call in (lambda: batch.set_problem_hypers("LBD", 0.0), lambda: batch.set_hyper("NU", 0.0), lambda: batch.set_problem_limits(0.5, 0.1),
                 lambda: batch.set_problem_hypers("R", 1.0, ids=[3]), lambda: batch.set_problem_hypers("R", [1.0, 2.0], ids=[1, 0])):
        with pytest.raises(ValueError):
            call()
    step_both(batch, handles, S, f"{kind} after the refusals")
    compare(batch, handles, False, f"{kind} after the refusals", hidden=kind == "GRU")
    close_all(batch, handles)
