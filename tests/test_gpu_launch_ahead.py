"""-m gpu: the launched-ahead form of the MPPI step (include/ctk_hip_ahead.h; csrc/ctk_mppi.hip: ctk_mppi_ahead) — in a tight loop the
kernel of step k+1 is launched while step k runs and waits, bounded by a fuse, for its request.  It must be a pure scheduling change:
every u and the plan bit-identical to a twin handle with the form off, whatever happens between the steps (gaps, a refilled buffer,
other API entries), every wait bounded, and nothing launched ahead for a caller that is slow or has switched it off.

A loop is "tight" when each step arrives within the fuse (20 us) of the previous result, so the two handles of a pair are stepped one
after the other over the same precomputed states, never interleaved (the twin's step would be the gap)."""
import gc
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from control_toolkit_amd import CtkEngine
from control_toolkit_amd._capi import AHEAD_ARM_AFTER, AHEAD_DEFAULT_FUSE_US, environment_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40
S0 = {"CartPole": np.array([0.05, -0.1, 2.8, 0.4], np.float32), "Quad2D": np.array([0.3, -0.2, 0.7, 0.1, 0.25, -0.4], np.float32)}


def states(env, n):
    """the loop's states, fixed in advance: the same for both handles of a pair"""
    S = environment_info(env)[0]
    d = np.linspace(0.01, -0.02, S).astype(np.float32)
    return [(S0[env] + np.float32(t) * d).astype(np.float32) for t in range(n)]


def engine(env, N, H, ahead, **kw):
    e = CtkEngine("mppi", "ODE", environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=1, seed=3, **kw)
    if not ahead:
        e.launch_ahead(False)
    return e


def pool_of(e, n=4, seed=1):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    pool = [torch.randn((int(e.samples_needed()),), generator=g, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return pool


def tight_loop(step, S, ptrs, sleep_before=()):
    """every u of the loop; nothing but the step (and the asked-for sleeps) between two steps"""
    out = []
    gc.disable()
    try:
        for t, s in enumerate(S):
            if t in sleep_before:
                time.sleep(0.002)
            out.append(step(s, ptrs[t & 3] if ptrs else None).copy())
    finally:
        gc.enable()
    return out


def same(us_a, us_b):
    assert len(us_a) == len(us_b)
    for t, (x, y) in enumerate(zip(us_a, us_b)):
        assert x.tobytes() == y.tobytes(), f"step {t}: {x} != {y}"


# ---- 1: tight steps, at CtkEngine.step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["buffer", "rng"])
@pytest.mark.parametrize("env,N,H", [("CartPole", 128, 12), ("CartPole", 64, 12), ("Quad2D", 64, 10)])
def test_tight_engine_steps_equal_the_twin_and_are_taken(env, N, H, sampler):
    a, b = engine(env, N, H, False), engine(env, N, H, True)
    assert b.ahead_stats()["available"] == 1 and b.ahead_stats()["on"] == 1 and b.ahead_stats()["fuse_us"] == AHEAD_DEFAULT_FUSE_US
    pool = pool_of(a) if sampler == "buffer" else None
    ptrs = [p.data_ptr() for p in pool] if pool else None
    S = states(env, STEPS)
    ua = tight_loop(a.step, S, ptrs)
    ub = tight_loop(b.step, S, ptrs)
    st = b.ahead_stats()
    print(f"{env} N={N} H={H} {sampler}: {st}")
    same(ua, ub)
    assert st["pending"] == 1
    np.testing.assert_array_equal(b.read("U_NOM"), a.read("U_NOM"))        # (the read cancels the queued kernel first)
    np.testing.assert_array_equal(b.read("J"), a.read("J"))
    assert st["taken"] >= STEPS - AHEAD_ARM_AFTER - 1
    assert a.ahead_stats()["launched"] == 0
    assert b.ahead_kernel() == f"ctk_mppi_ahead<{0 if env == 'CartPole' else 1}>" and a.ahead_kernel() == ""
    assert b.dominant_kernel() == a.dominant_kernel()                        # the launched kernel's name, whichever kernel served
    a.close(); b.close()


def controller(launch_ahead, rng_mode, N=128, H=12):
    from control_toolkit_amd.Controllers.controller_mpc import controller_mpc
    from control_toolkit_amd.Predictors import PredictorWrapper
    from control_toolkit_amd.Cost_Functions import CostFunctionWrapper
    oc = dict(seed=1, mpc_horizon=H, num_rollouts=N, mpc_timestep=0.02, rng_mode=rng_mode, device=0, cc_weight=1.0, R=1.0, LBD=100.0, NU=1000.0,
              SQRTRHOINV=0.03, period_interpolation_inducing_points=1, launch_ahead=launch_ahead)
    cc = {"mpc": {"optimizer": "mppi-hip", "predictor_specification": "ODE", "cost_function_specification": "default", "computation_library": "hip",
                  "controller_logging": False, "calculate_optimal_trajectory": False, "device": "gpu:0"}}
    c = controller_mpc("CartPole", (np.array([-1.0], np.float32), np.array([1.0], np.float32)), {"target_position": 0.0, "target_equilibrium": 1.0},
                       config_controllers=cc, config_optimizers={"mppi-hip": oc}, predictor=PredictorWrapper(), cost_function=CostFunctionWrapper(watch=False))
    c.configure()
    return c


@pytest.mark.parametrize("sampler", ["buffer", "rng"])
def test_tight_controller_steps_equal_the_twin_and_are_taken(sampler):
    from control_toolkit_amd.others.globals_and_utils import DeviceBufferRng
    ca, cb = controller(False, "device"), controller(True, "device")
    pool = pool_of(ca.optimizer.engine) if sampler == "buffer" else None
    S = states("CartPole", STEPS)
    us = []
    for c in (ca, cb):
        if pool:
            c.optimizer.rng = DeviceBufferRng([p.data_ptr() for p in pool], seed=1)
        us.append(tight_loop(lambda s, _p: np.asarray(c.step(s), np.float32).reshape(-1), S, None))
    st = cb.optimizer.engine.ahead_stats()
    print(f"controller_mpc.step {sampler}: {st}")
    same(us[0], us[1])
    np.testing.assert_array_equal(cb.optimizer.engine.read("U_NOM"), ca.optimizer.engine.read("U_NOM"))
    assert st["taken"] >= STEPS - AHEAD_ARM_AFTER - 1
    assert ca.optimizer.engine.ahead_stats()["launched"] == 0                # the optimizer key `launch_ahead: false`
    ca.optimizer.engine.close(); cb.optimizer.engine.close()


# ---- 2: gaps -------------------------------------------------------------------------------------------------------------------------
def test_gaps_leave_launches_untaken_and_the_form_disarms_and_rearms():
    """12 tight steps (the form arms), the 40-step loop with a 2 ms sleep before every 5th step (each slept step finds its kernel gone:
    untaken, the step is launched as ever; one untaken launch at a time does not disarm), two more slept steps behind the loop's last, which was one (consecutive
    untaken launches: disarmed), 12 tight steps (armed again).  The rule needs ARM_AFTER tight steps to arm, so a loop whose
    only gaps come four tight steps apart would never let it arm: the tight steps around the loop are what makes its sleeps bite."""
    N, H = 128, 12
    a, b = engine("CartPole", N, H, False), engine("CartPole", N, H, True)
    ptrs = [p.data_ptr() for p in pool_of(a)]
    n = 12 + STEPS + 2 + 12
    sleeps = {12 + t for t in range(STEPS) if t % 5 == 4} | {12 + STEPS, 12 + STEPS + 1}
    S = states("CartPole", n)
    ua = tight_loop(a.step, S, ptrs, sleeps)
    marks = {}
    def step_b(s, p, _t=[0]):
        if _t[0] in (12, 12 + STEPS, 12 + STEPS + 2):
            marks[_t[0]] = b.ahead_stats()
        _t[0] += 1
        return b.step(s, p)                                                   # a failing step raises: "no step returns an error"
    ub = tight_loop(step_b, S, ptrs, sleeps)
    st = b.ahead_stats()
    print(f"gaps: {marks} end {st}")
    same(ua, ub)
    np.testing.assert_array_equal(b.read("U_NOM"), a.read("U_NOM"))
    assert marks[12]["armed"] == 1 and marks[12]["arms"] == 1 and marks[12]["untaken"] == 0
    assert marks[12 + STEPS]["untaken"] >= STEPS // 5 and marks[12 + STEPS]["armed"] == 1    # single gaps: untaken, still armed
    assert marks[12 + STEPS + 2]["armed"] == 0                                                # two in a row: disarmed
    assert st["untaken"] > 0 and st["armed"] == 1 and st["arms"] == 2                         # ... and armed again
    assert st["launched"] == st["taken"] + st["untaken"] + st["cancelled"] + st["pending"]
    a.close(); b.close()


# ---- 3: one buffer refilled in place -----------------------------------------------------------------------------------------------------
def test_a_refilled_buffer_is_read_when_the_request_arrives():
    """one buffer, new contents before every step (torch's stream alone is synchronised, as tests/test_gpu_resident.py does it: the
    queued kernel runs while the buffer is filled and must not have read it, nor keep a cached line of it)"""
    import torch
    N, H = 128, 12
    S = states("CartPole", STEPS)
    us = []
    for ahead in (False, True):
        e = engine("CartPole", N, H, ahead)
        g = torch.Generator(device="cuda"); g.manual_seed(7)
        buf = torch.empty((int(e.samples_needed()),), device="cuda")
        out = []
        for s in S:
            buf.normal_(generator=g)
            torch.cuda.current_stream().synchronize()
            out.append(e.step(s, buf.data_ptr()).copy())
        us.append((out, e.read("U_NOM"), e.ahead_stats()))
        e.close()
    print(f"refilled buffer: {us[1][2]}")
    same(us[0][0], us[1][0])
    np.testing.assert_array_equal(us[1][1], us[0][1])


# ---- 4: every API entry between armed steps ------------------------------------------------------------------------------------------------
def test_every_api_entry_between_armed_steps_cancels_and_changes_nothing():
    import torch
    N, H = 128, 12
    S = states("CartPole", 12 + 6 * 3 + 1)
    res = []
    for ahead in (False, True):
        e = engine("CartPole", N, H, ahead)
        ptrs = [p.data_ptr() for p in pool_of(e)]
        log = tight_loop(e.step, S[:12], ptrs)
        c0 = e.ahead_stats()
        if ahead:
            assert c0["armed"] == 1 and c0["pending"] == 1
        t = 12
        def three():
            nonlocal t
            log.extend(tight_loop(e.step, S[t:t + 3], ptrs)); t += 3
        log.append(e.read("U_NOM").copy().reshape(-1)); three()
        st = e.get_state(); e.set_state(st); three()
        tw = e.get_param("terminal_weight"); e.set_param("terminal_weight", 0.5 * tw + 0.1); three()
        e.set_param("terminal_weight", tw); three()
        plan = np.zeros((1, H, 1), np.float32)
        _, j = e.rollout(S[t], plan, want_traj=False); log.append(np.asarray(j, np.float32).reshape(-1)); three()
        e.reset(); three()
        log.extend(tight_loop(e.step, S[t:t + 1], ptrs))
        c1 = e.ahead_stats()
        t0 = time.perf_counter(); torch.cuda.synchronize(); sync_s = time.perf_counter() - t0
        log.append(e.read("U_NOM").copy().reshape(-1))
        res.append((log, c0, c1, sync_s))
        t0 = time.perf_counter(); e.step(S[0], ptrs[0]); e.close(); close_s = time.perf_counter() - t0       # close() with a kernel pending returns
        assert close_s < 5.0
    (la, _, _, _), (lb, c0, c1, sync_s) = res
    print(f"api entries: before {c0} after {c1}; torch.cuda.synchronize() after the last step: {sync_s * 1e6:.1f} us")
    same(la, lb)
    # the six entries that followed a step directly found a queued kernel (the form stays armed across them): read, get_state,
    # set_param twice, rollout, reset
    assert c1["cancelled"] - c0["cancelled"] == 6
    assert c1["launched"] == c1["taken"] + c1["untaken"] + c1["cancelled"] + c1["pending"]
    assert sync_s < 1.0                                                        # it returns; recorded above, not asserted near the fuse


# ---- 5: switching off ------------------------------------------------------------------------------------------------------------------------
def test_switched_off_handles_never_launch_ahead():
    N, H = 128, 12
    e = engine("CartPole", N, H, False)
    ptrs = [p.data_ptr() for p in pool_of(e)]
    tight_loop(e.step, states("CartPole", 20), ptrs)
    st = e.ahead_stats()
    assert st["launched"] == 0 and st["on"] == 0 and st["available"] == 1 and e.ahead_kernel() == ""
    e.launch_ahead(True, fuse_us=50.0)                                         # ... and on again: the rule starts over
    assert e.ahead_stats()["fuse_us"] == 50.0 and e.ahead_stats()["armed"] == 0
    tight_loop(e.step, states("CartPole", 20), ptrs)
    assert e.ahead_stats()["taken"] >= 20 - AHEAD_ARM_AFTER - 1
    with pytest.raises(ValueError):
        e.launch_ahead(True, fuse_us=1.0e5)
    e.close()


def test_the_process_switch_turns_it_off_for_every_handle():
    code = ("import numpy as np, torch\n"
            "from control_toolkit_amd import CtkEngine\n"
            "e = CtkEngine('mppi', 'ODE', num_rollouts=128, mpc_horizon=12, dt=0.02, seed=3)\n"
            "s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)\n"
            "for _ in range(20): e.step(s, None)\n"
            "st = e.ahead_stats(); e.close()\n"
            "print('STATS', st['launched'], st['available'], st['on'])\n")
    env = dict(os.environ, CTK_MPPI_NO_AHEAD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "STATS 0 0 0" in r.stdout, r.stdout


# ---- 6: the name -------------------------------------------------------------------------------------------------------------------------------
def test_dominant_kernel_keeps_the_four_argument_name_and_ahead_kernel_names_the_kernel_once_it_served():
    """dominant_kernel() is the four-argument kernel's name before a step was served ahead and stays it afterwards (existing callers and
    tests read it after long tight loops: tests/test_gpu_mppi_early_poll.py); the real name of the serving kernel is ahead_kernel()'s"""
    N, H = 128, 12
    e = engine("CartPole", N, H, True)
    ptrs = [p.data_ptr() for p in pool_of(e)]
    S = states("CartPole", 12)
    four = e.dominant_kernel()
    assert four == "ctk_mppi_rollout<0, 0, false, false>" and e.ahead_kernel() == ""
    gc.disable()
    try:
        names = []
        for t, s in enumerate(S):
            e.step(s, ptrs[t & 3])
            names.append((e.dominant_kernel(), e.ahead_kernel(), e.ahead_stats()["taken"]))
    finally:
        gc.enable()
    for dom, ahead, taken in names:                                           # (asking for a name is no device call)
        assert dom == four and ahead == ("ctk_mppi_ahead<0>" if taken > 0 else ""), names
    assert names[-1][2] > 0
    e.profile_enable(True, every=1)                                            # a timed step is a launched step
    e.step(S[0], ptrs[0])
    assert e.dominant_kernel() == four and e.ahead_kernel() == "ctk_mppi_ahead<0>"
    e.profile_enable(False)
    e.close()
