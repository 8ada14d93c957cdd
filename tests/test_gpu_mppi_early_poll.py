"""-m gpu: the pipelined poll of the early u (ctk_mppi_merge.h: mppi_early_u keeps LL_EARLY_DEPTH passes of {value, seq} loads in flight
and takes a word from the first pass that shows it) publishes what the late order publishes, bit for bit.  The late order is the
diagnostic switch CTK_MPPI_LATE_U, read once per process: ONE child process per order runs every case below from the same seeds, and
u, J and u_nom — read right after every step of a closed loop of 12 steps — are compared bitwise, with buffer samples and with the
in-kernel sampler.

Sizes, all on the CartPole ODE predictor at H = 8 with period 1 (P = 8) and period 4 (P = 2):
    N 64     1 block     the poll sees only its own words
    N 128    2 blocks
    N 1024   16 blocks   the headline's grid
    N 4160   65 blocks   lane 0 of the second 64-block batch alone (every other lane of that batch loads a clamped address)
    N 8192   128 blocks  the largest early-u grid
and H = 1 (c0 + 1 == P: the fourth word does not exist, its load re-reads the third) where the engine accepts it; where it does not,
both children must refuse alike.

Uneven load: the headline (N 1024, H 50, period 1, buffer samples) is stepped 200 times while a second engine (N 65536, its own
handle and stream, the same process) steps concurrently from a thread, so that blocks of the small grid start late and out of
order: every step's u against the late-order child's run of the same inputs (a closed loop: one differing bit would change every
later input as well).  The poll's time-out is not forced."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, threading
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from control_toolkit_amd import CtkEngine
cases = json.loads(sys.argv[2]); out = sys.argv[3]
res = {}
def advance(s, u):                           # a closed loop: the next state depends on the input this step produced
    d = np.zeros_like(s); d[0] = s[1]; d[1] = u.ravel()[0]; d[2] = s[3]; d[3] = -np.sin(s[2])
    return (s + np.float32(0.02) * d).astype(np.float32)
def closed_loop(e, N, steps, sampler, full):
    P, C = e.inducing_points(), e.C
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    pool = [torch.randn((N * P * C,), generator=g, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
    us, Js, unoms = [], [], []
    for t in range(steps):
        u = np.asarray(e.step(s, None if sampler == "device" else pool[t % 3].data_ptr()), np.float32).copy()
        us.append(u)
        if full:
            Js.append(np.asarray(e.read("J"), np.float32).copy()); unoms.append(np.asarray(e.read("U_NOM"), np.float32).copy())
        s = advance(s, u)
    return us, Js, unoms
for c in cases:
    key = c["id"]
    try:
        e = CtkEngine("mppi", "ODE", environment="CartPole", num_rollouts=c["N"], mpc_horizon=c["H"], dt=0.02,
                      period_interpolation_inducing_points=c["p"], seed=7)
    except Exception as ex:                  # a size the engine refuses: both children must refuse it alike
        res[key + "/refused"] = np.array(type(ex).__name__)
        continue
    if c.get("load"):
        big = CtkEngine("mppi", "ODE", environment="CartPole", num_rollouts=65536, mpc_horizon=8, dt=0.02,
                        period_interpolation_inducing_points=1, seed=11, pystep=False)
        stream = torch.cuda.Stream()
        big.set_stream(stream.cuda_stream)
        stop, count = threading.Event(), [0]
        def load():
            sb = np.array([0.0, 0.1, 3.0, -0.2], np.float32)
            while not stop.is_set():
                big.step(sb); count[0] += 1
        th = threading.Thread(target=load); th.start()
        try:
            us, Js, unoms = closed_loop(e, c["N"], c["steps"], c["sampler"], False)
        finally:
            stop.set(); th.join()
        torch.cuda.synchronize()
        res[key + "/load_steps"] = np.array(count[0])
        big.close()
    else:
        us, Js, unoms = closed_loop(e, c["N"], c["steps"], c["sampler"], True)
        res[key + "/J"] = np.stack(Js); res[key + "/u_nom"] = np.stack(unoms)
    res[key + "/u"] = np.stack(us)
    res[key + "/kernel"] = np.array(e.dominant_kernel())
    e.close()
np.savez(out, **res)
"""

STEPS = 12
CASES = [dict(id=f"N{N}_H8_p{p}_{sampler}", N=N, H=8, p=p, sampler=sampler, steps=STEPS)
         for N in (64, 128, 1024, 4160, 8192) for p in (1, 4) for sampler in ("buffer", "device")]
CASES += [dict(id=f"N{N}_H1_p1_{sampler}", N=N, H=1, p=1, sampler=sampler, steps=STEPS) for N in (64, 128) for sampler in ("buffer", "device")]
LOADED = dict(id="loaded_N1024_H50_p1_buffer", N=1024, H=50, p=1, sampler="buffer", steps=200, load=True)


@pytest.fixture(scope="module")
def orders(tmp_path_factory):
    """(early, late): every case, ONE child process per order"""
    tmp = tmp_path_factory.mktemp("early_poll")
    got = []
    for late in (False, True):
        env = dict(os.environ)
        env.pop("CTK_MPPI_LATE_U", None)
        if late:
            env["CTK_MPPI_LATE_U"] = "1"
        out = str(tmp / ("late.npz" if late else "early.npz"))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(CASES + [LOADED]), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"child ({'late' if late else 'early'} u) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got.append(np.load(out))
    return got


def both_ran(early, late, key):
    """False: both children refused the size alike"""
    if key + "/refused" in early.files or key + "/refused" in late.files:
        assert key + "/refused" in early.files and key + "/refused" in late.files
        assert str(early[key + "/refused"]) == str(late[key + "/refused"])
        return False
    ke, kl = str(early[key + "/kernel"]), str(late[key + "/kernel"])
    assert ke == "ctk_mppi_rollout<0, 0, false, false>", ke          # FORM 0: the early order really ran ...
    assert kl.startswith("ctk_mppi_rollout<0, 0, false, false, "), kl  # ... and so did the late one
    return True


def same_bits(early, late, key, name):
    a, b = early[key + "/" + name], late[key + "/" + name]
    assert a.shape == b.shape and np.isfinite(a).all()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{key}: {name}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_pipelined_early_poll_is_bit_identical_to_the_late_order(orders, case):
    early, late = orders
    key = case["id"]
    if not both_ran(early, late, key):
        return
    for name in ("u", "J", "u_nom"):
        same_bits(early, late, key, name)
    u, u_nom = early[key + "/u"], early[key + "/u_nom"]
    assert u.shape[0] == u_nom.shape[0] == STEPS
    # the published value IS the plan's first entry (in the early order the two come from different places in the kernel)
    np.testing.assert_array_equal(u.reshape(STEPS, -1)[:, 0].view(np.uint32), u_nom.reshape(STEPS, -1)[:, 0].view(np.uint32))


def test_every_u_under_uneven_load_is_the_late_orders(orders):
    early, late = orders
    key = LOADED["id"]
    assert both_ran(early, late, key)
    assert early[key + "/u"].shape[0] == LOADED["steps"]
    assert int(early[key + "/load_steps"]) > 0 and int(late[key + "/load_steps"]) > 0, "the second engine did not step beside the first"
    same_bits(early, late, key, "u")
