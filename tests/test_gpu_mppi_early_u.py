"""-m gpu: the MPPI rollout kernel that publishes u = u_nom_new[0] AHEAD of the plan update (ctk_mppi_body_5_post.inc: EARLY_U, what FORM 0
of ctk_mppi_rollout does in a merge + update launch of the analytic predictor with one control input) computes what the late order
computes, bit for bit.  The late order is the diagnostic switch CTK_MPPI_LATE_U (read once per process), so each form runs in a child
process of its own; both run the same closed loop from the same seeds, and u, J and u_nom — read right after every step — are compared
bitwise.

Sizes: the smallest at which the early path can go wrong — one block with P = 2 (c0 + 1 the last real column) and P = 1 (c0 + 1 the
tile's zero pad), two blocks with invalid lanes in the second, the headline (BASELINE configs[1]) with a sample buffer and with the
in-kernel sampler, an interpolated plan (entry 0 reads two columns with weights from the table), 64 blocks (one full lane batch of the
early merge), 128 blocks of narrow records (two lane batches), and the launches the early order is gated off for: more than one 8-deep
poll batch of record words (N 8192 / H 20: 128 x 22 words, and N 16384 / H 20 / period 10: 256 records — the wide tail) and two control
inputs (Quad2D).  There the switch must change nothing, the kernel's name included.

Ordering: what a caller may do the moment step() returns while the launch is still finishing the plan update — refill the step's sample
buffer in place on another stream, reset(), get_state() / set_state() into a fresh engine — gives the same results in both orders; and
in the early order the published u equals u_nom[0] read after the step, bitwise, for every step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from control_toolkit_amd import CtkEngine
case = json.loads(sys.argv[2]); out = sys.argv[3]
N, H, p, env, mode = case["N"], case["H"], case["p"], case.get("env", "CartPole"), case.get("mode", "loop")
def engine():
    return CtkEngine("mppi", "ODE", environment=env, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, seed=7)
try:
    e = engine()
except Exception as ex:                      # a size the engine refuses (H = 1): both children must refuse it alike
    np.savez(out, refused=np.array(type(ex).__name__))
    sys.exit(0)
P, C = e.inducing_points(), e.C
g = torch.Generator(device="cuda"); g.manual_seed(5)
pool = [torch.randn((N * P * C,), generator=g, device="cuda") for _ in range(3)]
torch.cuda.synchronize()
s = np.array([0.05, -0.1, 2.8, 0.4, 0.02, -0.03][:e.S], np.float32)
us, Js, unoms = [], [], []
def advance(s, u):                           # a closed loop: the next state depends on the input this step produced
    d = np.zeros_like(s); d[0] = s[1]; d[1] = u.ravel()[0]; d[2] = s[3]; d[3] = -np.sin(s[2])
    return (s + np.float32(0.02) * d).astype(np.float32)
def record(e, u):
    us.append(u); Js.append(np.asarray(e.read("J"), np.float32).copy()); unoms.append(np.asarray(e.read("U_NOM"), np.float32).copy())
steps = 8 if mode in ("loop", "refill") else 4
for t in range(steps):
    if mode == "refill":
        buf = pool[0].data_ptr()
    else:
        buf = None if case["sampler"] == "device" or (case["sampler"] == "mixed" and t % 2) else pool[t % 3].data_ptr()
    u = np.asarray(e.step(s, buf), np.float32).copy()
    if mode == "refill":
        # the moment step() returns: new draws into the SAME buffer, on torch's stream (not the engine's), then everything settles
        pool[0].normal_(generator=g)
        torch.cuda.synchronize()
    if mode == "reset" and t == 0:
        e.reset()                            # directly after a step; three more steps follow
        us.append(u)
    elif mode == "state" and t == 2:
        st = e.get_state()                   # directly after a step, into a fresh engine, which takes the last step
        us.append(u)
        e.close()
        e = engine()
        e.set_state(st)
    else:
        record(e, u)
    s = advance(s, u)
kernel = e.dominant_kernel()
e.close()
np.savez(out, u=np.stack(us), J=np.stack(Js), u_nom=np.stack(unoms), kernel=np.array(kernel))
"""

# early: the launch takes the early order unless CTK_MPPI_LATE_U is set (one control input, at most 128 records and 2048 record words)
CASES = [
    dict(N=64, H=2, p=1, sampler="buffer", early=True),
    dict(N=64, H=1, p=1, sampler="buffer", early=True),
    dict(N=100, H=7, p=1, sampler="device", early=True),
    dict(N=1024, H=50, p=1, sampler="buffer", early=True, headline=True),
    dict(N=1024, H=50, p=1, sampler="device", early=True, headline=True),
    dict(N=1000, H=40, p=10, sampler="mixed", early=True),
    dict(N=4096, H=20, p=1, sampler="buffer", early=True),
    dict(N=8192, H=10, p=1, sampler="buffer", early=True),      # 128 records of 12 words: two lane batches of the early merge
    dict(N=8192, H=20, p=1, sampler="buffer", early=False),     # 128 records of 22 words: more than one 8-deep poll batch, the wide tail
    dict(N=16384, H=20, p=10, sampler="buffer", early=False),   # 256 records: the wide tail
    dict(N=1024, H=20, p=1, sampler="buffer", early=False, env="Quad2D"),
]
HEADLINE = dict(N=1024, H=50, p=1, sampler="buffer", early=True, headline=True)


def run_child(tmp_path, case, late):
    env = dict(os.environ)
    env.pop("CTK_MPPI_LATE_U", None)
    if late:
        env["CTK_MPPI_LATE_U"] = "1"
    out = str(tmp_path / ("late.npz" if late else "early.npz"))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(case), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child ({'late' if late else 'early'} u) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(out)


def compare(tmp_path, case):
    early, late = run_child(tmp_path, case, False), run_child(tmp_path, case, True)
    if "refused" in early.files or "refused" in late.files:
        assert "refused" in early.files and "refused" in late.files and str(early["refused"]) == str(late["refused"])
        return None, None
    ke, kl = str(early["kernel"]), str(late["kernel"])
    if case["early"]:
        assert ke != kl, (ke, kl)                                   # the two orders really ran
        assert ke == "ctk_mppi_rollout<0, 0, false, false>", ke     # FORM 0: the four-argument kernel
        assert kl.startswith("ctk_mppi_rollout<0, 0, false, false, "), kl
    else:
        assert ke == kl, (ke, kl)                                   # gated off: the switch changes nothing
    assert np.isfinite(early["J"]).all() and np.isfinite(early["u"]).all()
    for name in ("u", "J", "u_nom"):
        assert early[name].shape == late[name].shape
        np.testing.assert_array_equal(early[name].view(np.uint32), late[name].view(np.uint32), err_msg=name)
    return early, late


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.get('env', 'CartPole')}_N{c['N']}_H{c['H']}_p{c['p']}_{c['sampler']}")
def test_early_u_is_bit_identical_to_the_late_order(tmp_path, case):
    early, _ = compare(tmp_path, case)
    if early is not None and case.get("env", "CartPole") == "CartPole":
        # the published value IS the plan's first entry (in the early order the two come from different places in the kernel)
        assert early["u"].shape[0] == early["u_nom"].shape[0] == 8
        np.testing.assert_array_equal(early["u"].reshape(8, -1)[:, 0].view(np.uint32), early["u_nom"].reshape(8, -1)[:, 0].view(np.uint32))


@pytest.mark.parametrize("mode", ["refill", "reset", "state"])
def test_what_a_caller_does_right_after_step_is_ordered_behind_the_plan_update(tmp_path, mode):
    early, _ = compare(tmp_path, dict(HEADLINE, mode=mode))
    assert early is not None
    if mode == "refill":
        np.testing.assert_array_equal(early["u"].reshape(8, -1)[:, 0].view(np.uint32), early["u_nom"].reshape(8, -1)[:, 0].view(np.uint32))
