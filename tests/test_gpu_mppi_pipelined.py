"""-m gpu: the MPPI recurrence with sin / cos carried one step ahead (ctk_env.h: recur_env_range, PIPE) computes what the previous
recurrence computed, bit for bit.  The previous loop is the diagnostic switch CTK_MPPI_OLD_RECUR (read once per process), so each form
runs in a child process of its own; both run the same closed loop and J, u and u_nom are compared bitwise after every step.
Cases: BASELINE configs[1] (N 1024 / H 50 / period 1) with a sample buffer and with the in-kernel sampler, a period-10 case, a size that
takes the wide tail (256 records: CTK_MPPI_FORM_WIDE_TAIL), and the resident form."""
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
N, H, p, resident = case["N"], case["H"], case["p"], case["resident"]
e = CtkEngine("mppi", "ODE", num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, seed=7)
if resident:
    e.resident_enable(True, idle_us=100000.0)
P = e.inducing_points()
g = torch.Generator(device="cuda"); g.manual_seed(5)
pool = [torch.randn((N * P,), generator=g, device="cuda") for _ in range(3)]
s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
us, Js, unoms = [], [], []
for t in range(8):
    buf = None if case["sampler"] == "device" or (case["sampler"] == "mixed" and t % 2) else pool[t % 3].data_ptr()
    u = np.asarray(e.step(s, buf), np.float32).copy()
    us.append(u)
    if not resident:                     # (a read ends the resident kernel: the last step's J / u_nom are read below)
        Js.append(np.asarray(e.read("J"), np.float32).copy()); unoms.append(np.asarray(e.read("U_NOM"), np.float32).copy())
    # a closed loop: the next state depends on the input this step produced
    s = (s + np.float32(0.02) * np.array([s[1], u.ravel()[0], s[3], -np.sin(s[2])], np.float32)).astype(np.float32)
kernel = e.dominant_kernel()             # (before the reads: they end the resident kernel, and the handle names the launched one again)
Js.append(np.asarray(e.read("J"), np.float32).copy()); unoms.append(np.asarray(e.read("U_NOM"), np.float32).copy())
e.close()
np.savez(out, u=np.stack(us), J=np.stack(Js), u_nom=np.stack(unoms), kernel=np.array(kernel))
"""

CASES = [
    dict(N=1024, H=50, p=1, sampler="buffer", resident=False),
    dict(N=1024, H=50, p=1, sampler="device", resident=False),
    dict(N=1000, H=40, p=10, sampler="mixed", resident=False),
    dict(N=16384, H=20, p=10, sampler="buffer", resident=False),
    dict(N=1024, H=50, p=1, sampler="mixed", resident=True),
]


def run_child(tmp_path, case, old):
    env = dict(os.environ)
    env.pop("CTK_MPPI_OLD_RECUR", None)
    if old:
        env["CTK_MPPI_OLD_RECUR"] = "1"
    out = str(tmp_path / ("old.npz" if old else "new.npz"))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(case), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child ({'old' if old else 'pipelined'} recurrence) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(out)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c['N']}_H{c['H']}_p{c['p']}_{c['sampler']}{'_resident' if c['resident'] else ''}")
def test_pipelined_recurrence_is_bit_identical_to_the_old_loop(tmp_path, case):
    new, old = run_child(tmp_path, case, False), run_child(tmp_path, case, True)
    kn, ko = str(new["kernel"]), str(old["kernel"])
    if case["resident"]:
        assert kn.startswith("ctk_mppi_resident<0, ") and kn != ko, (kn, ko)
    else:
        assert kn.startswith("ctk_mppi_rollout<0, 0, false, false") and kn != ko, (kn, ko)      # the two forms really ran
    assert np.isfinite(new["J"]).all()
    for name in ("u", "J", "u_nom"):
        assert new[name].shape == old[name].shape
        np.testing.assert_array_equal(new[name].view(np.uint32), old[name].view(np.uint32), err_msg=name)
