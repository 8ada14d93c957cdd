#!/usr/bin/env python3
"""Where does a step() spend its wall time?  (diagnostic; not a benchmark)

Run plainly it measures the path this process gets (the pre-bound call where _ctk_pystep is built) and then starts itself once more
with CTK_PYSTEP=0, so that the ctypes path stands beside it; every line names the path that ran (engine.step_path)."""
import os, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from control_toolkit_amd import CtkEngine

def timeit(fn, n=300, warm=30):
    for _ in range(warm): fn()
    ts = []
    for _ in range(n):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    ts = np.array(ts) * 1e6
    return f"median {np.median(ts):7.2f} us  p10 {np.percentile(ts,10):7.2f}  p90 {np.percentile(ts,90):7.2f}"

s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
for (N, H) in [(64, 1), (1024, 50)]:
    e = CtkEngine("mppi", "ODE", num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=1, seed=1)
    noise = torch.randn((N, H, 1), device="cuda")
    ptr = noise.data_ptr()
    up = np.zeros(1, np.float32)
    tag = f"[{e.step_path:6s}] MPPI N={N} H={H}:"
    print(tag, "device buffer          ", timeit(lambda: e.step(s, ptr)))
    print(tag, "device buffer + u_prev ", timeit(lambda: e.step(s, ptr, u_prev=up)))
    print(tag, "device rng             ", timeit(lambda: e.step(s, None)))
    print(tag, "float64 state (fallback)", timeit(lambda s64=s.astype(np.float64): e.step(s64, ptr)))
    e.profile_enable(True)
    for _ in range(50): e.step(s, ptr)
    k = e.profile_read()
    print(f"   rollout kernel (dispatch timestamps): mean {k.mean()*1e3:.2f} us")
    e.close()
import ctypes
print("python no-op ctypes call:", timeit(lambda: e._lib.ctk_abi_version()))
if os.environ.get("CTK_PYSTEP", "1") != "0":
    sys.stdout.flush()
    print("---- the same with CTK_PYSTEP=0 (a child process: the switch is read once per process) ----", flush=True)
    subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, CTK_PYSTEP="0"), check=True)
