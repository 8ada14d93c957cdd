#!/usr/bin/env python3
"""Where does ctk_step's own host time go at mppi_cfg2 (MPPI N 1024 / H 50 / period 1, device sample buffers)?  Diagnostic, not a
benchmark: a -DCTK_HOST_STAMPS build of the library (never the product one) keeps steady_clock stamps in the handle — ctk_step entered,
before the launch call, the launch call returned, {u, seq} seen — and exports ctk_diag_host_split to read their sums.

  python3 tools/host_split.py --build      # compile tools/_variants/libctk_hip_HOST_STAMPS.so (git-ignored; needs hipcc, no GPU)
  python3 tools/host_split.py              # run on the GPU: loads that library through CTK_HIP_LIBRARY, prints the split

The stamped library is the product's sources with four clock reads per step added (about 20 ns each), so its step is that much longer."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "tools", "_variants", "libctk_hip_HOST_STAMPS.so")


def build():
    obj = os.path.join(ROOT, "tools", "_variants", "obj_HOST_STAMPS")
    subprocess.run(["make", "-C", os.path.join(ROOT, "control_toolkit_amd", "csrc"), "-j8", f"BUILD={obj}", f"LIB={VARIANT}",
                    "EXTRA=-DCTK_HOST_STAMPS", VARIANT], check=True)
    print(VARIANT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--steps", type=int, default=500, help="steps per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-ahead", action="store_true", help="switch the launched-ahead form off (the split of the launched step)")
    a = ap.parse_args()
    if a.build:
        return build()
    if not os.path.exists(VARIANT):
        raise SystemExit(f"{VARIANT} is not there: run with --build first")
    os.environ["CTK_HIP_LIBRARY"] = VARIANT
    sys.path.insert(0, ROOT)
    import time
    import numpy as np
    import torch
    from control_toolkit_amd import CtkEngine

    N, H = 1024, 50
    e = CtkEngine("mppi", "ODE", num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=1, seed=1)
    if a.no_ahead:
        e.launch_ahead(False)
    read = e._lib.ctk_diag_host_split
    read.restype, read.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    out = (ctypes.c_double * 4)()
    bufs = [torch.randn((N, H, 1), device="cuda") for _ in range(16)]
    ptrs = [b.data_ptr() for b in bufs]
    torch.cuda.synchronize()
    s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
    for i in range(100):
        e.step(s, ptrs[i & 15])
    read(e._h, out)
    ahead = e.ahead_stats()["taken"] > 0
    print(f"MPPI N={N} H={H} p=1, device sample buffers, step_path {e.step_path}, kernel {e.ahead_kernel() if ahead else e.dominant_kernel()}")
    if ahead:
        # a step served by the kernel launched ahead (include/ctk_hip_ahead.h): the stamps stand at the request's store and at workgroup 0's
        # "taken" word; the launch call of the NEXT step's kernel lies inside the third interval, under this step's kernel
        print(f"launched ahead: {e.ahead_stats()}")
        print("block  steps  wall us/step  entry->request stored  request stored->taken seen  taken seen->{u,seq} seen  sum  (us per step)")
    else:
        print("block  steps  wall us/step  entry->launch call  inside launch call  launch return->{u,seq} seen  sum  (us per step)")
    rows = []
    for b in range(a.blocks):
        t0 = time.perf_counter()
        for i in range(a.steps):
            e.step(s, ptrs[i & 15])
        wall = (time.perf_counter() - t0) / a.steps * 1e6
        assert read(e._h, out) == 0 and int(out[0]) == a.steps, list(out)
        pre, launch, wait = (out[k] / out[0] * 1e-3 for k in (1, 2, 3))
        rows.append((wall, pre, launch, wait))
        print(f"{b:5d}  {a.steps:5d}  {wall:12.2f}  {pre:18.2f}  {launch:18.2f}  {wait:27.2f}  {pre + launch + wait:5.2f}")
    med = np.median(np.array(rows), axis=0)
    print(f"median        {med[0]:12.2f}  {med[1]:18.2f}  {med[2]:18.2f}  {med[3]:27.2f}  {med[1] + med[2] + med[3]:5.2f}")
    print(f"(wall - sum = {med[0] - med[1] - med[2] - med[3]:.2f} us: the Python wrapper, the call into the library and ctk_step's return)")
    if ahead:
        print(f"request stored -> {{u, seq}} seen: {med[2] + med[3]:.2f} us; launched ahead at the end: {e.ahead_stats()}")
    e.close()


if __name__ == "__main__":
    main()
