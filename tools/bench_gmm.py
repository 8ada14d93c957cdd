#!/usr/bin/env python3
"""Step time of the CEM-GMM optimizer, sampling inside the rollout kernel and with materialised plans (CTK_GMM_MATERIALIZE=1), next to plain CEM in its launch-per-phase form (CTK_NO_CEM_FUSED=1, the form CEM-GMM is
built from) and in its default one-launch form, CartPole / analytic predictor, on-device draws.  Not a bench.py line; the table
goes to profiles/ and DESIGN.md.

    python tools/bench_gmm.py [--steps 300] [--runs 4]
    python tools/bench_gmm.py --trace N H K      # 100 cem_gmm steps at one size and nothing else: the program to put behind
                                                 # `rocprofv3 --kernel-trace --stats --` (CTK_GMM_MATERIALIZE=1 for the other form)

Every cell: the optimizer step through CtkEngine.step with the in-kernel sampler, state changing every call, median of `--steps`
calls after 30 untimed ones; the variants are alternated `--runs` times and the median (range) of the runs is printed."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(200, 40, 40, 3), (4096, 30, 409, 3)]      # (N, H, K, outer iterations): the template's cem-gmm-tf entry; BASELINE configs[2]
VARIANTS = [("cem_gmm in-rollout", "cem_gmm", {}), ("cem_gmm materialised", "cem_gmm", {"CTK_GMM_MATERIALIZE": "1"}), ("cem launch-per-phase", "cem", {"CTK_NO_CEM_FUSED": "1"}), ("cem one-launch", "cem", {})]


def run(opt, envvars, N, H, K, its, steps):
    from control_toolkit_amd import CtkEngine
    saved = {k: os.environ.get(k) for k in envvars}
    os.environ.update(envvars)
    try:
        e = CtkEngine(opt, "ODE", num_rollouts=N, mpc_horizon=H, dt=0.02, seed=1, cem_outer_it=its, cem_best_k=K)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    s = np.array([0.1, 0.0, 0.2, 0.0], np.float32)
    t = np.empty(steps)
    for i in range(30 + steps):
        s[0] = 0.1 + 0.01 * (i % 7)
        t0 = time.perf_counter()
        e.step(s, None)                 # synchronous: returns when u is valid
        if i >= 30:
            t[i - 30] = time.perf_counter() - t0
    name = e.dominant_kernel()
    e.close()
    return float(np.median(t) * 1e6), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--trace", type=int, nargs=3, metavar=("N", "H", "K"), help="only run 100 cem_gmm steps at this size (for a kernel trace)")
    a = ap.parse_args()
    if a.trace:
        N, H, K = a.trace
        run("cem_gmm", {}, N, H, K, 3, 70)       # 30 + 70 steps
        return
    for N, H, K, its in SIZES:
        print(f"# N {N}, H {H}, K {K}, {its} outer iterations, CartPole ODE, device draws; us / step, median of {a.steps} calls per run")
        cells = {label: [] for label, _, _ in VARIANTS}
        names = {}
        for r in range(a.runs):
            for label, opt, envvars in VARIANTS:
                med, names[label] = run(opt, envvars, N, H, K, its, a.steps)
                cells[label].append(med)
                print(f"  run {r} {label:<22}{med:9.2f}")
        for label, _, _ in VARIANTS:
            v = np.array(cells[label])
            print(f"median of {a.runs} {label:<22}{np.median(v):9.2f} us (range {v.min():.2f}-{v.max():.2f})   rollout kernel: {names[label]}")


if __name__ == "__main__":
    main()
