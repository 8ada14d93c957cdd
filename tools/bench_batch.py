#!/usr/bin/env python3
"""Throughput of B independent MPPI controllers: one CtkMppiBatch.step (leg a) against B CtkEngine.step calls in a loop (leg b, all an
engine without the batch object offers), per problem BASELINE cfg2 (MPPI, N 1024 / H 50, CartPole ODE) with the on-device sampler.

Both legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when both legs saw the same
minutes); the figures are host-clock medians over --steps calls per leg after --warmup.  Every call is synchronous (it returns when the
result is on the host), so a host clock around it measures the whole step.

    python tools/bench_batch.py --out profiles/r07_mppi_batch.txt            # the table
    python tools/bench_batch.py --only batch --sizes 16 --steps 300          # one leg alone (the kernel trace's subject)

On a tree without CtkMppiBatch the script still runs leg (b): the same command gives the parent commit's figure."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine   # noqa: E402
try:
    from control_toolkit_amd import CtkMppiBatch   # noqa: E402
except ImportError:                                 # a tree from before the batch object: leg (b) only
    CtkMppiBatch = None

CFG2 = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1)


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def measure(B, steps, warmup, rounds, legs):
    rng = np.random.default_rng(B)
    S = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S[:, 2] += 2.8
    seeds = [100 + p for p in range(B)]
    batch = CtkMppiBatch(B, seeds=seeds, **CFG2) if "batch" in legs else None
    engines = [CtkEngine("mppi", "ODE", seed=seeds[p], **CFG2) for p in range(B)] if "loop" in legs else []
    rows = [S[p] for p in range(B)]

    def leg_a():
        batch.step(S)

    def leg_b():
        for e, s in zip(engines, rows):
            e.step(s)
    if batch:
        timed(leg_a, warmup)
    if engines:
        timed(leg_b, warmup)
    a, b = [], []
    per = max(1, steps // rounds)
    for _ in range(rounds):                         # alternate the legs
        if batch:
            a += timed(leg_a, per)
        if engines:
            b += timed(leg_b, per)
    name = batch.dominant_kernel() if batch else engines[0].dominant_kernel()
    if batch:
        batch.close()
    for e in engines:
        e.close()
    return a, b, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", choices=["batch", "loop"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_batch: no GPU (nothing here is measured on a CPU)")
    legs = {"batch", "loop"} if args.only is None else {args.only}
    if CtkMppiBatch is None:
        legs.discard("batch")
        if not legs:
            sys.exit("bench_batch: this tree has no CtkMppiBatch")
    lines = [f"# tools/bench_batch.py {args.label}: per problem MPPI N 1024 / H 50 / period 1, CartPole ODE, device Philox; host-clock medians over "
             f"{args.steps} calls per leg ({args.rounds} alternating rounds) after {args.warmup} warm-up calls",
             "# (a) one CtkMppiBatch.step of B problems    (b) B CtkEngine.step calls in a loop    us/call | us/problem | problem-steps/s",
             f"{'B':>4s} {'(a) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} {'steps/s':>10s} | {'(b) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} {'steps/s':>10s} | {'(a)/(b)':>8s}"]
    print("\n".join(lines), flush=True)
    for B in [int(x) for x in args.sizes.split(",")]:
        a, b, name = measure(B, args.steps, args.warmup, args.rounds, legs)

        def cols(v):
            if not v:
                return f"{'-':>12s} {'-':>8s} {'-':>8s} {'-':>8s} {'-':>10s}"
            q = statistics.quantiles(v, n=10)
            m = statistics.median(v)
            return f"{m:12.2f} {q[0]:8.2f} {q[-1]:8.2f} {m / B:8.2f} {B / m * 1e6:10.0f}"
        ratio = f"{statistics.median(a) / statistics.median(b):8.3f}" if a and b else f"{'-':>8s}"
        line = f"{B:4d} {cols(a)} | {cols(b)} | {ratio}"
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# kernel of leg {'(a)' if 'batch' in legs else '(b)'}: {name}")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
