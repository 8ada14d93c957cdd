#!/usr/bin/env python3
"""Throughput of B independent MPPI controllers with the MLP predictor: one CtkMppiMlpBatch.step (leg a) against B
CtkEngine("mppi", "MLP").step calls in a loop (leg b, all a tree without the batch object offers) on the same library in the same
process, per problem BASELINE cfg2's size (N 1024 / H 50, period 1, CartPole) with the on-device sampler and a network per problem.
Leg (w) prices online adaptation: set_problem_weights of all B problems (one transfer) ahead of every batch step.

The legs alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same minutes); the figures are
host-clock medians over --steps calls per leg after --warmup.  Every call is synchronous (it returns when the result is on the host), so
a host clock around it measures the whole step.  The run-to-run spread of (b) is reported beside the ratio: the largest relative
deviation of a round's median of (b) from the median of all its calls.

    python tools/bench_mlp_batch.py --out profiles/r14_mlp_batch.txt            # the table
    python tools/bench_mlp_batch.py --only batch --sizes 8 --steps 300          # one leg alone (the kernel trace's subject)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine, CtkMppiMlpBatch   # noqa: E402
from control_toolkit_amd._capi import mlp_weight_count   # noqa: E402

CFG2 = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1)


def networks(B):
    """B 5-32-32-4 tanh networks, weights N(0, 1 / fan_in), biases N(0, 0.1): [B, 1380]"""
    out = np.empty((B, mlp_weight_count(4, 1)), np.float32)
    for p in range(B):
        rng = np.random.default_rng(1000 + p)
        parts = [rng.normal(0, 1 / np.sqrt(5), 32 * 5), rng.normal(0, 0.1, 32), rng.normal(0, 1 / np.sqrt(32), 32 * 32), rng.normal(0, 0.1, 32),
                 rng.normal(0, 1 / np.sqrt(32), 4 * 32), rng.normal(0, 0.1, 4)]
        out[p] = np.concatenate(parts)
    return out


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
    W = networks(B)
    batch = None
    if legs & {"batch", "adapt"}:
        batch = CtkMppiMlpBatch(B, seeds=seeds, **CFG2)
        batch.set_problem_weights(W)
    engines = [CtkEngine("mppi", "MLP", seed=seeds[p], **CFG2) for p in range(B)] if "loop" in legs else []
    for e, w in zip(engines, W):
        e.set_predictor_weights(w)
    rows = [S[p] for p in range(B)]

    def leg_a():
        batch.step(S)

    def leg_b():
        for e, s in zip(engines, rows):
            e.step(s)

    def leg_w():
        batch.set_problem_weights(W)
        batch.step(S)
    run = [(n, f) for n, f in (("batch", leg_a), ("loop", leg_b), ("adapt", leg_w)) if n in legs]
    for _, f in run:
        timed(f, warmup)
    out = {n: [] for n, _ in run}
    round_medians = []
    per = max(1, steps // rounds)
    for _ in range(rounds):                         # alternate the legs
        for n, f in run:
            t = timed(f, per)
            out[n] += t
            if n == "loop":
                round_medians.append(statistics.median(t))
    spread = max(abs(m / statistics.median(out["loop"]) - 1.0) for m in round_medians) if round_medians else None
    names = (batch.dominant_kernel() if batch else "-", engines[0].dominant_kernel() if engines else "-")
    if batch:
        batch.close()
    for e in engines:
        e.close()
    return out, spread, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32,64")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", choices=["batch", "loop", "adapt"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mlp_batch: no GPU (nothing here is measured on a CPU)")
    legs = {"batch", "loop", "adapt"} if args.only is None else {args.only}
    lines = [f"# tools/bench_mlp_batch.py {args.label}: per problem MPPI N 1024 / H 50 / period 1, CartPole MLP 5-32-32-4 (a network per problem), device "
             f"Philox; host-clock medians over {args.steps} calls per leg ({args.rounds} alternating rounds) after {args.warmup} warm-up calls",
             "# (a) one CtkMppiMlpBatch.step of B problems   (b) B CtkEngine('mppi', 'MLP').step calls in a loop   (w) set_problem_weights of all B + (a)",
             "# spread(b): largest relative deviation of a round's median of (b) from the median of all its calls",
             f"{'B':>4s} {'(a) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} {'steps/s':>10s} | {'(b) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} "
             f"{'steps/s':>10s} | {'(a)/(b)':>8s} {'spread(b)':>9s} | {'(w) us/call':>12s} {'p10':>8s} {'p90':>8s} {'(w)-(a)':>8s} {'(w)/(b)':>8s}"]
    print("\n".join(lines), flush=True)
    names = ("-", "-")
    for B in [int(x) for x in args.sizes.split(",")]:
        out, spread, names = measure(B, args.steps, args.warmup, args.rounds, legs)
        a, b, w = out.get("batch", []), out.get("loop", []), out.get("adapt", [])

        def cols(v):
            if not v:
                return f"{'-':>12s} {'-':>8s} {'-':>8s} {'-':>8s} {'-':>10s}"
            q = statistics.quantiles(v, n=10)
            m = statistics.median(v)
            return f"{m:12.2f} {q[0]:8.2f} {q[-1]:8.2f} {m / B:8.2f} {B / m * 1e6:10.0f}"

        def ratio(x, y):
            return f"{statistics.median(x) / statistics.median(y):8.3f}" if x and y else f"{'-':>8s}"
        if w:
            q = statistics.quantiles(w, n=10)
            wcols = f"{statistics.median(w):12.2f} {q[0]:8.2f} {q[-1]:8.2f} " + (f"{statistics.median(w) - statistics.median(a):8.2f}" if a else f"{'-':>8s}")
        else:
            wcols = f"{'-':>12s} {'-':>8s} {'-':>8s} {'-':>8s}"
        line = f"{B:4d} {cols(a)} | {cols(b)} | {ratio(a, b)} {(f'{spread:9.3f}' if spread is not None else '-'):>9s} | {wcols} {ratio(w, b)}"
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# kernel of (a): {names[0]}    kernel of (b): {names[1]}")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
