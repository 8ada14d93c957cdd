#!/usr/bin/env python3
"""Throughput of B independent MPPI controllers with the GRU predictor: one CtkMppiGruBatch.step (leg a: one rollout launch and one
hidden-state launch for all B) against B CtkEngine("mppi", "GRU").step calls in a loop (leg b, all a tree without the batch object
offers: B rollout launches of 64 workgroups and B one-workgroup hidden-state launches) on the same library in the same process, per
problem BASELINE cfg2's size (N 1024 / H 50, period 1, CartPole) with the on-device sampler, a network and a carried hidden state per
problem.

The legs alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same minutes); the figures are
host-clock medians over --steps calls per leg after --warmup.  Every call is synchronous (it returns when u is on the host; the
hidden-state launch runs behind that on the stream, in both legs), so a host clock around it measures the whole step as a caller sees
it.  The run-to-run spread of (b) is reported beside the ratio: the largest relative deviation of a round's median of (b) from the
median of all its calls.

    python tools/bench_gru_batch.py --out profiles/r28_gru_batch.txt            # the table
    python tools/bench_gru_batch.py --only batch --sizes 4 --steps 300          # one leg alone (the kernel trace's subject)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine, CtkMppiGruBatch   # noqa: E402
from control_toolkit_amd._capi import gru_weight_count   # noqa: E402

CFG2 = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1)


def networks(B):
    """B 5-32-32-4 GRUs in the raw layout (per layer W_i, W_h, b_i, b_h, then W_o, b_o): weights N(0, 1 / fan_in), biases N(0, 0.1)"""
    out = np.empty((B, gru_weight_count(4, 1)), np.float32)
    for p in range(B):
        rng = np.random.default_rng(1000 + p)
        parts = []
        for fan_in in (5, 32):
            parts += [rng.normal(0, 1 / np.sqrt(fan_in), 96 * fan_in), rng.normal(0, 1 / np.sqrt(32), 96 * 32), rng.normal(0, 0.1, 96), rng.normal(0, 0.1, 96)]
        parts += [rng.normal(0, 1 / np.sqrt(32), 4 * 32), rng.normal(0, 0.1, 4)]
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
    if "batch" in legs:
        batch = CtkMppiGruBatch(B, seeds=seeds, **CFG2)
        batch.set_problem_weights(W)
    engines = [CtkEngine("mppi", "GRU", seed=seeds[p], **CFG2) for p in range(B)] if "loop" in legs else []
    for e, w in zip(engines, W):
        e.set_predictor_weights(w)
    rows = [S[p] for p in range(B)]

    def leg_a():
        batch.step(S)

    def leg_b():
        for e, s in zip(engines, rows):
            e.step(s)
    run = [(n, f) for n, f in (("batch", leg_a), ("loop", leg_b)) if n in legs]
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
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", choices=["batch", "loop"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gru_batch: no GPU (nothing here is measured on a CPU)")
    legs = {"batch", "loop"} if args.only is None else {args.only}
    lines = [f"# tools/bench_gru_batch.py {args.label}: per problem MPPI N 1024 / H 50 / period 1, CartPole GRU 5-32-32-4 (a network and a hidden state per "
             f"problem), device Philox; host-clock medians over {args.steps} calls per leg ({args.rounds} alternating rounds) after {args.warmup} warm-up calls",
             "# (a) one CtkMppiGruBatch.step of B problems   (b) B CtkEngine('mppi', 'GRU').step calls in a loop",
             "# spread(b): largest relative deviation of a round's median of (b) from the median of all its calls; the ratio counts where 1 - (a)/(b) > spread(b)",
             f"{'B':>4s} {'(a) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} {'steps/s':>10s} | {'(b) us/call':>12s} {'p10':>8s} {'p90':>8s} {'us/prob':>8s} "
             f"{'steps/s':>10s} | {'(a)/(b)':>8s} {'spread(b)':>9s} {'below 1 by more':>15s}"]
    print("\n".join(lines), flush=True)
    names = ("-", "-")
    for B in [int(x) for x in args.sizes.split(",")]:
        out, spread, names = measure(B, args.steps, args.warmup, args.rounds, legs)
        a, b = out.get("batch", []), out.get("loop", [])

        def cols(v):
            if not v:
                return f"{'-':>12s} {'-':>8s} {'-':>8s} {'-':>8s} {'-':>10s}"
            q = statistics.quantiles(v, n=10)
            m = statistics.median(v)
            return f"{m:12.2f} {q[0]:8.2f} {q[-1]:8.2f} {m / B:8.2f} {B / m * 1e6:10.0f}"
        if a and b:
            r = statistics.median(a) / statistics.median(b)
            verdict = f"{r:8.3f} {spread:9.3f} {('yes' if 1.0 - r > spread else 'no'):>15s}"
        else:
            verdict = f"{'-':>8s} {'-':>9s} {'-':>15s}"
        line = f"{B:4d} {cols(a)} | {cols(b)} | {verdict}"
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# kernel of (a): {names[0]} + ctk_gru_advance_batch    kernel of (b): {names[1]} + ctk_gru_advance")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
