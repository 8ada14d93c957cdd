#!/usr/bin/env python3
"""Cost of rolling caller-supplied plans out for B problems, per problem BASELINE cfg2 (MPPI, N 1024 / H 50, CartPole), trajectories
returned:

  (a)  batch.rollouts.rollout(S, None)              every problem's own plan, read on the device: one transfer, one launch, one copy back
  (b1) batch.rollouts.rollout(S, plans), M = 1      plans from the host
  (b64) ... M = 64
  (c1) B x CtkEngine.rollout(S[p], plans[p]), M = 1  one prepared engine per problem: what a batch's user had before.  THE REFERENCE LEG
  (c64) ... M = 64
and for the MLP batch (the learned model against the analytic plant of its closed loop)
  (d)  rollout(S, None, model="controller")   against   rollout(S, None, model="plant")

The legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes).  Each round times `calls` calls of a leg as a whole with the host clock and divides by the count; the figures are the median,
the lowest and the highest round.  The band of a reference leg, (highest - lowest) / 2, stands beside it: a batch leg is called faster
only where its median lies below the reference leg's by more than that band.

    python tools/bench_batch_rollout.py --out profiles/r33_batch_rollout_table.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine, CtkMppiBatch, CtkMppiMlpBatch   # noqa: E402
from oracle import ctk_oracle as O   # noqa: E402  (the MLP's default weights only)

CFG2 = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1)
H = CFG2["mpc_horizon"]


def rounds_of(legs, calls, warmup, rounds):
    for leg in legs:
        for _ in range(warmup):
            leg()
    out = [[] for _ in legs]
    for _ in range(rounds):                         # alternate the legs
        for leg, v in zip(legs, out):
            t0 = time.perf_counter()
            for _ in range(calls):
                leg()
            v.append((time.perf_counter() - t0) * 1e6 / calls)
    return out


def measure(B, calls, warmup, rounds):
    rng = np.random.default_rng(B)
    S = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S[:, 2] += 2.8
    plans = {M: rng.uniform(-1, 1, (B, M, H, 1)).astype(np.float32) for M in (1, 64)}
    batch = CtkMppiBatch(B, seeds=[100 + p for p in range(B)], **CFG2)
    batch.set_problem_params("m_pole", [0.087 * (0.8 + 0.5 * p / max(1, B - 1)) for p in range(B)])
    batch.step(S)
    engines = [CtkEngine("mppi", "ODE", seed=100 + p, **CFG2) for p in range(B)]
    for p, e in enumerate(engines):
        e.set_param("m_pole", batch.get_problem_param("m_pole", p))
    view = batch.rollouts

    def loop(M):
        for p, e in enumerate(engines):
            e.rollout(S[p], plans[M][p])
    legs = (lambda: view.rollout(S, None), lambda: view.rollout(S, plans[1]), lambda: view.rollout(S, plans[64]), lambda: loop(1), lambda: loop(64))
    out = rounds_of(legs, calls, warmup, rounds)
    batch.close()
    for e in engines:
        e.close()
    return out


def measure_mlp(B, calls, warmup, rounds):
    rng = np.random.default_rng(B)
    S = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S[:, 2] += 2.8
    batch = CtkMppiMlpBatch(B, seeds=[100 + p for p in range(B)], **CFG2)
    batch.set_problem_weights(np.stack([O.mlp_default_weights(100 + p) for p in range(B)]))
    batch.step(S)
    view = batch.rollouts
    out = rounds_of((lambda: view.rollout(S, None), lambda: view.rollout(S, None, model="plant")), calls, warmup, rounds)
    batch.close()
    return out


def cell(v):
    return f"{statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_batch_rollout: no GPU (nothing here is measured on a CPU)")
    head = f"{'median':>10s} {'lowest':>8s} {'highest':>8s}"
    lines = [f"# tools/bench_batch_rollout.py {args.label}: per problem N 1024 / H 50, CartPole, trajectories returned; us per call for ALL B problems",
             f"# = host clock around {args.calls} calls / {args.calls}; median, lowest, highest of {args.rounds} alternating rounds after {args.warmup} warm-up calls",
             "# (a) own plans    (b1)/(b64) M plans per problem from the host    (c1)/(c64) the loop of B CtkEngine.rollout calls, the reference leg;",
             "# band = ((c) highest - (c) lowest) / 2; below: the batch leg's median lies under the reference leg's by more than its band",
             f"{'B':>4s} | (a) {head} | (b1) {head} | (b64) {head} | (c1) {head} {'band':>7s} | (c64) {head} {'band':>7s} | (a),(b1) below (c1)  (b64) below (c64)"]
    print("\n".join(lines), flush=True)
    for B in [int(x) for x in args.sizes.split(",")]:
        a, b1, b64, c1, c64 = measure(B, args.calls, args.warmup, args.rounds)
        band1, band64 = 0.5 * (max(c1) - min(c1)), 0.5 * (max(c64) - min(c64))
        med = statistics.median
        ok1 = med(c1) - med(a) > band1 and med(c1) - med(b1) > band1
        ok64 = med(c64) - med(b64) > band64
        line = (f"{B:4d} |     {cell(a)} |      {cell(b1)} |       {cell(b64)} |      {cell(c1)} {band1:7.1f} |       {cell(c64)} {band64:7.1f} | "
                f"{'yes' if ok1 else 'no':>19s}  {'yes' if ok64 else 'no':>17s}")
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# (d) the MLP batch, own plans: model=controller (the network) | model=plant (the analytic plant of the closed loop)")
    lines.append(f"{'B':>4s} | ctrl {head} | plant {head}")
    print("\n".join(lines[-2:]), flush=True)
    for B in [int(x) for x in args.sizes.split(",")]:
        dc, dp = measure_mlp(B, args.calls, args.warmup, args.rounds)
        lines.append(f"{B:4d} |      {cell(dc)} |       {cell(dp)}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
