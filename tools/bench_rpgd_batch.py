#!/usr/bin/env python3
"""Throughput of B independent RPGD controllers: one CtkRpgdBatch.step (leg a) against B CtkEngine("rpgd", generic_kernels=True).step
calls in a loop (leg b, all an engine without the batch object offers; the template handle the batch's contract refers to), per problem
N 32 / H 50 / period 10 / 20 Adam iterations / keep 8, with the on-device sampler.  --env selects CartPole (template kernels), Quad2D or
Hover.

All legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes); the figures are host-clock medians over --steps calls per leg after --warmup.  Every call is synchronous (it returns when the
result is on the host), so a host clock around it measures the whole step.  Leg (b) is the yardstick and runs TWICE per round (b1, b2,
two sets of handles): |b1 - b2| is the run-to-run band a difference has to exceed.

    python tools/bench_rpgd_batch.py --sizes 1,2,4,8,16,32,64,128,256 --out profiles/rpgd_batch.txt       # the table
    python tools/bench_rpgd_batch.py --env Hover --sizes 1,16,256
    python tools/bench_rpgd_batch.py --only batch --sizes 16 --steps 300                                   # one leg alone (the kernel trace's subject)
On a tree without CtkRpgdBatch the script still runs leg (b): the same command gives the parent commit's figure."""
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
    from control_toolkit_amd import CtkRpgdBatch   # noqa: E402
except ImportError:                                 # a tree from before the batch object: leg (b) only
    CtkRpgdBatch = None

CONFIG = dict(num_rollouts=32, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=10, outer_its=20, opt_keep_k=8, resamp_per=10,
              sample_whole_control_space=1)
LEGS = ("a", "b1", "b2")


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def measure(cfg, B, steps, warmup, rounds, legs):
    rng = np.random.default_rng(B)
    batch = CtkRpgdBatch(B, seeds=[100 + p for p in range(B)], **cfg) if "a" in legs else None
    sets = {k: [CtkEngine("rpgd", "ODE", seed=100 + p, generic_kernels=True, **cfg) for p in range(B)] for k in ("b1", "b2") if k in legs}
    n_states = batch.S if batch else sets["b1"][0].S
    S = rng.uniform(-0.3, 0.3, (B, n_states)).astype(np.float32)
    if n_states == 4:
        S[:, 2] += 2.8
    rows = [S[p] for p in range(B)]
    if batch:
        batch.reset()
    for v in sets.values():
        for e in v:
            e.reset()

    def loop(engines):
        def run():
            for e, s in zip(engines, rows):
                e.step(s)
        return run
    fns = {k: loop(v) for k, v in sets.items()}
    if batch:
        fns["a"] = lambda: batch.step(S)
    order = [k for k in LEGS if k in fns]
    for k in order:
        timed(fns[k], warmup)
    out = {k: [] for k in order}
    per = max(1, steps // rounds)
    for _ in range(rounds):                         # alternate the legs
        for k in order:
            out[k] += timed(fns[k], per)
    names = {"a": batch.dominant_kernel() if batch else None}
    for k, v in sets.items():
        names[k] = v[0].dominant_kernel()
    if batch:
        batch.close()
    for v in sets.values():
        for e in v:
            e.close()
    return out, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=["CartPole", "Quad2D", "Hover"], default="CartPole")
    ap.add_argument("--sizes", default="1,2,4,8,16,32,64,128,256")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", choices=["batch", "loop"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rpgd_batch: no GPU (nothing here is measured on a CPU)")
    legs = {"a", "b1", "b2"} if args.only is None else ({"a"} if args.only == "batch" else {"b1"})
    if CtkRpgdBatch is None:
        legs.discard("a")
        if not legs:
            sys.exit("bench_rpgd_batch: this tree has no CtkRpgdBatch")
    cfg = dict(CONFIG, environment=args.env)
    lines = [f"# tools/bench_rpgd_batch.py {args.label}: per problem RPGD N {cfg['num_rollouts']} / H {cfg['mpc_horizon']} / period "
             f"{cfg['period_interpolation_inducing_points']} / {cfg['outer_its']} iterations / keep {cfg['opt_keep_k']}, {args.env} ODE (template kernels), "
             f"device Philox; host-clock medians in us per call over {args.steps} calls per leg ({args.rounds} alternating rounds) after "
             f"{args.warmup} warm-up calls",
             "# (a) one CtkRpgdBatch.step of B problems   (b1), (b2) B CtkEngine('rpgd', generic_kernels=True).step calls in a loop, twice: "
             "|b1 - b2| is the run-to-run band",
             f"{'B':>4s} {'(a)':>10s} {'a/prob':>8s} {'(b1)':>10s} {'(b2)':>10s} {'b1/prob':>8s} {'band b':>8s} {'(a)/(b1)':>9s} {'(a)-(b1)':>10s}"]
    print("\n".join(lines), flush=True)
    names = {}
    for B in [int(x) for x in args.sizes.split(",")]:
        out, names = measure(cfg, B, args.steps, args.warmup, args.rounds, legs)
        med = {k: statistics.median(v) for k, v in out.items() if v}

        def col(k, w=10, div=1):
            return f"{med[k] / div:{w}.2f}" if k in med else f"{'-':>{w}s}"

        def diff(x, y, w=10, absolute=False):
            if x not in med or y not in med:
                return f"{'-':>{w}s}"
            d = med[x] - med[y]
            return f"{abs(d) if absolute else d:{w}.2f}"
        ratio = f"{med['a'] / med['b1']:9.3f}" if "a" in med and "b1" in med else f"{'-':>9s}"
        line = f"{B:4d} {col('a')} {col('a', 8, B)} {col('b1')} {col('b2')} {col('b1', 8, B)} {diff('b1', 'b2', 8, True)} {ratio} {diff('a', 'b1')}"
        lines.append(line)
        print(line, flush=True)
    lines.append("# kernels: " + ", ".join(f"({k}) {v}" for k, v in names.items() if v))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
