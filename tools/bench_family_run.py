#!/usr/bin/env python3
"""Cost per closed-loop step of B independent CEM or RPGD controllers on CartPole with the on-device sampler, the loop on the device
against the host loop a batch offered before.  Three configurations: CEM at BASELINE cfg3 (N 4096 / H 30 / K 409 / 3 iterations, B 4), CEM
at N 512 (H 30 / K 51 / 3 iterations, B 32) and RPGD at N 32 / H 50 / period 10 / 20 Adam iterations / keep 8 (B 16).  Four legs:

  (a) BatchClosedLoop(batch).run(S0, K) / K            the plant integrated on the device between the controller launches
  (b) step + a NumPy plant on the host                  what these batches offered before: bench.py's plant arithmetic over the B rows
  (e) BatchClosedLoop(batch).episodes(S0, K) / K        the noisy plant with the realised cost, sigmas on every problem
  (c) step + NumPy plant + rng.normal + NumPy cost      what a user did before for the same: every step a round trip

The legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes).  Each round times K closed-loop steps of a leg as a whole with the host clock and divides by K; the figures are the median, the
lowest and the highest round.  The band is half the range of the host-loop leg: the device loop counts as a gain only where (b) - (a)
exceeds the band of (b), and (c) - (e) the band of (c).  The table says so either way; the exit status is 0 whatever it says.

    python tools/bench_family_run.py --out profiles/r23_family_closed_loop.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from control_toolkit_amd import BatchClosedLoop, CtkCemBatch, CtkRpgdBatch   # noqa: E402
from bench_batch_run import host_plant                  # noqa: E402
from bench_batch_episodes import SIGMA_W, SIGMA_V, host_cost   # noqa: E402
from bench_cem_batch import CONFIGS as CEM_CONFIGS      # noqa: E402
from bench_rpgd_batch import CONFIG as RPGD_CONFIG      # noqa: E402

# name -> (class, keywords, B, what the table calls it)
CASES = {
    "cem_cfg3": (CtkCemBatch, CEM_CONFIGS["cfg3"], 4, "CEM N 4096 / H 30 / K 409 / 3 iterations (BASELINE cfg3)"),
    "cem_n512": (CtkCemBatch, CEM_CONFIGS["n512"], 32, "CEM N 512 / H 30 / K 51 / 3 iterations"),
    "rpgd": (CtkRpgdBatch, RPGD_CONFIG, 16, "RPGD N 32 / H 50 / period 10 / 20 Adam iterations / keep 8"),
}


def measure(case, steps, warmup, rounds):
    cls, cfg, B, _ = CASES[case]
    rng = np.random.default_rng(B)
    S0 = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S0[:, 2] += 2.8
    U0 = np.zeros((B, 1), np.float32)
    batch = cls(B, seeds=[100 + p for p in range(B)], **cfg)
    if cls is CtkRpgdBatch:
        batch.reset()
    loop = BatchClosedLoop(batch)
    noise = np.random.default_rng(1000 + B)

    def leg_a(k):
        loop.run(S0, k, u_prev=U0)

    def leg_b(k):
        s = S0
        for i in range(k):
            u = batch.step(s, u_prev=U0 if i == 0 else None)
            s = host_plant(s, u)

    def leg_e(k):
        loop.set_noise(process=SIGMA_W, measurement=SIGMA_V)
        loop.episodes(S0, k, u_prev=U0)

    def leg_c(k):
        s, y, up = S0, S0, U0
        costs = np.empty((B, k), np.float32)
        for i in range(k):
            u = batch.step(y, u_prev=up if i == 0 else None)
            costs[:, i] = host_cost(s, u, up)
            n = noise.normal(size=(2, B, 4)).astype(np.float32)
            s = host_plant(s, u) + SIGMA_W * n[0]
            y = s + SIGMA_V * n[1]
            up = u
    legs = (leg_a, leg_b, leg_e, leg_c)
    for leg in legs:
        leg(warmup)
    out = [[] for _ in legs]
    for _ in range(rounds):                         # alternate the legs
        for leg, v in zip(legs, out):
            t0 = time.perf_counter()
            leg(steps)
            v.append((time.perf_counter() - t0) * 1e6 / steps)
    name = batch.dominant_kernel()
    batch.close()
    return out, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=200, help="closed-loop steps per leg and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_family_run: no GPU (nothing here is measured on a CPU)")
    col = lambda tag: f"{tag + ' us/step':>13s} {'lowest':>8s} {'highest':>8s}"                # noqa: E731
    lines = [f"# tools/bench_family_run.py {args.label}: CartPole ODE, device Philox; us per closed-loop step of B problems = host clock around {args.steps}",
             f"# steps / {args.steps}; median [lowest .. highest] of {args.rounds} alternating rounds after {args.warmup} warm-up steps",
             f"# (a) BatchClosedLoop.run    (b) step + NumPy plant    (e) BatchClosedLoop.episodes, sigma_w {SIGMA_W} / sigma_v {SIGMA_V} on every problem",
             "# (c) step + NumPy plant + rng.normal + NumPy stage cost    band = (highest - lowest) / 2 of the host-loop leg named",
             f"{'case':>9s} {'B':>3s} | {col('(a)')} | {col('(b)')} {'band(b)':>8s} | {col('(e)')} | {col('(c)')} {'band(c)':>8s} | "
             f"{'(b)-(a)':>8s} {'gain':>5s} {'(c)-(e)':>8s} {'gain':>5s}"]
    print("\n".join(lines), flush=True)
    notes = []
    for case in args.cases.split(","):
        (a, b, e, c), name = measure(case, args.steps, args.warmup, args.rounds)
        ma, mb, me, mc = (statistics.median(v) for v in (a, b, e, c))
        band_b, band_c = 0.5 * (max(b) - min(b)), 0.5 * (max(c) - min(c))
        line = (f"{case:>9s} {CASES[case][2]:3d} | {ma:13.2f} {min(a):8.2f} {max(a):8.2f} | {mb:13.2f} {min(b):8.2f} {max(b):8.2f} {band_b:8.2f} | "
                f"{me:13.2f} {min(e):8.2f} {max(e):8.2f} | {mc:13.2f} {min(c):8.2f} {max(c):8.2f} {band_c:8.2f} | "
                f"{mb - ma:8.2f} {'yes' if mb - ma > band_b else 'no':>5s} {mc - me:8.2f} {'yes' if mc - me > band_c else 'no':>5s}")
        lines.append(line)
        notes.append(f"# {case}: {CASES[case][3]}, B {CASES[case][2]}; controller kernel {name}")
        print(line, flush=True)
    lines += notes
    lines.append("# gain: the host-loop leg's median lies above the device loop's by more than the host-loop leg's band")
    print("\n".join(notes))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
