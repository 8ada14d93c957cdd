#!/usr/bin/env python3
"""Cost per closed-loop step of B independent MPPI controllers against NOISY plants with the realised cost, per problem BASELINE cfg2
(MPPI, N 1024 / H 50, CartPole ODE) with the on-device sampler, four ways:

  (r)  closed_loop.run(S0, K) / K                    the deterministic run: existing code, the yardstick
  (a0) closed_loop.episodes(S0, K) / K               all sigmas 0: the price of the cost, the two further traces and the other operands
  (a)  closed_loop.episodes(S0, K) / K               process and measurement noise on every problem: plus the draws
  (c)  step(Y) + NumPy plant + rng.normal + NumPy cost   what a user did before: bench.py's plant arithmetic, vectorised over the B rows,
                                                     two normal draws per state and a hand-written stage cost, every step a round trip

The legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes).  Each round times K closed-loop steps of a leg as a whole with the host clock and divides by K; the figures are the median, the
lowest and the highest round.  The band of a leg is (highest - lowest) / 2: (a) is called faster than (c) only where its median lies
below (c)'s by more than (c)'s band; (a) - (r) and (a0) - (r) stand beside the band of (r), without a threshold.

    python tools/bench_batch_episodes.py --out profiles/r21_batch_episodes.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from control_toolkit_amd import CtkMppiBatch   # noqa: E402
from bench_batch_run import CFG2, host_plant   # noqa: E402

SIGMA_W, SIGMA_V = 0.01, 0.02
# the host cost of leg (c): CartPole's stage cost with the default weights (distance, potential energy, kinetic energy of the pole, input,
# input change), vectorised over the B rows
_DD, _EP, _EKP, _CC, _CCRC, _XS, _TARGET = 600.0, 20000.0, 80.0, 1.0, 1.0, 0.198, 0.0


def host_cost(s, u, up):
    dxn = (s[:, 0] - _TARGET) / _XS
    omc = 1.0 - np.cos(s[:, 2])
    du = u[:, 0] - up[:, 0]
    return (_DD * dxn * dxn + 0.25 * _EP * omc * omc + _EKP * s[:, 3] * s[:, 3] + _CC * u[:, 0] * u[:, 0] + _CCRC * du * du).astype(np.float32)


def measure(B, steps, warmup, rounds):
    rng = np.random.default_rng(B)
    S0 = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S0[:, 2] += 2.8
    U0 = np.zeros((B, 1), np.float32)
    batch = CtkMppiBatch(B, seeds=[100 + p for p in range(B)], **CFG2)
    loop = batch.closed_loop
    noise = np.random.default_rng(1000 + B)

    def leg_r(k):
        loop.run(S0, k, u_prev=U0)

    def leg_a0(k):
        loop.clear_noise()
        loop.episodes(S0, k, u_prev=U0)

    def leg_a(k):
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
    legs = (leg_r, leg_a0, leg_a, leg_c)
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
    ap.add_argument("--sizes", default="1,16,64,128")
    ap.add_argument("--steps", type=int, default=500, help="closed-loop steps per leg and round")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_batch_episodes: no GPU (nothing here is measured on a CPU)")
    col = lambda tag: f"{tag + ' us/step':>13s} {'lowest':>8s} {'highest':>8s}"                # noqa: E731
    lines = [f"# tools/bench_batch_episodes.py {args.label}: per problem MPPI N 1024 / H 50 / period 1, CartPole ODE, device Philox; us per closed-loop step of B",
             f"# problems = host clock around {args.steps} steps / {args.steps}; median [lowest .. highest] of {args.rounds} alternating rounds after {args.warmup} warm-up steps",
             f"# (r) closed_loop.run    (a0) closed_loop.episodes, all sigmas 0    (a) closed_loop.episodes, sigma_w {SIGMA_W} / sigma_v {SIGMA_V} on every problem",
             "# (c) step(Y) + NumPy plant + rng.normal + NumPy stage cost on the host    band = (highest - lowest) / 2 of the leg named",
             f"{'B':>4s} | {col('(r)')} {'band(r)':>8s} | {col('(a0)')} | {col('(a)')} | {col('(c)')} {'band(c)':>8s} | "
             f"{'(a0)-(r)':>9s} {'(a)-(r)':>8s} {'(c)-(a)':>8s} {'(a) below (c) by more than band(c)':>35s}"]
    print("\n".join(lines), flush=True)
    name, ok = "", True
    for B in [int(x) for x in args.sizes.split(",")]:
        (r, a0, a, c), name = measure(B, args.steps, args.warmup, args.rounds)
        mr, m0, ma, mc = (statistics.median(v) for v in (r, a0, a, c))
        band_r, band_c = 0.5 * (max(r) - min(r)), 0.5 * (max(c) - min(c))
        below = mc - ma > band_c
        ok = ok and below
        line = (f"{B:4d} | {mr:13.2f} {min(r):8.2f} {max(r):8.2f} {band_r:8.2f} | {m0:13.2f} {min(a0):8.2f} {max(a0):8.2f} | "
                f"{ma:13.2f} {min(a):8.2f} {max(a):8.2f} | {mc:13.2f} {min(c):8.2f} {max(c):8.2f} {band_c:8.2f} | "
                f"{m0 - mr:9.2f} {ma - mr:8.2f} {mc - ma:8.2f} {'yes' if below else 'no':>35s}")
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# controller kernel: {name}; plant kernels: ctk_batch_plant<0> (r), ctk_batch_plant_noisy<0> (a0, a)")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
