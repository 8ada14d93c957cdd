#!/usr/bin/env python3
"""Cost per closed-loop step of B independent MPPI controllers, per problem BASELINE cfg2 (MPPI, N 1024 / H 50, CartPole ODE) with the
on-device sampler, three ways:

  (a) closed_loop.run(S0, K) / K          the plant integrated on the device between the controller launches, one synchronisation per run
  (b) step + a NumPy plant on the host    what a batch offered before: the arithmetic of bench.py's plant_step, vectorised over the B rows
  (c) step + closed_loop.plant_step       the loop that (a) is bit for bit, every step a round trip

The legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes).  Each round times K closed-loop steps of a leg as a whole with the host clock and divides by K; the figures are the median, the
lowest and the highest round.  The band of (b), (highest - lowest) / 2, stands beside them: (a) is called faster only where its median
lies below (b)'s by more than that band.

    python tools/bench_batch_run.py --out profiles/r20_batch_run.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkMppiBatch   # noqa: E402

CFG2 = dict(num_rollouts=1024, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=1)

# the host plant of leg (b): bench.py's plant_step (double-precision cart-pole Euler step, default parameters), over B rows at once
_G, _MC, _MP, _L, _UMAX, _MF, _JF = 9.81, 0.230, 0.087, 0.1975, 2.62, 4.77, 2.5e-4
_INV_MT = 1.0 / (_MC + _MP)
_KML, _KJF, _K43L, _KMM = _MP * _L, _JF / (_MP * _L), _L * (4.0 / 3.0), _MP * _L * _INV_MT


def host_plant(s, u, dt=0.02):
    x, v, th, om = (s[:, i].astype(np.float64) for i in range(4))
    sn, cs = np.sin(th), np.cos(th)
    tmp = (_UMAX * u[:, 0].astype(np.float64) + _KML * om * om * sn - _MF * v) * _INV_MT
    thdd = (_G * sn - cs * tmp - _KJF * om) / (_K43L - _KMM * cs * cs)
    xdd = tmp - _KMM * thdd * cs
    return np.stack([x + dt * v, v + dt * xdd, th + dt * om, om + dt * thdd], axis=1).astype(np.float32)


def measure(B, steps, warmup, rounds):
    rng = np.random.default_rng(B)
    S0 = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S0[:, 2] += 2.8
    batch = CtkMppiBatch(B, seeds=[100 + p for p in range(B)], **CFG2)
    loop = batch.closed_loop

    def leg_a(k):
        loop.run(S0, k)

    def leg_b(k):
        s = S0
        for _ in range(k):
            s = host_plant(s, batch.step(s))

    def leg_c(k):
        s = S0
        for _ in range(k):
            s = loop.plant_step(s, batch.step(s))
    legs = (leg_a, leg_b, leg_c)
    for leg in legs:
        leg(warmup)
    out = [[], [], []]
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
        sys.exit("bench_batch_run: no GPU (nothing here is measured on a CPU)")
    lines = [f"# tools/bench_batch_run.py {args.label}: per problem MPPI N 1024 / H 50 / period 1, CartPole ODE, device Philox; us per closed-loop step of B",
             f"# problems = host clock around {args.steps} steps / {args.steps}; median [lowest .. highest] of {args.rounds} alternating rounds after {args.warmup} warm-up steps",
             "# (a) closed_loop.run    (b) step + NumPy plant on the host    (c) step + closed_loop.plant_step    band = ((b) highest - (b) lowest) / 2",
             f"{'B':>4s} | {'(a) us/step':>12s} {'lowest':>8s} {'highest':>8s} | {'(b) us/step':>12s} {'lowest':>8s} {'highest':>8s} {'band':>7s} | "
             f"{'(c) us/step':>12s} {'lowest':>8s} {'highest':>8s} | {'(b)-(a)':>8s} {'(a) below (b) by more than the band':>36s}"]
    print("\n".join(lines), flush=True)
    name = ""
    for B in [int(x) for x in args.sizes.split(",")]:
        (a, b, c), name = measure(B, args.steps, args.warmup, args.rounds)
        ma, mb, mc = (statistics.median(v) for v in (a, b, c))
        band = 0.5 * (max(b) - min(b))
        line = (f"{B:4d} | {ma:12.2f} {min(a):8.2f} {max(a):8.2f} | {mb:12.2f} {min(b):8.2f} {max(b):8.2f} {band:7.2f} | "
                f"{mc:12.2f} {min(c):8.2f} {max(c):8.2f} | {mb - ma:8.2f} {'yes' if mb - ma > band else 'no':>36s}")
        lines.append(line)
        print(line, flush=True)
    lines.append(f"# controller kernel: {name}; plant kernel: ctk_batch_plant<0>")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
