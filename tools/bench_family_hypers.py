#!/usr/bin/env python3
"""What a sweep of a CEM or RPGD hyper-parameter costs: B controllers (CartPole ODE, device Philox) of
  cem    BASELINE cfg3 at N 512 (H 30, 3 outer iterations, cem_best_k 51)       rpgd   N 32 / H 50 / period 10, 20 Adam iterations a step
stepped as

  (a) one batch.step, the shared form (ctk_cem_batch / ctk_g_rpgd_batch)          (d) ... with a new value for every problem before every step
  (b) ... after set_problem_params, the _pp form                                      (cem_stdev_min / learning_rate; it travels with the records)
  (b') a second batch like (b): the spread between two equal legs                 (e) B batches of ONE problem each: a sweep without this form
  (c) ... after FamilyHypers.set_problem_hypers with every problem at the          (f) B CtkEngine handles in a loop
      defaults, the _hp form

All legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes, and only beyond the spread of (b) against (b')); the figures are host-clock medians over --steps calls per leg after --warmup.
Every call is synchronous, so a host clock around it measures the whole step.

    python tools/bench_family_hypers.py --out profiles/r32_family_hypers.txt

On a tree without the per-problem hyper-parameters the script runs (a), (b), (b'), (e) and (f): the same command gives the parent's figures."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import control_toolkit_amd                                                  # noqa: E402
from control_toolkit_amd import CtkCemBatch, CtkEngine, CtkRpgdBatch        # noqa: E402

FamilyHypers = getattr(control_toolkit_amd, "FamilyHypers", None)          # None: a tree from before the per-problem hyper-parameters
FAMILIES = {
    "cem": dict(cls=CtkCemBatch, opt="cem", sizes="4,32", engine={}, default=("cem_stdev_min", 0.01), sweep=("cem_stdev_min", 0.005, 0.05),
                cfg=dict(num_rollouts=512, mpc_horizon=30, dt=0.02, cem_outer_it=3, cem_best_k=51, cem_initial_action_stdev=0.5, cem_stdev_min=0.01)),
    "rpgd": dict(cls=CtkRpgdBatch, opt="rpgd", sizes="16,64", engine=dict(generic_kernels=True), default=("learning_rate", 0.05), sweep=("learning_rate", 0.01, 0.1),
                 cfg=dict(num_rollouts=32, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=10, outer_its=20, resamp_per=10, opt_keep_k=8,
                          learning_rate=0.05)),
}
LEGS = ("a", "b", "b'", "c", "d", "e", "f")


def measure(family, B, steps, warmup, rounds, legs):
    F = FAMILIES[family]
    rng = np.random.default_rng(B)
    S = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S[:, 2] += 2.8
    seeds = [100 + p for p in range(B)]
    made, calls, named = [], {}, {}                 # everything to close; leg -> its call; leg -> the batch whose kernel the table names

    def batch(n=B, first=0):
        b = F["cls"](n, seeds=seeds[first:first + n], **F["cfg"])
        if family == "rpgd":
            b.reset()
        made.append(b)
        return b

    if "a" in legs:
        a = batch()
        calls["a"], named["a"] = (lambda: a.step(S)), a
    for leg in ("b", "b'"):
        if leg in legs:
            b = batch()
            b.set_problem_params("target_position", np.zeros(B, np.float32))        # the default, per problem
            calls[leg], named[leg] = (lambda b=b: b.step(S)), b
    if "c" in legs:
        c = batch()
        FamilyHypers(c).set_problem_hypers(F["default"][0], np.full(B, F["default"][1], np.float32))   # the default, per problem
        calls["c"], named["c"] = (lambda: c.step(S)), c
    if "d" in legs:
        d = batch()
        view = FamilyHypers(d)
        name, lo, hi = F["sweep"]
        vals = [np.linspace(lo, hi, B).astype(np.float32), np.linspace(hi, lo, B).astype(np.float32)]
        turn = [0]

        def leg_d():
            turn[0] ^= 1
            view.set_problem_hypers(name, vals[turn[0]])
            d.step(S)
        calls["d"], named["d"] = leg_d, d
    if "e" in legs:
        ones = [batch(1, p) for p in range(B)]
        rows = [S[p:p + 1] for p in range(B)]

        def leg_e():
            for o, s in zip(ones, rows):
                o.step(s)
        calls["e"] = leg_e
    if "f" in legs:
        engines = [CtkEngine(F["opt"], "ODE", seed=seeds[p], **F["engine"], **F["cfg"]) for p in range(B)]
        if family == "rpgd":
            for e in engines:
                e.reset()
        made.extend(engines)

        def leg_f():
            for e, p in zip(engines, range(B)):
                e.step(S[p])
        calls["f"] = leg_f

    def timed(fn, n):
        out = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e6)
        return out

    for fn in calls.values():
        timed(fn, warmup)
    got = {leg: [] for leg in calls}
    per = max(1, steps // rounds)
    for _ in range(rounds):                         # alternate the legs
        for leg, fn in calls.items():
            got[leg] += timed(fn, per)
    kernels = {leg: x.dominant_kernel() for leg, x in named.items()}
    for x in made:
        x.close()
    return got, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="cem,rpgd")
    ap.add_argument("--sizes", default=None, help="B values for every family (default: 4,32 for cem, 16,64 for rpgd)")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    legs = [x for x in args.legs.split(",") if x in LEGS]
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_family_hypers: no GPU (nothing here is measured on a CPU)")
    if FamilyHypers is None:
        legs = [x for x in legs if x not in ("c", "d")]
    lines = [f"# tools/bench_family_hypers.py {args.label}: CartPole ODE, device Philox; cem: cfg3 at N 512; rpgd: N 32 / H 50 / 20 iterations; host-clock "
             f"medians over {args.steps} calls per leg ({args.rounds} alternating rounds) after {args.warmup} warm-up calls",
             "# (a) shared form  (b) _pp form  (b') _pp form again: the spread  (c) _hp form, defaults  (d) _hp form, a new value per problem before "
             "every step  (e) B batches of one problem  (f) B handles",
             f"{'family':>6s} {'B':>4s} {'leg':>4s} {'us/call':>10s} {'p10':>9s} {'p90':>9s} {'us/prob':>9s} {'vs (b)':>8s}  kernel"]
    print("\n".join(lines), flush=True)
    for family in [f for f in args.families.split(",") if f in FAMILIES]:
        for B in [int(x) for x in (args.sizes or FAMILIES[family]["sizes"]).split(",")]:
            got, kernels = measure(family, B, args.steps, args.warmup, args.rounds, legs)
            base = statistics.median(got["b"]) if "b" in got else None
            for leg, v in got.items():
                q = statistics.quantiles(v, n=10)
                m = statistics.median(v)
                line = (f"{family:>6s} {B:4d} {leg:>4s} {m:10.2f} {q[0]:9.2f} {q[-1]:9.2f} {m / B:9.2f} {(f'{m / base:8.3f}' if base else '       -')}  "
                        f"{kernels.get(leg, '')}")
                lines.append(line)
                print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
