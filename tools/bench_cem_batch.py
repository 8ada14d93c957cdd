#!/usr/bin/env python3
"""Throughput of B independent CEM controllers: one CtkCemBatch.step (leg a) against B CtkEngine("cem").step calls in a loop (leg b, all
an engine without the batch object offers), per problem BASELINE cfg3 (CEM, N 4096 / H 30 / K 409 / 3 iterations, CartPole ODE) or the
small population N 512 / H 30 / K 51, with the on-device sampler.

All legs run in ONE process and alternate in rounds (the machine is shared: a difference is only trusted when the legs saw the same
minutes); the figures are host-clock medians over --steps calls per leg after --warmup.  Every call is synchronous (it returns when the
result is on the host), so a host clock around it measures the whole step.  Leg (b) is the yardstick and runs TWICE per round (b1, b2,
two sets of handles): |b1 - b2| is the run-to-run band a difference has to exceed.

    python tools/bench_cem_batch.py --config cfg3 --sizes 1,2,4,8,16 --out profiles/cem_batch_cfg3.txt     # the table
    python tools/bench_cem_batch.py --config n512 --sizes 1,8,32,64
    python tools/bench_cem_batch.py --only batch --sizes 4 --steps 300                                      # one leg alone (the kernel trace's subject)
    python tools/bench_cem_batch.py --parent-lib /path/to/parent/libctk_hip.so --sizes 1                    # legs p1, p2: B handles through ANOTHER
                                                                                                            # build of the library (no regression of the handle)
On a tree without CtkCemBatch the script still runs leg (b): the same command gives the parent commit's figure."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine, _capi   # noqa: E402
try:
    from control_toolkit_amd import CtkCemBatch   # noqa: E402
except ImportError:                                 # a tree from before the batch object: leg (b) only
    CtkCemBatch = None

CONFIGS = {
    "cfg3": dict(num_rollouts=4096, mpc_horizon=30, dt=0.02, cem_outer_it=3, cem_best_k=409, cem_initial_action_stdev=0.5, cem_stdev_min=0.01),
    "n512": dict(num_rollouts=512, mpc_horizon=30, dt=0.02, cem_outer_it=3, cem_best_k=51, cem_initial_action_stdev=0.5, cem_stdev_min=0.01),
}
LEGS = ("a", "b1", "b2", "p1", "p2")


def bind_other_build(path):
    """another build of the library, bound like the product library except that symbols it does not export are left out (an older
    build has fewer); the handle entry points the legs p1 / p2 need must be there"""
    import torch  # noqa: F401  (one HIP runtime per process: control_toolkit_amd._capi.load_library)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    for need in ("ctk_create", "ctk_step", "ctk_destroy", "ctk_dominant_kernel"):
        if not hasattr(lib, need):
            sys.exit(f"bench_cem_batch: {path} does not export {need}")
    return lib


def engines_on(lib, cfg, seeds):
    """CtkEngine("cem") handles whose calls go to `lib` (None: the product library; the binding is the same, only the library differs)"""
    if lib is None:
        return [CtkEngine("cem", "ODE", seed=s, **cfg) for s in seeds]
    product = _capi.environment_library
    _capi.environment_library = lambda name: (lib, _capi.ENVIRONMENTS[name])
    try:
        return [CtkEngine("cem", "ODE", seed=s, **cfg) for s in seeds]
    finally:
        _capi.environment_library = product


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def measure(cfg, B, steps, warmup, rounds, legs, parent):
    rng = np.random.default_rng(B)
    S = rng.uniform(-0.3, 0.3, (B, 4)).astype(np.float32)
    S[:, 2] += 2.8
    seeds = [100 + p for p in range(B)]
    rows = [S[p] for p in range(B)]
    batch = CtkCemBatch(B, seeds=seeds, **cfg) if "a" in legs else None
    sets = {k: engines_on(parent if k[0] == "p" else None, cfg, seeds) for k in ("b1", "b2", "p1", "p2") if k in legs}

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
    ap.add_argument("--config", choices=sorted(CONFIGS), default="cfg3")
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", choices=["batch", "loop"], default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of libctk_hip.so for the legs p1 / p2 (B handles through it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cem_batch: no GPU (nothing here is measured on a CPU)")
    legs = {"a", "b1", "b2"} if args.only is None else ({"a"} if args.only == "batch" else {"b1"})
    parent = bind_other_build(args.parent_lib) if args.parent_lib else None
    if parent is not None:
        legs |= {"p1", "p2"}
    if CtkCemBatch is None:
        legs.discard("a")
        if not legs:
            sys.exit("bench_cem_batch: this tree has no CtkCemBatch")
    cfg = CONFIGS[args.config]
    lines = [f"# tools/bench_cem_batch.py {args.label}: per problem CEM N {cfg['num_rollouts']} / H {cfg['mpc_horizon']} / K {cfg['cem_best_k']} / "
             f"{cfg['cem_outer_it']} iterations, CartPole ODE, device Philox; host-clock medians in us per call over {args.steps} calls per leg "
             f"({args.rounds} alternating rounds) after {args.warmup} warm-up calls",
             "# (a) one CtkCemBatch.step of B problems   (b1), (b2) B CtkEngine('cem').step calls in a loop, twice: |b1 - b2| is the run-to-run band",
             "# (p1), (p2) the same loop through the other build of the library (--parent-lib), twice",
             f"{'B':>4s} {'(a)':>10s} {'a/prob':>8s} {'(b1)':>10s} {'(b2)':>10s} {'b1/prob':>8s} {'band b':>8s} {'(a)/(b1)':>9s} {'(a)-(b1)':>10s} {'(p1)':>10s} {'(p2)':>10s} {'band p':>8s} {'(b1)-(p1)':>10s}"]
    print("\n".join(lines), flush=True)
    names = {}
    for B in [int(x) for x in args.sizes.split(",")]:
        out, names = measure(cfg, B, args.steps, args.warmup, args.rounds, legs, parent)
        med = {k: statistics.median(v) for k, v in out.items() if v}

        def col(k, w=10, div=1):
            return f"{med[k] / div:{w}.2f}" if k in med else f"{'-':>{w}s}"

        def diff(x, y, w=10, absolute=False):
            if x not in med or y not in med:
                return f"{'-':>{w}s}"
            d = med[x] - med[y]
            return f"{abs(d) if absolute else d:{w}.2f}"
        ratio = f"{med['a'] / med['b1']:9.3f}" if "a" in med and "b1" in med else f"{'-':>9s}"
        line = (f"{B:4d} {col('a')} {col('a', 8, B)} {col('b1')} {col('b2')} {col('b1', 8, B)} {diff('b1', 'b2', 8, True)} {ratio} {diff('a', 'b1')} "
                f"{col('p1')} {col('p2')} {diff('p1', 'p2', 8, True)} {diff('b1', 'p1')}")
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
