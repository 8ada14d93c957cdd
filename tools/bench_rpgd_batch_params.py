#!/usr/bin/env python3
"""What per-problem parameters cost a CtkRpgdBatch: per problem RPGD N 32 / H 50 / period 10 / 20 Adam iterations / keep 8 (the sizes of
tools/bench_rpgd_batch.py), CartPole ODE through the template kernels, on-device sampler, B problems, one process, the legs alternating in
rounds (the machine is shared: a difference is only trusted when the legs saw the same minutes).  Host-clock medians over --steps calls
per leg after --warmup; every call is synchronous.

    (a) one batch step in the shared form                         ctk_g_rpgd_batch<0>
    (b) one batch step in the per-problem form, no parameter change between steps      ctk_g_rpgd_batch_pp<0>
    (c) set_problem_params("target_position", new[B]) followed by one step, every step
    (d) what a tree without per-problem parameters offers for (c): B template handles, each set_param + step
    (p1), (p2) with --parent-lib PATH: leg (a) through ANOTHER build of the library (the parent commit's), twice; the difference of the
        two is the run-to-run band that (a) is read against

    python tools/bench_rpgd_batch_params.py --parent-lib /path/to/parent/libctk_hip.so --out profiles/rpgd_batch_params.txt
    python tools/bench_rpgd_batch_params.py --only b --sizes 16          # one leg alone (the kernel trace's subject)"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from control_toolkit_amd import CtkEngine, CtkRpgdBatch, _capi   # noqa: E402

CONFIG = dict(num_rollouts=32, mpc_horizon=50, dt=0.02, period_interpolation_inducing_points=10, outer_its=20, opt_keep_k=8, resamp_per=10,
              sample_whole_control_space=1)
LEGS = ("a", "b", "c", "d", "p1", "p2")


def bind_other_build(path):
    """another build of the library, bound like the product library except that symbols it does not export are left out (an older
    build has fewer); the batch entry points that leg (a) needs must be there"""
    import torch  # noqa: F401  (one HIP runtime per process: control_toolkit_amd._capi.load_library)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    for need in ("ctk_rpgd_batch_create", "ctk_rpgd_batch_step", "ctk_rpgd_batch_reset", "ctk_rpgd_batch_destroy", "ctk_rpgd_batch_dominant_kernel"):
        if not hasattr(lib, need):
            sys.exit(f"bench_rpgd_batch_params: {path} does not export {need}")
    return lib


def batch_on(lib, cfg, B, seeds):
    """a CtkRpgdBatch whose calls go to `lib` (the binding is the same; only the library differs)"""
    if lib is None:
        return CtkRpgdBatch(B, seeds=seeds, **cfg)
    product = _capi.environment_library
    _capi.environment_library = lambda name: (lib, _capi.ENVIRONMENTS[name])
    try:
        return CtkRpgdBatch(B, seeds=seeds, **cfg)
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
    rows = [S[p] for p in range(B)]
    seeds = [100 + p for p in range(B)]
    targets = [rng.uniform(-0.15, 0.15, B).astype(np.float32) for _ in range(16)]       # drawn ahead: the legs time calls, not the generator
    lists = [[float(v) for v in t] for t in targets]
    shared = batch_on(None, cfg, B, seeds) if "a" in legs else None
    own = batch_on(None, cfg, B, seeds) if "b" in legs else None
    moving = batch_on(None, cfg, B, seeds) if "c" in legs else None
    engines = [CtkEngine("rpgd", "ODE", seed=seeds[p], generic_kernels=True, **cfg) for p in range(B)] if "d" in legs else []
    par = {k: batch_on(parent, cfg, B, seeds) for k in ("p1", "p2") if k in legs}
    for o in [shared, own, moving, *par.values(), *engines]:
        if o:
            o.reset()
    if own:
        own.set_problem_params("target_position", targets[0])
    count = {"c": 0, "d": 0}

    def leg_c():
        count["c"] += 1
        moving.set_problem_params("target_position", targets[count["c"] % 16])
        moving.step(S)

    def leg_d():
        count["d"] += 1
        t = lists[count["d"] % 16]
        for e, s, v in zip(engines, rows, t):
            e.set_param("target_position", v)
            e.step(s)
    fns = {}
    if shared:
        fns["a"] = lambda: shared.step(S)
    if own:
        fns["b"] = lambda: own.step(S)
    if moving:
        fns["c"] = leg_c
    if engines:
        fns["d"] = leg_d
    for k, obj in par.items():
        fns[k] = (lambda o: lambda: o.step(S))(obj)
    for fn in fns.values():
        timed(fn, warmup)
    out = {k: [] for k in fns}
    per = max(1, steps // rounds)
    for _ in range(rounds):                         # alternate the legs
        for k, fn in fns.items():
            out[k] += timed(fn, per)
    names = {k: o.dominant_kernel() for k, o in (("a", shared), ("b", own), ("c", moving)) if o}
    names.update({k: o.dominant_kernel() for k, o in par.items()})
    for o in [shared, own, moving, *par.values(), *engines]:
        if o:
            o.close()
    return out, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256", help="B values")
    ap.add_argument("--steps", type=int, default=300, help="timed calls per leg and size (>= 200 for a reported figure)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", default=None, help="comma-separated legs out of a,b,c,d,p1,p2")
    ap.add_argument("--parent-lib", default=None, help="another build of libctk_hip.so for the legs p1 / p2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rpgd_batch_params: no GPU (nothing here is measured on a CPU)")
    legs = set(LEGS) if args.only is None else set(args.only.split(","))
    if not legs <= set(LEGS):
        sys.exit(f"bench_rpgd_batch_params: legs are {', '.join(LEGS)}")
    parent = bind_other_build(args.parent_lib) if args.parent_lib else None
    if parent is None:
        legs -= {"p1", "p2"}
    order = [k for k in LEGS if k in legs]
    cfg = dict(CONFIG, environment="CartPole")
    lines = [f"# tools/bench_rpgd_batch_params.py {args.label}: per problem RPGD N {cfg['num_rollouts']} / H {cfg['mpc_horizon']} / period "
             f"{cfg['period_interpolation_inducing_points']} / {cfg['outer_its']} iterations / keep {cfg['opt_keep_k']}, CartPole ODE (template kernels), "
             f"device Philox; host-clock medians [p10, p90] in us over {args.steps} calls per leg ({args.rounds} alternating rounds) after "
             f"{args.warmup} warm-up calls",
             "# (a) batch step, shared form   (b) batch step, per-problem form, parameters unchanged   (c) set_problem_params(target_position, new[B]) + step",
             "# (d) B template handles: set_param + step each   (p1), (p2) leg (a) through the other build of the library, twice: |p1 - p2| is the run-to-run band",
             f"{'B':>4s} " + " ".join(f"{'(' + k + ')':>28s}" for k in order) + f" | {'a-p1':>7s} {'p2-p1':>7s} {'b-a':>7s} {'c-b':>7s} {'c-d':>11s} {'(c)/(d)':>8s}"]
    print("\n".join(lines), flush=True)
    names = {}
    for B in [int(x) for x in args.sizes.split(",")]:
        out, names = measure(cfg, B, args.steps, args.warmup, args.rounds, legs, parent)
        med = {k: statistics.median(v) for k, v in out.items()}

        def col(k):
            q = statistics.quantiles(out[k], n=10)
            return f"{med[k]:10.2f} [{q[0]:7.1f},{q[-1]:8.1f}]".rjust(28)

        def diff(x, y, w=7, ratio=False):
            if x not in med or y not in med:
                return f"{'-':>8s}" if ratio else f"{'-':>{w}s}"
            return f"{med[x] / med[y]:8.3f}" if ratio else f"{med[x] - med[y]:+{w}.2f}"
        line = (f"{B:4d} " + " ".join(col(k) for k in order) + f" | {diff('a', 'p1')} {diff('p2', 'p1')} {diff('b', 'a')} {diff('c', 'b')} "
                f"{diff('c', 'd', 11)} {diff('c', 'd', ratio=True)}")
        lines.append(line)
        print(line, flush=True)
    lines.append("# kernels: " + ", ".join(f"({k}) {v}" for k, v in names.items()))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
