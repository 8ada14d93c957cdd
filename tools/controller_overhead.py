#!/usr/bin/env python3
"""What does controller_mpc.step cost on the host, above ctk_step?  (diagnostic; needs no GPU)

A real controller_mpc around mppi-hip, built as bench.py builds it, steps a stub library with ctk_step's signature that does nothing
(tests/_controller_native_helpers.py holds its source; this tool compiles it into a temporary directory).  Printed, in us per step (the
minimum of 5 loops of 20 000 steps): the native path (the bound controller and optimizer steps of _ctk_pystep), the same controller
held on Python by `native_step: false`, and each fallback of the native path: a float64 state, logging on, a parameter changed
before every step."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _controller_native_helpers as H  # noqa: E402
from control_toolkit_amd.others.globals_and_utils import DeviceBufferRng, DeviceRng  # noqa: E402

LOOPS, STEPS = 5, 20000


def per_step_us(step, before=None):
    best = float("inf")
    for _ in range(LOOPS):
        t0 = time.perf_counter()
        if before is None:
            for _ in range(STEPS):
                step()
        else:
            for i in range(STEPS):
                before(i); step()
        best = min(best, time.perf_counter() - t0)
    return best / STEPS * 1e6


def main():
    with tempfile.TemporaryDirectory() as d:
        lib = H.load_stub(H.build_stub(d))
        lib.stub_config(4, 1, 0, 0)
        s = np.array([0.05, -0.1, 2.8, 0.4], np.float32)
        s64 = s.astype(np.float64)
        pool = [0x7E0000000000 + 0x1000 * i for i in range(16)]
        rows = []

        def controller(native, rng="buffer", **kw):
            c = H.make_controller(lib, native_step=native, N=1024, H=50, **kw)
            c.optimizer.rng = DeviceBufferRng(pool, seed=1) if rng == "buffer" else DeviceRng(1)
            c.step(s); c.step(s)
            return c

        def row(label, c, us):
            o = c.optimizer
            rows.append((label, us, o.step_path, o.native_step_count, o.declined_step_count))

        for rng in ("buffer", "device-rng"):
            c = controller(True, rng)
            if c.optimizer._fast is None:
                print("control_toolkit_amd._ctk_pystep is not built (or CTK_PYSTEP=0): there is no native path to measure", file=sys.stderr)
                return 1
            row(f"native path, samples {rng}", c, per_step_us(lambda: c.step(s)))
            c = controller(False, rng)
            row(f"native_step: false, samples {rng}", c, per_step_us(lambda: c.step(s)))
        c = controller(True)
        row("native, optimizer.step alone (no bound controller step)", c, per_step_us(lambda: c.optimizer.step(s)))
        c = controller(True)
        python_step = c.step.__wrapped__
        row("native optimizer step under the Python controller step", c, per_step_us(lambda: python_step(s)))
        c = controller(True)
        row("fallback: float64 state", c, per_step_us(lambda: c.step(s64)))
        c = controller(False)
        row("  the same with native_step: false", c, per_step_us(lambda: c.step(s64)))
        c = controller(True, controller_logging=True)
        row("fallback: controller_logging on", c, per_step_us(lambda: (c.step(s), [v.clear() for v in c.logs.values()])))
        c = controller(False, controller_logging=True)
        row("  the same with native_step: false", c, per_step_us(lambda: (c.step(s), [v.clear() for v in c.logs.values()])))
        for native in (True, False):
            c = controller(native)
            params = c.cost_function.parameters

            def change(i, params=params):
                params["dd_weight"] = 600.0 + (i & 1)
            row("fallback: a cost parameter changed before every step" if native else "  the same with native_step: false", c,
                per_step_us(lambda: c.step(s), change))
        print(f"controller_mpc.step on a stub ctk_step, MPPI N=1024 H=50, us per step (min of {LOOPS} x {STEPS})")
        for label, us, path, native_steps, declined in rows:
            print(f"  {label:58s} {us:6.2f} us   last step: {path:6s}  native steps {native_steps:7d}  declined {declined:7d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
