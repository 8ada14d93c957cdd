"""What the in-kernel Philox4x32-10 sampler (samples = None, CTK_LOC_NONE) draws, stated once for every optimizer, in plain NumPy.

`expected_samples(opt, cfg, seed, position, phase)` is exactly the array the host-sample mode of ctk_step / ctk_reset takes for the
same call (include/ctk_hip.h, "the hot path"), assembled from oracle.ctk_oracle.device_noise and nothing else: feeding it to the
oracle is what a device-draw step of a handle at Philox position `position` must reproduce.  The counter of a draw is
(global row, block of 4 columns, call, stream), the key (seed_lo, seed_hi); `plan(...)` lists the (stream, call, first row, rows,
cols, kind) blocks of one call, `counters(...)` the Philox counters they consume.

cfg: a dict with N, H, C and, where the optimizer has them, P (inducing points), its (outer iterations of THIS step), K (elites),
k (RPGD keepers), kind ("uniform" / "normal", RPGD's sampling_distribution 0 / 1), offset (global_rollout_offset, default 0).

`normal_f64` pushes the same integer words through Box-Muller in float64 (the device's float32 argument 2*pi*u2 kept, sqrt / log /
sin / cos in float64): the high-precision reference of the transform."""
import math

import numpy as np

from oracle import ctk_oracle as O

GMM_UNIFORM_STREAM = 0x40000000   # + outer iteration (tests/gmm_oracle.py: UNIFORM_STREAM)

OPTIMIZERS = ("mppi", "cem", "cem_naive_grad", "random_action", "rpgd", "gradient", "cem_grad_bharadhwaj", "cem_gmm")


def plan(opt, cfg, position, phase="step"):
    """the draw blocks of one call, in the order of the host-sample layout: [(stream, call, first_row, rows, cols, kind)]"""
    N, H, C = cfg["N"], cfg["H"], cfg["C"]
    off = cfg.get("offset", 0)
    if phase == "reset":
        if opt == "rpgd":
            return [(0, position, off, N, cfg["P"] * C, cfg.get("kind", "uniform"))]
        if opt == "gradient":
            return [(0, position, off, N, H * C, "uniform")]
        return []                                      # the other optimizers' resets draw nothing
    if opt == "mppi":
        return [(0, position, off, N, cfg["P"] * C, "normal")]
    if opt in ("cem", "cem_naive_grad"):
        return [(it, position, off, N, H * C, "normal") for it in range(cfg["its"])]
    if opt == "random_action":
        return [(0, position, off, N, H * C, "uniform")]
    if opt == "rpgd":                                  # a RESAMPLING step (the others draw nothing)
        return [(0, position, off, N - cfg["k"], cfg["P"] * C, cfg.get("kind", "uniform"))]
    if opt == "gradient":                              # the tail input of every plan: word c of column block 0
        return [(0, position, off, N, C, "uniform")]
    if opt == "cem_grad_bharadhwaj":
        K = cfg["K"]
        return [(0, position, off, K, H * C, "normal")] + [(it, position, off + K, N - K, H * C, "normal") for it in range(cfg["its"])]
    if opt == "cem_gmm":                               # per iteration: the normals, then one uniform per rollout
        out = []
        for it in range(cfg["its"]):
            out += [(it, position, off, N, H * C, "normal"), (GMM_UNIFORM_STREAM + it, position, off, N, 1, "uniform")]
        return out
    raise ValueError(f"unknown optimizer {opt!r}")


def expected_samples(opt, cfg, seed, position, phase="step"):
    """flat fp32 array: the `samples` of ctk_step (phase "step") or the `draws` of ctk_reset (phase "reset") that reproduce a
    CTK_LOC_NONE call of a handle with this seed at Philox position `position`"""
    blocks = [O.device_noise(seed, stream, call, row0, rows, cols, kind).reshape(-1)
              for stream, call, row0, rows, cols, kind in plan(opt, cfg, position, phase)]
    return np.concatenate(blocks).astype(np.float32) if blocks else np.zeros(0, np.float32)


def samples_documented(opt, cfg, phase="step"):
    """the size include/ctk_hip.h documents for ctk_samples_needed (and for the draws of ctk_reset), written out independently"""
    N, H, C = cfg["N"], cfg["H"], cfg["C"]
    if phase == "reset":
        return N * cfg["P"] * C if opt == "rpgd" else N * H * C if opt == "gradient" else 0
    return {"mppi": lambda: N * cfg["P"] * C, "cem": lambda: cfg["its"] * N * H * C, "cem_naive_grad": lambda: cfg["its"] * N * H * C,
            "random_action": lambda: N * H * C, "rpgd": lambda: (N - cfg["k"]) * cfg["P"] * C, "gradient": lambda: N * C,
            "cem_grad_bharadhwaj": lambda: cfg["K"] * H * C + cfg["its"] * (N - cfg["K"]) * H * C,
            "cem_gmm": lambda: cfg["its"] * (N * H * C + N)}[opt]()


def counters(opt, cfg, position, phase="step"):
    """the Philox counters (row, column block, call, stream) one call consumes, as an int64 array [n, 4]"""
    out = []
    for stream, call, row0, rows, cols, _ in plan(opt, cfg, position, phase):
        r, b = np.meshgrid(np.arange(row0, row0 + rows, dtype=np.int64), np.arange((cols + 3) // 4, dtype=np.int64), indexing="ij")
        out.append(np.stack([r.ravel(), b.ravel(), np.full(r.size, call, np.int64), np.full(r.size, stream, np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def schedule(opt, cfg, steps=3):
    """(phase, position, draws?) of a fresh handle over reset + `steps` steps: the position advances by one after a reset that draws
    and after EVERY completed step (ctk_api.hip: rpgd_reset, finish_step), an RPGD step that does not resample included"""
    pos, out = 0, []
    if opt in ("rpgd", "gradient"):
        out.append(("reset", pos, True)); pos += 1
    for t in range(steps):
        draws = opt != "rpgd" or t % cfg.get("resamp_per", 1) == 0
        out.append(("step", pos, draws)); pos += 1
    return out


def normal_f64(seed, stream, call, first_row, rows, cols):
    """device_noise(kind="normal") with the transform in float64: u1 in (0,1], u2 in [0,1) and the argument 2*pi*u2 as the device
    forms them (float32), then sqrt(-2 log u1) * cos / sin in float64"""
    nblk = (cols + 3) // 4
    r = np.arange(first_row, first_row + rows, dtype=np.uint32)[:, None]
    b = np.arange(nblk, dtype=np.uint32)[None, :]
    ctr = np.stack(np.broadcast_arrays(r, b, np.uint32(call), np.uint32(stream)), axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    x = O.philox4x32(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    out = []
    for a, c in ((0, 1), (2, 3)):
        u1 = O.u32_to_unit_open(x[..., a]).astype(np.float64)
        th = (O.f32(2.0 * math.pi) * O.u32_to_unit_halfopen(x[..., c])).astype(np.float32).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        out += [rad * np.cos(th), rad * np.sin(th)]
    return np.stack(out, axis=-1).reshape(rows, nblk * 4)[:, :cols]


def small_u1(seed, stream, call, first_row, rows, cols, below=1e-3):
    """mask [rows, cols] of the normal draws whose radius comes from a u1 < `below`: where a (0,1] / [0,1) mix-up in u1 shows most"""
    nblk = (cols + 3) // 4
    r = np.arange(first_row, first_row + rows, dtype=np.uint32)[:, None]
    b = np.arange(nblk, dtype=np.uint32)[None, :]
    ctr = np.stack(np.broadcast_arrays(r, b, np.uint32(call), np.uint32(stream)), axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    x = O.philox4x32(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    ua, ub = O.u32_to_unit_open(x[..., 0]) < below, O.u32_to_unit_open(x[..., 2]) < below
    return np.stack([ua, ua, ub, ub], axis=-1).reshape(rows, nblk * 4)[:, :cols]


# ---- the shapes tests/test_gpu_device_rng.py runs (the CPU tests bound the oracle's own Box-Muller rounding on the same ones) ----------
SEED = (0x5EED0BAD << 32) | 0x00C0FFEE      # the high word is not zero: seed_hi reaches the key
MPPI_ODE_SHAPES = [(1024, 50, 1, 0), (70, 7, 1, 4099), (130, 35, 10, 0), (1, 1, 1, 0)]      # (N, H, period, global_rollout_offset)
CEM_ODE_SHAPES = [(130, 7, 13, 3), (1024, 30, 100, 2)]                                      # (N, H, K, iterations)
J_RTOL = 3e-5                               # the J tolerance of test_gpu_mppi.py / test_gpu_cem_random.py (oracle-seeded cases)
S0 = np.array([0.1, -0.2, 2.5, 0.7], np.float32)
