"""The names in the refusals of the four batch families (ctk_batch_*, ctk_mlp_batch_*, ctk_cem_batch_*, ctk_rpgd_batch_*): every entry
that takes a problem index or an id list, called through the library with an index outside the batch (and, for an id list, with a
descending pair), returns CTK_ERR_INVALID_ARGUMENT, and the batch's last error starts with THAT entry's exported name and names no
other family.  The MLP family, which runs the MPPI family's code, besides refuses step, run and episodes of a problem without weights
under its own names and moves nothing.  No call here launches anything."""
import ctypes as C

import numpy as np
import pytest

from control_toolkit_amd import CtkCemBatch, CtkMppiBatch, CtkMppiMlpBatch, CtkRpgdBatch
import test_gpu_cem_batch
import test_gpu_mlp_batch
import test_gpu_mppi_batch
import test_gpu_rpgd_batch

pytestmark = pytest.mark.gpu

B = 2
ERR_INVALID_ARGUMENT, ERR_STATE = 1, 5           # include/ctk_hip.h: enum ctk_status
PREFIXES = {"mppi": ("ctk_batch_", "ctk_problem_"), "mlp": ("ctk_mlp_batch_", "ctk_mlp_problem_"),
            "cem": ("ctk_cem_batch_", "ctk_cem_problem_"), "rpgd": ("ctk_rpgd_batch_", "ctk_rpgd_problem_")}


def make(family):
    """the family's batch of B problems at the smallest configuration of its own test file, materialize_trajectories off"""
    if family == "mppi":
        env, N, H, p, extra, _ = test_gpu_mppi_batch.CONFIGS["cartpole_small"]
        return CtkMppiBatch(B, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, environment=env,
                            materialize_trajectories=False, **extra)
    if family == "mlp":
        N, H, p = test_gpu_mlp_batch.SIZES[0]
        assert (N, H, p) == (16, 5, 2)
        return CtkMppiMlpBatch(B, num_rollouts=N, mpc_horizon=H, dt=0.02, period_interpolation_inducing_points=p, materialize_trajectories=False)
    if family == "cem":
        return CtkCemBatch(B, **test_gpu_cem_batch.common_kw("one_workgroup", False))
    return CtkRpgdBatch(B, materialize_trajectories=False, **test_gpu_rpgd_batch.CONFIGS["cartpole_small"]())


def entries(family, F, cap):
    """name -> (kind, call): kind "ids" — call(n, ids) with an id list, "index" — call(p) with a problem index; every other argument
    is valid (F: a float buffer of cap floats, large enough for whatever a call of B problems and one step would write)"""
    batch, problem = (x.rstrip("_") for x in PREFIXES[family])
    rpgd = family == "rpgd"
    out = {
        f"{batch}_step": ("ids", (lambda n, ids: (n, ids, F, None, None, 0, 0, F)) if rpgd else (lambda n, ids: (n, ids, F, None, None, 0, F))),
        f"{batch}_reset": ("ids", (lambda n, ids: (n, ids, None, 0)) if rpgd else (lambda n, ids: (n, ids))),
        f"{batch}_read": ("index", lambda p: (p, 1, F, cap)),
        f"{batch}_get_state": ("index", lambda p: (p, F, cap)),
        f"{batch}_set_state": ("index", lambda p: (p, F, 1)),
        f"{batch}_rng_set_position": ("index", lambda p: (p, 0)),
        f"{problem}_set_param": ("ids", lambda n, ids: (n, ids, 0, F)),
        f"{batch}_plant_set_param": ("ids", lambda n, ids: (n, ids, 0, F)),
        f"{batch}_plant_set_noise": ("ids", lambda n, ids: (n, ids, 0, F)),
        f"{batch}_plant_set_noise_seed": ("ids", lambda n, ids: (n, ids, F)),
        f"{batch}_plant_noise_set_position": ("index", lambda p: (p, 0)),
        f"{batch}_plant_step": ("ids", lambda n, ids: (n, ids, F, F, 0, F)),
        f"{batch}_plant_step_noisy": ("ids", lambda n, ids: (n, ids, F, F, F, 0, F, F, F)),
        f"{batch}_run": ("ids", lambda n, ids: (n, ids, F, None, 1, 0, F, F, None)),
        f"{batch}_episodes": ("ids", lambda n, ids: (n, ids, F, None, None, 1, 0, F, F, F, F, None)),
    }
    if family == "mlp":
        out["ctk_mlp_problem_set_weights"] = ("ids", lambda n, ids: (n, ids, F, test_gpu_mlp_batch.weights(100).size))
    return out


def refused(batch, family, name, args, code=ERR_INVALID_ARGUMENT):
    """the call is refused with `code`; the message starts with the entry's own name and names no other family.  Returns the message."""
    rc = getattr(batch._lib, name)(batch._h, *args)
    msg = batch._b.last_error(batch._h).decode()
    assert rc == code, f"{name}{args[:2]}: return code {rc}, message {msg!r}"
    assert msg.startswith(name + ": "), f"{name}: the message starts with another name: {msg!r}"
    for other, prefixes in PREFIXES.items():
        if other != family:
            assert not any(x in msg for x in prefixes), f"{name}: the message names the {other} family: {msg!r}"
    return msg


@pytest.mark.parametrize("family", list(PREFIXES))
def test_refusals_carry_the_entry_s_own_name(family):
    batch = make(family)
    try:
        buf = np.zeros(4096, np.float32)
        F = buf.ctypes.data_as(C.c_void_p)
        outside = np.array([B], np.int32)
        descending = np.array([1, 0], np.int32)
        before = [batch.rng_position(p) for p in range(B)]
        for name, (kind, args) in entries(family, F, buf.size).items():
            if kind == "index":
                assert f"problem index {B} is outside 0 .. {B - 1}" in refused(batch, family, name, args(B))
            else:
                assert f"problem index {B} is outside 0 .. {B - 1}" in refused(batch, family, name, args(1, outside.ctypes.data_as(C.c_void_p)))
                assert "ids must be strictly ascending" in refused(batch, family, name, args(2, descending.ctypes.data_as(C.c_void_p)))
        if family == "mlp":        # no problem has weights: refused under this family's names before anything is launched
            table = entries(family, F, buf.size)
            for name in ("ctk_mlp_batch_step", "ctk_mlp_batch_run", "ctk_mlp_batch_episodes"):
                msg = refused(batch, family, name, table[name][1](0, None), code=ERR_STATE)
                assert msg == (f"{name}: no network weights for problem(s) 0, 1 (ctk_mlp_batch_set_weights / ctk_mlp_problem_set_weights "
                               "before stepping); nothing was launched")
        assert [batch.rng_position(p) for p in range(B)] == before
        assert not buf.any()                         # no call wrote a result
    finally:
        batch.close()
