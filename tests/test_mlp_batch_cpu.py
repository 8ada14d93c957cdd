"""CPU tests (-m "not gpu") of the batched MPPI with the MLP predictor (control_toolkit_amd._capi.CtkMppiMlpBatch, include/ctk_hip.h:
ctk_mlp_batch_* / ctk_mlp_problem_*): the family is declared, bound and exported beside the existing ones, which are what they were; what
needs no device is refused BEFORE the library is asked for one; the library's own refusals that depend on the configuration alone come
before its device probe; without a GPU a valid construction fails loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import ctk_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
KW = dict(num_rollouts=256, mpc_horizon=20, dt=0.02)
BATCH = ["create", "destroy", "last_error", "size", "samples_needed", "step", "reset", "read", "get_state", "set_state", "set_param",
         "get_param", "rng_get_position", "rng_set_position", "dominant_kernel", "weight_count", "set_weights"]
PROBLEM = ["set_param", "get_param", "params_differ", "set_weights", "have_weights"]
# the sizes of tests/test_gpu_mlp_batch.py, as (N, H, period)
SIZES = [(16, 5, 2), (70, 12, 5), (1000, 35, 10), (1024, 50, 1), (4096, 14, 1)]


def header_names(pattern):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(pattern, src)))


def test_class_is_exported():
    import control_toolkit_amd
    from control_toolkit_amd._capi import CtkMppiMlpBatch, CtkMppiBatch
    assert control_toolkit_amd.CtkMppiMlpBatch is CtkMppiMlpBatch and "CtkMppiMlpBatch" in control_toolkit_amd.__all__
    for m in ("step", "reset", "read", "read_all", "get_state", "set_state", "set_param", "get_param", "set_problem_params", "get_problem_param",
              "get_problem_params", "params_differ", "rng_position", "set_rng_position", "dominant_kernel", "samples_needed", "close",
              "weight_count", "set_weights", "set_problem_weights", "have_weights"):
        assert callable(getattr(CtkMppiMlpBatch, m)), m
    assert not hasattr(CtkMppiBatch, "set_weights")         # the analytic batch is what it was


def test_every_symbol_is_declared_bound_and_exported():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    batch = header_names(r"\b(ctk_mlp_batch_[a-z_0-9]+)\s*\(")
    problem = header_names(r"\b(ctk_mlp_problem_[a-z_0-9]+)\s*\(")
    assert batch == sorted("ctk_mlp_batch_" + n for n in BATCH)
    assert problem == sorted("ctk_mlp_problem_" + n for n in PROBLEM)
    lib = load_library()
    for n in batch + problem:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)                                 # AttributeError: not exported
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
    # the signatures are those of the MPPI family
    for n in BATCH[:15]:
        assert SYMBOLS["ctk_mlp_batch_" + n] == SYMBOLS["ctk_batch_" + n], n
    for n in PROBLEM[:3]:
        assert SYMBOLS["ctk_mlp_problem_" + n] == SYMBOLS["ctk_problem_" + n], n
    assert len(SYMBOLS["ctk_mlp_problem_set_weights"][1]) == 5 and len(SYMBOLS["ctk_mlp_batch_set_weights"][1]) == 3


def test_the_existing_families_are_what_they_were():
    from control_toolkit_amd._capi import load_library
    assert len(header_names(r"\b(ctk_batch_[a-z_0-9]+)\s*\(")) == 15
    for fam in ("ctk_problem_", "ctk_cem_problem_", "ctk_rpgd_problem_"):
        assert len(header_names(rf"\b({fam}[a-z_0-9]+)\s*\(")) == 3, fam
    assert load_library().ctk_abi_version() == 6            # additive: the ABI version stays
    assert re.search(r"CTK_ABI_VERSION 6\b", open(HEADER).read())


def test_constructor_refuses_before_any_device_is_touched(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import CtkMppiMlpBatch

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one problem"):
            CtkMppiMlpBatch(bad, **KW)
    with pytest.raises(ValueError, match=r"one entry per problem \(4\), got 3"):
        CtkMppiMlpBatch(4, seeds=[1, 2, 3], **KW)
    for opt in ("cem", "rpgd"):
        with pytest.raises(NotImplementedError, match="MPPI controllers only"):
            CtkMppiMlpBatch(4, optimizer=opt, **KW)
    with pytest.raises(NotImplementedError, match="CtkMppiBatch"):
        CtkMppiMlpBatch(4, predictor="ODE", **KW)
    with pytest.raises(NotImplementedError, match="hidden state has no batch form"):
        CtkMppiMlpBatch(4, predictor="GRU", **KW)
    with pytest.raises(NotImplementedError, match="CartPole"):
        CtkMppiMlpBatch(4, environment="Quad2D", **KW)
    with pytest.raises(NotImplementedError, match="generic_kernels True"):
        CtkMppiMlpBatch(4, generic_kernels=True, **KW)
    with pytest.raises(NotImplementedError, match=r"32 units per hidden layer \(predictor_hidden \(64, 32\)\)"):
        CtkMppiMlpBatch(4, predictor_hidden=(64, 32), **KW)
    for bad in ((8,), (8, 0), (1, 2, 3)):
        with pytest.raises(ValueError, match="two widths"):
            CtkMppiMlpBatch(4, predictor_hidden=bad, **KW)


def test_weight_count_arithmetic():
    from control_toolkit_amd._capi import mlp_weight_count
    assert mlp_weight_count(4, 1) == O.mlp_num_weights() == 1380
    assert mlp_weight_count(4, 1, (8, 12)) == O.mlp_num_weights(hidden=(8, 12)) == 5 * 8 + 8 + 8 * 12 + 12 + 12 * 4 + 4
    assert mlp_weight_count(4, 1, (32, 7)) == O.mlp_num_weights(hidden=(32, 7))
    assert O.mlp_default_weights(3, hidden=(8, 12)).size == mlp_weight_count(4, 1, (8, 12))


def make_cfg(**over):
    from control_toolkit_amd import _capi
    kw = dict(KW)
    kw.update({k: over.pop(k) for k in list(over) if k in ("num_rollouts", "mpc_horizon", "dt")})
    period = over.pop("period", 1)
    name = over.pop("env", "CartPole")
    S, Cn, _ = _capi.environment_info(name)
    env = (name, _capi.environment_library(name)[1], S, Cn)
    cfg = _capi._make_config("mppi", "MLP", env[1], env[0], env[3], action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=period,
                             seed=0, device=0, intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=env[2],
                             num_control_inputs=env[3], generic_kernels=False, **kw)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg, n):
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    rc = lib.ctk_mlp_batch_create(ctypes.byref(cfg), n, None, ctypes.byref(out))
    msg = lib.ctk_mlp_batch_last_error(None).decode()
    if out.value:
        lib.ctk_mlp_batch_destroy(out)
    return rc, msg, bool(out.value)


SIZES_IN_MSG = "num_rollouts 256, mpc_horizon 20, 20 inducing points, network 5IN-32H1-32H2-4OUT"


def test_library_refuses_by_configuration_before_it_probes_the_device():
    """CTK_ERR_UNSUPPORTED (2) with the sizes in the message; none of these needs a GPU"""
    rc, msg, made = create(make_cfg(optimizer=1), 4)
    assert rc == 2 and not made and "ctk_mlp_batch_create: a batch steps MPPI controllers only (cfg.optimizer == 1)" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor=0), 4)
    assert rc == 2 and not made and "cfg.predictor == 0" in msg and "use ctk_batch_create" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor=2), 4)
    assert rc == 2 and not made and "cfg.predictor == 2" in msg and "hidden state has no batch form" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(env="Quad2D"), 4)
    assert rc == 2 and not made and "environment Quad2D" in msg and "template network kernels" in msg and "num_rollouts 256" in msg
    rc, msg, made = create(make_cfg(generic_kernels=1), 4)
    assert rc == 2 and not made and "generic_kernels == 1" in msg and "template network kernels" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor_hidden1=64), 4)
    assert rc == 2 and not made and "32 units per hidden layer" in msg and "network 5IN-64H1-32H2-4OUT" in msg
    rc, msg, made = create(make_cfg(predictor_hidden2=33), 4)
    assert rc == 2 and not made and "network 5IN-32H1-33H2-4OUT" in msg
    rc, msg, made = create(make_cfg(), 0)
    assert rc == 2 and not made and "ctk_mlp_batch_create" in msg and "n_problems == 0" in msg
    # the fit: 32 rollouts per block record here
    rc, msg, made = create(make_cfg(num_rollouts=4096, mpc_horizon=15), 2)               # 128 x 17 = 2 176 words > 2 048
    assert rc == 2 and not made and "num_rollouts 4096, mpc_horizon 15, 15 inducing points x 1 inputs = 128 block records of 17 words" in msg
    assert "narrow in-launch hand-off" in msg and "ctk_mlp_batch_create" in msg
    rc, msg, made = create(make_cfg(num_rollouts=4128, mpc_horizon=5), 2)                # 129 records
    assert rc == 2 and not made and "129 block records of 7 words" in msg and "narrow in-launch hand-off" in msg
    rc, msg, made = create(make_cfg(num_rollouts=8193, mpc_horizon=5), 2)                # a handle of this size runs the 64-trajectory form
    assert rc == 2 and not made and "num_rollouts 8193" in msg and "pair form" in msg
    rc, msg, made = create(make_cfg(num_rollouts=64, mpc_horizon=1000), 2)               # LDS
    assert rc == 2 and not made and "160 KiB" in msg and "mpc_horizon 1000" in msg
    rc, msg, made = create(make_cfg(struct_size=8), 2)
    assert rc == 1 and not made and "ctk_mlp_batch_create: ctk_config size mismatch" in msg
    # NULL handles answer like the other families'
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    assert lib.ctk_mlp_batch_size(None) == 0 and lib.ctk_mlp_batch_weight_count(None) == 0 and lib.ctk_mlp_problem_have_weights(None, 0) == 0
    assert lib.ctk_mlp_batch_set_weights(None, None, 0) == 1 and lib.ctk_mlp_batch_step(None, 0, None, None, None, None, 0, None) == 1


def test_the_fit_accepts_the_tested_sizes():
    """every size of the GPU tests passes the configuration checks (what is left to fail without a GPU is the device probe, which comes
    behind them); one step of the horizon beyond the last size is refused"""
    import torch
    for N, H, p in SIZES:
        rc, msg, made = create(make_cfg(num_rollouts=N, mpc_horizon=H, period=p), 3)
        if torch.cuda.is_available():
            assert rc == 0 and made, msg
        else:
            assert rc == 4 and not made and "no HIP device" in msg, (N, H, p, msg)
    rc, msg, made = create(make_cfg(num_rollouts=4096, mpc_horizon=15), 3)
    assert rc == 2 and not made


def test_valid_batch_without_a_gpu_fails_loudly():
    import torch
    from control_toolkit_amd import CtkMppiMlpBatch, CtkError
    if torch.cuda.is_available():
        b = CtkMppiMlpBatch(3, **KW)                          # with a device the same call succeeds
        assert len(b) == 3 and b.samples_needed() == 256 * 20 and b.weight_count() == 1380 and not b.have_weights(0)
        b.close()
        return
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiMlpBatch(3, **KW)
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiMlpBatch(3, seeds=[5, 6, 2 ** 63 + 1], predictor_hidden=(8, 12), num_rollouts=64, mpc_horizon=10, dt=0.02)
    with pytest.raises(TypeError, match="unknown engine arguments"):
        CtkMppiMlpBatch(3, nonsense=1, **KW)
