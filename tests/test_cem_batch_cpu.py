"""CPU tests (-m "not gpu") of the batched-CEM binding (control_toolkit_amd._capi.CtkCemBatch, include/ctk_hip.h: ctk_cem_batch_*): what
needs no device is refused BEFORE the library is asked for one, the library's own refusals that depend on the configuration alone come
before its device probe, and without a GPU a valid construction fails loudly."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
KW = dict(num_rollouts=200, mpc_horizon=40, dt=0.02, cem_outer_it=3, cem_best_k=40)
FAMILY = ["create", "destroy", "last_error", "size", "samples_needed", "step", "reset", "read", "get_state", "set_state", "set_param",
          "get_param", "rng_get_position", "rng_set_position", "dominant_kernel"]


def test_class_is_exported():
    import control_toolkit_amd
    from control_toolkit_amd._capi import CtkCemBatch
    assert control_toolkit_amd.CtkCemBatch is CtkCemBatch and "CtkCemBatch" in control_toolkit_amd.__all__
    for name in ("__len__", "samples_needed", "step", "reset", "read", "read_all", "get_state", "set_state", "set_param", "get_param",
                 "rng_position", "set_rng_position", "dominant_kernel", "close"):
        assert callable(getattr(CtkCemBatch, name)), name


def test_every_cem_batch_symbol_is_bound_with_argument_types():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ctk_cem_batch_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted("ctk_cem_batch_" + n for n in FAMILY)        # the MPPI family, one for one
    lib = load_library()
    for n in names:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
        assert len(args) >= 1
    assert lib.ctk_abi_version() == 6                       # additive: the ABI version stays
    assert len(SYMBOLS["ctk_cem_batch_step"][1]) == 8 and len(SYMBOLS["ctk_cem_batch_create"][1]) == 4
    assert len(SYMBOLS["ctk_cem_batch_samples_needed"][1]) == 2        # (batch, problem): the count is per problem


def test_constructor_refuses_before_any_device_is_touched(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import CtkCemBatch

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one problem"):
            CtkCemBatch(bad, **KW)
    with pytest.raises(ValueError, match=r"one entry per problem \(4\), got 3"):
        CtkCemBatch(4, seeds=[1, 2, 3], **KW)
    for opt in ("mppi", "rpgd", "cem_gmm", "cem_naive_grad", "cem_grad_bharadhwaj"):
        with pytest.raises(NotImplementedError, match="plain CEM controllers only"):
            CtkCemBatch(4, optimizer=opt, **KW)
    for pred in ("MLP", "GRU"):
        with pytest.raises(NotImplementedError, match=r"analytic \(ODE\) predictor only"):
            CtkCemBatch(4, predictor=pred, **KW)
    with pytest.raises(TypeError, match="unknown engine arguments"):
        CtkCemBatch(3, nonsense=1, **KW)


def make_cfg(**over):
    from control_toolkit_amd import _capi
    kw = dict(KW)
    kw.update({k: over.pop(k) for k in list(over) if k in KW})
    cfg = _capi._make_config("cem", "ODE", 0, "CartPole", 1, action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=1, seed=0,
                             device=0, intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=4,
                             num_control_inputs=1, generic_kernels=False, **kw)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg, n):
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    rc = lib.ctk_cem_batch_create(ctypes.byref(cfg), n, None, ctypes.byref(out))
    msg = lib.ctk_cem_batch_last_error(None).decode()
    if out.value:
        lib.ctk_cem_batch_destroy(out)
    return rc, msg, bool(out.value)


def test_library_refuses_by_configuration_before_it_probes_the_device():
    """CTK_ERR_UNSUPPORTED (2) with the sizes in the message; none of these needs a GPU"""
    rc, msg, made = create(make_cfg(optimizer=0), 4)
    assert rc == 2 and not made and "plain CEM controllers only (cfg.optimizer == 0)" in msg
    for variant in (5, 6, 7):                                                             # naive-grad, Bharadhwaj, GMM
        rc, msg, made = create(make_cfg(optimizer=variant), 4)
        assert rc == 2 and not made and f"plain CEM controllers only (cfg.optimizer == {variant})" in msg and "single handles" in msg
    rc, msg, made = create(make_cfg(predictor=1), 4)
    assert rc == 2 and not made and "(ODE) predictor only (cfg.predictor == 1)" in msg
    rc, msg, made = create(make_cfg(num_rollouts=16384, cem_best_k=40), 2)                # 256 workgroups of 64 rollouts
    assert rc == 2 and not made and "num_rollouts 16384 = 256 workgroups" in msg and "at most 128 workgroups" in msg
    rc, msg, made = create(make_cfg(num_rollouts=64, mpc_horizon=200, cem_best_k=8), 2)   # two sample tiles + the plans: 768 bytes per column
    assert rc == 2 and not made and "mpc_horizon 200 x 1 inputs = 200 columns" in msg and "128 KiB" in msg
    lds = int(re.search(r"(\d+) bytes of LDS", msg).group(1))
    assert lds > 128 * 1024
    rc, msg, made = create(make_cfg(num_rollouts=64, mpc_horizon=8, cem_best_k=65), 2)
    assert rc == 2 and not made and "cem_best_k 65 exceeds num_rollouts 64" in msg
    rc, msg, made = create(make_cfg(), 0)
    assert rc == 2 and not made and "n_problems == 0" in msg
    rc, msg, made = create(make_cfg(struct_size=8), 2)
    assert rc == 1 and not made and "size mismatch" in msg
    # the MPPI family is what it was: it still refuses CEM
    from control_toolkit_amd._capi import load_library
    lib, out = load_library(), ctypes.c_void_p()
    cfg = make_cfg()
    assert lib.ctk_batch_create(ctypes.byref(cfg), 4, None, ctypes.byref(out)) == 2 and not out.value
    assert b"MPPI controllers only" in lib.ctk_batch_last_error(None)


def test_valid_batch_without_a_gpu_fails_loudly():
    import torch
    from control_toolkit_amd import CtkCemBatch, CtkError
    if torch.cuda.is_available():
        b = CtkCemBatch(3, **KW)                              # with a device the same call succeeds
        assert len(b) == 3 and b.samples_needed() == 3 * 200 * 40 and b.samples_needed(2) == 3 * 200 * 40
        b.close()
        return
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkCemBatch(3, **KW)
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkCemBatch(3, seeds=[5, 6, 2 ** 63 + 1], environment="Quad2D", num_rollouts=128, mpc_horizon=20, dt=0.02, cem_outer_it=2, cem_best_k=20)
