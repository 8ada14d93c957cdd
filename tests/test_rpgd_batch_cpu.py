"""CPU tests (-m "not gpu") of the batched-RPGD binding (control_toolkit_amd._capi.CtkRpgdBatch, include/ctk_hip.h: ctk_rpgd_batch_*): what
needs no device is refused BEFORE the library is asked for one, the library's own refusals that depend on the configuration alone come
before its device probe, and without a GPU a valid construction fails loudly."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
KW = dict(num_rollouts=32, mpc_horizon=20, dt=0.02, period_interpolation_inducing_points=5, outer_its=3, opt_keep_k=8, resamp_per=2,
          sample_whole_control_space=1)
FAMILY = ["create", "destroy", "last_error", "size", "samples_needed", "step", "reset", "read", "get_state", "set_state", "set_param",
          "get_param", "rng_get_position", "rng_set_position", "dominant_kernel"]


def test_class_is_exported():
    import control_toolkit_amd
    from control_toolkit_amd._capi import CtkRpgdBatch
    assert control_toolkit_amd.CtkRpgdBatch is CtkRpgdBatch and "CtkRpgdBatch" in control_toolkit_amd.__all__
    for name in ("__len__", "samples_needed", "step", "reset", "read", "read_all", "get_state", "set_state", "set_param", "get_param",
                 "rng_position", "set_rng_position", "dominant_kernel", "close"):
        assert callable(getattr(CtkRpgdBatch, name)), name
    assert "generic_kernels=True" in CtkRpgdBatch.__doc__ and "None means True" in CtkRpgdBatch.__doc__


def test_every_rpgd_batch_symbol_is_bound_with_argument_types():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ctk_rpgd_batch_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted("ctk_rpgd_batch_" + n for n in FAMILY)
    cem = sorted(set(re.findall(r"\bctk_cem_batch_([a-z_0-9]+)\s*\(", src)))
    assert cem == sorted(FAMILY)                             # the CEM family's names, one for one
    lib = load_library()
    for n in names:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
        assert len(args) >= 1
    assert lib.ctk_abi_version() == 6                       # additive: the ABI version stays
    assert len(SYMBOLS["ctk_rpgd_batch_create"][1]) == 4
    assert len(SYMBOLS["ctk_rpgd_batch_step"][1]) == 9      # the CEM step's arguments and the number of samples given
    assert len(SYMBOLS["ctk_rpgd_batch_reset"][1]) == 5     # (batch, n_ids, ids, draws, draws_loc): RPGD's reset draws the populations
    assert len(SYMBOLS["ctk_rpgd_batch_samples_needed"][1]) == 2       # (batch, problem): the count is per problem


def test_constructor_refuses_before_any_device_is_touched(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import CtkRpgdBatch

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one problem"):
            CtkRpgdBatch(bad, **KW)
    with pytest.raises(ValueError, match=r"one entry per problem \(4\), got 3"):
        CtkRpgdBatch(4, seeds=[1, 2, 3], **KW)
    for opt in ("mppi", "cem", "gradient", "random_action", "cem_gmm"):
        with pytest.raises(NotImplementedError, match="RPGD controllers only"):
            CtkRpgdBatch(4, optimizer=opt, **KW)
    for pred in ("MLP", "GRU"):
        with pytest.raises(NotImplementedError, match=r"analytic \(ODE\) predictor only"):
            CtkRpgdBatch(4, predictor=pred, **KW)
    with pytest.raises(TypeError, match="unknown engine arguments"):
        CtkRpgdBatch(3, nonsense=1, **KW)


def make_cfg(generic_kernels=True, **over):
    from control_toolkit_amd import _capi
    kw = dict(KW)
    kw.update({k: over.pop(k) for k in list(over) if k in KW})
    period = kw.pop("period_interpolation_inducing_points")
    cfg = _capi._make_config("rpgd", "ODE", 0, "CartPole", 1, action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=period,
                             seed=0, device=0, intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=4,
                             num_control_inputs=1, generic_kernels=generic_kernels, **kw)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg, n, family="ctk_rpgd_batch"):
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    rc = getattr(lib, family + "_create")(ctypes.byref(cfg), n, None, ctypes.byref(out))
    msg = getattr(lib, family + "_last_error")(None).decode()
    if out.value:
        getattr(lib, family + "_destroy")(out)
    return rc, msg, bool(out.value)


def test_library_refuses_by_configuration_before_it_probes_the_device():
    """CTK_ERR_UNSUPPORTED (2) with the sizes in the message; none of these needs a GPU"""
    for opt in (0, 1, 3, 4):                                  # MPPI, CEM, random action, the gradient variant
        rc, msg, made = create(make_cfg(optimizer=opt), 4)
        assert rc == 2 and not made and f"RPGD controllers only (cfg.optimizer == {opt}, num_rollouts 32, mpc_horizon 20)" in msg
        assert "CTK_OPT_GRADIENT" in msg and "single handles" in msg
    rc, msg, made = create(make_cfg(predictor=1), 4)
    assert rc == 2 and not made and "(ODE) predictor only (cfg.predictor == 1, num_rollouts 32, mpc_horizon 20)" in msg
    rc, msg, made = create(make_cfg(num_rollouts=65), 2)
    assert rc == 2 and not made and "num_rollouts 65 exceeds 64" in msg and "one workgroup" in msg
    rc, msg, made = create(make_cfg(num_rollouts=16, opt_keep_k=17), 2)
    assert rc == 2 and not made and "opt_keep_k 17 exceeds num_rollouts 16" in msg
    rc, msg, made = create(make_cfg(materialize_trajectories=1), 2)
    assert rc == 2 and not made and "materialize_trajectories" in msg and "no seam" in msg and "num_rollouts 32, mpc_horizon 20" in msg
    rc, msg, made = create(make_cfg(mpc_horizon=400), 2)     # plans + gradients [400][65] floats each, before any tape
    assert rc == 2 and not made and "mpc_horizon 400 x 1 inputs = 400 columns" in msg and "160 KiB" in msg
    lds = int(re.search(r"need (\d+) bytes of LDS", msg).group(1))
    assert lds == (2 * 400 * 65 + 64) * 4 and lds > 160 * 1024
    rc, msg, made = create(make_cfg(), 0)
    assert rc == 2 and not made and "n_problems == 0" in msg
    rc, msg, made = create(make_cfg(generic_kernels=False), 2)
    assert rc == 2 and not made and "tuned descent" in msg and "no batch form" in msg and "template kernels do" in msg
    assert "num_rollouts 32, mpc_horizon 20" in msg
    rc, msg, made = create(make_cfg(struct_size=8), 2)
    assert rc == 1 and not made and "size mismatch" in msg
    # the CEM and MPPI families are what they were: they still refuse RPGD
    rc, msg, made = create(make_cfg(), 4, "ctk_cem_batch")
    assert rc == 2 and not made and "plain CEM controllers only (cfg.optimizer == 2)" in msg
    rc, msg, made = create(make_cfg(), 4, "ctk_batch")
    assert rc == 2 and not made and "MPPI controllers only" in msg


def test_valid_batch_without_a_gpu_fails_loudly():
    import torch
    from control_toolkit_amd import CtkRpgdBatch, CtkError
    if torch.cuda.is_available():
        b = CtkRpgdBatch(3, **KW)                             # with a device the same call succeeds
        assert len(b) == 3 and b.samples_needed() == (32 - 8) * 5 and b.samples_needed(2) == (32 - 8) * 5   # P = ceil(19 / 5) + 1
        assert b.samples_needed_reset() == 32 * 5
        b.close()
        return
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkRpgdBatch(3, **KW)
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkRpgdBatch(3, seeds=[5, 6, 2 ** 63 + 1], environment="Quad2D", num_rollouts=32, mpc_horizon=10, dt=0.02, outer_its=2, opt_keep_k=8)
