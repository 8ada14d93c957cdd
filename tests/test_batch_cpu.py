"""CPU tests (-m "not gpu") of the batched-MPPI binding (control_toolkit_amd._capi.CtkMppiBatch, include/ctk_hip.h: ctk_batch_*): what
needs no device is refused BEFORE the library is asked for one, the library's own refusals that depend on the configuration alone come
before its device probe, and without a GPU a valid construction fails loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
KW = dict(num_rollouts=256, mpc_horizon=20, dt=0.02)


def test_class_is_exported():
    import control_toolkit_amd
    from control_toolkit_amd._capi import CtkMppiBatch
    assert control_toolkit_amd.CtkMppiBatch is CtkMppiBatch and "CtkMppiBatch" in control_toolkit_amd.__all__


def test_every_batch_symbol_is_bound_with_argument_types():
    from control_toolkit_amd._capi import load_library, SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ctk_batch_[a-z_0-9]+)\s*\(", src)))
    assert len(names) == 15 and "ctk_batch_step" in names and "ctk_batch_create" in names
    lib = load_library()
    for n in names:
        assert n in SYMBOLS, f"{n} is declared in the header but not bound"
        res, args = SYMBOLS[n]
        fn = getattr(lib, n)
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
        assert len(args) >= 1
    assert lib.ctk_abi_version() == 6                       # additive: the ABI version stays
    assert len(SYMBOLS["ctk_batch_step"][1]) == 8 and len(SYMBOLS["ctk_batch_create"][1]) == 4


def test_constructor_refuses_before_any_device_is_touched(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import CtkMppiBatch

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one problem"):
            CtkMppiBatch(bad, **KW)
    with pytest.raises(ValueError, match=r"one entry per problem \(4\), got 3"):
        CtkMppiBatch(4, seeds=[1, 2, 3], **KW)
    with pytest.raises(NotImplementedError, match="MPPI controllers only"):
        CtkMppiBatch(4, optimizer="cem", **KW)
    with pytest.raises(NotImplementedError, match="MPPI controllers only"):
        CtkMppiBatch(4, optimizer="rpgd", **KW)
    for pred in ("MLP", "GRU"):
        with pytest.raises(NotImplementedError, match=r"analytic \(ODE\) predictor only"):
            CtkMppiBatch(4, predictor=pred, **KW)


def test_step_arguments_are_checked_without_a_device():
    from control_toolkit_amd._capi import batch_step_args, batch_ids
    B, S, Cn, per = 6, 4, 1, 256 * 20
    ok = np.zeros((B, S), np.float32)
    ids, n, smp = batch_step_args(B, S, Cn, per, ok)
    assert ids is None and n == B and smp is None
    ids, n, smp = batch_step_args(B, S, Cn, per, ok[:3], np.zeros((3, 256, 20, 1)), np.zeros((3, 1)), [0, 2, 5])
    assert ids.dtype == np.int32 and list(ids) == [0, 2, 5] and n == 3 and smp.dtype == np.float32 and smp.flags.c_contiguous
    assert batch_step_args(B, S, Cn, per, ok, 0x7F0000000000)[2] == 0x7F0000000000          # a device pointer passes through
    for bad in ([2, 1], [1, 1], [0, 3, 2]):
        with pytest.raises(ValueError, match="strictly ascending"):
            batch_step_args(B, S, Cn, per, ok[:len(bad)], ids=bad)
    with pytest.raises(ValueError, match=r"0 \.\. 5"):
        batch_ids(B, [0, 6])
    with pytest.raises(ValueError, match=r"0 \.\. 5"):
        batch_ids(B, [-1, 2])
    with pytest.raises(ValueError, match="non-empty"):
        batch_ids(B, [])
    with pytest.raises(ValueError, match="non-empty"):
        batch_ids(B, [0.5, 1.5])
    with pytest.raises(ValueError, match=r"states must have shape \(6, 4\)"):
        batch_step_args(B, S, Cn, per, np.zeros((5, S)))
    with pytest.raises(ValueError, match=r"states must have shape \(6, 4\)"):
        batch_step_args(B, S, Cn, per, np.zeros((B, 5)))
    with pytest.raises(ValueError, match=r"states must have shape \(2, 4\)"):
        batch_step_args(B, S, Cn, per, ok, ids=[1, 2])
    with pytest.raises(ValueError, match=r"u_prev must have shape \(6, 1\)"):
        batch_step_args(B, S, Cn, per, ok, u_prev=np.zeros((5, 1)))
    with pytest.raises(ValueError, match=r"u_prev must have shape \(6, 2\)"):
        batch_step_args(B, S, 2, per, ok, u_prev=np.zeros(6))
    with pytest.raises(ValueError, match=r"consumes 6 x 5120 draws"):
        batch_step_args(B, S, Cn, per, ok, np.zeros((B, 256, 19, 1)))
    with pytest.raises(ValueError, match=r"consumes 6 x 5120 draws"):
        batch_step_args(B, S, Cn, per, ok, np.zeros((3, 512, 20, 1)))                        # the right count in the wrong rows
    with pytest.raises(ValueError, match=r"consumes 2 x 5120 draws"):
        batch_step_args(B, S, Cn, per, ok[:2], np.zeros((B, 256, 20, 1)), ids=[0, 1])


def make_cfg(**over):
    from control_toolkit_amd import _capi
    kw = dict(KW)
    kw.update({k: over.pop(k) for k in list(over) if k in ("num_rollouts", "mpc_horizon", "dt")})
    cfg = _capi._make_config("mppi", "ODE", 0, "CartPole", 1, action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=1, seed=0,
                             device=0, intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=4,
                             num_control_inputs=1, generic_kernels=False, **kw)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg, n):
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    rc = lib.ctk_batch_create(ctypes.byref(cfg), n, None, ctypes.byref(out))
    msg = lib.ctk_batch_last_error(None).decode()
    if out.value:
        lib.ctk_batch_destroy(out)
    return rc, msg, bool(out.value)


def test_library_refuses_by_configuration_before_it_probes_the_device():
    """CTK_ERR_UNSUPPORTED (2) with the sizes in the message; none of these needs a GPU"""
    rc, msg, made = create(make_cfg(optimizer=1), 4)
    assert rc == 2 and not made and "MPPI controllers only (cfg.optimizer == 1)" in msg
    rc, msg, made = create(make_cfg(predictor=1), 4)
    assert rc == 2 and not made and "(ODE) predictor only (cfg.predictor == 1)" in msg
    rc, msg, made = create(make_cfg(), 0)
    assert rc == 2 and not made and "n_problems == 0" in msg
    rc, msg, made = create(make_cfg(num_rollouts=4096, mpc_horizon=50), 4)               # FORM 0's tail: 64 x 52 = 3 328 words > 2 048
    assert rc == 2 and not made and "num_rollouts 4096, mpc_horizon 50, 50 inducing points x 1 inputs = 64 block records of 52 words" in msg
    assert "narrow in-launch hand-off" in msg
    rc, msg, made = create(make_cfg(num_rollouts=32768, mpc_horizon=10), 2)              # the throughput sizes
    assert rc == 2 and not made and "num_rollouts 32768" in msg and "throughput" in msg
    rc, msg, made = create(make_cfg(num_rollouts=64, mpc_horizon=1000), 2)               # LDS
    assert rc == 2 and not made and "160 KiB" in msg and "mpc_horizon 1000" in msg
    rc, msg, made = create(make_cfg(struct_size=8), 2)
    assert rc == 1 and not made and "size mismatch" in msg


def test_a_refused_creation_is_read_through_every_last_error():
    """the text of a refused creation is ONE thread-local of the library, whichever source file the family's host code is in: after a
    refused ctk_rpgd_batch_create every *_last_error(NULL) returns that text, and a refused ctk_create replaces it in all of them"""
    from control_toolkit_amd._capi import load_library
    lib, out = load_library(), ctypes.c_void_p()
    readers = ("ctk_rpgd_batch_last_error", "ctk_cem_batch_last_error", "ctk_batch_last_error", "ctk_mlp_batch_last_error", "ctk_last_error")
    cfg = make_cfg()
    assert lib.ctk_rpgd_batch_create(ctypes.byref(cfg), 0, None, ctypes.byref(out)) == 2 and not out.value
    texts = [getattr(lib, r)(None).decode() for r in readers]
    assert texts[0].startswith("ctk_rpgd_batch_create: a batch holds at least one problem (n_problems == 0)")
    assert texts == [texts[0]] * len(readers)
    bad = make_cfg(struct_size=8)
    assert lib.ctk_create(ctypes.byref(bad), ctypes.byref(out)) == 1 and not out.value
    texts = [getattr(lib, r)(None).decode() for r in readers]
    assert texts[0] == "ctk_create: ctk_config size mismatch (ABI)"
    assert texts == [texts[0]] * len(readers)


def test_handle_creation_failures_keep_their_code_text_and_null_handle():
    """ctk_create's own failure path: a refusal by configuration is read through every family's *_last_error(NULL); a valid
    configuration on a machine without a GPU fails at the device probe with CTK_ERR_NO_DEVICE (4) and its text; both leave *out NULL"""
    import torch
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    readers = ("ctk_last_error", "ctk_batch_last_error", "ctk_mlp_batch_last_error", "ctk_cem_batch_last_error", "ctk_rpgd_batch_last_error")
    out = ctypes.c_void_p(1)                                  # not NULL: the call itself must clear it
    bad = make_cfg(struct_size=8)
    assert lib.ctk_create(ctypes.byref(bad), ctypes.byref(out)) == 1 and out.value is None
    assert [getattr(lib, r)(None).decode() for r in readers] == ["ctk_create: ctk_config size mismatch (ABI)"] * len(readers)
    out = ctypes.c_void_p(1)
    cfg = make_cfg()
    rc = lib.ctk_create(ctypes.byref(cfg), ctypes.byref(out))
    if torch.cuda.is_available():                             # with a device the same call succeeds
        assert rc == 0 and out.value
        lib.ctk_destroy(out)
        return
    assert rc == 4 and out.value is None
    assert [getattr(lib, r)(None).decode() for r in readers] == ["ctk_create: no HIP device visible (libctk_hip has no CPU fallback)"] * len(readers)


def test_valid_batch_without_a_gpu_fails_loudly():
    import torch
    from control_toolkit_amd import CtkMppiBatch, CtkError
    if torch.cuda.is_available():
        b = CtkMppiBatch(3, **KW)                             # with a device the same call succeeds
        assert len(b) == 3 and b.samples_needed() == 256 * 20
        b.close()
        return
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiBatch(3, **KW)
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiBatch(3, seeds=[5, 6, 2 ** 63 + 1], environment="Quad2D", num_rollouts=64, mpc_horizon=10, dt=0.02)
    with pytest.raises(TypeError, match="unknown engine arguments"):
        CtkMppiBatch(3, nonsense=1, **KW)


# The public interface of the four batch classes, as it stood before they were given one base class: every public method of each class
# with str(inspect.signature(...)), the constructor among them.  A method that moves into the base keeps its name and signature here.
_CTOR_TAIL = ("num_rollouts: 'int', mpc_horizon: 'int', dt: 'float', action_low: 'float' = -1.0, action_high: 'float' = 1.0, "
              "period_interpolation_inducing_points: 'int' = 1, seed: 'int' = 0, device: 'int' = 0, intermediate_steps: 'int' = 1, "
              "materialize_trajectories: 'bool' = False, global_rollout_offset: 'int' = 0, num_states: 'int' = None, "
              "num_control_inputs: 'int' = None, generic_kernels: 'bool' = %s, **kw)")
_COMMON = {
    "close": "(self)",
    "dominant_kernel": "(self) -> 'str'",
    "get_param": "(self, name: 'str') -> 'float'",
    "get_problem_param": "(self, name: 'str', problem: 'int') -> 'float'",
    "get_problem_params": "(self, name: 'str') -> 'np.ndarray'",
    "get_state": "(self, problem: 'int') -> 'np.ndarray'",
    "params_differ": "(self) -> 'int'",
    "read": "(self, name: 'str', problem: 'int') -> 'np.ndarray'",
    "read_all": "(self, name: 'str') -> 'np.ndarray'",
    "rng_position": "(self, problem: 'int') -> 'int'",
    "set_param": "(self, name: 'str', value: 'float')",
    "set_problem_params": "(self, name: 'str', values, ids=None)",
    "set_rng_position": "(self, problem: 'int', call: 'int')",
    "set_state": "(self, problem: 'int', state)",
    "step": "(self, S, samples=None, u_prev=None, ids=None) -> 'np.ndarray'",
}
INTERFACE = {
    "CtkMppiBatch": dict(
        _COMMON, reset="(self, ids=None)", samples_needed="(self) -> 'int'",
        __init__="(self, num_problems: 'int', *, environment: 'str' = 'CartPole', seeds=None, optimizer: 'str' = 'mppi', "
                 "predictor: 'str' = 'ODE', " + _CTOR_TAIL % "False"),
    "CtkMppiMlpBatch": dict(
        _COMMON, reset="(self, ids=None)", samples_needed="(self) -> 'int'", have_weights="(self, problem: 'int') -> 'bool'",
        set_problem_weights="(self, W, ids=None)", set_weights="(self, w)", weight_count="(self) -> 'int'",
        __init__="(self, num_problems: 'int', *, seeds=None, predictor_hidden=None, environment: 'str' = 'CartPole', "
                 "optimizer: 'str' = 'mppi', predictor: 'str' = 'MLP', " + _CTOR_TAIL % "False"),
    "CtkCemBatch": dict(
        _COMMON, reset="(self, ids=None)", samples_needed="(self, problem: 'int' = 0) -> 'int'",
        __init__="(self, num_problems: 'int', *, environment: 'str' = 'CartPole', seeds=None, optimizer: 'str' = 'cem', "
                 "predictor: 'str' = 'ODE', " + _CTOR_TAIL % "False"),
    "CtkRpgdBatch": dict(
        _COMMON, reset="(self, draws=None, ids=None)", samples_needed="(self, problem: 'int' = 0) -> 'int'",
        samples_needed_reset="(self) -> 'int'", state_size="(self) -> 'int'", descent_lds="(environment: 'str', mpc_horizon: 'int')",
        __init__="(self, num_problems: 'int', *, environment: 'str' = 'CartPole', seeds=None, optimizer: 'str' = 'rpgd', "
                 "predictor: 'str' = 'ODE', " + _CTOR_TAIL % "None"),
}


@pytest.mark.parametrize("cname", sorted(INTERFACE))
def test_public_interface_of_the_batch_classes_is_pinned(cname):
    import inspect
    from control_toolkit_amd import _capi
    cls = getattr(_capi, cname)
    have = {n: str(inspect.signature(getattr(cls, n))) for n in dir(cls) if (not n.startswith("_") or n == "__init__") and callable(getattr(cls, n))}
    assert set(have) == set(INTERFACE[cname]), sorted(set(have) ^ set(INTERFACE[cname]))
    for n, sig in INTERFACE[cname].items():
        assert have[n] == sig, f"{cname}.{n}: {have[n]}"
    assert issubclass(_capi.CtkMppiMlpBatch, _capi.CtkMppiBatch)
