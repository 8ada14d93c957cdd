"""CPU tests (-m "not gpu") of the batched MPPI with the GRU predictor (control_toolkit_amd._capi.CtkMppiGruBatch, include/ctk_hip.h:
ctk_gru_batch_* / ctk_gru_problem_*, include/ctk_hip_gru.h: its closed-loop entries): the family is declared, bound and exported beside
the existing ones, which are what they were — their refusal of the GRU included; what needs no device is refused BEFORE the library is
asked for one; the library's own refusals that depend on the configuration alone come before its device probe; the fit takes a handle's
form at every size, with the expected form computed here from ctk_launch.h's ctk_ll_records_ok / ctk_ll_tail_wide; without a GPU a
valid construction fails loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
GRU_HEADER = os.path.join(ROOT, "include", "ctk_hip_gru.h")
LAUNCH = os.path.join(ROOT, "control_toolkit_amd", "csrc", "ctk_launch.h")
KW = dict(num_rollouts=256, mpc_horizon=20, dt=0.02)
SHARED = ["create", "destroy", "last_error", "size", "samples_needed", "step", "reset", "read", "get_state", "set_state", "set_param",
          "get_param", "rng_get_position", "rng_set_position", "dominant_kernel"]
BATCH = SHARED + ["weight_count", "set_weights", "fit"]
PROBLEM = ["set_param", "get_param", "params_differ", "set_weights", "have_weights", "get_hidden", "set_hidden"]
LOOP = ["plant_set_param", "plant_get_param", "plant_clear_params", "plant_step", "run", "plant_set_noise", "plant_get_noise",
        "plant_clear_noise", "plant_set_noise_seed", "plant_get_noise_seed", "plant_noise_get_position", "plant_noise_set_position",
        "plant_step_noisy", "episodes"]
SIZES_IN_MSG = "num_rollouts 256, mpc_horizon 20, 20 inducing points, network 5IN-32H1-32H2-4OUT"


def header_names(pattern, path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(pattern, src)))


def test_class_is_exported():
    import control_toolkit_amd
    from control_toolkit_amd._capi import CtkMppiGruBatch, CtkMppiBatch, CtkMppiMlpBatch
    assert control_toolkit_amd.CtkMppiGruBatch is CtkMppiGruBatch and "CtkMppiGruBatch" in control_toolkit_amd.__all__
    assert issubclass(CtkMppiGruBatch, CtkMppiBatch) and (CtkMppiGruBatch._BATCH, CtkMppiGruBatch._PROBLEM) == ("ctk_gru_batch", "ctk_gru_problem")
    for m in ("step", "reset", "read", "read_all", "get_state", "set_state", "set_param", "get_param", "set_problem_params", "get_problem_param",
              "get_problem_params", "params_differ", "rng_position", "set_rng_position", "dominant_kernel", "samples_needed", "close",
              "weight_count", "set_weights", "set_problem_weights", "have_weights", "get_hidden", "set_hidden"):
        assert callable(getattr(CtkMppiGruBatch, m)), m
    assert isinstance(CtkMppiGruBatch.closed_loop, property)
    for other in (CtkMppiBatch, CtkMppiMlpBatch):                                # the other batches are what they were
        assert not hasattr(other, "get_hidden") and not hasattr(other, "set_hidden")


def test_every_symbol_is_declared_bound_and_exported():
    from control_toolkit_amd._capi import load_library, SYMBOLS, GRU_LOOP_SYMBOLS, RUN_SYMBOLS, EPISODE_SYMBOLS, LOOP_SYMBOLS
    batch = header_names(r"\b(ctk_gru_batch_[a-z_0-9]+)\s*\(")
    problem = header_names(r"\b(ctk_gru_problem_[a-z_0-9]+)\s*\(")
    loop = header_names(r"\b(ctk_[a-z_0-9]+)\s*\(", GRU_HEADER)
    assert batch == sorted("ctk_gru_batch_" + n for n in BATCH)
    assert problem == sorted("ctk_gru_problem_" + n for n in PROBLEM)
    assert loop == sorted("ctk_gru_batch_" + n for n in LOOP) == sorted(GRU_LOOP_SYMBOLS)
    assert not set(GRU_LOOP_SYMBOLS) & (set(SYMBOLS) | set(RUN_SYMBOLS) | set(EPISODE_SYMBOLS) | set(LOOP_SYMBOLS))
    assert re.search(r'^#include "ctk_hip_gru.h"', open(HEADER).read(), flags=re.M)        # a caller includes one header
    lib = load_library()
    for n in batch + problem + loop:
        res, args = SYMBOLS[n] if n in SYMBOLS else GRU_LOOP_SYMBOLS[n]
        fn = getattr(lib, n)                                 # AttributeError: not exported
        assert fn.argtypes is not None and list(fn.argtypes) == list(args) and fn.restype == res, n
    # the signatures are those of the MLP family, entry by entry
    for n in SHARED + ["weight_count", "set_weights"]:
        assert SYMBOLS["ctk_gru_batch_" + n] == SYMBOLS["ctk_mlp_batch_" + n], n
    for n in PROBLEM[:5]:
        assert SYMBOLS["ctk_gru_problem_" + n] == SYMBOLS["ctk_mlp_problem_" + n], n
    both = dict(RUN_SYMBOLS, **EPISODE_SYMBOLS)
    for n in LOOP:
        assert GRU_LOOP_SYMBOLS["ctk_gru_batch_" + n] == both["ctk_mlp_batch_" + n], n
    assert len(SYMBOLS["ctk_gru_problem_get_hidden"][1]) == 4 and len(SYMBOLS["ctk_gru_problem_set_hidden"][1]) == 4
    # NULL handles answer like the other families'
    assert lib.ctk_gru_batch_size(None) == 0 and lib.ctk_gru_batch_weight_count(None) == 0 and lib.ctk_gru_problem_have_weights(None, 0) == 0
    assert lib.ctk_gru_batch_set_weights(None, None, 0) == 1 and lib.ctk_gru_batch_step(None, 0, None, None, None, None, 0, None) == 1
    assert lib.ctk_gru_problem_get_hidden(None, 0, None, None) == 1 and lib.ctk_gru_problem_set_hidden(None, 0, None, None) == 1
    assert lib.ctk_gru_batch_run(None, 0, None, None, None, 1, 0, None, None, None) == 1


def test_the_existing_families_are_what_they_were():
    from control_toolkit_amd._capi import load_library
    assert len(header_names(r"\b(ctk_batch_[a-z_0-9]+)\s*\(")) == 15
    assert len(header_names(r"\b(ctk_mlp_batch_[a-z_0-9]+)\s*\(")) == 17 and len(header_names(r"\b(ctk_mlp_problem_[a-z_0-9]+)\s*\(")) == 5
    for fam in ("ctk_problem_", "ctk_cem_problem_", "ctk_rpgd_problem_"):
        assert len(header_names(rf"\b({fam}[a-z_0-9]+)\s*\(")) == 3, fam
    assert load_library().ctk_abi_version() == 6            # additive: the ABI version stays
    assert re.search(r"CTK_ABI_VERSION 6\b", open(HEADER).read())


def make_cfg(**over):
    from control_toolkit_amd import _capi
    kw = dict(KW)
    kw.update({k: over.pop(k) for k in list(over) if k in ("num_rollouts", "mpc_horizon", "dt")})
    period = over.pop("period", 1)
    name = over.pop("env", "CartPole")
    S, Cn, _ = _capi.environment_info(name)
    env = (name, _capi.environment_library(name)[1], S, Cn)
    cfg = _capi._make_config("mppi", "GRU", env[1], env[0], env[3], action_low=-1.0, action_high=1.0, period_interpolation_inducing_points=period,
                             seed=0, device=0, intermediate_steps=1, materialize_trajectories=False, global_rollout_offset=0, num_states=env[2],
                             num_control_inputs=env[3], generic_kernels=False, **kw)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg, n, family="ctk_gru_batch"):
    from control_toolkit_amd._capi import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    rc = getattr(lib, family + "_create")(ctypes.byref(cfg), n, None, ctypes.byref(out))
    msg = getattr(lib, family + "_last_error")(None).decode()
    if out.value:
        getattr(lib, family + "_destroy")(out)
    return rc, msg, bool(out.value)


def test_the_other_families_still_refuse_the_gru():
    """byte for byte the messages they had: the C entries and the classes"""
    from control_toolkit_amd import CtkMppiBatch, CtkMppiMlpBatch
    rc, msg, made = create(make_cfg(), 4, "ctk_batch")
    assert rc == 2 and not made
    assert msg == ("ctk_batch_create: the batch kernel rolls out the analytic (ODE) predictor only (cfg.predictor == 2); network predictors run as "
                   "single handles (ctk_create)")
    rc, msg, made = create(make_cfg(), 4, "ctk_mlp_batch")
    assert rc == 2 and not made
    assert msg == ("ctk_mlp_batch_create: this family rolls out the MLP predictor only (cfg.predictor == 2); the GRU's carried hidden state has no "
                   "batch form, such a controller runs as a single handle (ctk_create) (" + SIZES_IN_MSG + ")")
    with pytest.raises(NotImplementedError, match=r"analytic \(ODE\) predictor only \(predictor 'GRU'\)"):
        CtkMppiBatch(4, predictor="GRU", **KW)
    with pytest.raises(NotImplementedError, match="the GRU's carried hidden state has no batch form"):
        CtkMppiMlpBatch(4, predictor="GRU", **KW)


def test_constructor_refuses_before_any_device_is_touched(monkeypatch):
    from control_toolkit_amd import _capi
    from control_toolkit_amd._capi import CtkMppiGruBatch

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_capi, "environment_library", no_library)
    monkeypatch.setattr(_capi, "load_library", no_library)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one problem"):
            CtkMppiGruBatch(bad, **KW)
    with pytest.raises(ValueError, match=r"one entry per problem \(4\), got 3"):
        CtkMppiGruBatch(4, seeds=[1, 2, 3], **KW)
    for opt in ("cem", "rpgd"):
        with pytest.raises(NotImplementedError, match="MPPI controllers only"):
            CtkMppiGruBatch(4, optimizer=opt, **KW)
    with pytest.raises(NotImplementedError, match="CtkMppiBatch"):
        CtkMppiGruBatch(4, predictor="ODE", **KW)
    with pytest.raises(NotImplementedError, match="CtkMppiMlpBatch"):
        CtkMppiGruBatch(4, predictor="MLP", **KW)
    with pytest.raises(NotImplementedError, match="CartPole"):
        CtkMppiGruBatch(4, environment="Quad2D", **KW)
    with pytest.raises(NotImplementedError, match="generic_kernels True"):
        CtkMppiGruBatch(4, generic_kernels=True, **KW)
    with pytest.raises(NotImplementedError, match=r"32 units per hidden layer \(predictor_hidden \(33, 32\)\)"):
        CtkMppiGruBatch(4, predictor_hidden=(33, 32), **KW)
    for bad in ((8,), (8, 0), (1, 2, 3)):
        with pytest.raises(ValueError, match="two widths"):
            CtkMppiGruBatch(4, predictor_hidden=bad, **KW)


def test_weight_count_arithmetic():
    from oracle import ctk_oracle as O
    from control_toolkit_amd._capi import gru_weight_count
    assert gru_weight_count(4, 1) == O.gru_num_weights() == 10212
    a, b = 8, 20
    assert gru_weight_count(4, 1, (a, b)) == (3 * a * 5 + 3 * a * a + 6 * a) + (3 * b * a + 3 * b * b + 6 * b) + (b * 4 + 4)


def test_library_refuses_by_configuration_before_it_probes_the_device():
    """every refusal is CTK_ERR_UNSUPPORTED (2) with the sizes in the message; none of these needs a GPU"""
    rc, msg, made = create(make_cfg(optimizer=1), 4)
    assert rc == 2 and not made and "ctk_gru_batch_create: a batch steps MPPI controllers only (cfg.optimizer == 1)" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor=0), 4)
    assert rc == 2 and not made and "ctk_gru_batch_create" in msg and "cfg.predictor == 0" in msg and "use ctk_batch_create" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor=1), 4)
    assert rc == 2 and not made and "cfg.predictor == 1" in msg and "use ctk_mlp_batch_create" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(env="Quad2D"), 4)
    assert rc == 2 and not made and "environment Quad2D" in msg and "template network kernels" in msg and "num_rollouts 256" in msg
    rc, msg, made = create(make_cfg(generic_kernels=1), 4)
    assert rc == 2 and not made and "generic_kernels == 1" in msg and "template network kernels" in msg and SIZES_IN_MSG in msg
    rc, msg, made = create(make_cfg(predictor_hidden1=33), 4)
    assert rc == 2 and not made and "1 to 32 units per hidden layer" in msg and "network 5IN-33H1-32H2-4OUT" in msg
    rc, msg, made = create(make_cfg(predictor_hidden2=64), 4)
    assert rc == 2 and not made and "network 5IN-32H1-64H2-4OUT" in msg
    rc, msg, made = create(make_cfg(predictor_hidden1=-1), 4)
    assert rc == 2 and not made and "1 to 32 units per hidden layer" in msg and "network 5IN--1H1-32H2-4OUT" in msg
    rc, msg, made = create(make_cfg(), 0)
    assert rc == 2 and not made and "ctk_gru_batch_create" in msg and "n_problems == 0" in msg
    # the fit: 16 rollouts per block record here; a handle of this size runs rollout, merge and update as separate launches
    rc, msg, made = create(make_cfg(num_rollouts=8192, mpc_horizon=20), 2)
    assert rc == 2 and not made and "ctk_gru_batch_create" in msg
    assert "num_rollouts 8192, mpc_horizon 20, 20 inducing points x 1 inputs = 512 block records of 22 words" in msg
    assert "does not hand its block records over in-launch" in msg
    rc, msg, made = create(make_cfg(num_rollouts=16 * 513, mpc_horizon=1), 2)          # 513 records
    assert rc == 2 and not made and "513 block records of 3 words" in msg
    rc, msg, made = create(make_cfg(num_rollouts=64, mpc_horizon=1000), 2)             # LDS
    assert rc == 2 and not made and "160 KiB" in msg and "mpc_horizon 1000" in msg
    rc, msg, made = create(make_cfg(struct_size=8), 2)
    assert rc == 1 and not made and "ctk_gru_batch_create: ctk_config size mismatch" in msg


# ---- the fit against the two predicates a handle's launch uses (ctk_launch.h), restated here over the constants parsed from that header ----
def launch_constants():
    src = open(LAUNCH).read()

    def const(name):
        m = re.search(rf"\b{name}\s*=\s*([0-9 *]+)[,;]", src)
        assert m, name
        return eval(m.group(1))                               # "128" or "8 * 256"
    return {n: const(n) for n in ("CTK_MPPI_FUSE_MAX_BLOCKS_LL", "CTK_MPPI_FUSE_MAX_BLOCKS_LL_NARROW", "CTK_MPPI_FUSE_MAX_WORDS_LL_NARROW",
                                  "CTK_MPPI_LL_NARROW_WORDS")}


def ll_records_ok(k, blocks, cols):                           # ctk_launch.h: ctk_ll_records_ok
    return blocks <= k["CTK_MPPI_FUSE_MAX_BLOCKS_LL"] or (blocks <= k["CTK_MPPI_FUSE_MAX_BLOCKS_LL_NARROW"] and
                                                          blocks * (2 + cols) <= k["CTK_MPPI_FUSE_MAX_WORDS_LL_NARROW"])


def ll_tail_wide(k, blocks, cols):                            # ctk_launch.h: ctk_ll_tail_wide
    return blocks > k["CTK_MPPI_FUSE_MAX_BLOCKS_LL"] or blocks * (2 + cols) > k["CTK_MPPI_LL_NARROW_WORDS"]


# (N, H, period): the GPU tests' sizes, the sizes beside the tail switch, a shard of configs[4] (256 narrow records), the refused ones
FIT_SIZES = [(16, 5, 2), (70, 12, 5), (1024, 30, 1), (1024, 31, 1), (1024, 50, 1), (2048, 40, 10), (4096, 14, 1), (8192, 20, 1), (8208, 1, 1)]


def test_the_fit_takes_a_handles_form():
    from control_toolkit_amd._capi import gru_batch_fit, load_library
    k = launch_constants()
    assert k == {"CTK_MPPI_FUSE_MAX_BLOCKS_LL": 128, "CTK_MPPI_FUSE_MAX_BLOCKS_LL_NARROW": 512, "CTK_MPPI_FUSE_MAX_WORDS_LL_NARROW": 4096,
                 "CTK_MPPI_LL_NARROW_WORDS": 2048}
    for N, H, p in FIT_SIZES:
        fits, blocks, words, wide, lds = gru_batch_fit(N, H, p)
        P = words - 2
        assert blocks == -(-N // 16) and 1 <= P <= H and (p > 1 or P == H), (N, H, p)
        assert fits == ll_records_ok(k, blocks, P), (N, H, p)               # (none of these sizes is near the LDS limits)
        assert wide == (fits and ll_tail_wide(k, blocks, P)), (N, H, p)
        assert not fits or 0 < lds <= 160 * 1024
    # the cases by name
    assert gru_batch_fit(1024, 50, 1)[:4] == (True, 64, 52, True)           # the headline size: 3 328 words, the wide tail
    assert gru_batch_fit(1024, 30, 1)[:4] == (True, 64, 32, False)          # 64 x 32 = 2 048 words: the last narrow one
    assert gru_batch_fit(1024, 31, 1)[:4] == (True, 64, 33, True)
    fits, blocks, words, wide, _ = gru_batch_fit(2048, 40, 10)
    assert fits and blocks == 128 and wide == ll_tail_wide(k, 128, words - 2)
    assert gru_batch_fit(8192, 20, 1)[:3] == (False, 512, 22)
    with pytest.raises(ValueError):
        gru_batch_fit(0, 20, 1)
    assert load_library().ctk_gru_batch_fit(1024, 50, 1, None, None, None, None) == 0       # every out pointer may be NULL
    assert load_library().ctk_gru_batch_fit(8192, 20, 1, None, None, None, None) == 2


def test_creation_follows_the_fit():
    """every size the fit accepts passes the configuration checks (what is left to fail without a GPU is the device probe, which comes behind
    them); every size it refuses is CTK_ERR_UNSUPPORTED"""
    import torch
    from control_toolkit_amd._capi import gru_batch_fit
    for N, H, p in FIT_SIZES:
        rc, msg, made = create(make_cfg(num_rollouts=N, mpc_horizon=H, period=p), 3)
        if not gru_batch_fit(N, H, p)[0]:
            assert rc == 2 and not made and f"num_rollouts {N}" in msg, (N, H, p, msg)
        elif torch.cuda.is_available():
            assert rc == 0 and made, msg
        else:
            assert rc == 4 and not made and "no HIP device" in msg, (N, H, p, msg)


def test_valid_batch_without_a_gpu_fails_loudly():
    import torch
    from control_toolkit_amd import CtkMppiGruBatch, CtkError
    if torch.cuda.is_available():
        b = CtkMppiGruBatch(3, **KW)                          # with a device the same call succeeds
        assert len(b) == 3 and b.samples_needed() == 256 * 20 and b.weight_count() == 10212 and not b.have_weights(0)
        assert b.get_hidden().shape == (3, 2, 32) and not b.get_hidden().any()
        b.close()
        return
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiGruBatch(3, **KW)
    with pytest.raises(CtkError, match="no HIP device|No HIP|no CPU fallback"):
        CtkMppiGruBatch(3, seeds=[5, 6, 2 ** 63 + 1], predictor_hidden=(8, 20), num_rollouts=64, mpc_horizon=10, dt=0.02)
    with pytest.raises(TypeError, match="unknown engine arguments"):
        CtkMppiGruBatch(3, nonsense=1, **KW)
