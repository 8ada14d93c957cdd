"""ctypes binding of include/ctk_hip.h (the stub a reference maintainer would add; the reference's
own precedent for a ctypes boundary is Controllers/controller_C.py:261-274).

Fails loudly: if libctk_hip.so is missing or cannot be loaded, importing the engine raises; if
no gfx950 device is usable, `CtkEngine(...)` raises.  Nothing here computes on the CPU."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libctk_hip.so"
_lib = None

OPTIMIZERS = {"mppi": 0, "cem": 1, "rpgd": 2, "random_action": 3, "gradient": 4, "cem_naive_grad": 5,
              "cem_grad_bharadhwaj": 6, "cem_gmm": 7}
PREDICTORS = {"ODE": 0, "MLP": 1, "GRU": 2}
ENVIRONMENTS = {"CartPole": 0, "Quad2D": 1, "Hover": 2}          # include/ctk_hip.h: enum ctk_environment
MAX_STATES, MAX_INPUTS = 8, 4
# CartPole's parameter names in id order (enum ctk_param); `environment_params(name)` asks the library for any environment's
PARAMS = ("g", "m_cart", "m_pole", "L", "u_max", "M_fric", "J_fric", "target_position", "target_equilibrium",
          "dd_weight", "ep_weight", "ekp_weight", "cc_weight", "ccrc_weight", "R", "x_scale", "terminal_weight")
BUFFERS = {"Q": 0, "J": 1, "TRAJ": 2, "U_NOM": 3, "STD": 4, "ADAM_M": 5, "ADAM_V": 6, "AGES": 7, "BEST_IDX": 8, "PLAN": 9, "AGES_LOGGED": 10,
           "MIX_MU": 11, "MIX_STD": 12, "MIX_PROB": 13, "MIX_LABEL": 14}   # CEM-GMM (include/ctk_hip.h: enum ctk_buffer)
LOC_NONE, LOC_HOST, LOC_DEVICE = 0, 1, 2
MLP_NUM_WEIGHTS = 1380


class CtkError(RuntimeError):
    pass


class CtkConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("optimizer", C.c_int32), ("predictor", C.c_int32), ("device", C.c_int32),
        ("num_rollouts", C.c_int32), ("mpc_horizon", C.c_int32), ("num_states", C.c_int32),
        ("num_control_inputs", C.c_int32), ("period_interpolation_inducing_points", C.c_int32),
        ("intermediate_steps", C.c_int32), ("materialize_trajectories", C.c_int32),
        ("global_rollout_offset", C.c_int32), ("seed", C.c_uint64), ("dt", C.c_float),
        ("environment", C.c_int32), ("generic_kernels", C.c_int32),
        ("action_low", C.c_float * MAX_INPUTS), ("action_high", C.c_float * MAX_INPUTS),
        ("cc_weight", C.c_float), ("R", C.c_float), ("LBD", C.c_float), ("NU", C.c_float), ("SQRTRHOINV", C.c_float),
        ("cem_outer_it", C.c_int32), ("cem_best_k", C.c_int32), ("warmup", C.c_int32), ("warmup_iterations", C.c_int32),
        ("cem_initial_action_stdev", C.c_float), ("cem_stdev_min", C.c_float),
        ("outer_its", C.c_int32), ("resamp_per", C.c_int32), ("shift_previous", C.c_int32), ("opt_keep_k", C.c_int32),
        ("sampling_distribution", C.c_int32), ("sample_whole_control_space", C.c_int32),
        ("sample_stdev", C.c_float), ("sample_mean", C.c_float), ("sample_min", C.c_float), ("sample_max", C.c_float),
        ("learning_rate", C.c_float), ("gradmax_clip", C.c_float), ("adam_beta_1", C.c_float),
        ("adam_beta_2", C.c_float), ("adam_epsilon", C.c_float), ("adam_rule", C.c_int32),
        ("predictor_hidden1", C.c_int32), ("predictor_hidden2", C.c_int32),
    ]


def library_path() -> str:
    """The in-tree product library.  CTK_HIP_LIBRARY points a diagnostic run (tools/rpgd_split.sh: timing variants whose
    results are meaningless) at another build WITHOUT touching the product file; it is announced on stderr so that a test or
    bench line can never be attributed to the product library by mistake."""
    override = os.environ.get("CTK_HIP_LIBRARY")
    if override:
        import sys
        print(f"[ctk] CTK_HIP_LIBRARY override: loading {override} instead of the product library", file=sys.stderr)
        return override
    return os.path.join(_HERE, _LIB_NAME)


# every symbol include/ctk_hip.h declares: name -> (restype, argtypes)
_FP = C.POINTER(C.c_float)
_H = C.c_void_p
SYMBOLS = {
    "ctk_abi_version": (C.c_int, []),
    "ctk_create": (C.c_int, [C.POINTER(CtkConfig), C.POINTER(_H)]),
    "ctk_destroy": (None, [_H]),
    "ctk_reset": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "ctk_last_error": (C.c_char_p, [_H]),
    "ctk_set_stream": (C.c_int, [_H, C.c_void_p]),
    "ctk_get_stream": (C.c_void_p, [_H]),
    "ctk_set_param": (C.c_int, [_H, C.c_int, C.c_float]),
    "ctk_get_param": (C.c_int, [_H, C.c_int, _FP]),
    "ctk_env_info": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ctk_param_name": (C.c_char_p, [C.c_int, C.c_int]),
    "ctk_environment_name": (C.c_char_p, [C.c_int]),
    "ctk_param_default": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "ctk_predictor_weight_count": (C.c_size_t, [_H]),
    "ctk_set_predictor_weights": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_predictor_weight_count_shaped": (C.c_size_t, [_H, C.c_int, C.c_int]),
    "ctk_set_predictor_weights_shaped": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "ctk_predictor_hidden_size": (C.c_size_t, [_H]),
    "ctk_predictor_update": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "ctk_predictor_get_hidden": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_predictor_set_hidden": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_samples_needed": (C.c_size_t, [_H]),
    "ctk_rng_get_position": (C.c_int, [_H, C.POINTER(C.c_uint32)]),
    "ctk_rng_set_position": (C.c_int, [_H, C.c_uint32]),
    "ctk_rollout": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ctk_mppi_partial_size": (C.c_size_t, [_H]),
    "ctk_mppi_step_begin": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_mppi_step_end": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_shard_candidates_size": (C.c_size_t, [_H]),
    "ctk_shard_iterations": (C.c_int, [_H]),
    "ctk_shard_iter_begin": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_shard_iter_end": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "ctk_shard_finish": (C.c_int, [_H, C.c_void_p]),
    "ctk_rpgd_keepers_size": (C.c_size_t, [_H]),
    "ctk_rpgd_fresh_rows": (C.c_size_t, [_H, C.c_int]),
    "ctk_rpgd_step_begin": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ctk_rpgd_step_end": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_read": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ctk_state_size": (C.c_size_t, [_H]),
    "ctk_get_state": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_set_state": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_profile_enable": (C.c_int, [_H, C.c_int]),
    "ctk_profile_read": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ctk_dominant_kernel": (C.c_char_p, [_H]),
    "ctk_p2p_alloc": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "ctk_p2p_connect": (C.c_int, [_H, C.c_void_p]),
    "ctk_p2p_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ctk_p2p_close": (C.c_int, [_H]),
    "ctk_log_enable": (C.c_int, [_H, C.c_size_t]),
    "ctk_log_count": (C.c_size_t, [_H]),
    "ctk_log_read": (C.c_int, [_H, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ctk_resident_enable": (C.c_int, [_H, C.c_int, C.c_double]),
    "ctk_resident_stop": (C.c_int, [_H]),
    "ctk_resident_stats": (C.c_int, [_H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}

# the five batch families (ctk_batch_*, ctk_mlp_batch_*, ctk_gru_batch_*, ctk_cem_batch_*, ctk_rpgd_batch_*; _H is the family's batch
# pointer there): the signatures they share under a family's (batch prefix, problem prefix), then what differs, by name
_BATCH_FAMILIES = (("ctk_batch", "ctk_problem"), ("ctk_mlp_batch", "ctk_mlp_problem"), ("ctk_gru_batch", "ctk_gru_problem"),
                   ("ctk_cem_batch", "ctk_cem_problem"), ("ctk_rpgd_batch", "ctk_rpgd_problem"))
_BATCH_SHARED = {
    "create": (C.c_int, [C.POINTER(CtkConfig), C.c_int, C.c_void_p, C.POINTER(_H)]),
    "destroy": (None, [_H]),
    "last_error": (C.c_char_p, [_H]),
    "size": (C.c_int, [_H]),
    "samples_needed": (C.c_size_t, [_H]),
    "step": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "reset": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "read": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "get_state": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_size_t]),
    "set_state": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_size_t]),
    "set_param": (C.c_int, [_H, C.c_int, C.c_float]),
    "get_param": (C.c_int, [_H, C.c_int, _FP]),
    "rng_get_position": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint32)]),
    "rng_set_position": (C.c_int, [_H, C.c_int, C.c_uint32]),
    "dominant_kernel": (C.c_char_p, [_H]),
}
_PROBLEM_SHARED = {                                   # per-problem parameters of a batch (the batch pointer again)
    "set_param": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "get_param": (C.c_int, [_H, C.c_int, C.c_int, _FP]),
    "params_differ": (C.c_int, [_H]),
}
for _batch, _problem in _BATCH_FAMILIES:
    SYMBOLS.update({f"{_batch}_{name}": sig for name, sig in _BATCH_SHARED.items()})
    SYMBOLS.update({f"{_problem}_{name}": sig for name, sig in _PROBLEM_SHARED.items()})
SYMBOLS.update({
    # the draws of a CEM or RPGD problem's next step depend on the problem
    "ctk_cem_batch_samples_needed": (C.c_size_t, [_H, C.c_int]),
    "ctk_rpgd_batch_samples_needed": (C.c_size_t, [_H, C.c_int]),
    # an RPGD step takes the count of the caller's samples, an RPGD reset draws
    "ctk_rpgd_batch_step": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "ctk_rpgd_batch_reset": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "ctk_rpgd_template_descent_lds": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    # the networks of the MLP family
    "ctk_mlp_batch_weight_count": (C.c_size_t, [_H]),
    "ctk_mlp_batch_set_weights": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_mlp_problem_set_weights": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "ctk_mlp_problem_have_weights": (C.c_int, [_H, C.c_int]),
    # the networks and carried hidden states of the GRU family; its fit needs no batch
    "ctk_gru_batch_weight_count": (C.c_size_t, [_H]),
    "ctk_gru_batch_set_weights": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ctk_gru_problem_set_weights": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "ctk_gru_problem_have_weights": (C.c_int, [_H, C.c_int]),
    "ctk_gru_problem_get_hidden": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "ctk_gru_problem_set_hidden": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "ctk_gru_batch_fit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
})

# closed-loop episodes of the MPPI batches on the device (include/ctk_hip_run.h, which ctk_hip.h includes): the same table for the entry
# points declared there; _bind_library binds both
_PLANT_RUN = {
    "plant_set_param": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "plant_get_param": (C.c_int, [_H, C.c_int, C.c_int, _FP]),
    "plant_clear_params": (C.c_int, [_H]),
    "plant_step": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "run": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
RUN_SYMBOLS = {f"{family}_{name}": sig for family in ("ctk_batch", "ctk_mlp_batch") for name, sig in _PLANT_RUN.items()}

# stochastic closed-loop episodes with the realised cost (include/ctk_hip_episode.h, which ctk_hip.h includes): a third table, bound with
# the other two
_PLANT_EPISODE = {
    "plant_set_noise": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "plant_get_noise": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "plant_clear_noise": (C.c_int, [_H]),
    "plant_set_noise_seed": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "plant_get_noise_seed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint64)]),
    "plant_noise_get_position": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint32)]),
    "plant_noise_set_position": (C.c_int, [_H, C.c_int, C.c_uint32]),
    "plant_step_noisy": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "episodes": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p]),
}
EPISODE_SYMBOLS = {f"{family}_{name}": sig for family in ("ctk_batch", "ctk_mlp_batch") for name, sig in _PLANT_EPISODE.items()}

# the same closed loops for the CEM and RPGD batches (include/ctk_hip_loop.h, which ctk_hip.h includes): the entries of the two tables
# above under these families' names, with the same signatures; a fourth table, bound with the other three
LOOP_SYMBOLS = {f"{family}_{name}": sig for family in ("ctk_cem_batch", "ctk_rpgd_batch")
                for name, sig in list(_PLANT_RUN.items()) + list(_PLANT_EPISODE.items())}

# ... and for the GRU batch (include/ctk_hip_gru.h, which ctk_hip.h includes): a fifth table, bound with the other four
GRU_LOOP_SYMBOLS = {f"ctk_gru_batch_{name}": sig for name, sig in list(_PLANT_RUN.items()) + list(_PLANT_EPISODE.items())}

# per-problem MPPI hyper-parameters and input limits of the three MPPI batches (include/ctk_hip_hyper.h, which ctk_hip.h includes): a
# sixth table, bound with the other five.  HYPERS: enum ctk_hyper.
HYPERS = {"cc_weight": 0, "R": 1, "LBD": 2, "NU": 3, "SQRTRHOINV": 4}
_PROBLEM_HYPER = {
    "set_hyper": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "get_hyper": (C.c_int, [_H, C.c_int, C.c_int, _FP]),
    "set_limits": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "get_limits": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p]),
    "hypers_differ": (C.c_int, [_H]),
}
HYPER_SYMBOLS = {}
for _batch, _problem in _BATCH_FAMILIES[:3]:
    HYPER_SYMBOLS.update({f"{_problem}_{name}": sig for name, sig in _PROBLEM_HYPER.items()})
    HYPER_SYMBOLS[f"{_batch}_set_hyper"] = (C.c_int, [_H, C.c_int, C.c_float])

# per-problem hyper-parameters and input limits of the CEM and RPGD batches (include/ctk_hip_family_hyper.h, which ctk_hip.h includes): a
# table of its own, bound with the others.  CEM_HYPERS: enum ctk_cem_hyper; RPGD_HYPERS: enum ctk_rpgd_hyper.  The counts cross the ABI
# as floats and must be integral (_FAMILY_COUNTS).
CEM_HYPERS = {"cem_best_k": 0, "cem_initial_action_stdev": 1, "cem_stdev_min": 2, "cem_outer_it": 3}
RPGD_HYPERS = {"learning_rate": 0, "adam_beta_1": 1, "adam_beta_2": 2, "adam_epsilon": 3, "gradmax_clip": 4, "sample_stdev": 5, "sample_mean": 6,
               "uniform_dist_min": 7, "uniform_dist_max": 8, "outer_its": 9, "resamp_per": 10}
_FAMILY_HYPERS = {"cem": CEM_HYPERS, "rpgd": RPGD_HYPERS}
_FAMILY_COUNTS = {"cem_best_k": 1, "cem_outer_it": 1, "outer_its": 0, "resamp_per": 1}        # name -> the smallest admissible value
FAMILY_HYPER_SYMBOLS = {}
for _batch, _problem in _BATCH_FAMILIES[3:]:
    FAMILY_HYPER_SYMBOLS.update({f"{_problem}_{name}": sig for name, sig in _PROBLEM_HYPER.items()})
    FAMILY_HYPER_SYMBOLS[f"{_batch}_set_hyper"] = (C.c_int, [_H, C.c_int, C.c_float])


# rollouts of caller-supplied plans on every batch family (include/ctk_hip_rollout.h, which ctk_hip.h includes): one signature under the
# five families' names; a table of its own, bound with the others.  ROLLOUT_MODELS: enum ctk_rollout_model.
ROLLOUT_MODELS = {"controller": 0, "plant": 1}
_BATCH_ROLLOUT = (C.c_int, [_H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
ROLLOUT_SYMBOLS = {f"{_batch}_rollout": _BATCH_ROLLOUT for _batch, _problem in _BATCH_FAMILIES}


# the launched-ahead form of the MPPI step (include/ctk_hip_ahead.h, which ctk_hip.h includes): a table of its own, bound with the others
class AheadRule(C.Structure):
    _fields_ = [("streak", C.c_int32), ("armed", C.c_int32), ("untaken", C.c_int32), ("arms", C.c_int32)]


class AheadCounters(C.Structure):
    _fields_ = [("launched", C.c_uint64), ("taken", C.c_uint64), ("untaken", C.c_uint64), ("cancelled", C.c_uint64), ("arms", C.c_uint64),
                ("armed", C.c_int32), ("pending", C.c_int32), ("available", C.c_int32), ("on", C.c_int32)]


AHEAD_ARM_AFTER, AHEAD_DISARM_AFTER, AHEAD_DEFAULT_FUSE_US = 8, 2, 20.0
AHEAD_NONE, AHEAD_TAKEN, AHEAD_UNTAKEN = 0, 1, 2
AHEAD_SYMBOLS = {
    "ctk_ahead_rule_step": (C.c_int, [C.POINTER(AheadRule), C.c_int, C.c_double, C.c_double, C.c_int]),
    "ctk_ahead_enable": (C.c_int, [_H, C.c_int, C.c_double]),
    "ctk_ahead_stats": (C.c_int, [_H, C.POINTER(AheadCounters), C.POINTER(C.c_double)]),
    "ctk_ahead_kernel": (C.c_char_p, [_H]),
}


# user environments (include/ctk_user_env.h): name -> path of the library that was compiled with that model (control_toolkit_amd/build_env.py:
# register_environment); their environment id inside that library is CTK_ENV_USER
USER_ENVIRONMENTS = {}
ENV_USER = 3
_user_libs = {}


def load_library(path: str = None):
    """Load libctk_hip.so (built in-tree by control_toolkit_amd/csrc/Makefile).  Raises CtkError
    if it is missing — there is deliberately no other implementation to fall back to.
    path: a library compiled with a user environment (build_env.py); every such library carries the whole engine."""
    global _lib
    if path is not None:
        if path not in _user_libs:
            _user_libs[path] = _bind_library(path)
        return _user_libs[path]
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one
    # process leave the second one without devices ("No HIP GPUs are available").  Import torch
    # first so that libctk_hip.so binds to the runtime already loaded (torch is only plumbing
    # here: device memory for collectives, streams, torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    _lib = _bind_library(library_path())
    return _lib


def _bind_library(path: str):
    try:
        import torch  # noqa: F401  (see load_library: one HIP runtime per process)
    except ImportError:
        pass
    if not os.path.exists(path):
        raise CtkError(f"{path} not found: build it with `make -C control_toolkit_amd/csrc` "
                       f"(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise CtkError(f"cannot load {path}: {e}") from e
    for name, (res, args) in list(SYMBOLS.items()) + list(RUN_SYMBOLS.items()) + list(EPISODE_SYMBOLS.items()) + list(LOOP_SYMBOLS.items()) + \
            list(GRU_LOOP_SYMBOLS.items()) + list(HYPER_SYMBOLS.items()) + list(FAMILY_HYPER_SYMBOLS.items()) + list(AHEAD_SYMBOLS.items()) + \
            list(ROLLOUT_SYMBOLS.items()):
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.ctk_abi_version() != 6:
        raise CtkError(f"{path}: ABI version mismatch")
    return lib


def environment_library(name: str):
    """(library, environment id) that implement environment `name`: the product library for the built ones, the library compiled
    with the model for a registered user environment"""
    if name in ENVIRONMENTS:
        return load_library(), ENVIRONMENTS[name]
    if name in USER_ENVIRONMENTS:
        return load_library(USER_ENVIRONMENTS[name]), ENV_USER
    raise NotImplementedError(f"environment {name!r} is not built (have: {sorted(ENVIRONMENTS)} + registered user environments "
                              f"{sorted(USER_ENVIRONMENTS)}; control_toolkit_amd.build_env.register_environment compiles a model header)")


def environment_info(name: str):
    """(S, C, parameter names in id order) of an environment, as the library defines them (ctk_env_info / ctk_param_name)."""
    lib, eid = environment_library(name)
    S, Cn, n = C.c_int(), C.c_int(), C.c_int()
    if lib.ctk_env_info(eid, C.byref(S), C.byref(Cn), C.byref(n)) != 0:
        raise CtkError(f"ctk_env_info({name}) failed")
    return S.value, Cn.value, tuple(lib.ctk_param_name(eid, i).decode() for i in range(n.value))


def environment_defaults(name: str) -> dict:
    """parameter name -> the value a new handle starts with (ctk_param_default)"""
    lib, eid = environment_library(name)
    _, _, names = environment_info(name)
    out, v = {}, C.c_float()
    for i, n in enumerate(names):
        if lib.ctk_param_default(eid, i, C.byref(v)) != 0:
            raise CtkError(f"ctk_param_default({name}, {i}) failed")
        out[n] = float(v.value)
    return out


# the pre-bound step call (csrc/ctk_pystep.cpp -> _ctk_pystep): an optional accelerator of CtkEngine.step.  Not built, built for
# another interpreter, or CTK_PYSTEP=0 in the environment: the engine keeps its ctypes path.  Looked up once per process.
_pystep = None


def _pystep_module():
    global _pystep
    if _pystep is None:
        _pystep = False
        if os.environ.get("CTK_PYSTEP", "1") != "0":
            try:
                from . import _ctk_pystep
                _pystep = _ctk_pystep
            except ImportError:
                pass
    return _pystep or None


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None) -> np.ndarray:
    out = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if shape is not None and tuple(out.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


# the optimizer keywords of a ctk_config; the defaults keep unrelated optimizers' fields valid
_CONFIG_DEFAULTS = dict(cc_weight=1.0, R=1.0, LBD=100.0, NU=1000.0, SQRTRHOINV=0.03, cem_outer_it=1, cem_best_k=1,
                        warmup=0, warmup_iterations=0, cem_initial_action_stdev=0.5, cem_stdev_min=0.01,
                        outer_its=1, resamp_per=1, shift_previous=1, opt_keep_k=1, sampling_distribution=0,
                        sample_whole_control_space=0, sample_stdev=0.5, sample_mean=0.0, sample_min=-1.0, sample_max=1.0, learning_rate=0.05,
                        gradmax_clip=5.0, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1e-8, adam_rule=0, predictor_hidden1=0, predictor_hidden2=0)


def _make_config(optimizer: str, predictor: str, env_id: int, environment: str, Cn: int, *, num_rollouts, mpc_horizon, dt, action_low,
                 action_high, period_interpolation_inducing_points, seed, device, intermediate_steps, materialize_trajectories,
                 global_rollout_offset, num_states, num_control_inputs, generic_kernels, **kw) -> "CtkConfig":
    """the ctk_config of an engine (CtkEngine) or of a batch (CtkMppiBatch) from the constructor keywords"""
    cfg = CtkConfig()
    cfg.struct_size = C.sizeof(CtkConfig)
    cfg.optimizer, cfg.predictor, cfg.device = OPTIMIZERS[optimizer], PREDICTORS[predictor], device
    cfg.num_rollouts, cfg.mpc_horizon = int(num_rollouts), int(mpc_horizon)
    cfg.num_states, cfg.num_control_inputs = int(num_states), int(num_control_inputs)
    cfg.period_interpolation_inducing_points = int(period_interpolation_inducing_points)
    cfg.intermediate_steps = int(intermediate_steps)
    cfg.materialize_trajectories = int(bool(materialize_trajectories))
    cfg.global_rollout_offset = int(global_rollout_offset)
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.dt = float(dt)
    cfg.environment, cfg.generic_kernels = env_id, int(bool(generic_kernels))
    lo = np.broadcast_to(np.asarray(action_low, np.float32).reshape(-1), (Cn,)) if np.size(action_low) in (1, Cn) else None
    hi = np.broadcast_to(np.asarray(action_high, np.float32).reshape(-1), (Cn,)) if np.size(action_high) in (1, Cn) else None
    if lo is None or hi is None:
        raise ValueError(f"control limits must be scalars or have {Cn} entries (num_control_inputs of {environment})")
    for c in range(Cn):
        cfg.action_low[c], cfg.action_high[c] = float(lo[c]), float(hi[c])
    defaults = dict(_CONFIG_DEFAULTS)
    unknown = set(kw) - set(defaults)
    if unknown:
        raise TypeError(f"unknown engine arguments: {sorted(unknown)}")
    defaults.update(kw)
    for k, v in defaults.items():
        setattr(cfg, k, type(getattr(cfg, k))(v))
    return cfg


class CtkEngine:
    """Owns one ctk_handle (one optimizer instance on one GPU)."""

    def __init__(self, optimizer: str, predictor: str, *, num_rollouts: int, mpc_horizon: int, dt: float,
                 action_low: float = -1.0, action_high: float = 1.0, period_interpolation_inducing_points: int = 1,
                 seed: int = 0, device: int = 0, intermediate_steps: int = 1, materialize_trajectories: bool = False,
                 global_rollout_offset: int = 0, num_states: int = None, num_control_inputs: int = None,
                 environment: str = "CartPole", generic_kernels: bool = False, predictor_hidden=None, pystep: bool = None, **kw):
        """action_low / action_high: scalars (every input) or one value per control input.  environment: the plant +
        cost the kernels implement ("CartPole", "Quad2D", "Hover"); num_states / num_control_inputs default to its dimensions and
        are checked against them.  generic_kernels: run the environment-agnostic template kernels even where a hand-tuned
        one exists.  pystep: False keeps step() on the ctypes call even where the pre-bound call (_ctk_pystep) is available;
        None / True use it where it is (see step_path)."""
        lib, env_id = environment_library(environment)
        S, Cn, self.param_names = environment_info(environment)
        self.environment, self.S, self.C = environment, S, Cn
        num_states = S if num_states is None else num_states
        num_control_inputs = Cn if num_control_inputs is None else num_control_inputs
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"unknown optimizer {optimizer!r}")
        if predictor not in PREDICTORS:
            raise NotImplementedError(f"predictor_specification {predictor!r} is not built (have: {list(PREDICTORS)})")
        # hidden widths of a network predictor (the <h1>H1-<h2>H2 of the reference's network names): widths above 32 (MLP, up to 64) build
        # the handle on the 64-unit kernels; narrower networks are embedded exactly when their weights are set
        self.predictor_hidden = None if predictor_hidden is None else (int(predictor_hidden[0]), int(predictor_hidden[1]))
        self.native_hidden = (64, 64) if (self.predictor_hidden and max(self.predictor_hidden) > 32) else (32, 32)
        if self.predictor_hidden is not None:
            kw = dict(kw, predictor_hidden1=self.predictor_hidden[0], predictor_hidden2=self.predictor_hidden[1])
        cfg = _make_config(optimizer, predictor, env_id, environment, Cn, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                           action_low=action_low, action_high=action_high,
                           period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                           intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                           global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                           generic_kernels=generic_kernels, **kw)
        self._lib, self.cfg = lib, cfg
        self.optimizer, self.predictor = optimizer, predictor
        self.N, self.H = int(num_rollouts), int(mpc_horizon)
        self._h = _H()
        rc = lib.ctk_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = lib.ctk_last_error(None).decode()
            self._h = _H()
            raise (ValueError if rc == 1 else NotImplementedError if rc == 2 else CtkError)(msg)
        # preallocated argument buffers: the per-step call path does no allocation and no ndarray->ctypes casts
        self._u = np.zeros(Cn, np.float32)
        self._s = np.zeros(S, np.float32)
        self._up = np.zeros(Cn, np.float32)
        self._u_p, self._s_p, self._up_p = self._u.ctypes.data, self._s.ctypes.data, self._up.ctypes.data
        self._step_fn = lib.ctk_step
        self._bound = None
        self._fast_step = None   # the optimizer's bound step around this engine (Optimizers/__init__.py: _bind_native_step), for close()
        if pystep is None or pystep:
            self._bind_step()

    # ---- plumbing ------------------------------------------------------------------------------
    def _bind_step(self):
        """step() through the pre-bound call where the module is there: ctk_step's address in the library this engine loaded, the
        handle, the sizes and self._u's memory are fixed once (ctk_pystep.cpp)"""
        mod = _pystep_module()
        if mod is not None:
            self._bound = mod.bind(C.cast(self._step_fn, C.c_void_p).value, self._h.value, self.S, self.C, self._u)

    @property
    def step_path(self) -> str:
        """which call step() makes: "bound" (_ctk_pystep) or "ctypes" """
        return "bound" if self._bound is not None else "ctypes"

    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.ctk_last_error(self._h).decode()
            raise (ValueError if rc == 1 else NotImplementedError if rc == 2 else CtkError)(f"[ctk {rc}] {msg}")

    def close(self):
        if getattr(self, "_fast_step", None) is not None:   # first of all: it calls ctk_step with this handle on its own
            self._fast_step.invalidate()
            self._fast_step = None
        if getattr(self, "_bound", None) is not None:   # before ctk_destroy: the bound call must never see a freed handle
            self._bound.invalidate()
            self._bound = None
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ctk_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- API -----------------------------------------------------------------------------------
    def reset(self, draws=None, loc: int = LOC_NONE):
        if draws is not None and loc == LOC_NONE:
            loc = LOC_HOST
        d = _f32(draws) if (draws is not None and loc == LOC_HOST) else None
        self._check(self._lib.ctk_reset(self._h, _ptr(d) if d is not None else (draws if loc == LOC_DEVICE else None), loc))

    def get_stream(self) -> int:
        """the HIP stream the handle issues on right now (after resident_enable: a high-priority stream of its own)"""
        return int(self._lib.ctk_get_stream(self._h) or 0)

    def set_stream(self, stream_ptr: int):
        self._check(self._lib.ctk_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_param(self, name: str, value: float):
        self._check(self._lib.ctk_set_param(self._h, self.param_names.index(name), float(value)))

    def get_param(self, name: str) -> float:
        v = C.c_float()
        self._check(self._lib.ctk_get_param(self._h, self.param_names.index(name), C.byref(v)))
        return v.value

    def predictor_weight_count(self, hidden=None) -> int:
        if hidden is None:
            return int(self._lib.ctk_predictor_weight_count(self._h))
        return int(self._lib.ctk_predictor_weight_count_shaped(self._h, int(hidden[0]), int(hidden[1])))

    def set_predictor_weights(self, w, hidden=None):
        """hidden = (h1, h2): the network's hidden widths (the <h1>H1-<h2>H2 of the reference's network names); None = what the engine was
        created for (predictor_hidden, default 32 / 32).  Widths below the handle's own (32, or 64 for an engine created with
        predictor_hidden above 32) are embedded exactly; wider ones raise NotImplementedError with the sizes."""
        w = _f32(w).ravel()
        if hidden is None:
            hidden = self.predictor_hidden or self.native_hidden
        hidden = (int(hidden[0]), int(hidden[1]))
        if hidden == self.native_hidden:
            self._check(self._lib.ctk_set_predictor_weights(self._h, _ptr(w), w.size))
        else:
            self._check(self._lib.ctk_set_predictor_weights_shaped(self._h, _ptr(w), w.size, hidden[0], hidden[1]))
        self.hidden_sizes = hidden

    # recurrent predictor state (GRU): predictor.update(s, Q0), optimizer_mppi.py:195-197
    def predictor_hidden_size(self) -> int:
        return int(self._lib.ctk_predictor_hidden_size(self._h))

    def predictor_update(self, s, u=None):
        s = _f32(s).ravel()
        u = None if u is None else _f32(u).ravel()
        self._check(self._lib.ctk_predictor_update(self._h, _ptr(s), _ptr(u)))

    def predictor_get_hidden(self) -> np.ndarray:
        out = np.empty(self.predictor_hidden_size(), np.float32)
        self._check(self._lib.ctk_predictor_get_hidden(self._h, _ptr(out), out.size))
        return out.reshape(2, -1)

    def predictor_set_hidden(self, hidden=None):
        hid = None if hidden is None else _f32(hidden).ravel()
        self._check(self._lib.ctk_predictor_set_hidden(self._h, _ptr(hid), 0 if hid is None else hid.size))

    def samples_needed(self) -> int:
        return int(self._lib.ctk_samples_needed(self._h))

    def rng_position(self) -> int:
        v = C.c_uint32()
        self._check(self._lib.ctk_rng_get_position(self._h, C.byref(v)))
        return int(v.value)

    def set_rng_position(self, call: int):
        self._check(self._lib.ctk_rng_set_position(self._h, int(call) & 0xFFFFFFFF))

    def samples_needed_reset(self) -> int:
        """RPGD: raw draws optimizer_reset consumes (N * P * C)."""
        return self.N * int(self._lib.ctk_mppi_partial_size(self._h) - 2)

    def inducing_points(self) -> int:
        """P of the interpolator (others/Interpolator.py:79-84) as the engine uses it"""
        return int(self._lib.ctk_mppi_partial_size(self._h) - 2) // self.C

    def step(self, s, samples=None, loc: int = None, u_prev=None) -> np.ndarray:
        """samples: None (device Philox), a host ndarray (parity mode) or an int device pointer."""
        bound = self._bound
        if bound is not None:
            # the pre-bound call takes float32 buffers of the right sizes as they are; NotImplemented = an argument that needs
            # the conversions (or the error texts) below, and ctk_step has not been called
            if samples is None:
                rc = bound(s, u_prev, None, LOC_NONE)
            elif type(samples) is int:
                rc = bound(s, u_prev, samples, LOC_DEVICE)
            else:
                arr = _f32(samples)
                rc = bound(s, u_prev, arr.ctypes.data, LOC_HOST) if arr.size == self.samples_needed() else NotImplemented
            if rc is not NotImplemented:
                if rc:
                    self._check(rc)
                return self._u.copy()
        try:
            self._s[:] = np.asarray(s).reshape(-1)
        except ValueError:
            raise ValueError(f"state must have {self.S} entries") from None
        up_p = None
        if u_prev is not None:
            self._up[:] = np.asarray(u_prev).reshape(-1)[:self.C]
            up_p = self._up_p
        if samples is None:
            sp, loc = None, LOC_NONE
        elif type(samples) is int:
            sp, loc = samples, LOC_DEVICE
        else:
            arr = _f32(samples)
            need = self.samples_needed()
            if arr.size != need:
                raise ValueError(f"step consumes {need} draws, got {arr.size}")
            sp, loc = arr.ctypes.data, LOC_HOST
        rc = self._step_fn(self._h, self._s_p, up_p, sp, loc, self._u_p)
        if rc:
            self._check(rc)
        return self._u.copy()

    def rollout(self, s, Q, u_prev=0.0, want_traj=True):
        Q = _f32(Q)
        n = Q.shape[0]
        Q = np.ascontiguousarray(Q.reshape(n, self.H, self.C))
        s = _f32(s).reshape(-1)
        if s.size != self.S:
            raise ValueError(f"state must have {self.S} entries")
        up = np.ascontiguousarray(np.broadcast_to(_f32(u_prev).reshape(-1), (self.C,)))
        traj = np.empty((n, self.H + 1, self.S), np.float32) if want_traj else None
        J = np.empty((n,), np.float32)
        self._check(self._lib.ctk_rollout(self._h, _ptr(s), _ptr(up), _ptr(Q), n, _ptr(traj), _ptr(J)))
        return traj, J

    def mppi_partial_size(self) -> int:
        return int(self._lib.ctk_mppi_partial_size(self._h))

    def mppi_step_begin(self, s, partial_dev_ptr: int, samples=None, u_prev=None):
        s = _f32(s).reshape(-1)
        up = None if u_prev is None else _f32(u_prev).reshape(-1)[:self.C].copy()
        if samples is None:
            sp, loc = None, LOC_NONE
        elif isinstance(samples, int):
            sp, loc = C.c_void_p(samples), LOC_DEVICE
        else:
            arr = _f32(samples); sp, loc = _ptr(arr), LOC_HOST
        self._check(self._lib.ctk_mppi_step_begin(self._h, _ptr(s), _ptr(up), sp, loc, C.c_void_p(partial_dev_ptr)))

    def mppi_step_end(self, parts_dev_ptr: int, n_parts: int) -> np.ndarray:
        self._check(self._lib.ctk_mppi_step_end(self._h, C.c_void_p(parts_dev_ptr), int(n_parts), _ptr(self._u)))
        return self._u.copy()

    # ---- sharded MPPI over peer-to-peer stores (include/ctk_hip.h: ctk_p2p_*) -------------------------
    def p2p_alloc(self, rank: int, world: int) -> bytes:
        buf = C.create_string_buffer(64)
        self._check(self._lib.ctk_p2p_alloc(self._h, int(rank), int(world), buf))
        return bytes(buf.raw)

    def p2p_connect(self, handles) -> None:
        blob = b"".join(bytes(h) for h in handles)
        self._check(self._lib.ctk_p2p_connect(self._h, C.c_char_p(blob)))

    def p2p_step(self, s, samples=None, u_prev=None) -> np.ndarray:
        s = _f32(s).reshape(-1)
        up = None if u_prev is None else _f32(u_prev).reshape(-1)[:self.C].copy()
        if samples is None:
            sp, loc = None, LOC_NONE
        elif isinstance(samples, int):
            sp, loc = C.c_void_p(samples), LOC_DEVICE
        else:
            arr = _f32(samples); sp, loc = _ptr(arr), LOC_HOST
        self._check(self._lib.ctk_p2p_step(self._h, _ptr(s), _ptr(up), sp, loc, _ptr(self._u)))
        return self._u.copy()

    def p2p_close(self) -> None:
        self._check(self._lib.ctk_p2p_close(self._h))

    # ---- sharded CEM / random-action ---------------------------------------------------------------
    def shard_candidates_size(self) -> int:
        return int(self._lib.ctk_shard_candidates_size(self._h))

    def shard_iterations(self) -> int:
        return int(self._lib.ctk_shard_iterations(self._h))

    def shard_iter_begin(self, s, cand_dev_ptr: int, samples=None, u_prev=None):
        self._s[:] = np.asarray(s).reshape(-1)
        up_p = None
        if u_prev is not None:
            self._up[:] = np.asarray(u_prev).reshape(-1)[:self.C]
            up_p = self._up_p
        if samples is None:
            sp, loc = None, LOC_NONE
        elif type(samples) is int:
            sp, loc = samples, LOC_DEVICE
        else:
            arr = _f32(samples)
            if arr.size != self.N * self.H * self.C:
                raise ValueError(f"one iteration consumes {self.N * self.H * self.C} draws, got {arr.size}")
            sp, loc = arr.ctypes.data, LOC_HOST
        self._check(self._lib.ctk_shard_iter_begin(self._h, self._s_p, up_p, sp, loc, cand_dev_ptr))

    def shard_iter_end(self, cands_all_ptr: int, n_ranks: int):
        self._check(self._lib.ctk_shard_iter_end(self._h, cands_all_ptr, int(n_ranks)))

    def shard_finish(self) -> np.ndarray:
        self._check(self._lib.ctk_shard_finish(self._h, self._u_p))
        return self._u.copy()

    # ---- sharded RPGD ---------------------------------------------------------------------------------
    def rpgd_keepers_size(self) -> int:
        return int(self._lib.ctk_rpgd_keepers_size(self._h))

    def rpgd_fresh_rows(self, n_ranks: int) -> int:
        return int(self._lib.ctk_rpgd_fresh_rows(self._h, int(n_ranks)))

    def rpgd_step_begin(self, s, keep_dev_ptr: int, u_prev=None):
        self._s[:] = np.asarray(s).reshape(-1)
        up_p = None
        if u_prev is not None:
            self._up[:] = np.asarray(u_prev).reshape(-1)[:self.C]
            up_p = self._up_p
        self._check(self._lib.ctk_rpgd_step_begin(self._h, self._s_p, up_p, keep_dev_ptr))

    def rpgd_step_end(self, keep_all_ptr: int, n_ranks: int, draws=None) -> np.ndarray:
        if draws is None:
            dp, loc = None, LOC_NONE
        elif type(draws) is int:
            dp, loc = draws, LOC_DEVICE
        else:
            arr = _f32(draws); dp, loc = arr.ctypes.data, LOC_HOST
        self._check(self._lib.ctk_rpgd_step_end(self._h, keep_all_ptr, int(n_ranks), dp, loc, self._u_p))
        return self._u.copy()

    def read(self, name: str) -> np.ndarray:
        N, H, S, Cn = self.N, self.H, self.S, self.C
        cap = max(N * (H + 1) * S, N * H * Cn, 1)
        buf = np.empty(cap, np.float32)
        n = C.c_size_t()
        self._check(self._lib.ctk_read(self._h, BUFFERS[name], _ptr(buf), cap, C.byref(n)))
        out = buf[: n.value].copy()
        shapes = {"Q": (N, H, Cn), "J": (N,), "TRAJ": (N, H + 1, S), "U_NOM": (1, H, Cn), "STD": (1, H, Cn),
                  "ADAM_M": (N, H, Cn), "ADAM_V": (N, H, Cn), "AGES": (N,), "PLAN": (N, H, Cn), "AGES_LOGGED": (N,),
                  "MIX_MU": (2, H, Cn), "MIX_STD": (2, H, Cn), "MIX_PROB": (2,), "MIX_LABEL": (-1,)}
        if name == "BEST_IDX":
            return out.astype(np.int64)
        return out.reshape(shapes[name])

    # resident MPPI step (include/ctk_hip.h: ctk_resident_*): the first step launches a kernel that stays on the device and serves the
    # following steps from a pinned mailbox; it leaves by itself after idle_us without a request, and at once on resident_stop() or any
    # other call that touches device state
    def resident_enable(self, on: bool = True, idle_us: float = 200.0, read_ahead: bool = False):
        """read_ahead: the caller's promise that the device sample buffers it hands to step() keep their contents while the resident
        form is enabled (a static pool): they are then read between steps.  Without it a buffer is read when its request arrives, so
        refilling one buffer in place between steps is safe."""
        self._check(self._lib.ctk_resident_enable(self._h, (2 if read_ahead else 1) if on else 0, float(idle_us)))

    def resident_stop(self):
        self._check(self._lib.ctk_resident_stop(self._h))

    def resident_stats(self) -> dict:
        a, b, r, m = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.ctk_resident_stats(self._h, C.byref(a), C.byref(b), C.byref(r), C.byref(m)))
        return {"launches": int(a.value), "steps": int(b.value), "running": bool(r.value), "mailbox": "device memory" if m.value else "pinned host memory"}

    # launched-ahead MPPI step (include/ctk_hip_ahead.h): in a tight loop the kernel of the next step is launched while this one runs and
    # waits, for at most fuse_us, for its request.  On by default where the handle can use it; the results do not depend on it.
    def launch_ahead(self, on: bool = True, fuse_us: float = 0.0):
        """fuse_us <= 0 keeps the current fuse (default AHEAD_DEFAULT_FUSE_US)"""
        self._check(self._lib.ctk_ahead_enable(self._h, 1 if on else 0, float(fuse_us)))

    def ahead_stats(self) -> dict:
        c, f = AheadCounters(), C.c_double()
        self._check(self._lib.ctk_ahead_stats(self._h, C.byref(c), C.byref(f)))
        out = {n: int(getattr(c, n)) for n, _ in AheadCounters._fields_}
        out["fuse_us"] = f.value
        return out

    def ahead_kernel(self) -> str:
        """the kernel that serves the steps launched ahead, as a kernel trace prints it; "" until one was served (dominant_kernel() keeps
        naming the launched kernel)"""
        return (self._lib.ctk_ahead_kernel(self._h) or b"").decode()

    # device-resident step log (include/ctk_hip.h: ctk_log_*)
    def log_enable(self, capacity_steps: int):
        self._check(self._lib.ctk_log_enable(self._h, int(capacity_steps)))
        self.log_capacity = int(capacity_steps)

    def log_count(self) -> int:
        return int(self._lib.ctk_log_count(self._h))

    def log_read(self, name: str, first_step: int, n_steps: int) -> np.ndarray:
        N, H = self.N, self.H
        shape = {"Q": (N, H, self.C), "J": (N,), "TRAJ": (N, H + 1, self.S), "AGES": (N,)}[name]
        out = np.empty((int(n_steps),) + shape, np.float32)
        n = C.c_size_t()
        self._check(self._lib.ctk_log_read(self._h, BUFFERS[name], int(first_step), int(n_steps), _ptr(out), out.size, C.byref(n)))
        assert n.value == out.size
        return out

    def get_state(self) -> np.ndarray:
        n = int(self._lib.ctk_state_size(self._h))
        buf = np.empty(n, np.float32)
        self._check(self._lib.ctk_get_state(self._h, _ptr(buf), n))
        return buf

    def set_state(self, state):
        st = _f32(state).ravel()
        self._check(self._lib.ctk_set_state(self._h, _ptr(st), st.size))

    def profile_enable(self, on=True, every: int = 1):
        """time every `every`-th launch of the dominant kernel (dispatch timestamps); on=False disables"""
        self._check(self._lib.ctk_profile_enable(self._h, int(every) if on else 0))

    def profile_read(self) -> np.ndarray:
        buf = np.empty(4096, np.float32)
        n = C.c_size_t()
        self._check(self._lib.ctk_profile_read(self._h, _ptr(buf), buf.size, C.byref(n)))
        return buf[: n.value].copy()

    def dominant_kernel(self) -> str:
        return self._lib.ctk_dominant_kernel(self._h).decode()


# ---- batched MPPI (include/ctk_hip.h: ctk_batch_*) ------------------------------------------------------------------------------------
def batch_ids(num_problems: int, ids) -> Optional[np.ndarray]:
    """the id list of a batch call: None (all problems), or strictly ascending problem indices as int32"""
    if ids is None:
        return None
    arr = np.ascontiguousarray(np.asarray(ids).reshape(-1))
    if arr.size < 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("ids must be a non-empty list of problem indices (or None: all problems)")
    if arr.min() < 0 or arr.max() >= num_problems:
        raise ValueError(f"ids must lie in 0 .. {num_problems - 1} (the batch holds {num_problems} problems)")
    if np.any(np.diff(arr) <= 0):
        raise ValueError("ids must be strictly ascending")
    return arr.astype(np.int32)


def batch_step_args(num_problems: int, S: int, Cn: int, per_problem: int, states, samples=None, u_prev=None, ids=None):
    """Checks the arguments of CtkMppiBatch.step without touching a device: ids (batch_ids), states [n, S], u_prev None or [n, C],
    samples None, an int device pointer or a host array of n * per_problem draws ([n, N, P, C]).  Returns (ids, n, samples as fp32 or
    as given); states and u_prev are copied by the caller into its preallocated buffers."""
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    st = np.asarray(states)
    if st.shape != (n, S) and not (n == 1 and st.shape == (S,)):
        raise ValueError(f"states must have shape ({n}, {S}): one row per stepped problem, got {tuple(st.shape)}")
    if u_prev is not None:
        up = np.asarray(u_prev)
        if up.shape != (n, Cn) and not (Cn == 1 and up.shape == (n,)):
            raise ValueError(f"u_prev must have shape ({n}, {Cn}): one row per stepped problem, got {tuple(up.shape)}")
    if samples is not None and type(samples) is not int:
        samples = _f32(samples)
        if samples.size != n * per_problem or (samples.ndim > 1 and samples.shape[0] != n):
            raise ValueError(f"step of {n} problems consumes {n} x {per_problem} draws ([n, N, P, C]), got shape {tuple(samples.shape)}")
    return idv, n, samples


def batch_run_args(num_problems: int, S: int, Cn: int, states, steps, u_prev=None, ids=None, plant_substeps=None, samples=None,
                   what=None):
    """Checks the arguments of CtkMppiBatch.run / plant_step without touching a device, the way batch_step_args checks a step's: ids,
    start states [n, S], u_prev None or [n, C] (what: the names a plant step's messages give the two), steps >= 1, plant_substeps None or >= 1, and samples, which must be None (a run draws
    from the device Philox only).  Returns (ids, n, the sub-step count as the library takes it: 0 = the controller's)."""
    if samples is not None:
        raise NotImplementedError("a run draws from the device Philox only: it has no place for per-step host or device sample buffers "
                                  "(samples must be None; step() takes them)")
    try:
        idv, n, _ = batch_step_args(num_problems, S, Cn, 0, states, None, u_prev, ids)
    except ValueError as e:
        if what is None:
            raise
        raise ValueError(str(e).replace("states must", f"{what[0]} must").replace("u_prev must", f"{what[1]} must")) from None
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError(f"a run has at least one step (steps == {steps!r})")
    if plant_substeps is None:
        return idv, n, 0
    if isinstance(plant_substeps, bool) or not isinstance(plant_substeps, (int, np.integer)) or plant_substeps < 1:
        raise ValueError(f"plant_substeps must be an integer >= 1 or None (the controller's intermediate_steps), got {plant_substeps!r}")
    return idv, n, int(plant_substeps)


_F32_MAX = float(np.finfo(np.float32).max)


def batch_noise_args(num_problems: int, S: int, sigma, ids=None, what: str = "process"):
    """Checks one noise argument of BatchClosedLoop.set_noise without touching a device: ids (batch_ids), sigma a scalar, [S] or [n, S]
    of finite standard deviations >= 0 that fit float32.  Returns (ids, n, sigma as fp32 [n, S])."""
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    try:
        sg = np.asarray(sigma, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} noise must be a number or an array of numbers, got {sigma!r}") from None
    if sg.ndim == 0 or sg.shape == (S,):
        sg = np.broadcast_to(sg, (n, S))
    if sg.shape != (n, S):
        raise ValueError(f"{what} noise must be a scalar, ({S},) or ({n}, {S}): one row per listed problem, got shape {tuple(sg.shape)}")
    ok = (sg >= 0.0) & (sg <= _F32_MAX)                            # NaN compares false
    if not ok.all():
        j, i = (int(x[0]) for x in np.nonzero(~ok))
        raise ValueError(f"{what} noise: a standard deviation is finite and >= 0, got {float(sg[j, i])!r} for problem {j if idv is None else int(idv[j])}, state {i}")
    return idv, n, np.ascontiguousarray(sg, dtype=np.float32)


def batch_episode_args(num_problems: int, S: int, Cn: int, states, steps, u_prev=None, ids=None, plant_substeps=None, observations=None):
    """Checks the arguments of BatchClosedLoop.episodes without touching a device: those of a run (batch_run_args) and Y0, None or [n, S]
    like the start states.  Returns (ids, n, the sub-step count as the library takes it)."""
    idv, n, sub = batch_run_args(num_problems, S, Cn, states, steps, u_prev, ids, plant_substeps, None)
    if observations is not None:
        y = np.asarray(observations)
        if y.shape != (n, S) and not (n == 1 and y.shape == (S,)):
            raise ValueError(f"Y0 must have shape ({n}, {S}): one row per listed problem, like S0, got {tuple(y.shape)}")
    return idv, n, sub


def batch_rollout_args(num_problems: int, S: int, Cn: int, H: int, num_rollouts: int, states, plans=None, u_prev=None, ids=None,
                       model="controller", plant_substeps=None):
    """Checks the arguments of BatchRollout.rollout without touching a device, the way batch_step_args checks a step's.  ids: None (all
    problems) or problem indices in any order, each at most once (the rows of a rollout are independent).  states [n, S]; u_prev None
    (zeros), a scalar, [C] or [n, C]; plans None (every listed problem's own current plan), an int device pointer to [n, M, H, C] —
    then M is taken as 1 unless plans is a (pointer, M) pair —, [n, M, H, C], or [M, H, C] (for C == 1 also without the last axis),
    which is given to every listed problem; 1 <= M <= num_rollouts; model "controller" or "plant"; plant_substeps None or an integer
    >= 1, for the plant model only.  Returns (ids as int32 or None, n, states fp32 [n, S], u_prev fp32 [n, C] or None, plans: None,
    the int pointer or fp32 [n, M, H, C], M, the model's number, the sub-step count as the library takes it)."""
    idv = None
    if ids is not None:
        idv = np.ascontiguousarray(np.asarray(ids).reshape(-1))
        if idv.size < 1 or not np.issubdtype(idv.dtype, np.integer):
            raise ValueError("ids must be a non-empty list of problem indices (or None: all problems)")
        if idv.min() < 0 or idv.max() >= num_problems:
            raise ValueError(f"ids must lie in 0 .. {num_problems - 1} (the batch holds {num_problems} problems)")
        if np.unique(idv).size != idv.size:
            raise ValueError("ids must name each problem at most once (any order)")
        idv = idv.astype(np.int32)
    n = num_problems if idv is None else int(idv.size)
    st = np.asarray(states)
    if st.shape != (n, S) and not (n == 1 and st.shape == (S,)):
        raise ValueError(f"states must have shape ({n}, {S}): one row per listed problem, got {tuple(st.shape)}")
    st = _f32(st).reshape(n, S)
    up = None
    if u_prev is not None:
        up = np.asarray(u_prev, dtype=np.float32)
        if up.ndim == 0 or up.shape == (Cn,):
            up = np.broadcast_to(up, (n, Cn))
        elif Cn == 1 and up.shape == (n,):
            up = up.reshape(n, 1)
        if up.shape != (n, Cn):
            raise ValueError(f"u_prev must be a scalar, ({Cn},) or ({n}, {Cn}): one row per listed problem, got {tuple(np.shape(u_prev))}")
        up = np.ascontiguousarray(up, dtype=np.float32)
    if model not in ROLLOUT_MODELS:
        raise ValueError(f"model must be one of {sorted(ROLLOUT_MODELS)}, got {model!r}")
    sub = 0
    if plant_substeps is not None:
        if model != "plant":
            raise ValueError("plant_substeps belongs to model='plant' (the controller model rolls out with the controller's intermediate_steps)")
        if isinstance(plant_substeps, bool) or not isinstance(plant_substeps, (int, np.integer)) or plant_substeps < 1:
            raise ValueError(f"plant_substeps must be an integer >= 1 or None (the controller's intermediate_steps), got {plant_substeps!r}")
        sub = int(plant_substeps)
    M = 1
    if plans is not None:
        if isinstance(plans, tuple) and len(plans) == 2 and type(plans[0]) is int:
            plans, M = plans[0], plans[1]
            if isinstance(M, bool) or not isinstance(M, (int, np.integer)):
                raise ValueError(f"a device-pointer plans is (pointer, M) with an integer M, got M == {M!r}")
            M = int(M)
        elif type(plans) is not int:
            pl = np.asarray(plans, dtype=np.float32)
            if Cn == 1 and pl.ndim in (2, 3) and pl.shape[-1] == H and not (pl.ndim == 3 and pl.shape[1:] == (H, 1)):
                pl = pl[..., None]
            if pl.ndim == 3 and pl.shape[1:] == (H, Cn):
                pl = np.broadcast_to(pl, (n,) + pl.shape)
            if pl.ndim != 4 or pl.shape[0] != n or pl.shape[2:] != (H, Cn):
                raise ValueError(f"plans must have shape ({n}, M, {H}, {Cn}) or (M, {H}, {Cn}) for every listed problem, got {tuple(np.shape(plans))}")
            M = int(pl.shape[1])
            plans = np.ascontiguousarray(pl, dtype=np.float32)
        if not 1 <= M <= num_rollouts:
            raise ValueError(f"a rollout takes 1 <= M <= num_rollouts ({num_rollouts}) plans per problem, got M == {M}")
    return idv, n, st, up, plans, M, ROLLOUT_MODELS[model], sub


class Episodes(NamedTuple):
    """what BatchClosedLoop.episodes returns: the true states [n, steps + 1, S], what the controllers were given [n, steps + 1, S], the
    inputs [n, steps, C] and the realised stage costs [n, steps]"""
    states: np.ndarray
    observations: np.ndarray
    inputs: np.ndarray
    costs: np.ndarray


def batch_param_args(param_names, num_problems: int, name, values, ids=None):
    """Checks the arguments of CtkMppiBatch.set_problem_params / CtkCemBatch.set_problem_params / CtkRpgdBatch.set_problem_params
    without touching a device: the parameter name against the environment's names, ids (batch_ids), values a finite scalar (every
    listed problem) or one finite value per listed problem ([n]).  Returns (parameter id, ids, n, values as fp32 [n])."""
    if name not in param_names:
        raise ValueError(f"unknown parameter {name!r} for this environment (it has {', '.join(param_names)})")
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    try:
        vals = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"values of {name!r} must be a number or an array of numbers, got {values!r}") from None
    if vals.ndim == 0:
        vals = np.full(n, float(vals))
    if vals.shape != (n,):
        raise ValueError(f"{name!r}: one value per listed problem ({n}) or a scalar, got shape {tuple(vals.shape)}")
    if not (np.abs(vals) <= _F32_MAX).all():                       # NaN compares false: refused with the infinities and what overflows fp32
        j = int(np.flatnonzero(~(np.abs(vals) <= _F32_MAX))[0])
        raise ValueError(f"{name!r} must be finite in fp32: {vals[j]!r} for problem {j if idv is None else int(idv[j])}")
    out = vals.astype(np.float32)
    return param_names.index(name), idv, n, out


def batch_hyper_args(num_problems: int, name, values, ids=None, Cn: int = 1):
    """Checks the arguments of CtkMppiBatch.set_problem_hypers / set_hyper / set_problem_limits without touching a device: the name
    against HYPERS, ids (batch_ids), values a scalar (every listed problem) or one value per listed problem ([n]), each finite in fp32,
    LBD > 0, NU != 0.  Returns (hyper id, ids, n, values as fp32 [n]).  name "limits": values is (low, high), each a scalar, [Cn] or
    [n, Cn] with low <= high (batch_limit_args); returns (None, ids, n, (low, high) as fp32 [n, Cn])."""
    if name == "limits":
        try:
            low, high = values
        except (TypeError, ValueError):
            raise ValueError(f"limits are a pair (low, high), got {values!r}") from None
        idv, n, lo, hi = batch_limit_args(num_problems, Cn, low, high, ids)
        return None, idv, n, (lo, hi)
    if name not in HYPERS:
        raise ValueError(f"unknown hyper-parameter {name!r} (MPPI has {', '.join(HYPERS)}; \"limits\" for the input limits)")
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    try:
        vals = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"values of {name!r} must be a number or an array of numbers, got {values!r}") from None
    if vals.ndim == 0:
        vals = np.full(n, float(vals))
    if vals.shape != (n,):
        raise ValueError(f"{name!r}: one value per listed problem ({n}) or a scalar, got shape {tuple(vals.shape)}")
    ok = np.abs(vals) <= _F32_MAX                                  # NaN compares false: refused with the infinities and what overflows fp32
    what = "must be finite in fp32"
    with np.errstate(over="ignore"):
        out = vals.astype(np.float32)
    if ok.all() and name == "LBD":
        ok, what = out > 0.0, "must be > 0"                        # as the library sees it: after the rounding to fp32
    if ok.all() and name == "NU":
        ok, what = out != 0.0, "must not be 0"
    if not ok.all():
        j = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{name!r} {what}: {float(vals[j])!r} for problem {j if idv is None else int(idv[j])}")
    return HYPERS[name], idv, n, out


def batch_limit_args(num_problems: int, Cn: int, low, high, ids=None):
    """Checks the arguments of CtkMppiBatch.set_problem_limits without touching a device: ids (batch_ids), low and high each a scalar,
    [C] or [n, C], finite in fp32, low <= high for every input.  Returns (ids, n, low, high as fp32 [n, C])."""
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    out = []
    for what, v in (("low", low), ("high", high)):
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a number or an array of numbers, got {v!r}") from None
        if a.ndim == 0 or a.shape == (Cn,):
            a = np.broadcast_to(a, (n, Cn))
        if a.shape != (n, Cn):
            raise ValueError(f"{what} must be a scalar, ({Cn},) or ({n}, {Cn}): one row per listed problem, got shape {tuple(a.shape)}")
        ok = np.abs(a) <= _F32_MAX
        if not ok.all():
            j, c = (int(x[0]) for x in np.nonzero(~ok))
            raise ValueError(f"{what} must be finite in fp32: {float(a[j, c])!r} for problem {j if idv is None else int(idv[j])}, input {c}")
        out.append(np.ascontiguousarray(a, dtype=np.float32))
    bad = ~(out[0] <= out[1])
    if bad.any():
        j, c = (int(x[0]) for x in np.nonzero(bad))
        raise ValueError(f"low must be <= high for every input: {float(out[0][j, c])!r} > {float(out[1][j, c])!r} for problem "
                         f"{j if idv is None else int(idv[j])}, input {c}")
    return idv, n, out[0], out[1]


def family_hyper_args(family: str, num_problems: int, name, values, ids=None, Cn: int = 1, num_rollouts: int = None):
    """Checks the arguments of FamilyHypers.set_problem_hypers / set_hyper / set_problem_limits without touching a device.  family: "cem"
    or "rpgd"; the name against CEM_HYPERS / RPGD_HYPERS, ids (batch_ids), values a scalar (every listed problem) or one value per listed
    problem ([n]), each finite in fp32; a count (cem_best_k, cem_outer_it, outer_its, resamp_per) integral and within the rule the
    batch's creation applies (1 <= cem_best_k <= num_rollouts where num_rollouts is given, cem_outer_it >= 1, outer_its >= 0,
    resamp_per >= 1).  Returns (hyper id, ids, n, values as fp32 [n]).  name "limits": values is (low, high), each a scalar, [Cn] or
    [n, Cn] with low <= high (batch_limit_args); returns (None, ids, n, (low, high) as fp32 [n, Cn])."""
    if family not in _FAMILY_HYPERS:
        raise ValueError(f"family is 'cem' or 'rpgd', not {family!r} (the MPPI batches have batch_hyper_args)")
    table = _FAMILY_HYPERS[family]
    if name == "limits":
        try:
            low, high = values
        except (TypeError, ValueError):
            raise ValueError(f"limits are a pair (low, high), got {values!r}") from None
        idv, n, lo, hi = batch_limit_args(num_problems, Cn, low, high, ids)
        return None, idv, n, (lo, hi)
    if name not in table:
        raise ValueError(f"unknown hyper-parameter {name!r} ({family.upper()} has {', '.join(table)}; \"limits\" for the input limits)")
    idv = batch_ids(num_problems, ids)
    n = num_problems if idv is None else int(idv.size)
    try:
        vals = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"values of {name!r} must be a number or an array of numbers, got {values!r}") from None
    if vals.ndim == 0:
        vals = np.full(n, float(vals))
    if vals.shape != (n,):
        raise ValueError(f"{name!r}: one value per listed problem ({n}) or a scalar, got shape {tuple(vals.shape)}")
    ok = np.abs(vals) <= _F32_MAX                                  # NaN compares false: refused with the infinities and what overflows fp32
    what = "must be finite in fp32"
    with np.errstate(over="ignore"):
        out = vals.astype(np.float32)
    if ok.all() and name in _FAMILY_COUNTS:
        ok, what = vals == np.floor(vals), "must be integral"
        if ok.all():
            ok, what = (vals >= _FAMILY_COUNTS[name]) & (vals < 2.0 ** 31), f"must be >= {_FAMILY_COUNTS[name]}"
        if ok.all() and name == "cem_best_k" and num_rollouts is not None:
            ok, what = vals <= num_rollouts, f"must be <= num_rollouts ({num_rollouts})"
    if not ok.all():
        j = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{name!r} {what}: {float(vals[j])!r} for problem {j if idv is None else int(idv[j])}")
    return table[name], idv, n, out


class _CtkBatch:
    """What the batch classes share: the handle, the argument buffers, the error mapping, the parameter tables and the Philox positions.
    A family is its two entry-point prefixes (_BATCH: the calls on a batch, _PROBLEM: the per-problem parameter calls); its entries are
    looked up by name once, when the batch is created (_open)."""

    _BATCH = _PROBLEM = None
    _BATCH_ENTRIES = ("create", "destroy", "last_error", "samples_needed", "step", "reset", "read", "get_state", "set_state", "set_param",
                      "get_param", "rng_get_position", "rng_set_position", "dominant_kernel")
    _PROBLEM_ENTRIES = ("set_param", "get_param", "params_differ")

    # what needs no device is checked before the library is asked for one: _count, _seeds, _known and the class's own refusals
    @staticmethod
    def _count(num_problems) -> int:
        if int(num_problems) < 1:
            raise ValueError(f"a batch holds at least one problem (num_problems == {num_problems})")
        return int(num_problems)

    @staticmethod
    def _seeds(B: int, seeds):
        if seeds is not None:
            seeds = np.ascontiguousarray(np.asarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in np.asarray(seeds, dtype=object).reshape(-1)], np.uint64))
            if seeds.size != B:
                raise ValueError(f"seeds must have one entry per problem ({B}), got {seeds.size}")
        return seeds

    @staticmethod
    def _known(kw):
        unknown = set(kw) - set(_CONFIG_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown engine arguments: {sorted(unknown)}")

    def _open(self, B: int, seeds, optimizer: str, predictor: str, environment: str, *, num_states, num_control_inputs, **cfg_kw):
        """the library of `environment`, the configuration, the family's entries, the handle and the argument buffers"""
        lib, env_id = environment_library(environment)
        S, Cn, self.param_names = environment_info(environment)
        self.environment, self.S, self.C, self.B = environment, S, Cn, B
        cfg = _make_config(optimizer, predictor, env_id, environment, Cn, num_states=S if num_states is None else num_states,
                           num_control_inputs=Cn if num_control_inputs is None else num_control_inputs, **cfg_kw)
        self._lib, self.cfg = lib, cfg
        self.N, self.H = int(cfg.num_rollouts), int(cfg.mpc_horizon)
        self._b = SimpleNamespace(**{e: getattr(lib, f"{self._BATCH}_{e}") for e in self._BATCH_ENTRIES})
        self._p = SimpleNamespace(**{e: getattr(lib, f"{self._PROBLEM}_{e}") for e in self._PROBLEM_ENTRIES})
        self._h = _H()
        rc = self._b.create(C.byref(cfg), B, _ptr(seeds), C.byref(self._h))
        if rc != 0:
            msg = self._b.last_error(None).decode()
            self._h = _H()
            raise (ValueError if rc == 1 else NotImplementedError if rc == 2 else CtkError)(msg)
        # preallocated argument buffers, as CtkEngine.step's: rows 0 .. n-1 are the stepped problems'
        self._s = np.zeros((B, S), np.float32)
        self._up = np.zeros((B, Cn), np.float32)
        self._u = np.zeros((B, Cn), np.float32)
        self._ids = np.zeros(B, np.int32)
        self._s_p, self._up_p, self._u_p, self._ids_p = (a.ctypes.data for a in (self._s, self._up, self._u, self._ids))
        self._step_fn = self._b.step

    def _check(self, rc: int):
        if rc != 0:
            msg = self._b.last_error(self._h).decode()
            raise (ValueError if rc == 1 else NotImplementedError if rc == 2 else CtkError)(f"[ctk {rc}] {msg}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._b.destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.B

    def _problem(self, problem: int) -> int:
        if not 0 <= int(problem) < self.B:
            raise ValueError(f"problem index {problem} is outside 0 .. {self.B - 1}")
        return int(problem)

    def _step_args(self, n: int, idv, S, u_prev, samples):
        """the front of a step, after its arguments were checked (batch_step_args): states, u_prev and ids into rows 0 .. n-1 of the
        buffers.  Returns the pointers (ids, u_prev, samples) and where the samples are (LOC_*)."""
        self._s[:n] = S                # checked to be [n, S] (or [S] for one problem, which broadcasts): the assignment converts
        up_p = None
        if u_prev is not None:
            self._up[:n] = np.asarray(u_prev).reshape(n, self.C)
            up_p = self._up_p
        ids_p = None
        if idv is not None:
            self._ids[:n] = idv
            ids_p = self._ids_p
        if samples is None:
            sp, loc = None, LOC_NONE
        elif type(samples) is int:
            sp, loc = samples, LOC_DEVICE
        else:
            sp, loc = samples.ctypes.data, LOC_HOST
        return ids_p, up_p, sp, loc

    def _read(self, what: str, shapes: dict, name: str, problem: int) -> np.ndarray:
        if name not in shapes:
            raise ValueError(f"{what} has the buffers {sorted(shapes)}, not {name!r}")
        out = np.empty(shapes[name], np.float32)
        self._check(self._b.read(self._h, self._problem(problem), BUFFERS[name], _ptr(out), out.size))
        return out.astype(np.int64) if name == "BEST_IDX" else out

    def read_all(self, name: str) -> np.ndarray:
        return np.stack([self.read(name, p) for p in range(self.B)])

    def _get_state(self, problem: int, size: int) -> np.ndarray:
        buf = np.empty(size, np.float32)
        self._check(self._b.get_state(self._h, self._problem(problem), _ptr(buf), buf.size))
        return buf

    def set_state(self, problem: int, state):
        st = _f32(state).ravel()
        self._check(self._b.set_state(self._h, self._problem(problem), _ptr(st), st.size))

    def set_param(self, name: str, value: float):
        """parameter `name` of every problem (that column of every problem's table; the other parameters stay per problem)"""
        self._check(self._b.set_param(self._h, self.param_names.index(name), float(value)))

    def get_param(self, name: str) -> float:
        """the last value set_param gave the whole batch (the default before that); a problem's own value: get_problem_param"""
        v = C.c_float()
        self._check(self._b.get_param(self._h, self.param_names.index(name), C.byref(v)))
        return v.value

    def set_problem_params(self, name: str, values, ids=None):
        """parameter `name` of the problems in ids (None: all): values a scalar or [n], one per listed problem in the order of ids.  The
        next step re-derives the constants of the problems touched; from the first call on the batch runs the per-problem form of its
        kernel (params_differ, dominant_kernel)."""
        pid, idv, n, vals = batch_param_args(self.param_names, self.B, name, values, ids)
        self._check(self._p.set_param(self._h, n, _ptr(idv), pid, _ptr(vals)))

    def get_problem_param(self, name: str, problem: int) -> float:
        if name not in self.param_names:
            raise ValueError(f"unknown parameter {name!r} for this environment (it has {', '.join(self.param_names)})")
        v = C.c_float()
        if self._p.get_param(self._h, self._problem(problem), self.param_names.index(name), C.byref(v)) != 0:
            raise CtkError(f"{self._PROBLEM}_get_param({problem}, {name!r}) failed")
        return v.value

    def get_problem_params(self, name: str) -> np.ndarray:
        """[B] parameter `name` of every problem"""
        return np.array([self.get_problem_param(name, p) for p in range(self.B)], np.float32)

    def params_differ(self) -> int:
        """1 once a set_problem_params has succeeded on this batch (sticky), else 0"""
        return int(self._p.params_differ(self._h))

    def rng_position(self, problem: int) -> int:
        v = C.c_uint32()
        self._check(self._b.rng_get_position(self._h, self._problem(problem), C.byref(v)))
        return int(v.value)

    def set_rng_position(self, problem: int, call: int):
        self._check(self._b.rng_set_position(self._h, self._problem(problem), int(call) & 0xFFFFFFFF))

    def dominant_kernel(self) -> str:
        return self._b.dominant_kernel(self._h).decode()

    @property
    def rollouts(self) -> "BatchRollout":
        """rollouts of caller-supplied plans, every listed problem in one launch: rollouts.rollout(S, plans), .optimal_trajectory(S)
        (BatchRollout).  A view of this batch, as closed_loop and hypers are: it owns nothing and is not kept."""
        return BatchRollout(self)


class CtkMppiBatch(_CtkBatch):
    """Owns one ctk_batch: num_problems independent MPPI controllers of ONE configuration (the MPPI keywords of CtkEngine), stepped by
    one kernel launch per step.  Problem p behaves bit for bit like CtkEngine("mppi", "ODE", seed=seeds[p], ...) given the same calls,
    set_param among them: set_problem_params gives every problem its own plant, cost weights and targets, set_param the same value to all.
    batch.hypers (BatchHypers: set_problem_hypers, set_hyper, set_problem_limits ...) gives every problem its own MPPI hyper-parameters
    and input limits: problem p is then the CtkEngine created with those values.  seeds: one per problem (default seed + p)."""

    _BATCH, _PROBLEM = "ctk_batch", "ctk_problem"

    def __init__(self, num_problems: int, *, environment: str = "CartPole", seeds=None, optimizer: str = "mppi", predictor: str = "ODE",
                 num_rollouts: int, mpc_horizon: int, dt: float, action_low: float = -1.0, action_high: float = 1.0,
                 period_interpolation_inducing_points: int = 1, seed: int = 0, device: int = 0, intermediate_steps: int = 1,
                 materialize_trajectories: bool = False, global_rollout_offset: int = 0, num_states: int = None,
                 num_control_inputs: int = None, generic_kernels: bool = False, **kw):
        B = self._count(num_problems)
        if optimizer != "mppi":
            raise NotImplementedError(f"a batch steps MPPI controllers only (optimizer {optimizer!r}); the other optimizers run as CtkEngine")
        if predictor != "ODE":
            raise NotImplementedError(f"the batch kernel rolls out the analytic (ODE) predictor only (predictor {predictor!r}); "
                                      "network predictors run as CtkEngine")
        self._open(B, self._seeds(B, seeds), "mppi", "ODE", environment, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                   action_low=action_low, action_high=action_high,
                   period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                   intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                   global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                   generic_kernels=generic_kernels, **kw)
        self._per = int(self._b.samples_needed(self._h))

    # ---- per-problem MPPI hyper-parameters and input limits (include/ctk_hip_hyper.h); the MLP and GRU batches inherit them ----
    @property
    def hypers(self) -> "BatchHypers":
        """THE interface to the per-problem MPPI hyper-parameters and input limits: hypers.set_problem_hypers(name, values, ids),
        .set_hyper(name, value), .get_problem_hyper(name, problem), .get_problem_hypers(name), .set_problem_limits(low, high, ids),
        .get_problem_limits(problem), .hypers_differ() (BatchHypers).  A view of this batch, as closed_loop is: it owns nothing, and it is
        not kept (a kept view would tie the batch into a reference cycle and delay the release of its device memory)."""
        return BatchHypers(self)

    def __getattr__(self, name):
        # CONVENIENCE ONLY, and deliberately not methods: batch.set_problem_hypers(...) is batch.hypers.set_problem_hypers(...) for the
        # seven names of BatchHypers.CALLS.  The batch classes' method lists are pinned (tests/test_batch_cpu.py), so the calls are
        # defined, documented and introspectable on the view; dir(batch), help() and completion show them there, not here.
        if name in BatchHypers.CALLS:
            return getattr(self.hypers, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def samples_needed(self) -> int:
        """draws one problem's step consumes (N * P * C)"""
        return self._per

    def step(self, S, samples=None, u_prev=None, ids=None) -> np.ndarray:
        """S [n, num_states], one row per stepped problem in the order of ids (None: all problems).  samples: None (device Philox), a
        host array [n, N, P, C] or an int device pointer to such an array.  u_prev [n, C] or None (every problem's own last output).
        Returns u [n, C].  CtkError naming the problems whose in-launch hand-off timed out: the other problems' rows are valid (`last_u`)."""
        idv, n, samples = batch_step_args(self.B, self.S, self.C, self._per, S, samples, u_prev, ids)
        ids_p, up_p, sp, loc = self._step_args(n, idv, S, u_prev, samples)
        rc = self._step_fn(self._h, n, ids_p, self._s_p, up_p, sp, loc, self._u_p)
        self.last_u = self._u[:n].copy()
        if rc:
            self._check(rc)
        return self.last_u

    def reset(self, ids=None):
        idv = batch_ids(self.B, ids)
        self._check(self._b.reset(self._h, 0 if idv is None else idv.size, _ptr(idv)))

    def read(self, name: str, problem: int) -> np.ndarray:
        N, H, S, Cn = self.N, self.H, self.S, self.C
        return self._read("a batch", {"Q": (N, H, Cn), "J": (N,), "TRAJ": (N, H + 1, S), "U_NOM": (1, H, Cn)}, name, problem)

    @property
    def closed_loop(self) -> "BatchClosedLoop":
        """closed-loop episodes on the device, plant step included: closed_loop.run(S0, steps), .plant_step(S, U), .set_plant_params,
        .get_plant_params, .clear_plant_params (BatchClosedLoop).  A view of this batch: it owns nothing."""
        return BatchClosedLoop(self)

    def get_state(self, problem: int) -> np.ndarray:
        return self._get_state(problem, self.H * self.C + self.C)


# ---- rollouts of caller-supplied plans on a batch (include/ctk_hip_rollout.h) ------------------------------------------------------------------
class BatchRollout:
    """batch.rollouts of any of the five batch classes, or BatchRollout(batch): predictor.predict_core + cost.get_trajectory_cost of
    caller-supplied plans for every listed problem in ONE launch (kernels ctk_batch_rollout<ENV, PRED, TRAJ> / ctk_g_batch_rollout<ENV, TRAJ>).
    Row j equals, bit for bit, CtkEngine(<the batch's configuration>).rollout(S[j], plans[j], u_prev[j]) of an engine that was given
    problem ids[j]'s parameters, weights and hidden state.  A view of the batch: it owns nothing, and a rollout changes nothing — no
    plan, output, J / Q / TRAJ buffer, Philox position, sequence number or hidden state of any problem."""

    CALLS = ("rollout", "optimal_trajectory")

    def __init__(self, batch):
        self._batch = batch

    def rollout(self, S, plans=None, u_prev=None, ids=None, model="controller", plant_substeps=None, want_traj=True):
        """S [n, num_states], one row per problem in ids (None: all; any order).  plans [n, M, H, C], or [M, H, C] given to every listed
        problem (a robustness sweep over the problems' parameters), or None: every problem's own current plan (M = 1), read on the
        device; a device pointer goes in as (int pointer, M).  Plans are taken as given, not clipped.  u_prev: the input before the
        first one (None: zeros, as CtkEngine.rollout).  model "controller": each problem's own controller parameters, weights and hidden
        state; "plant": the analytic plant of its closed loop (closed_loop.set_plant_params; plant_substeps Euler sub-steps, None =
        intermediate_steps) — for an MLP or GRU batch, what the true plant does with the plan against what the network predicts.
        Returns (traj [n, M, H + 1, num_states] or None, J [n, M])."""
        b = self._batch
        idv, n, st, up, plans, M, model_id, sub = batch_rollout_args(b.B, b.S, b.C, b.H, b.N, S, plans, u_prev, ids, model, plant_substeps)
        if plans is None:
            pp, loc = None, LOC_NONE
        elif type(plans) is int:
            pp, loc = plans, LOC_DEVICE
        else:
            pp, loc = plans.ctypes.data, LOC_HOST
        traj = np.empty((n, M, b.H + 1, b.S), np.float32) if want_traj else None
        J = np.empty((n, M), np.float32)
        fn = getattr(b._lib, f"{b._BATCH}_rollout")
        b._check(fn(b._h, n, _ptr(idv), _ptr(st), _ptr(up), pp, loc, M, model_id, sub, _ptr(traj), _ptr(J)))
        return traj, J

    def optimal_trajectory(self, S, ids=None) -> np.ndarray:
        """[n, H + 1, num_states]: the trajectory every listed problem's current plan predicts from S — the reference's
        optimal_trajectory (optimizer_mppi.py:199-202) for a whole batch"""
        return self.rollout(S, None, ids=ids)[0][:, 0]


# ---- per-problem MPPI hyper-parameters and input limits of an MPPI batch (include/ctk_hip_hyper.h) ----------------------------------------------
class BatchHypers:
    """CtkMppiBatch.hypers / CtkMppiMlpBatch.hypers / CtkMppiGruBatch.hypers: every problem's own cc_weight, R, LBD, NU, SQRTRHOINV and
    input limits, settable at any time between steps.  Problem p then behaves bit for bit like CtkEngine("mppi", ..., seed=seeds[p])
    created with p's values; a change makes it equal to a fresh such handle that received the problem's state vector and Philox position
    (and hidden state).  A view of the batch: it owns nothing.  CEM and RPGD batches have a view of their own, with their own
    hyper-parameters: FamilyHypers(batch)."""

    CALLS = ("set_problem_hypers", "set_hyper", "get_problem_hyper", "get_problem_hypers", "set_problem_limits", "get_problem_limits", "hypers_differ")

    def __init__(self, batch):
        self._batch = batch

    def _entry(self, entry: str):
        """the family's hyper-parameter entry `entry` (of the problem prefix; "batch_set_hyper": the whole-batch one)"""
        b = self._batch
        return getattr(b._lib, f"{b._BATCH}_set_hyper" if entry == "batch_set_hyper" else f"{b._PROBLEM}_{entry}")

    def set_problem_hypers(self, name: str, values, ids=None):
        """MPPI hyper-parameter `name` (cc_weight, R, LBD, NU, SQRTRHOINV: the constructor arguments of that name, NOT the environment's
        cost parameters R / cc_weight, which set_problem_params sets) of the problems in ids (None: all): values a scalar or [n], one
        per listed problem in the order of ids.  Takes effect at the next step; from the first call on the batch runs the _hp form of
        its kernel (hypers_differ, dominant_kernel).  Problem p then behaves like CtkEngine("mppi", ..., seed=seeds[p], <name>=value)."""
        b = self._batch
        hid, idv, n, vals = batch_hyper_args(b.B, name, values, ids)
        b._check(self._entry("set_hyper")(b._h, n, _ptr(idv), hid, _ptr(vals)))

    def set_hyper(self, name: str, value: float):
        """MPPI hyper-parameter `name` of every problem"""
        b = self._batch
        hid, _, _, vals = batch_hyper_args(b.B, name, value, None)
        b._check(self._entry("batch_set_hyper")(b._h, hid, float(vals[0])))

    def get_problem_hyper(self, name: str, problem: int) -> float:
        b = self._batch
        if name not in HYPERS:
            raise ValueError(f"unknown hyper-parameter {name!r} (MPPI has {', '.join(HYPERS)})")
        v = C.c_float()
        if self._entry("get_hyper")(b._h, b._problem(problem), HYPERS[name], C.byref(v)) != 0:
            raise CtkError(f"{b._PROBLEM}_get_hyper({problem}, {name!r}) failed")
        return v.value

    def get_problem_hypers(self, name: str) -> np.ndarray:
        """[B] hyper-parameter `name` of every problem"""
        return np.array([self.get_problem_hyper(name, p) for p in range(self._batch.B)], np.float32)

    def set_problem_limits(self, low, high, ids=None):
        """the input limits (action_low, action_high) of the problems in ids (None: all): each a scalar, [C] or [n, C].  As
        set_problem_hypers: the next step clips to them, reset() refills the plan with their middle."""
        b = self._batch
        _, idv, n, (lo, hi) = batch_hyper_args(b.B, "limits", (low, high), ids, b.C)
        b._check(self._entry("set_limits")(b._h, n, _ptr(idv), _ptr(lo), _ptr(hi)))

    def get_problem_limits(self, problem: int):
        """(low [C], high [C]) of a problem"""
        b = self._batch
        lo, hi = np.empty(b.C, np.float32), np.empty(b.C, np.float32)
        if self._entry("get_limits")(b._h, b._problem(problem), _ptr(lo), _ptr(hi)) != 0:
            raise CtkError(f"{b._PROBLEM}_get_limits({problem}) failed")
        return lo, hi

    def hypers_differ(self) -> int:
        """1 once a set_problem_hypers, set_hyper or set_problem_limits has succeeded on this batch (sticky), else 0"""
        b = self._batch
        return int(self._entry("hypers_differ")(b._h))


# ---- per-problem hyper-parameters and input limits of a CEM or RPGD batch (include/ctk_hip_family_hyper.h) --------------------------------------
class FamilyHypers:
    """FamilyHypers(cem_batch) / FamilyHypers(rpgd_batch) — the constructor is the way in, as BatchClosedLoop(cem_batch) is: those classes
    have no hypers attribute.  Every problem's own optimizer numbers and input limits, settable at any time between steps:
    CEM (CEM_HYPERS): cem_best_k, cem_initial_action_stdev, cem_stdev_min, cem_outer_it;
    RPGD (RPGD_HYPERS): learning_rate, adam_beta_1, adam_beta_2, adam_epsilon, gradmax_clip, sample_stdev, sample_mean, uniform_dist_min,
    uniform_dist_max, outer_its, resamp_per.
    Problem p then behaves bit for bit like CtkEngine("cem", "ODE", seed=seeds[p], ...) / CtkEngine("rpgd", "ODE", generic_kernels=True,
    seed=seeds[p], ...) created with p's values; a change makes it equal to a fresh such handle that received the problem's state vector
    and Philox position.  reset() keeps the values and refills from them.  From the first successful setter on the batch runs the _hp
    form of its kernel (hypers_differ, dominant_kernel).  A view of the batch: it owns nothing."""

    CALLS = BatchHypers.CALLS

    def __init__(self, batch):
        family = {"ctk_cem_batch": "cem", "ctk_rpgd_batch": "rpgd"}.get(getattr(batch, "_BATCH", None))
        if family is None:
            raise TypeError(f"FamilyHypers is the view of a CtkCemBatch or a CtkRpgdBatch, not of {type(batch).__name__} "
                            "(an MPPI batch has batch.hypers; a CtkEngine takes its hyper-parameters at creation)")
        self._batch, self.family, self.names = batch, family, _FAMILY_HYPERS[family]

    def _entry(self, entry: str):
        """the family's hyper-parameter entry `entry` (of the problem prefix; "batch_set_hyper": the whole-batch one)"""
        b = self._batch
        return getattr(b._lib, f"{b._BATCH}_set_hyper" if entry == "batch_set_hyper" else f"{b._PROBLEM}_{entry}")

    def set_problem_hypers(self, name: str, values, ids=None):
        """hyper-parameter `name` of the problems in ids (None: all): values a scalar or [n], one per listed problem in the order of
        ids.  Takes effect at the problem's next step."""
        b = self._batch
        hid, idv, n, vals = family_hyper_args(self.family, b.B, name, values, ids, num_rollouts=b.N)
        b._check(self._entry("set_hyper")(b._h, n, _ptr(idv), hid, _ptr(vals)))

    def set_hyper(self, name: str, value: float):
        """hyper-parameter `name` of every problem"""
        b = self._batch
        hid, _, _, vals = family_hyper_args(self.family, b.B, name, value, None, num_rollouts=b.N)
        b._check(self._entry("batch_set_hyper")(b._h, hid, float(vals[0])))

    def get_problem_hyper(self, name: str, problem: int) -> float:
        b = self._batch
        if name not in self.names:
            raise ValueError(f"unknown hyper-parameter {name!r} ({self.family.upper()} has {', '.join(self.names)})")
        v = C.c_float()
        if self._entry("get_hyper")(b._h, b._problem(problem), self.names[name], C.byref(v)) != 0:
            raise CtkError(f"{b._PROBLEM}_get_hyper({problem}, {name!r}) failed")
        return v.value

    def get_problem_hypers(self, name: str) -> np.ndarray:
        """[B] hyper-parameter `name` of every problem"""
        return np.array([self.get_problem_hyper(name, p) for p in range(self._batch.B)], np.float32)

    def set_problem_limits(self, low, high, ids=None):
        """the input limits (action_low, action_high) of the problems in ids (None: all): each a scalar, [C] or [n, C].  The next step
        clips to them; reset() refills from them (CEM: the mean with their middle; RPGD: the draws mapped onto them)."""
        b = self._batch
        _, idv, n, (lo, hi) = family_hyper_args(self.family, b.B, "limits", (low, high), ids, b.C)
        b._check(self._entry("set_limits")(b._h, n, _ptr(idv), _ptr(lo), _ptr(hi)))

    def get_problem_limits(self, problem: int):
        """(low [C], high [C]) of a problem"""
        b = self._batch
        lo, hi = np.empty(b.C, np.float32), np.empty(b.C, np.float32)
        if self._entry("get_limits")(b._h, b._problem(problem), _ptr(lo), _ptr(hi)) != 0:
            raise CtkError(f"{b._PROBLEM}_get_limits({problem}) failed")
        return lo, hi

    def hypers_differ(self) -> int:
        """1 once a set_problem_hypers, set_hyper or set_problem_limits has succeeded on this batch (sticky), else 0"""
        b = self._batch
        return int(self._entry("hypers_differ")(b._h))


# ---- closed-loop episodes of a batch on the device (include/ctk_hip_run.h: ctk_batch_run / ctk_batch_plant_*; ctk_hip_loop.h) ------------------
class BatchClosedLoop:
    """CtkMppiBatch.closed_loop / CtkMppiMlpBatch.closed_loop / CtkMppiGruBatch.closed_loop, and BatchClosedLoop(cem_batch) / BatchClosedLoop(rpgd_batch) for a
    CtkCemBatch or CtkRpgdBatch (the constructor is their way in: those classes have no closed_loop attribute): the batch's closed loops
    run on the device (kernel ctk_batch_plant<ENV>, or the family's ctk_cem_batch_plant<ENV> / ctk_rpgd_batch_plant<ENV>, between the
    controller launches), and the plants they run against.  A view of the batch: it owns nothing.  Problem p's plant has, for every
    parameter, the value set here (set_plant_params), else the problem's own current controller value: a batch that sets none controls
    exactly the plant it models.  For the MLP batch the learned network plans and the plant is the analytic CartPole.  With equal noise
    seeds, positions, sigmas and plant tables the noisy plants of all families draw the same disturbances: optimizers can be compared
    under common random numbers.  An RPGD problem must have been reset before its first run, as before its first step."""

    def __init__(self, batch):
        self._batch = batch

    def _entry(self, name: str):
        return getattr(self._batch._lib, f"{self._batch._BATCH}_{name}")

    @property
    def last_run_first_bad(self):
        """[n] per problem of the last run: the first step whose input is not finite, or -1 (None before the first run)"""
        return getattr(self._batch, "last_run_first_bad", None)

    def run(self, S0, steps: int, u_prev=None, ids=None, plant_substeps=None, samples=None):
        """`steps` closed-loop MPC steps of the problems in ids (None: all) from the states S0 [n, num_states], the plant integrated on
        the device between the controller launches: bit for bit the loop `u = batch.step(S); S = plant_step(S, u)`.  u_prev [n, C] is the
        first step's previous input (None: every problem's own last output).  plant_substeps: the plant's Euler sub-steps per dt (None:
        the controller's intermediate_steps).  The draws are the device Philox's: a run has no place for per-step sample buffers
        (samples must stay None).  Returns (states [n, steps + 1, S], inputs [n, steps, C]); last_run_first_bad [n] (here and on the
        batch) is, per problem, the first step whose input is not finite, or -1.  CtkError naming the problems whose in-launch hand-off
        timed out in some step: the traces are then in batch.last_run, valid for the other problems."""
        b = self._batch
        idv, n, sub = batch_run_args(b.B, b.S, b.C, S0, steps, u_prev, ids, plant_substeps, samples)
        ids_p, up_p, _, _ = b._step_args(n, idv, S0, u_prev, None)
        states = np.empty((n, int(steps) + 1, b.S), np.float32)
        inputs = np.empty((n, int(steps), b.C), np.float32)
        bad = np.full(n, -1, np.int32)
        rc = self._entry("run")(b._h, n, ids_p, b._s_p, up_p, int(steps), sub, _ptr(states), _ptr(inputs), _ptr(bad))
        b.last_run_first_bad = bad
        if rc:
            b.last_run = (states, inputs)
            b._check(rc)
        return states, inputs

    def plant_step(self, S, U, ids=None, plant_substeps=None) -> np.ndarray:
        """one step of the plants of the problems in ids (None: all) on the device: S [n, num_states], U [n, C] in the units step()
        returns.  Returns the next states [n, num_states].  No controller state, sequence number or Philox position changes."""
        b = self._batch
        idv, n, sub = batch_run_args(b.B, b.S, b.C, S, 1, U, ids, plant_substeps, None, what=("S", "U"))
        if U is None:
            raise ValueError(f"U must have shape ({n}, {b.C}): one row per listed problem, got None")
        s = _f32(np.asarray(S).reshape(n, b.S))
        u = _f32(np.asarray(U).reshape(n, b.C))
        out = np.empty((n, b.S), np.float32)
        b._check(self._entry("plant_step")(b._h, n, _ptr(idv), _ptr(s), _ptr(u), sub, _ptr(out)))
        return out

    def set_plant_params(self, name: str, values, ids=None):
        """parameter `name` of the PLANTS of the problems in ids (None: all): values a scalar or [n].  The controllers keep planning with
        their own values (set_param / set_problem_params); a plant parameter that was never set here follows its problem's controller."""
        b = self._batch
        pid, idv, n, vals = batch_param_args(b.param_names, b.B, name, values, ids)
        b._check(self._entry("plant_set_param")(b._h, n, _ptr(idv), pid, _ptr(vals)))

    def get_plant_params(self, name: str) -> np.ndarray:
        """[B] parameter `name` of every problem's plant: the override, else the problem's own controller value"""
        b = self._batch
        if name not in b.param_names:
            raise ValueError(f"unknown parameter {name!r} for this environment (it has {', '.join(b.param_names)})")
        v, out = C.c_float(), np.empty(b.B, np.float32)
        for p in range(b.B):
            if self._entry("plant_get_param")(b._h, p, b.param_names.index(name), C.byref(v)) != 0:
                raise CtkError(f"{b._BATCH}_plant_get_param({p}, {name!r}) failed")
            out[p] = v.value
        return out

    def clear_plant_params(self):
        """drop every plant override: each plant is again the one its controller models"""
        b = self._batch
        b._check(self._entry("plant_clear_params")(b._h))

    # ---- the stochastic plant and the realised cost (include/ctk_hip_episode.h; kernel ctk_batch_plant_noisy<ENV>) ----
    def set_noise(self, process=None, measurement=None, ids=None):
        """per-step standard deviations, in state units, of the process noise (added to the true next state) and the measurement noise
        (added to what the controller is given) of the problems in ids (None: all).  Each: None (leave as is), a scalar, [S] or [n, S].
        A component at 0 gets no noise.  run() and plant_step() ignore both."""
        b = self._batch
        checked = [(kind, batch_noise_args(b.B, b.S, sigma, ids, what)) for kind, what, sigma in ((0, "process", process), (1, "measurement", measurement))
                   if sigma is not None]
        for kind, (idv, n, sg) in checked:
            b._check(self._entry("plant_set_noise")(b._h, n, _ptr(idv), kind, _ptr(sg)))

    def get_noise(self):
        """(process [B, S], measurement [B, S]): every problem's standard deviations"""
        b = self._batch
        out = np.zeros((2, b.B, b.S), np.float32)
        for kind in (0, 1):
            for p in range(b.B):
                row = np.zeros(b.S, np.float32)
                if self._entry("plant_get_noise")(b._h, p, kind, _ptr(row)) != 0:
                    raise CtkError(f"{b._BATCH}_plant_get_noise({p}, {kind}) failed")
                out[kind, p] = row
        return out[0], out[1]

    def clear_noise(self):
        """every standard deviation back to 0; the noise seeds and positions stay"""
        b = self._batch
        b._check(self._entry("plant_clear_noise")(b._h))

    def set_noise_seeds(self, seeds, ids=None):
        """the Philox key of the noise of the problems in ids (None: all), one uint64 per listed problem (at creation: the controller's seed)"""
        b = self._batch
        idv = batch_ids(b.B, ids)
        n = b.B if idv is None else int(idv.size)
        sd = _CtkBatch._seeds(n, seeds)
        if sd is None:
            raise ValueError(f"seeds must have one entry per listed problem ({n}), got None")
        b._check(self._entry("plant_set_noise_seed")(b._h, n, _ptr(idv), _ptr(sd)))

    def get_noise_seeds(self) -> np.ndarray:
        """[B] uint64: every problem's noise seed"""
        b = self._batch
        v, out = C.c_uint64(), np.zeros(b.B, np.uint64)
        for p in range(b.B):
            if self._entry("plant_get_noise_seed")(b._h, p, C.byref(v)) != 0:
                raise CtkError(f"{b._BATCH}_plant_get_noise_seed({p}) failed")
            out[p] = v.value
        return out

    def noise_position(self, problem: int) -> int:
        """the problem's noise position: one per transition of the noisy plant (episodes, plant_step_noisy), 0 at creation"""
        b = self._batch
        v = C.c_uint32()
        b._check(self._entry("plant_noise_get_position")(b._h, b._problem(problem), C.byref(v)))
        return int(v.value)

    def set_noise_position(self, problem: int, pos: int):
        b = self._batch
        b._check(self._entry("plant_noise_set_position")(b._h, b._problem(problem), int(pos) & 0xFFFFFFFF))

    def plant_step_noisy(self, S, U, U_prev, ids=None, plant_substeps=None):
        """one transition of the noisy plants of the problems in ids (None: all): true states S [n, num_states], inputs U [n, C] and the
        inputs before them U_prev [n, C] (required: the cost's input-change term).  Returns (S_next, Y_next, cost): the true next states,
        what the controllers are given, and the realised stage cost of (S, U, U_prev) [n].  Advances the listed problems' noise
        positions; no controller state, sequence number or Philox position changes."""
        b = self._batch
        idv, n, sub = batch_run_args(b.B, b.S, b.C, S, 1, U, ids, plant_substeps, None, what=("S", "U"))
        if U is None:
            raise ValueError(f"U must have shape ({n}, {b.C}): one row per listed problem, got None")
        if U_prev is None:
            raise ValueError(f"U_prev must have shape ({n}, {b.C}): one row per listed problem, got None")
        batch_run_args(b.B, b.S, b.C, S, 1, U_prev, ids, None, None, what=("S", "U_prev"))
        s = _f32(np.asarray(S).reshape(n, b.S))
        u = _f32(np.asarray(U).reshape(n, b.C))
        up = _f32(np.asarray(U_prev).reshape(n, b.C))
        s_next, y_next, cost = np.empty((n, b.S), np.float32), np.empty((n, b.S), np.float32), np.empty(n, np.float32)
        b._check(self._entry("plant_step_noisy")(b._h, n, _ptr(idv), _ptr(s), _ptr(u), _ptr(up), sub, _ptr(s_next), _ptr(y_next), _ptr(cost)))
        return s_next, y_next, cost

    def episodes(self, S0, steps: int, u_prev=None, ids=None, plant_substeps=None, Y0=None) -> Episodes:
        """run() against the noisy plant, with the realised cost: `steps` closed-loop MPC steps of the problems in ids (None: all) from
        the TRUE states S0 [n, num_states]; the controllers are given the observations (Y0 [n, num_states] at the first step, None: S0).
        Bit for bit the loop `U = batch.step(Y); S, Y, c = plant_step_noisy(S, U, U_prev)`.  u_prev [n, C] is the input before the first
        one, for the controller and for the first cost (None: every problem's own last output, what set_state restored included).  Returns
        Episodes(states [n, steps + 1, S], observations [n, steps + 1, S], inputs [n, steps, C], costs [n, steps]); an episode continues
        from (states[:, -1], observations[:, -1]).  last_run_first_bad and the CtkError of a timed-out hand-off are run()'s (the traces
        are then in batch.last_run)."""
        b = self._batch
        idv, n, sub = batch_episode_args(b.B, b.S, b.C, S0, steps, u_prev, ids, plant_substeps, Y0)
        ids_p, up_p, _, _ = b._step_args(n, idv, S0, u_prev, None)
        y0 = None if Y0 is None else _f32(np.asarray(Y0).reshape(n, b.S))
        out = Episodes(np.empty((n, int(steps) + 1, b.S), np.float32), np.empty((n, int(steps) + 1, b.S), np.float32),
                       np.empty((n, int(steps), b.C), np.float32), np.empty((n, int(steps)), np.float32))
        bad = np.full(n, -1, np.int32)
        rc = self._entry("episodes")(b._h, n, ids_p, b._s_p, _ptr(y0), up_p, int(steps), sub, _ptr(out.states), _ptr(out.observations),
                                     _ptr(out.inputs), _ptr(out.costs), _ptr(bad))
        b.last_run_first_bad = bad
        if rc:
            b.last_run = out
            b._check(rc)
        return out

# ---- batched MPPI with the MLP predictor (include/ctk_hip.h: ctk_mlp_batch_* / ctk_mlp_problem_*) --------------------------------------
def mlp_weight_count(num_states: int, num_control_inputs: int, hidden=(32, 32)) -> int:
    """floats of one (S+C)-h1-h2-S MLP in the layout of ctk_set_predictor_weights: W1, b1, W2, b2, W3, b3 (ctk_mlp_batch_weight_count)"""
    i, s, (h1, h2) = int(num_states) + int(num_control_inputs), int(num_states), (int(hidden[0]), int(hidden[1]))
    return i * h1 + h1 + h1 * h2 + h2 + h2 * s + s


class CtkMppiMlpBatch(CtkMppiBatch):
    """Owns one ctk_mlp_batch: num_problems independent MPPI controllers of ONE configuration whose plant model is a learned MLP, stepped
    by one kernel launch per step.  Problem p behaves bit for bit like CtkEngine("mppi", "MLP", seed=seeds[p], predictor_hidden=...) given
    the same calls, set_predictor_weights and set_param among them.  The methods are CtkMppiBatch's; the network is the plant here, so
    every problem has its own: set_weights gives all problems one network, set_problem_weights the listed problems one each.  A problem
    steps only once it has weights.  predictor_hidden = (h1, h2): the hidden widths of all the batch's networks (default 32 / 32, at most
    32; narrower ones are embedded exactly).  CartPole only."""

    _BATCH, _PROBLEM = "ctk_mlp_batch", "ctk_mlp_problem"

    def __init__(self, num_problems: int, *, seeds=None, predictor_hidden=None, environment: str = "CartPole", optimizer: str = "mppi",
                 predictor: str = "MLP", num_rollouts: int, mpc_horizon: int, dt: float, action_low: float = -1.0, action_high: float = 1.0,
                 period_interpolation_inducing_points: int = 1, seed: int = 0, device: int = 0, intermediate_steps: int = 1,
                 materialize_trajectories: bool = False, global_rollout_offset: int = 0, num_states: int = None,
                 num_control_inputs: int = None, generic_kernels: bool = False, **kw):
        B = self._count(num_problems)
        if optimizer != "mppi":
            raise NotImplementedError(f"a batch steps MPPI controllers only (optimizer {optimizer!r}); the other optimizers run as CtkEngine")
        if predictor != "MLP":
            raise NotImplementedError(f"this batch rolls out the MLP predictor only (predictor {predictor!r}): the analytic one is CtkMppiBatch, "
                                      "the GRU's carried hidden state has no batch form (CtkEngine)")
        if environment != "CartPole" or generic_kernels:
            raise NotImplementedError(f"the MLP batch kernel is CartPole's matrix-core kernel (environment {environment!r}, generic_kernels "
                                      f"{bool(generic_kernels)}); the template network kernels run as CtkEngine")
        hidden = (32, 32) if predictor_hidden is None else tuple(int(x) for x in np.asarray(predictor_hidden).reshape(-1))
        if len(hidden) != 2 or min(hidden) < 1:
            raise ValueError(f"predictor_hidden must be two widths >= 1 (h1, h2), got {predictor_hidden!r}")
        if max(hidden) > 32:
            raise NotImplementedError(f"the MLP batch kernel holds 32 units per hidden layer (predictor_hidden {hidden}); wider networks run as CtkEngine")
        self.predictor_hidden = hidden
        if predictor_hidden is not None:
            kw = dict(kw, predictor_hidden1=hidden[0], predictor_hidden2=hidden[1])
        self._open(B, self._seeds(B, seeds), "mppi", "MLP", environment, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                   action_low=action_low, action_high=action_high,
                   period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                   intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                   global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                   generic_kernels=generic_kernels, **kw)
        self._per = int(self._b.samples_needed(self._h))
        self._wn = mlp_weight_count(self.S, self.C, hidden)

    def weight_count(self) -> int:
        """floats of one problem's network (predictor_hidden's widths)"""
        return int(self._lib.ctk_mlp_batch_weight_count(self._h))

    def set_weights(self, w):
        """one network [weight_count()] for every problem"""
        w = _f32(w).ravel()
        if w.size != self._wn:
            raise ValueError(f"a network of hidden widths {self.predictor_hidden} has {self._wn} weights, got {w.size}")
        self._check(self._lib.ctk_mlp_batch_set_weights(self._h, _ptr(w), w.size))

    def set_problem_weights(self, W, ids=None):
        """W [n, weight_count()]: one network per problem in ids (None: all problems), in the order of ids; one transfer for the call"""
        idv = batch_ids(self.B, ids)
        n = self.B if idv is None else int(idv.size)
        W = _f32(W)
        if W.shape != (n, self._wn) and not (n == 1 and W.shape == (self._wn,)):
            raise ValueError(f"weights must have shape ({n}, {self._wn}): one network per listed problem, got {tuple(W.shape)}")
        self._check(self._lib.ctk_mlp_problem_set_weights(self._h, n, _ptr(idv), _ptr(W), self._wn))

    def have_weights(self, problem: int) -> bool:
        return bool(self._lib.ctk_mlp_problem_have_weights(self._h, self._problem(problem)))


# ---- batched MPPI with the GRU predictor (include/ctk_hip.h: ctk_gru_batch_* / ctk_gru_problem_*) --------------------------------------
GRU_HIDDEN_SHAPE = (2, 32)                            # a problem's carried hidden state: h1[32], h2[32] (ctk_predictor_get_hidden's 64 floats)


def gru_weight_count(num_states: int, num_control_inputs: int, hidden=(32, 32)) -> int:
    """floats of one (S+C)-h1-h2-S GRU in the layout of ctk_set_predictor_weights: per layer W_i, W_h, b_i, b_h (gate rows r|z|n), then
    W_o, b_o (ctk_gru_batch_weight_count)"""
    i, s, (a, b) = int(num_states) + int(num_control_inputs), int(num_states), (int(hidden[0]), int(hidden[1]))
    return (3 * a * i + 3 * a * a + 6 * a) + (3 * b * a + 3 * b * b + 6 * b) + (b * s + s)


def gru_batch_fit(num_rollouts: int, mpc_horizon: int, period_interpolation_inducing_points: int = 1):
    """what CtkMppiGruBatch decides from the sizes alone, without a device (ctk_gru_batch_fit): (fits, block records per problem, words
    of one record, whether the launches take the wide {value, seq} tail, dynamic LDS bytes of a launch)"""
    blocks, words, wide, lds = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = load_library().ctk_gru_batch_fit(int(num_rollouts), int(mpc_horizon), int(period_interpolation_inducing_points), C.byref(blocks),
                                          C.byref(words), C.byref(wide), C.byref(lds))
    if rc == 1:
        raise ValueError("num_rollouts, mpc_horizon and period_interpolation_inducing_points must be >= 1")
    return rc == 0, blocks.value, words.value, bool(wide.value), int(lds.value)


class CtkMppiGruBatch(CtkMppiBatch):
    """Owns one ctk_gru_batch: num_problems independent MPPI controllers of ONE configuration whose plant model is a recurrent network
    (2 x 32 GRU + dense), stepped by one rollout launch and one hidden-state launch per step.  Problem p behaves bit for bit like
    CtkEngine("mppi", "GRU", seed=seeds[p], predictor_hidden=...) given the same calls — set_predictor_weights, set_param, step, reset,
    set_state, predictor_get_hidden / predictor_set_hidden among them — the carried hidden state after every step included: a stepped
    problem's advances by (the state it was given, the u it published), an unlisted problem's does not move.  The methods are
    CtkMppiMlpBatch's, plus get_hidden / set_hidden.  predictor_hidden = (h1, h2): the hidden widths of all the batch's networks (default
    32 / 32, at most 32; narrower ones are embedded exactly).  CartPole only."""

    _BATCH, _PROBLEM = "ctk_gru_batch", "ctk_gru_problem"

    def __init__(self, num_problems: int, *, seeds=None, predictor_hidden=None, environment: str = "CartPole", optimizer: str = "mppi",
                 predictor: str = "GRU", num_rollouts: int, mpc_horizon: int, dt: float, action_low: float = -1.0, action_high: float = 1.0,
                 period_interpolation_inducing_points: int = 1, seed: int = 0, device: int = 0, intermediate_steps: int = 1,
                 materialize_trajectories: bool = False, global_rollout_offset: int = 0, num_states: int = None,
                 num_control_inputs: int = None, generic_kernels: bool = False, **kw):
        B = self._count(num_problems)
        if optimizer != "mppi":
            raise NotImplementedError(f"a batch steps MPPI controllers only (optimizer {optimizer!r}); the other optimizers run as CtkEngine")
        if predictor != "GRU":
            raise NotImplementedError(f"this batch rolls out the GRU predictor only (predictor {predictor!r}): the analytic one is CtkMppiBatch, "
                                      "the MLP is CtkMppiMlpBatch")
        if environment != "CartPole" or generic_kernels:
            raise NotImplementedError(f"the GRU batch kernel is CartPole's matrix-core kernel (environment {environment!r}, generic_kernels "
                                      f"{bool(generic_kernels)}); the template network kernels run as CtkEngine")
        hidden = (32, 32) if predictor_hidden is None else tuple(int(x) for x in np.asarray(predictor_hidden).reshape(-1))
        if len(hidden) != 2 or min(hidden) < 1:
            raise ValueError(f"predictor_hidden must be two widths >= 1 (h1, h2), got {predictor_hidden!r}")
        if max(hidden) > 32:
            raise NotImplementedError(f"the GRU batch kernel holds 32 units per hidden layer (predictor_hidden {hidden}); no GRU kernel is built "
                                      "for wider networks")
        self.predictor_hidden = hidden
        if predictor_hidden is not None:
            kw = dict(kw, predictor_hidden1=hidden[0], predictor_hidden2=hidden[1])
        self._open(B, self._seeds(B, seeds), "mppi", "GRU", environment, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                   action_low=action_low, action_high=action_high,
                   period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                   intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                   global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                   generic_kernels=generic_kernels, **kw)
        self._per = int(self._b.samples_needed(self._h))
        self._wn = gru_weight_count(self.S, self.C, hidden)

    def weight_count(self) -> int:
        """floats of one problem's network (predictor_hidden's widths)"""
        return int(self._lib.ctk_gru_batch_weight_count(self._h))

    def set_weights(self, w):
        """one network [weight_count()] for every problem; every problem's hidden state becomes zero"""
        w = _f32(w).ravel()
        if w.size != self._wn:
            raise ValueError(f"a GRU of hidden widths {self.predictor_hidden} has {self._wn} weights, got {w.size}")
        self._check(self._lib.ctk_gru_batch_set_weights(self._h, _ptr(w), w.size))

    def set_problem_weights(self, W, ids=None):
        """W [n, weight_count()]: one network per problem in ids (None: all problems), in the order of ids.  The listed problems' hidden
        states become zero; no other problem's weights or hidden state is touched"""
        idv = batch_ids(self.B, ids)
        n = self.B if idv is None else int(idv.size)
        W = _f32(W)
        if W.shape != (n, self._wn) and not (n == 1 and W.shape == (self._wn,)):
            raise ValueError(f"weights must have shape ({n}, {self._wn}): one network per listed problem, got {tuple(W.shape)}")
        self._check(self._lib.ctk_gru_problem_set_weights(self._h, n, _ptr(idv), _ptr(W), self._wn))

    def have_weights(self, problem: int) -> bool:
        return bool(self._lib.ctk_gru_problem_have_weights(self._h, self._problem(problem)))

    def get_hidden(self, ids=None) -> np.ndarray:
        """[n, 2, 32]: the carried hidden state (h1, h2) of every problem in ids (None: all), in the order of ids"""
        idv = batch_ids(self.B, ids)
        n = self.B if idv is None else int(idv.size)
        out = np.empty((n,) + GRU_HIDDEN_SHAPE, np.float32)
        self._check(self._lib.ctk_gru_problem_get_hidden(self._h, n, _ptr(idv), _ptr(out)))
        return out

    def set_hidden(self, H=None, ids=None):
        """the hidden state of every problem in ids (None: all): H [n, 2, 32] (one [2, 32] broadcasts), or None for zeros"""
        idv = batch_ids(self.B, ids)
        n = self.B if idv is None else int(idv.size)
        if H is not None:
            H = _f32(H)
            if H.shape == GRU_HIDDEN_SHAPE or H.shape == (64,):
                H = np.broadcast_to(H.reshape(GRU_HIDDEN_SHAPE), (n,) + GRU_HIDDEN_SHAPE)
            if H.size != n * 64:
                raise ValueError(f"hidden states must have shape ({n}, 2, 32): one per listed problem, got {tuple(H.shape)}")
            H = np.ascontiguousarray(H, np.float32)
        self._check(self._lib.ctk_gru_problem_set_hidden(self._h, n, _ptr(idv), _ptr(H)))


# ---- batched CEM (include/ctk_hip.h: ctk_cem_batch_*) ---------------------------------------------------------------------------------
class CtkCemBatch(_CtkBatch):
    """Owns one ctk_cem_batch: num_problems independent plain-CEM controllers of ONE configuration (the CEM keywords of CtkEngine),
    stepped together by launches of one kernel.  Problem p behaves bit for bit like CtkEngine("cem", "ODE", seed=seeds[p], ...) given the
    same calls, set_param among them: set_problem_params gives every problem its own plant, cost weights and targets, set_param the same
    value to all.  seeds: one per problem (default seed + p)."""

    _BATCH, _PROBLEM = "ctk_cem_batch", "ctk_cem_problem"

    def __init__(self, num_problems: int, *, environment: str = "CartPole", seeds=None, optimizer: str = "cem", predictor: str = "ODE",
                 num_rollouts: int, mpc_horizon: int, dt: float, action_low: float = -1.0, action_high: float = 1.0,
                 period_interpolation_inducing_points: int = 1, seed: int = 0, device: int = 0, intermediate_steps: int = 1,
                 materialize_trajectories: bool = False, global_rollout_offset: int = 0, num_states: int = None,
                 num_control_inputs: int = None, generic_kernels: bool = False, **kw):
        B = self._count(num_problems)
        if optimizer != "cem":
            raise NotImplementedError(f"a CEM batch steps plain CEM controllers only (optimizer {optimizer!r}); MPPI has CtkMppiBatch, the CEM "
                                      "variants and the other optimizers run as CtkEngine")
        if predictor != "ODE":
            raise NotImplementedError(f"the batch kernel rolls out the analytic (ODE) predictor only (predictor {predictor!r}); "
                                      "network predictors run as CtkEngine")
        seeds = self._seeds(B, seeds)
        self._known(kw)
        self._open(B, seeds, "cem", "ODE", environment, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                   action_low=action_low, action_high=action_high,
                   period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                   intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                   global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                   generic_kernels=generic_kernels, **kw)
        self.K = int(self.cfg.cem_best_k)

    def samples_needed(self, problem: int = 0) -> int:
        """draws the NEXT step of `problem` consumes (its * N * H * C: a warm-up step after creation or reset is longer)"""
        return int(self._b.samples_needed(self._h, self._problem(problem)))

    def step(self, S, samples=None, u_prev=None, ids=None) -> np.ndarray:
        """S [n, num_states], one row per stepped problem in the order of ids (None: all problems).  samples: None (device Philox), a
        host array [n, its, N, H, C] or an int device pointer to such an array; with samples every listed problem must run the same
        number of outer iterations (ValueError naming them otherwise).  u_prev [n, C] or None (every problem's own last output).
        Returns u [n, C].  CtkError naming the problems whose in-launch hand-off timed out: the other problems' rows are valid (`last_u`)."""
        idv, n, _ = batch_step_args(self.B, self.S, self.C, 0, S, None, u_prev, ids)       # ids, states, u_prev
        if samples is not None and type(samples) is not int:
            # a host array (the parity path): its size against what the listed problems' next steps draw.  Where they differ in their
            # iteration counts the library refuses the call, naming them, before it reads a sample: the array goes through as it is
            samples = _f32(samples)
            needs = {self.samples_needed(p) for p in (range(self.B) if idv is None else idv.tolist())}
            per = needs.pop()
            if not needs and (samples.size != n * per or (samples.ndim > 1 and samples.shape[0] != n)):
                raise ValueError(f"step of {n} problems consumes {n} x {per} draws ([n, its, N, H, C]), got shape {tuple(samples.shape)}")
        ids_p, up_p, sp, loc = self._step_args(n, idv, S, u_prev, samples)
        rc = self._step_fn(self._h, n, ids_p, self._s_p, up_p, sp, loc, self._u_p)
        self.last_u = self._u[:n].copy()
        if rc:
            self._check(rc)
        return self.last_u

    def reset(self, ids=None):
        idv = batch_ids(self.B, ids)
        self._check(self._b.reset(self._h, 0 if idv is None else idv.size, _ptr(idv)))

    def read(self, name: str, problem: int) -> np.ndarray:
        N, H, S, Cn = self.N, self.H, self.S, self.C
        K = self.K
        if name == "BEST_IDX":                             # the problem's own cem_best_k (FamilyHypers; self.K until a setter changed it)
            v = C.c_float()
            self._check(self._lib.ctk_cem_problem_get_hyper(self._h, self._problem(problem), CEM_HYPERS["cem_best_k"], C.byref(v)))
            K = int(v.value)
        return self._read("a CEM batch", {"Q": (N, H, Cn), "J": (N,), "TRAJ": (N, H + 1, S), "U_NOM": (1, H, Cn), "STD": (1, H, Cn),
                                          "BEST_IDX": (K,)}, name, problem)

    def get_state(self, problem: int) -> np.ndarray:
        """mu[H,C] | std[H,C] | u[C] | count of one problem (CtkEngine.get_state of a CEM engine)"""
        return self._get_state(problem, 2 * self.H * self.C + self.C + 1)


# ---- batched RPGD (include/ctk_hip.h: ctk_rpgd_batch_*) -------------------------------------------------------------------------------
class CtkRpgdBatch(_CtkBatch):
    """Owns one ctk_rpgd_batch: num_problems independent RPGD controllers of ONE configuration (the RPGD keywords of CtkEngine) with at
    most 64 plans each, any subset of them stepped by ONE kernel launch: descent, keep-k selection and warm start of every listed problem.
    Problem p behaves bit for bit like CtkEngine("rpgd", "ODE", seed=seeds[p], generic_kernels=True, ...) given the same calls (reset,
    step, set_state, set_param, set_rng_position): set_problem_params gives every problem its own plant, cost weights and targets,
    set_param the same value to all.  seeds: one per problem (default seed + p).
    generic_kernels: None means True for this class — the batch kernel is the template descent; CartPole's tuned descent (what
    CtkEngine runs with generic_kernels=False) has no batch form, and generic_kernels=False for CartPole is refused rather than
    silently differing from such an engine.  The other environments have template kernels only."""

    _BATCH, _PROBLEM = "ctk_rpgd_batch", "ctk_rpgd_problem"

    def __init__(self, num_problems: int, *, environment: str = "CartPole", seeds=None, optimizer: str = "rpgd", predictor: str = "ODE",
                 num_rollouts: int, mpc_horizon: int, dt: float, action_low: float = -1.0, action_high: float = 1.0,
                 period_interpolation_inducing_points: int = 1, seed: int = 0, device: int = 0, intermediate_steps: int = 1,
                 materialize_trajectories: bool = False, global_rollout_offset: int = 0, num_states: int = None,
                 num_control_inputs: int = None, generic_kernels: bool = None, **kw):
        B = self._count(num_problems)
        if optimizer != "rpgd":
            raise NotImplementedError(f"an RPGD batch steps RPGD controllers only (optimizer {optimizer!r}); MPPI has CtkMppiBatch, plain CEM "
                                      "CtkCemBatch, the gradient variant and the other optimizers run as CtkEngine")
        if predictor != "ODE":
            raise NotImplementedError(f"the batch kernel descends through the analytic (ODE) predictor only (predictor {predictor!r}); "
                                      "network predictors run as CtkEngine")
        seeds = self._seeds(B, seeds)
        self._known(kw)
        self._open(B, seeds, "rpgd", "ODE", environment, num_rollouts=num_rollouts, mpc_horizon=mpc_horizon, dt=dt,
                   action_low=action_low, action_high=action_high,
                   period_interpolation_inducing_points=period_interpolation_inducing_points, seed=seed, device=device,
                   intermediate_steps=intermediate_steps, materialize_trajectories=materialize_trajectories,
                   global_rollout_offset=global_rollout_offset, num_states=num_states, num_control_inputs=num_control_inputs,
                   generic_kernels=True if generic_kernels is None else generic_kernels, **kw)
        self.K = int(self.cfg.opt_keep_k)
        self._need_fn = self._b.samples_needed

    def samples_needed(self, problem: int = 0) -> int:
        """draws the NEXT step of `problem` consumes: (N - opt_keep_k) * P * C when it resamples (count % resamp_per == 0), else 0"""
        return int(self._need_fn(self._h, self._problem(problem)))

    def samples_needed_reset(self) -> int:
        """draws the reset of ONE problem consumes (N * P * C)"""
        P = -(-(self.H - 1) // int(self.cfg.period_interpolation_inducing_points)) + 1
        return self.N * P * self.C

    def step(self, S, samples=None, u_prev=None, ids=None) -> np.ndarray:
        """S [n, num_states], one row per stepped problem in the order of ids (None: all problems).  samples: None (device Philox), or a
        host array (any shape) / an int device pointer holding the concatenation, in id order, of one [N - opt_keep_k, P, C] block for
        exactly those listed problems whose samples_needed is non-zero; a host array of another total size is a ValueError with both
        numbers and changes nothing.  u_prev [n, C] or None (every problem's own last output).  Returns u [n, C].  A listed problem that
        was never reset: CtkError naming it, nothing is launched."""
        idv, n, _ = batch_step_args(self.B, self.S, self.C, 0, S, None, u_prev, ids)       # ids, states, u_prev
        if samples is not None and type(samples) is not int:
            samples = _f32(samples)
        ids_p, up_p, sp, loc = self._step_args(n, idv, S, u_prev, samples)
        if sp is None:
            cnt = 0
        elif loc == LOC_HOST:
            cnt = samples.size
        else:                          # a device buffer has no size of its own: what the listed problems draw
            cnt = sum(self.samples_needed(p) for p in (range(self.B) if idv is None else idv.tolist()))
        rc = self._step_fn(self._h, n, ids_p, self._s_p, up_p, sp, cnt, loc, self._u_p)
        if rc:
            self._check(rc)
        self.last_u = self._u[:n].copy()
        return self.last_u

    def reset(self, draws=None, ids=None):
        """optimizer_reset of the listed problems (None: all) in one launch.  draws: None (device Philox, every problem at its own
        position), a host array [n, N, P, C] or an int device pointer to one, one block per listed problem in id order."""
        idv = batch_ids(self.B, ids)
        n = self.B if idv is None else int(idv.size)
        if draws is None:
            dp, loc = None, LOC_NONE
        elif type(draws) is int:
            dp, loc = draws, LOC_DEVICE
        else:
            draws = _f32(draws)
            if draws.size != n * self.samples_needed_reset():
                raise ValueError(f"reset of {n} problems consumes {n} x {self.samples_needed_reset()} draws ([n, N, P, C]), got shape {tuple(draws.shape)}")
            dp, loc = draws.ctypes.data, LOC_HOST
        self._check(self._b.reset(self._h, 0 if idv is None else idv.size, _ptr(idv), dp, loc))

    def read(self, name: str, problem: int) -> np.ndarray:
        N, H, Cn = self.N, self.H, self.C
        return self._read("an RPGD batch", {"Q": (N, H, Cn), "J": (N,), "U_NOM": (1, H, Cn), "PLAN": (N, H, Cn), "ADAM_M": (N, H, Cn),
                                            "ADAM_V": (N, H, Cn), "AGES": (N,), "AGES_LOGGED": (N,), "BEST_IDX": (self.K,)}, name, problem)

    def state_size(self) -> int:
        return 3 * self.N * self.H * self.C + self.N + self.C + 2

    @staticmethod
    def descent_lds(environment: str, mpc_horizon: int):
        """(dynamic LDS bytes of a problem's workgroup, whether the state tape is part of it) — ctk_rpgd_template_descent_lds; when the
        tape does not fit it lives in device memory, one slice per problem.  Needs no device."""
        lib, env_id = environment_library(environment)
        fits = C.c_int()
        return int(lib.ctk_rpgd_template_descent_lds(env_id, int(mpc_horizon), C.byref(fits))), bool(fits.value)

    def get_state(self, problem: int) -> np.ndarray:
        """population, Adam m, Adam v [N,H,C] | ages [N] | u [C] | adam_step | count of one problem (CtkEngine.get_state of an RPGD engine)"""
        return self._get_state(problem, self.state_size())

