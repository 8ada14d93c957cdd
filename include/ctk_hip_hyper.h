/* ctk_hip_hyper.h — per-problem MPPI hyper-parameters and input limits of the MPPI batches: part of the C ABI of libctk_hip.so, included
 * by ctk_hip.h (include that; this file holds the declarations so that the lists of entry points in the other headers stay what they
 * are).  Added without an ABI bump, as the batch families and the other four headers were: ctk_abi_version() stays 6. */
#ifndef CTK_HIP_HYPER_H
#define CTK_HIP_HYPER_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The optimizer's own numbers, per problem.  A batch is created from ONE ctk_config, and until one of the setters below succeeds every
 * problem runs with that configuration's cc_weight, R, LBD, NU, SQRTRHOINV and action_low / action_high, through exactly the launches
 * it always had.  From the first successful setter on (sticky, *_hypers_differ) the batch launches the _hp form of its kernel
 * (ctk_mppi_batch_hp<ENV, LOG>, ctk_mppi_batch_mlp_hp<LOG>, ctk_mppi_batch_gru_hp<LOG, FORM>; *_dominant_kernel names it), which reads
 * every problem's constants and limits from device memory.
 *
 * Contract: problem p behaves bit for bit like a handle created (ctk_create) from the batch's configuration with p's seed and p's
 * values in those seven fields, given the same calls.  The constants are derived by the function that derives a handle's, from a copy of
 * the configuration that carries the problem's values.  A change between two steps makes the problem equal to a fresh such handle
 * that received the problem's state vector (*_get_state -> ctk_set_state), its Philox position and, for the GRU batch, its hidden state.
 * Hyper-parameters and limits are not part of the state vector; *_reset keeps them and refills the plan with the middle of the
 * PROBLEM's limits (optimizer_mppi.py:229).  The plant of a closed loop does not read them.
 *
 * CTK_HYPER_R and CTK_HYPER_CC_WEIGHT are MPPI's correction-cost constants, the ctk_config fields R and cc_weight
 * (optimizer_mppi.py:155).  They are NOT the environment cost parameters of the same names (CTK_P_R, CTK_P_CC_WEIGHT: the stage
 * cost's input term), which *_problem_set_param sets.
 *
 * Refusals (CTK_ERR_INVALID_ARGUMENT, the message starts with the entry's name; nothing is changed and nothing is launched): an
 * index outside the batch, ids that are not strictly ascending, an unknown hyper-parameter, NULL values, a value that is not finite,
 * LBD <= 0, NU == 0, low > high for an input — the rules ctk_batch_create applies to the same fields. */
enum ctk_hyper {
    CTK_HYPER_CC_WEIGHT = 0,   /* optimizer_mppi.py:91  */
    CTK_HYPER_R = 1,           /* optimizer_mppi.py:92  */
    CTK_HYPER_LBD = 2,         /* optimizer_mppi.py:93  */
    CTK_HYPER_NU = 3,          /* optimizer_mppi.py:94  */
    CTK_HYPER_SQRTRHOINV = 4,  /* optimizer_mppi.py:95, :130 */
    CTK_HYPER_COUNT = 5
};

/* ids: n_ids strictly ascending problem indices, or NULL (then n_ids is ignored: every problem, in order).  n below: the problems
 * addressed.  C: the environment's num_control_inputs. */

/* ---- ctk_batch (the analytic predictor) ---- */
int ctk_problem_set_hyper(ctk_batch* b, int n_ids, const int32_t* ids, int hyper, const float* values);   /* values [n]: the constructor argument of optimizer_mppi.py:23-29 stored at :91-95, one optimizer instance per problem */
int ctk_problem_get_hyper(const ctk_batch* b, int problem, int hyper, float* out);                        /* the value stored at optimizer_mppi.py:91-95 */
int ctk_problem_set_limits(ctk_batch* b, int n_ids, const int32_t* ids, const float* low, const float* high);   /* low, high [n][C]: control_limits, Optimizers/__init__.py:42-44 */
int ctk_problem_get_limits(const ctk_batch* b, int problem, float* low, float* high);                     /* low, high [C]: Optimizers/__init__.py:43-44 */
int ctk_problem_hypers_differ(const ctk_batch* b);                                                         /* 1 once a setter of this header has succeeded (sticky), else 0 */
int ctk_batch_set_hyper(ctk_batch* b, int hyper, float value);                                             /* every problem: optimizer_mppi.py:91-95 of B instances with one value */

/* ---- ctk_mlp_batch ---- */
int ctk_mlp_problem_set_hyper(ctk_mlp_batch* b, int n_ids, const int32_t* ids, int hyper, const float* values);   /* optimizer_mppi.py:91-95 */
int ctk_mlp_problem_get_hyper(const ctk_mlp_batch* b, int problem, int hyper, float* out);                        /* optimizer_mppi.py:91-95 */
int ctk_mlp_problem_set_limits(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* low, const float* high);   /* Optimizers/__init__.py:42-44 */
int ctk_mlp_problem_get_limits(const ctk_mlp_batch* b, int problem, float* low, float* high);                     /* Optimizers/__init__.py:43-44 */
int ctk_mlp_problem_hypers_differ(const ctk_mlp_batch* b);
int ctk_mlp_batch_set_hyper(ctk_mlp_batch* b, int hyper, float value);                                            /* optimizer_mppi.py:91-95 */

/* ---- ctk_gru_batch ---- */
int ctk_gru_problem_set_hyper(ctk_gru_batch* b, int n_ids, const int32_t* ids, int hyper, const float* values);   /* optimizer_mppi.py:91-95 */
int ctk_gru_problem_get_hyper(const ctk_gru_batch* b, int problem, int hyper, float* out);                        /* optimizer_mppi.py:91-95 */
int ctk_gru_problem_set_limits(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* low, const float* high);   /* Optimizers/__init__.py:42-44 */
int ctk_gru_problem_get_limits(const ctk_gru_batch* b, int problem, float* low, float* high);                     /* Optimizers/__init__.py:43-44 */
int ctk_gru_problem_hypers_differ(const ctk_gru_batch* b);
int ctk_gru_batch_set_hyper(ctk_gru_batch* b, int hyper, float value);                                            /* optimizer_mppi.py:91-95 */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_HYPER_H */
