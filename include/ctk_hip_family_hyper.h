/* ctk_hip_family_hyper.h — per-problem optimizer hyper-parameters and input limits of the CEM and RPGD batches: part of the C ABI of
 * libctk_hip.so, included by ctk_hip.h (include that; this file holds the declarations so that the lists of entry points in the other
 * headers, ctk_hip_hyper.h's among them, stay what they are).  Added without an ABI bump, as the batch families and the other headers
 * were: ctk_abi_version() stays 6. */
#ifndef CTK_HIP_FAMILY_HYPER_H
#define CTK_HIP_FAMILY_HYPER_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The MPPI contract of ctk_hip_hyper.h, restated for these two families.  A batch is created from ONE ctk_config, and until one of the
 * setters below succeeds every problem runs with that configuration's values through exactly the launches it always had.  From the first
 * successful setter on (sticky, *_hypers_differ) the batch launches the _hp form of its kernel (ctk_cem_batch_hp<ENV, TRAJ>,
 * ctk_g_rpgd_batch_hp<ENV>; *_dominant_kernel names it), which reads every problem's values from device memory: they travel behind the
 * step records, in the records' transfer.
 *
 * Contract: problem p behaves bit for bit like a handle created (ctk_create; RPGD: with generic_kernels = 1) from the batch's
 * configuration with p's seed and p's values in the fields below, given the same calls.  A change between two steps makes the problem
 * equal to a fresh such handle that received the problem's state vector (*_get_state -> ctk_set_state) and its Philox position.  The
 * step count travels with the state: a changed problem does not repeat its warm-up, and its Adam step number keeps counting.
 * Hyper-parameters and limits are not part of the state vector; *_reset keeps them and refills from the PROBLEM's values (CEM: the mean
 * with the middle of its limits, the deviation with its cem_initial_action_stdev, optimizer_cem_tf.py:113-117; RPGD: the draws mapped
 * with its sampling constants and limits, optimizer_rpgd.py:275-296).  The plant of a closed loop does not read them.
 *
 * Values cross the ABI as float; the counts (cem_best_k, cem_outer_it, outer_its, resamp_per) must be integral, and every admissible
 * count is exact in fp32.  What stays shared, because it changes buffer shapes or the launch structure: warmup, warmup_iterations and
 * every size (both); opt_keep_k, sampling_distribution, sample_whole_control_space, shift_previous and adam_rule (RPGD).
 *
 * Refusals (CTK_ERR_INVALID_ARGUMENT, the message starts with the entry's name; nothing is changed and nothing is launched): an
 * index outside the batch, ids that are not strictly ascending, an unknown hyper-parameter, NULL values, a value that is not finite,
 * a count that is not integral, low > high for an input, and the rules *_create applies to the same fields: 1 <= cem_best_k <=
 * num_rollouts, cem_outer_it >= 1; outer_its >= 0, resamp_per >= 1.  The CEM step's refusal of caller-supplied samples for problems
 * with different iteration counts applies to the per-problem counts as it does to a warm-up step. */
enum ctk_cem_hyper {
    CTK_CEM_HYPER_BEST_K = 0,                /* optimizer_cem_tf.py:50 */
    CTK_CEM_HYPER_INITIAL_ACTION_STDEV = 1,  /* optimizer_cem_tf.py:48 */
    CTK_CEM_HYPER_STDEV_MIN = 2,             /* optimizer_cem_tf.py:49 */
    CTK_CEM_HYPER_OUTER_IT = 3,              /* optimizer_cem_tf.py:47 */
    CTK_CEM_HYPER_COUNT = 4
};
enum ctk_rpgd_hyper {
    CTK_RPGD_HYPER_LEARNING_RATE = 0,        /* optimizer_rpgd.py:226 */
    CTK_RPGD_HYPER_ADAM_BETA_1 = 1,          /* optimizer_rpgd.py:226 */
    CTK_RPGD_HYPER_ADAM_BETA_2 = 2,          /* optimizer_rpgd.py:227 */
    CTK_RPGD_HYPER_ADAM_EPSILON = 3,         /* optimizer_rpgd.py:227 */
    CTK_RPGD_HYPER_GRADMAX_CLIP = 4,         /* optimizer_rpgd.py:214 */
    CTK_RPGD_HYPER_SAMPLE_STDEV = 5,         /* optimizer_rpgd.py:197 */
    CTK_RPGD_HYPER_SAMPLE_MEAN = 6,          /* optimizer_rpgd.py:198 */
    CTK_RPGD_HYPER_UNIFORM_DIST_MIN = 7,     /* optimizer_rpgd.py:205 (read only with sample_whole_control_space == 0) */
    CTK_RPGD_HYPER_UNIFORM_DIST_MAX = 8,     /* optimizer_rpgd.py:206 */
    CTK_RPGD_HYPER_OUTER_ITS = 9,            /* optimizer_rpgd.py:195 */
    CTK_RPGD_HYPER_RESAMP_PER = 10,          /* optimizer_rpgd.py:208, :449 */
    CTK_RPGD_HYPER_COUNT = 11
};

/* ids: n_ids strictly ascending problem indices, or NULL (then n_ids is ignored: every problem, in order).  n below: the problems
 * addressed.  C: the environment's num_control_inputs. */

/* ---- ctk_cem_batch ---- */
int ctk_cem_problem_set_hyper(ctk_cem_batch* b, int n_ids, const int32_t* ids, int hyper, const float* values);   /* values [n]: the constructor argument of optimizer_cem_tf.py:24-28 stored at :47-50, one optimizer instance per problem */
int ctk_cem_problem_get_hyper(const ctk_cem_batch* b, int problem, int hyper, float* out);                        /* the value stored at optimizer_cem_tf.py:47-50 */
int ctk_cem_problem_set_limits(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* low, const float* high);   /* low, high [n][C]: control_limits, Optimizers/__init__.py:42-44 */
int ctk_cem_problem_get_limits(const ctk_cem_batch* b, int problem, float* low, float* high);                     /* low, high [C]: Optimizers/__init__.py:43-44 */
int ctk_cem_problem_hypers_differ(const ctk_cem_batch* b);                                                         /* 1 once a setter of this header has succeeded on b (sticky), else 0 */
int ctk_cem_batch_set_hyper(ctk_cem_batch* b, int hyper, float value);                                             /* every problem: optimizer_cem_tf.py:47-50 of B instances with one value */

/* ---- ctk_rpgd_batch ---- */
int ctk_rpgd_problem_set_hyper(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, int hyper, const float* values);   /* values [n]: the constructor argument of optimizer_rpgd.py:148-179 stored at :195-227 */
int ctk_rpgd_problem_get_hyper(const ctk_rpgd_batch* b, int problem, int hyper, float* out);                        /* the value stored at optimizer_rpgd.py:195-227 */
int ctk_rpgd_problem_set_limits(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* low, const float* high);   /* Optimizers/__init__.py:42-44; with sample_whole_control_space also optimizer_rpgd.py:202-203 */
int ctk_rpgd_problem_get_limits(const ctk_rpgd_batch* b, int problem, float* low, float* high);                     /* Optimizers/__init__.py:43-44 */
int ctk_rpgd_problem_hypers_differ(const ctk_rpgd_batch* b);
int ctk_rpgd_batch_set_hyper(ctk_rpgd_batch* b, int hyper, float value);                                            /* every problem: optimizer_rpgd.py:195-227 */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_FAMILY_HYPER_H */
