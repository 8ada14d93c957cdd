/* ctk_hip_run.h — closed-loop episodes of the MPPI batches on the device: part of the C ABI of libctk_hip.so, included by ctk_hip.h
 * (include that; this file holds the declarations so that the list of entry points per family in ctk_hip.h stays what it is).
 * Added without an ABI bump, as the batch families were. */
#ifndef CTK_HIP_RUN_H
#define CTK_HIP_RUN_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* closed-loop episodes on the device: ctk_batch_run runs n_steps MPC steps of every listed problem, the plant integrated on the device
 * between the controller launches (kernel ctk_batch_plant<ENV>: one Env<ENV>::step per problem and step, the one-step plant the rollout
 * kernels integrate, with the checked sin / cos), and returns the realised traces.  The host synchronises once per segment of a run.
 *  - CONTRACT: ctk_batch_run is bit for bit the loop { ctk_batch_step(s) -> u; ctk_batch_plant_step(s, u) -> s } on the same batch: the
 *    traces, and afterwards U_NOM, J, Q and TRAJ (the last step's), the ctk_batch_get_state vector, every problem's Philox position and
 *    the consumed sequence numbers; a later ctk_batch_step or ctk_batch_run continues as if the loop had been stepped;
 *  - the plant: problem p's plant has, for parameter id, the override set by ctk_batch_plant_set_param (ids and values as for
 *    ctk_problem_set_param), else the problem's own CURRENT controller value — a batch that never sets an override controls exactly the
 *    plant it models, and a later ctk_problem_set_param / ctk_batch_set_param moves the un-overridden plant with it.  An override does not
 *    change what the controller plans with and does not turn on the per-problem form of its kernel.  ctk_batch_plant_get_param reads the
 *    effective value, ctk_batch_plant_clear_params drops every override.  The plant's time step is cfg.dt; its Euler sub-step count is
 *    an argument (substeps >= 1, or 0 = cfg.intermediate_steps; negative: CTK_ERR_INVALID_ARGUMENT).  The plants' constants are
 *    re-derived for the problems whose effective table or sub-step count changed and travel in one transfer ahead of a run;
 *  - ctk_batch_plant_step: ONE launch of the plant kernel for the listed problems with the caller's states s [n,S] and inputs u [n,C]
 *    (in the units ctk_batch_step returns), s_next [n,S]; it changes no controller state, sequence number or Philox position;
 *  - ctk_batch_run: s0 [n,S]; u_prev [n,C] is the first step's previous input (NULL: every problem's own last output), the later
 *    steps take the problem's own last output; states_out [n][n_steps+1][S] (row 0 = s0), inputs_out [n][n_steps][C]; first_bad [n]
 *    (may be NULL) = the first step whose input is not finite, or -1.  The draws are the in-kernel Philox's (there is no place for
 *    per-step sample buffers).  All step records of a segment travel in one transfer; runs longer than a segment (256 steps;
 *    CTK_BATCH_RUN_SEGMENT_STEPS, environment, diagnostic, lowers it, never raises it) go segment by segment, and the results do not
 *    depend on the segmentation.  n_steps < 1: CTK_ERR_INVALID_ARGUMENT.  CTK_ERR_STATE = the in-launch hand-off timed out in some step
 *    of the problems the message names: that step published NaN, the plant propagated it, and first_bad says where; the other
 *    problems' traces are valid.  CTK_ERR_HIP: the counters reflect the steps that were launched, the traces are not valid. */
int ctk_batch_plant_set_param(ctk_batch* b, int n_ids, const int32_t* ids, int id, const float* values);   /* replaces: ctk_set_param on a second, "true plant" handle per problem */
int ctk_batch_plant_get_param(const ctk_batch* b, int problem, int id, float* value);   /* replaces: ctk_get_param of that handle */
int ctk_batch_plant_clear_params(ctk_batch* b);                                         /* replaces: re-creating it */
int ctk_batch_plant_step(ctk_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps,
                         float* s_next);                                                /* replaces: the caller's host plant, s' = f(s, u) per problem */
int ctk_batch_run(ctk_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev /* NULL = own last output */, int n_steps,
                  int plant_substeps, float* states_out /* [n][n_steps+1][S] */, float* inputs_out /* [n][n_steps][C] */,
                  int32_t* first_bad /* [n], may be NULL */);                           /* replaces: n_steps x { ctk_batch_step; host plant } */

/* closed-loop episodes on the device, the same for the MLP batch (ctk_mlp_batch_* of ctk_hip.h): the learned network plans, the PLANT is the analytic
 * CartPole with the problem's parameter table and the overrides set here.  A run that lists a problem without weights is CTK_ERR_STATE,
 * as a step is. */
int ctk_mlp_batch_plant_set_param(ctk_mlp_batch* b, int n_ids, const int32_t* ids, int id, const float* values);   /* ctk_batch_plant_set_param */
int ctk_mlp_batch_plant_get_param(const ctk_mlp_batch* b, int problem, int id, float* value);  /* ctk_batch_plant_get_param */
int ctk_mlp_batch_plant_clear_params(ctk_mlp_batch* b);                                         /* ctk_batch_plant_clear_params */
int ctk_mlp_batch_plant_step(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps,
                             float* s_next);                                                    /* ctk_batch_plant_step */
int ctk_mlp_batch_run(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev, int n_steps, int plant_substeps,
                      float* states_out, float* inputs_out, int32_t* first_bad);                /* ctk_batch_run */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_RUN_H */
