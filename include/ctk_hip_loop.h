/* ctk_hip_loop.h — closed-loop runs and episodes of the CEM and RPGD batches on the device: part of the C ABI of libctk_hip.so,
 * included by ctk_hip.h (include that; this file holds the declarations so that the lists of entry points in ctk_hip.h, ctk_hip_run.h
 * and ctk_hip_episode.h stay what they are).  Added without an ABI bump, as the batch families and those two headers were.
 *
 * For F in {ctk_cem_batch, ctk_rpgd_batch} the entries below are the ctk_batch_ entries of ctk_hip_run.h and ctk_hip_episode.h with the
 * handle type replaced: same arguments, same meaning, same return codes (a NULL handle: CTK_ERR_INVALID_ARGUMENT), the same plant (the
 * one-step plant of the rollout kernels with the problem's effective parameter table: override, else its own controller value), the
 * same noise (key = noise seed, stream 0x504C4E54, call = noise position, row 0), the same realised stage cost and the same segments
 * (256 steps; CTK_BATCH_RUN_SEGMENT_STEPS lowers it).  Kernels: ctk_cem_batch_plant<ENV> / ctk_cem_batch_plant_noisy<ENV> and
 * ctk_rpgd_batch_plant<ENV> / ctk_rpgd_batch_plant_noisy<ENV>, the bodies of ctk_batch_plant<ENV> / ctk_batch_plant_noisy<ENV> over the
 * family's step records.  Given equal noise seeds, positions, sigmas and plant tables, a transition of (s, u, u_prev) is bit for bit
 * the same in all families: two optimizers can be compared on one disturbance realisation.
 *  - CONTRACT: F_run is bit for bit the loop { F_step(s) -> u; F_plant_step(s, u) -> s } on the same batch, F_episodes the loop
 *    { F_step(y) -> u; F_plant_step_noisy(s, u, u_prev) -> s, y, c }: the traces, and afterwards every readable buffer, the
 *    F_get_state vector, the Philox and noise positions and the consumed sequence numbers; a later F_step, F_run or F_episodes
 *    continues as if the loop had been stepped.  The draws are the in-kernel Philox's.
 *  - CEM: step t of a segment runs warmup_iterations outer iterations exactly when it is the problem's first step after creation or
 *    reset (cfg.warmup), else cem_outer_it; its hand-off tags continue the problem's, each step by the rule of ctk_cem_batch_step (a
 *    step whose tags would wrap restarts at 1); a step of n problems is the launches ctk_cem_batch_step makes
 *    (CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH), then one plant launch.  CTK_ERR_STATE = the in-launch hand-off timed out in some step
 *    of the problems the message names, as for ctk_batch_run.
 *  - RPGD: step t runs the iterations, the Adam step offset and the resampling decision ctk_rpgd_batch_step would (first step after a
 *    reset: the warm-up count; resampling when the problem's step count is a multiple of resamp_per).  A listed problem that was never
 *    reset: CTK_ERR_STATE, nothing is launched.  This kernel has no in-launch hand-off, so there is no time-out to report.
 *  - the per-problem form (after F's *_problem_set_param): the constants of the listed problems travel once per segment, behind the
 *    segment's step records in their one transfer. */
#ifndef CTK_HIP_LOOP_H
#define CTK_HIP_LOOP_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the CEM batch (ctk_cem_batch_* of ctk_hip.h) */
int ctk_cem_batch_plant_set_param(ctk_cem_batch* b, int n_ids, const int32_t* ids, int id, const float* values);   /* ctk_batch_plant_set_param */
int ctk_cem_batch_plant_get_param(const ctk_cem_batch* b, int problem, int id, float* value);   /* ctk_batch_plant_get_param */
int ctk_cem_batch_plant_clear_params(ctk_cem_batch* b);                                         /* ctk_batch_plant_clear_params */
int ctk_cem_batch_plant_step(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps,
                             float* s_next);                                                    /* ctk_batch_plant_step */
int ctk_cem_batch_run(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev, int n_steps, int plant_substeps,
                      float* states_out, float* inputs_out, int32_t* first_bad);                /* ctk_batch_run */
int ctk_cem_batch_plant_set_noise(ctk_cem_batch* b, int n_ids, const int32_t* ids, int kind, const float* sigma);   /* ctk_batch_plant_set_noise */
int ctk_cem_batch_plant_get_noise(const ctk_cem_batch* b, int problem, int kind, float* sigma);                     /* ctk_batch_plant_get_noise */
int ctk_cem_batch_plant_clear_noise(ctk_cem_batch* b);                                                              /* ctk_batch_plant_clear_noise */
int ctk_cem_batch_plant_set_noise_seed(ctk_cem_batch* b, int n_ids, const int32_t* ids, const uint64_t* seeds);     /* ctk_batch_plant_set_noise_seed */
int ctk_cem_batch_plant_get_noise_seed(const ctk_cem_batch* b, int problem, uint64_t* seed);                        /* ctk_batch_plant_get_noise_seed */
int ctk_cem_batch_plant_noise_get_position(const ctk_cem_batch* b, int problem, uint32_t* pos);                     /* ctk_batch_plant_noise_get_position */
int ctk_cem_batch_plant_noise_set_position(ctk_cem_batch* b, int problem, uint32_t pos);                            /* ctk_batch_plant_noise_set_position */
int ctk_cem_batch_plant_step_noisy(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev,
                                   int substeps, float* s_next, float* y_next, float* cost);                         /* ctk_batch_plant_step_noisy */
int ctk_cem_batch_episodes(ctk_cem_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* y0, const float* u_prev, int n_steps,
                           int plant_substeps, float* states_out, float* obs_out, float* inputs_out, float* costs_out,
                           int32_t* first_bad);                                                                      /* ctk_batch_episodes */

/* the RPGD batch (ctk_rpgd_batch_* of ctk_hip.h) */
int ctk_rpgd_batch_plant_set_param(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, int id, const float* values);   /* ctk_batch_plant_set_param */
int ctk_rpgd_batch_plant_get_param(const ctk_rpgd_batch* b, int problem, int id, float* value);   /* ctk_batch_plant_get_param */
int ctk_rpgd_batch_plant_clear_params(ctk_rpgd_batch* b);                                         /* ctk_batch_plant_clear_params */
int ctk_rpgd_batch_plant_step(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps,
                              float* s_next);                                                     /* ctk_batch_plant_step */
int ctk_rpgd_batch_run(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev, int n_steps, int plant_substeps,
                       float* states_out, float* inputs_out, int32_t* first_bad);                 /* ctk_batch_run */
int ctk_rpgd_batch_plant_set_noise(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, int kind, const float* sigma);   /* ctk_batch_plant_set_noise */
int ctk_rpgd_batch_plant_get_noise(const ctk_rpgd_batch* b, int problem, int kind, float* sigma);                     /* ctk_batch_plant_get_noise */
int ctk_rpgd_batch_plant_clear_noise(ctk_rpgd_batch* b);                                                              /* ctk_batch_plant_clear_noise */
int ctk_rpgd_batch_plant_set_noise_seed(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const uint64_t* seeds);     /* ctk_batch_plant_set_noise_seed */
int ctk_rpgd_batch_plant_get_noise_seed(const ctk_rpgd_batch* b, int problem, uint64_t* seed);                        /* ctk_batch_plant_get_noise_seed */
int ctk_rpgd_batch_plant_noise_get_position(const ctk_rpgd_batch* b, int problem, uint32_t* pos);                     /* ctk_batch_plant_noise_get_position */
int ctk_rpgd_batch_plant_noise_set_position(ctk_rpgd_batch* b, int problem, uint32_t pos);                            /* ctk_batch_plant_noise_set_position */
int ctk_rpgd_batch_plant_step_noisy(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev,
                                    int substeps, float* s_next, float* y_next, float* cost);                          /* ctk_batch_plant_step_noisy */
int ctk_rpgd_batch_episodes(ctk_rpgd_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* y0, const float* u_prev, int n_steps,
                            int plant_substeps, float* states_out, float* obs_out, float* inputs_out, float* costs_out,
                            int32_t* first_bad);                                                                       /* ctk_batch_episodes */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_LOOP_H */
