/* ctk_hip_gru.h — closed-loop runs and episodes of the GRU batch on the device: part of the C ABI of libctk_hip.so, included by ctk_hip.h
 * (include that; this file holds the declarations so that the lists of entry points in ctk_hip_run.h, ctk_hip_episode.h and
 * ctk_hip_loop.h stay what they are).  Added without an ABI bump, as the batch families and those headers were. */
#ifndef CTK_HIP_GRU_H
#define CTK_HIP_GRU_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The entries of ctk_hip_run.h and ctk_hip_episode.h for the GRU batch (ctk_gru_batch_* of ctk_hip.h), with their signatures and their
 * contracts: the recurrent network plans, the PLANT is the analytic CartPole with the problem's parameter table and the overrides set
 * here.  Behind every step of a run or episode each listed problem's hidden state advances on the device by (what its controller was
 * given — the state in a run, the observation in an episode —, the u it published), ahead of the plant step.  So ctk_gru_batch_run is
 * bit for bit the loop { ctk_gru_batch_step(s) -> u; ctk_gru_batch_plant_step(s, u) -> s } and ctk_gru_batch_episodes the loop
 * { ctk_gru_batch_step(y) -> u; ctk_gru_batch_plant_step_noisy(s, u, u_prev) -> s, y, c }, the hidden states afterwards included.  A
 * run or episode that lists a problem without weights is CTK_ERR_STATE, as a step is, and launches nothing. */
int ctk_gru_batch_plant_set_param(ctk_gru_batch* b, int n_ids, const int32_t* ids, int id, const float* values);   /* ctk_batch_plant_set_param */
int ctk_gru_batch_plant_get_param(const ctk_gru_batch* b, int problem, int id, float* value);  /* ctk_batch_plant_get_param */
int ctk_gru_batch_plant_clear_params(ctk_gru_batch* b);                                         /* ctk_batch_plant_clear_params */
int ctk_gru_batch_plant_step(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, int substeps,
                             float* s_next);                                                    /* ctk_batch_plant_step */
int ctk_gru_batch_run(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* u_prev, int n_steps, int plant_substeps,
                      float* states_out, float* inputs_out, int32_t* first_bad);                /* ctk_batch_run */
int ctk_gru_batch_plant_set_noise(ctk_gru_batch* b, int n_ids, const int32_t* ids, int kind, const float* sigma);   /* ctk_batch_plant_set_noise */
int ctk_gru_batch_plant_get_noise(const ctk_gru_batch* b, int problem, int kind, float* sigma);                     /* ctk_batch_plant_get_noise */
int ctk_gru_batch_plant_clear_noise(ctk_gru_batch* b);                                                              /* ctk_batch_plant_clear_noise */
int ctk_gru_batch_plant_set_noise_seed(ctk_gru_batch* b, int n_ids, const int32_t* ids, const uint64_t* seeds);     /* ctk_batch_plant_set_noise_seed */
int ctk_gru_batch_plant_get_noise_seed(const ctk_gru_batch* b, int problem, uint64_t* seed);                        /* ctk_batch_plant_get_noise_seed */
int ctk_gru_batch_plant_noise_get_position(const ctk_gru_batch* b, int problem, uint32_t* pos);                     /* ctk_batch_plant_noise_get_position */
int ctk_gru_batch_plant_noise_set_position(ctk_gru_batch* b, int problem, uint32_t pos);                            /* ctk_batch_plant_noise_set_position */
int ctk_gru_batch_plant_step_noisy(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev,
                                   int substeps, float* s_next, float* y_next, float* cost);                         /* ctk_batch_plant_step_noisy */
int ctk_gru_batch_episodes(ctk_gru_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* y0, const float* u_prev, int n_steps,
                           int plant_substeps, float* states_out, float* obs_out, float* inputs_out, float* costs_out,
                           int32_t* first_bad);                                                                      /* ctk_batch_episodes */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_GRU_H */
