/* ctk_hip_episode.h — stochastic closed-loop episodes of the MPPI batches on the device, with the realised cost: part of the C ABI of
 * libctk_hip.so, included by ctk_hip.h (include that; this file holds the declarations so that the lists of entry points in ctk_hip.h
 * and ctk_hip_run.h stay what they are).  Added without an ABI bump, as the batch families and ctk_hip_run.h were. */
#ifndef CTK_HIP_EPISODE_H
#define CTK_HIP_EPISODE_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Problem p of a batch has two noise vectors, sigma_w [S] (process) and sigma_v [S] (measurement), per-step standard deviations in state
 * units, both 0 at creation; a noise seed (at creation: the problem's controller seed) and a noise position (uint32, 0 at creation).
 * One transition of problem p at position pos (kernel ctk_batch_plant_noisy<ENV>):
 *     n       = the normal draws [2 S] of the in-kernel Philox4x32-10 + Box-Muller with key = noise seed, stream 0x504C4E54, call pos,
 *               row 0 (columns [0, S) process, [S, 2 S) measurement)
 *     s_{k+1} = plant(s_k, u_k) + sigma_w * n[0:S]          the TRUE state; plant = the one of ctk_batch_plant_step, overrides included
 *     y_{k+1} = s_{k+1} + sigma_v * n[S:2S]                 what the controller is given
 *     c_k     = stage cost(s_k, u_k, u_{k-1})               with the PLANT's effective parameter table: a cost weight or target set with
 *                                                           ctk_batch_plant_set_param is a common yardstick, the controllers keep theirs
 *  - a component whose sigma is 0 is not added to (it is selected: -0.0 survives); a problem whose sigmas are all 0 draws nothing and its
 *    transition is bit for bit the one of ctk_batch_plant_step;
 *  - the position advances by one per transition of every listed problem, whatever its sigmas.  ctk_batch_run, ctk_batch_plant_step,
 *    ctk_batch_reset and ctk_batch_plant_clear_params never move it and ignore the sigmas.  Seed and position can be read and set: a
 *    disturbance realisation is replayable, and two controllers can be given common random numbers;
 *  - ctk_batch_plant_set_noise: kind 0 = process, 1 = measurement; sigma [n][S], every value finite and >= 0, else
 *    CTK_ERR_INVALID_ARGUMENT (as a bad kind, bad ids or a NULL pointer) and nothing is written.  ctk_batch_plant_clear_noise sets every
 *    sigma to 0; seeds and positions stay;
 *  - ctk_batch_plant_step_noisy: ONE launch of the noisy plant for the listed problems with the caller's true states s [n,S], inputs u
 *    [n,C] and previous inputs u_prev [n,C] (all required): s_next [n,S], y_next [n,S], cost [n].  It advances the listed problems' noise
 *    positions and nothing else;
 *  - ctk_batch_episodes: ctk_batch_run with the noisy plant.  s0 [n,S] the true start states, y0 [n,S] what the first step is given
 *    (NULL: s0); u_prev [n,C] the first step's previous input, for the controller and for c_0 (NULL: every problem's own last output, the
 *    one its first controller launch reads — what ctk_batch_set_state restored included; it is read back once per call, ahead of the
 *    launches: one small copy and synchronisation per call).  states_out and obs_out [n][n_steps+1][S] (row 0 = s0 and y0), inputs_out
 *    [n][n_steps][C], costs_out [n][n_steps], first_bad [n] (may be NULL) as for ctk_batch_run.
 *    CONTRACT: bit for bit the loop { ctk_batch_step(y) -> u; ctk_batch_plant_step_noisy(s, u, u_prev) -> s, y, c } on the same batch,
 *    the controller state, Philox and noise positions and sequence numbers afterwards included; an episode of a + b steps is an episode of
 *    a steps followed by one of b steps from (states_out[:, a], obs_out[:, a]); with all sigmas 0 the states and inputs are those of
 *    ctk_batch_run and obs_out == states_out.  Segments, the single synchronisation per segment, n_steps < 1, the sub-step count,
 *    CTK_ERR_STATE and CTK_ERR_HIP are ctk_batch_run's; the noise positions advance by the plant launches that were issued. */
int ctk_batch_plant_set_noise(ctk_batch* b, int n_ids, const int32_t* ids, int kind /* 0 process, 1 measurement */,
                              const float* sigma /* [n][S] */);                          /* replaces: the sigmas of the caller's host plant */
int ctk_batch_plant_get_noise(const ctk_batch* b, int problem, int kind, float* sigma /* [S] */);   /* replaces: reading them back */
int ctk_batch_plant_clear_noise(ctk_batch* b);                                           /* replaces: zeroing them */
int ctk_batch_plant_set_noise_seed(ctk_batch* b, int n_ids, const int32_t* ids, const uint64_t* seeds);   /* replaces: np.random.default_rng(seed) per problem */
int ctk_batch_plant_get_noise_seed(const ctk_batch* b, int problem, uint64_t* seed);     /* replaces: keeping that seed */
int ctk_batch_plant_noise_get_position(const ctk_batch* b, int problem, uint32_t* pos);  /* replaces: rng.bit_generator.state of the host generator */
int ctk_batch_plant_noise_set_position(ctk_batch* b, int problem, uint32_t pos);         /* replaces: restoring it */
int ctk_batch_plant_step_noisy(ctk_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev, int substeps,
                               float* s_next, float* y_next, float* cost);               /* replaces: host plant + rng.normal + a hand-written stage cost */
int ctk_batch_episodes(ctk_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* y0 /* NULL = s0 */,
                       const float* u_prev /* NULL = own last output */, int n_steps, int plant_substeps,
                       float* states_out /* [n][n_steps+1][S] */, float* obs_out /* [n][n_steps+1][S] */, float* inputs_out /* [n][n_steps][C] */,
                       float* costs_out /* [n][n_steps] */, int32_t* first_bad /* [n], may be NULL */);   /* replaces: n_steps x { ctk_batch_step; host plant; rng.normal; host cost } */

/* the same for the MLP batch: the learned network plans, the noisy plant is the analytic CartPole.  An episode that lists a problem
 * without weights is CTK_ERR_STATE, as a run is, and launches nothing. */
int ctk_mlp_batch_plant_set_noise(ctk_mlp_batch* b, int n_ids, const int32_t* ids, int kind, const float* sigma);   /* ctk_batch_plant_set_noise */
int ctk_mlp_batch_plant_get_noise(const ctk_mlp_batch* b, int problem, int kind, float* sigma);                     /* ctk_batch_plant_get_noise */
int ctk_mlp_batch_plant_clear_noise(ctk_mlp_batch* b);                                                              /* ctk_batch_plant_clear_noise */
int ctk_mlp_batch_plant_set_noise_seed(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const uint64_t* seeds);     /* ctk_batch_plant_set_noise_seed */
int ctk_mlp_batch_plant_get_noise_seed(const ctk_mlp_batch* b, int problem, uint64_t* seed);                        /* ctk_batch_plant_get_noise_seed */
int ctk_mlp_batch_plant_noise_get_position(const ctk_mlp_batch* b, int problem, uint32_t* pos);                     /* ctk_batch_plant_noise_get_position */
int ctk_mlp_batch_plant_noise_set_position(ctk_mlp_batch* b, int problem, uint32_t pos);                            /* ctk_batch_plant_noise_set_position */
int ctk_mlp_batch_plant_step_noisy(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* s, const float* u, const float* u_prev,
                                   int substeps, float* s_next, float* y_next, float* cost);                         /* ctk_batch_plant_step_noisy */
int ctk_mlp_batch_episodes(ctk_mlp_batch* b, int n_ids, const int32_t* ids, const float* s0, const float* y0, const float* u_prev, int n_steps,
                           int plant_substeps, float* states_out, float* obs_out, float* inputs_out, float* costs_out,
                           int32_t* first_bad);                                                                      /* ctk_batch_episodes */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_EPISODE_H */
