/* ctk_hip_rollout.h — rollouts of caller-supplied plans on the batch families: part of the C ABI of libctk_hip.so, included by ctk_hip.h
 * (include that; this file holds the declarations so that the list of entry points per family in ctk_hip.h stays what it is).
 * Added without an ABI bump, as the batch families were. */
#ifndef CTK_HIP_ROLLOUT_H
#define CTK_HIP_ROLLOUT_H
#include "ctk_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* which model rolls the plans out */
enum ctk_rollout_model {
    CTK_ROLLOUT_MODEL_CONTROLLER = 0,   /* what the problem's controller plans with: its predictor, its own parameters, weights and hidden state */
    CTK_ROLLOUT_MODEL_PLANT = 1         /* the analytic plant of the problem's closed loop: the effective plant table (ctk_hip_run.h) */
};

/* predictor.predict_core(s, Q) + cost.get_trajectory_cost for m caller-supplied plans of EVERY listed problem, in one transfer, one
 * launch, one copy back and one synchronisation: what a handle's ctk_rollout entry answers for one problem.  It backs the reference's
 * optimal_trajectory (optimizer_mppi.py:199-202, 222-223), plan scoring and robustness sweeps over the per-problem parameter tables.
 *  - CONTRACT: row j is bit for bit, in both outputs, what ctk_rollout of a handle of the batch's configuration returns for (S[j],
 *    u_prev[j], plans[j]) after that handle was given problem ids[j]'s parameters, weights and (GRU) hidden state; the kernel is the
 *    one that handle launches (CartPole with generic_kernels == 0: the four-wave kernel of its predictor, else the template kernel);
 *  - a rollout changes NOTHING else: the problems' J, Q, TRAJ, plans, outputs, get_state vectors, Philox positions, sequence
 *    numbers, hidden states, noise positions and plant overrides are what they were, and a later step continues as if it had not run;
 *  - n, ids: the listed problems (ids NULL: all, n ignored); any order, each problem at most once (rows are independent);
 *  - S [n,S]; u_prev [n,C], NULL = zeros (the previous input of the first stage cost);
 *  - plans [n,m,H,C] on the host or as a device pointer (plans_loc: CTK_LOC_HOST / CTK_LOC_DEVICE), taken as given: not clipped;
 *    plans NULL with m == 1: every listed problem's own current plan, read on the device from where *_read(U_NOM) reads it;
 *    1 <= m <= num_rollouts, a handle's own bound;
 *  - model CTK_ROLLOUT_MODEL_CONTROLLER: each problem's controller constants (the shared table, or its own once a *_problem_set_param
 *    has succeeded) and, for the MLP and GRU batches, its network; CTK_ROLLOUT_MODEL_PLANT: the analytic (ODE) predictor with the
 *    problem's effective plant table and plant_substeps Euler sub-steps (>= 1, or 0 = cfg.intermediate_steps), derived as ahead of
 *    *_run; plant_substeps is ignored for the controller model;
 *  - traj_out [n,m,H+1,S] and J_out [n,m]; each may be NULL;
 *  - CTK_ERR_INVALID_ARGUMENT (bad n, ids, m, plans_loc, model, negative sub-steps, m != 1 without plans) and CTK_ERR_STATE (a listed
 *    problem of a network batch has no weights and the network would roll out; an RPGD problem that was never reset is asked for its
 *    own plan): nothing is launched. */
int ctk_batch_rollout(ctk_batch* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,
                      int plant_substeps, float* traj_out, float* J_out);                /* replaces: one handle per problem, set_param x params, then predictor.predict_core + cost.get_trajectory_cost each */
int ctk_mlp_batch_rollout(ctk_mlp_batch* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,
                          int plant_substeps, float* traj_out, float* J_out);            /* replaces: the same with the MLP predictor (Predictors.py predict_core), or the analytic plant */
int ctk_gru_batch_rollout(ctk_gru_batch* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,
                          int plant_substeps, float* traj_out, float* J_out);            /* replaces: the same with the GRU predictor from each problem's carried hidden state */
int ctk_cem_batch_rollout(ctk_cem_batch* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,
                          int plant_substeps, float* traj_out, float* J_out);            /* replaces: predict_core + get_trajectory_cost per CEM controller (own plan: its mean) */
int ctk_rpgd_batch_rollout(ctk_rpgd_batch* b, int n, const int32_t* ids, const float* S, const float* u_prev, const float* plans, int plans_loc, int m, int model,
                           int plant_substeps, float* traj_out, float* J_out);           /* replaces: predict_core + get_trajectory_cost per RPGD controller (own plan: u_nom, optimizer_rpgd.py) */

#ifdef __cplusplus
}
#endif
#endif /* CTK_HIP_ROLLOUT_H */
