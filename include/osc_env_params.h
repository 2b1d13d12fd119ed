/*
 * osc_env_params.h -- per-environment friction, torque and normal-force bounds and task weights.
 * The model descriptor (osc_model_desc) holds one value of each for the whole batch; the entry
 * points below take, next to the usual inputs, an optional block of device arrays that replaces
 * them env by env (domain randomisation, per-terrain friction, derated actuators, policies that
 * output task weights or a normal-force cap).  Part of libosc_batch.so; same return codes as
 * osc_batch.h; additive to ABI 4 (every existing entry point is unchanged).
 */
#ifndef OSC_ENV_PARAMS_H_
#define OSC_ENV_PARAMS_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All DEVICE pointers, fp64, env-major.  Each field is nullable: NULL = the model's own value for
 * every env.  A NULL osc_env_params*, or one with every field NULL, gives the results of the
 * entry point without the _env suffix, bitwise. */
typedef struct {
  const double* mu;     /* [nenv]       friction coefficient of the pyramid rows                 */
  const double* u_lb;   /* [nenv][nu]   |v| >= infinity / 1e10 = no row, as in the descriptor     */
  const double* u_ub;   /* [nenv][nu]                                                            */
  const double* fz_lb;  /* [nenv]       replaces z_lb[2] (still multiplied by the contact mask)  */
  const double* fz_ub;  /* [nenv]       replaces z_ub[2]                                         */
  const double* w_pos;  /* [nenv][ns]   translational task weight per site                       */
  const double* w_rot;  /* [nenv][ns]   rotational task weight per site                          */
} osc_env_params;

/* Which kernel reads what: the weights act in the assembly (osc_batch_solve_env,
 * osc_batch_solve_warm_env, osc_batch_assemble_env); mu, the torque box and the fz bounds act in
 * the solve and in the dual kernel.  The solve_assembled entries take the whole block and read
 * only the latter five: the weights of the reduced QP are those its osc_batch_assemble_env call was
 * given.  w_torque, w_reg, infinity, eps_mu, max_iter and the wheel fields stay per model.
 *
 * Validity is checked per env on the device, where the rows are set up -- no host sync, no
 * host-side look at device data.  An env is invalid when it fails what osc_model_create enforces
 * on the same descriptor fields (u_lb < u_ub strictly on every joint) or carries a NaN, a
 * non-finite mu or a non-finite weight.  Such an env returns OSC_SOLVE_NUMERICAL with NaN
 * outputs, exactly as an env with NaN inputs does; every other env of the batch is unaffected,
 * bitwise.
 *
 * Warm start: the values may change from tick to tick; the warm start floors slacks and
 * multipliers as always.  A change in WHICH bounds exist for an env (a bound going from finite to
 * absent or back) changes the env's rows: the caller must clear that env's valid flag (the first
 * double of its warm-state record, osc_warm_state_bytes / nenv apart) so that it starts cold.
 *
 * `extras`: nullable; only its `y` (the duals) is used, wheel_dir must be NULL.  The
 * solve_assembled entries export no duals, as their counterparts: `y` must be NULL there.
 *
 * Refused with OSC_ERR_INVALID_ARGUMENT, nothing enqueued: a model with wheel rows; a model created
 * with refine_steps = 0; a pointer that is not 8-byte aligned.
 *
 * The _env entries run without the lockstep compaction of large cold batches (from four rounds of
 * wavefronts per SIMD): results are bitwise the same, throughput there is about 1 % lower. */
int osc_batch_solve_env(const osc_model* model, int32_t nenv, const double* M, const double* C,
                        const double* J, const double* b, const double* T,
                        const double* contact_mask, const osc_env_params* env_params,
                        const osc_solve_extras* extras, double* tau, double* x, int32_t* status,
                        int32_t* iters, void* workspace, size_t workspace_bytes, void* stream);

int osc_batch_solve_warm_env(const osc_model* model, int32_t nenv, const double* M,
                             const double* C, const double* J, const double* b, const double* T,
                             const double* contact_mask, const osc_env_params* env_params,
                             const osc_solve_extras* extras, double* tau, double* x,
                             int32_t* status, int32_t* iters, double* warm_state,
                             size_t warm_state_bytes, void* workspace, size_t workspace_bytes,
                             void* stream);

int osc_batch_assemble_env(const osc_model* model, int32_t nenv, const double* M, const double* C,
                           const double* J, const double* b, const double* T,
                           const double* contact_mask, const osc_env_params* env_params,
                           const osc_solve_extras* extras, void* workspace, size_t workspace_bytes,
                           void* stream);

int osc_batch_solve_assembled_env(const osc_model* model, int32_t nenv, const double* contact_mask,
                                  const osc_env_params* env_params, const osc_solve_extras* extras,
                                  double* tau, double* x, int32_t* status, int32_t* iters,
                                  void* workspace, size_t workspace_bytes, void* stream);

int osc_batch_solve_assembled_warm_env(const osc_model* model, int32_t nenv,
                                       const double* contact_mask,
                                       const osc_env_params* env_params,
                                       const osc_solve_extras* extras, double* tau, double* x,
                                       int32_t* status, int32_t* iters, double* warm_state,
                                       size_t warm_state_bytes, void* workspace,
                                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* OSC_ENV_PARAMS_H_ */
