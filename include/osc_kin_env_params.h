/*
 * osc_kin_env_params.h -- per-environment inertial parameters of the kinematics front end (body
 * mass, COM position, joint armature), and the joint-state tick and the rollout with per-env
 * parameters of both kinds: these and the QP's (osc_env_params.h: friction, torque and
 * normal-force bounds, task weights).  Domain randomisation for callers who hold qpos / qvel on the
 * device.  Part of libosc_batch.so; same return codes as osc_batch.h; additive to ABI 4 (every
 * existing entry point is unchanged).
 */
#ifndef OSC_KIN_ENV_PARAMS_H_
#define OSC_KIN_ENV_PARAMS_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_env_params.h"
#include "osc_kinematics.h"
#include "osc_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All DEVICE pointers, fp64, env-major, 8-byte aligned.  Each field is nullable: NULL = the model's
 * own value for every env.  nbody is the kinematics model's body count (osc_kin_model_nbody: after
 * the MJCF reader's split of multi-joint bodies), nv its dof count. */
typedef struct {
  const double* mass_scale;      /* [nenv][nbody]     s: m' = s m and Ib' = s Ib (density scaling:
                                                      the body-frame inertia about the COM scales
                                                      with the mass); a massless body stays so   */
  const double* com_offset;      /* [nenv][nbody][3]  d: ipos' = ipos + d, in the body frame; Ib
                                                      about the (moved) COM is unchanged         */
  const double* armature_scale;  /* [nenv][nv]        a: dof_armature' = a dof_armature, per dof */
} osc_kin_env_params;

/* Validity is checked per env on the device, in the kinematics kernel -- no host sync, no
 * host-side look at device data.  An env is invalid when any of its values is NaN or non-finite,
 * any mass_scale is <= 0 or any armature_scale is < 0.  Every entry of such an env's M and C is
 * written as NaN; the solve then returns OSC_SOLVE_NUMERICAL with NaN outputs for it, exactly as
 * for an env with NaN inputs, and the rollout freezes it.  Every other env of the batch is
 * unaffected, bitwise.  J, b and site_xpos do not depend on the inertial parameters: they are
 * bitwise osc_batch_kinematics' for every env, invalid ones included.
 *
 * Not covered (they take no kinematics parameters yet): the multi-robot tick and the two-model
 * kinematics grid (osc_mixed.h), the host feeds (osc_host_feed.h), the backward pass
 * (osc_backward*.h) and the controller shim (osc_controller.h).  Not expressible as scale + offset:
 * a point-mass payload (it changes Ib about the COM); per-env link geometry (body and site
 * positions) is not a parameter either. */

int osc_kin_model_nbody(const osc_kin_model* model, int32_t* nbody);

/* osc_batch_kinematics with per-env inertial parameters.  `params` NULL, or with every field NULL,
 * runs osc_batch_kinematics itself (bitwise).  OSC_ERR_INVALID_ARGUMENT, nothing enqueued: what
 * osc_batch_kinematics refuses; a parameter pointer that is not 8-byte aligned. */
int osc_batch_kinematics_env(const osc_kin_model* model, int32_t nenv, const double* qpos,
                             const double* qvel, const osc_kin_env_params* params, double* M,
                             double* C, double* J, double* b, double* site_xpos, void* stream);

/* The workspace of osc_batch_solve_qpos_env: [M | C | J | b | the solve's workspace]. */
int osc_qpos_env_workspace_bytes(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                 size_t* bytes);

/* The tick from joint states with both parameter blocks: osc_batch_kinematics_env, then
 * osc_batch_solve_env, or osc_batch_solve_warm_env when `warm_state` is given (NULL = cold).  With
 * `env_params` NULL or all-NULL the solve is the plain osc_batch_solve(_warm) -- which keeps the
 * lockstep compaction of large cold batches -- so that with `kin_params` NULL or all-NULL as well
 * the results are bitwise osc_batch_solve_qpos(_warm).  `extras`: nullable; only its `y` (the
 * duals, which need `x`) is used, wheel_dir must be NULL.
 * OSC_ERR_INVALID_ARGUMENT, nothing enqueued: a `kin` / `model` pair of different robots, nenv < 0,
 * a misaligned or too small workspace (osc_qpos_env_workspace_bytes; NULL = stream-ordered
 * scratch), a parameter pointer of either block that is not 8-byte aligned, wheel_dir, and, with a
 * non-NULL `env_params`, a model with wheel rows or one created with refine_steps = 0. */
int osc_batch_solve_qpos_env(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                             const double* qpos, const double* qvel, const double* T,
                             const double* contact_mask, const osc_env_params* env_params,
                             const osc_kin_env_params* kin_params, const osc_solve_extras* extras,
                             double* tau, double* x, int32_t* status, int32_t* iters,
                             double* warm_state, size_t warm_state_bytes, void* workspace,
                             size_t workspace_bytes, void* stream);

/* osc_rollout_workspace_bytes for osc_batch_rollout_env. */
int osc_rollout_env_workspace_bytes(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                    int32_t nticks, size_t* bytes);

/* osc_batch_rollout with every tick going through osc_batch_solve_qpos_env.  Both blocks are held
 * constant over the rollout, so which bounds exist never changes between ticks and the warm-start
 * rule of osc_env_params.h is met without the caller doing anything.  An env with invalid
 * parameters is frozen for the whole rollout (state unchanged, bad_ticks = nticks).  With both
 * blocks NULL the results are bitwise osc_batch_rollout's.  Refuses what osc_batch_rollout and
 * osc_batch_solve_qpos_env refuse, before the first launch. */
int osc_batch_rollout_env(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                          const osc_rollout_args* args, const osc_env_params* env_params,
                          const osc_kin_env_params* kin_params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_KIN_ENV_PARAMS_H_ */
