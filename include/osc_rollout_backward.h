/*
 * osc_rollout_backward.h -- backward pass of the closed-loop rollout (osc_rollout.h,
 * osc_kin_env_params.h): the vector-Jacobian product of K ticks of
 *   kinematics -> task targets -> solve -> semi-implicit Euler step
 * with respect to the initial state, the held targets and the two per-env parameter blocks, in one
 * device-resident call.  It composes the single-tick backward passes the library already has --
 * osc_batch_solve_backward_data / _env (osc_backward.h, osc_backward_env.h) and
 * osc_batch_kinematics_backward (osc_kin_backward.h) -- with the three pieces declared here: the
 * adjoint of the Euler step, the adjoint of the PD base-target producer, and the tick-to-tick
 * reduction.  Part of libosc_batch.so; same return codes as osc_batch.h; additive to ABI 4 (every
 * existing entry point, and every existing kernel, is unchanged).  All array pointers are DEVICE
 * pointers, fp64 unless noted, env-major, 8-byte aligned; `stream` is a hipStream_t (NULL =
 * default).
 *
 * A CHECKPOINTED backward: the forward call's histories are the checkpoints.  For t = K-1 .. 0 the
 * tick is recomputed from slab t (osc_batch_kinematics(_env), then the COLD solve with x and the
 * duals) and differentiated.  The solve returns the QP's exact optimum (the full-space refinement
 * ends at a KKT point), so a warm-started forward and this cold recompute agree to the solver's
 * ~1e-11; the gradients of a warm and of a cold forward agree to the chain's tolerance.  With
 * g_q, g_v the adjoints of slab t + 1 (cotangents included), per tick:
 *   step      v' = g_v + (d qpos_{t+1} / d qvel_{t+1})' g_q            (qpos' = integratePos(qpos, qvel', dt))
 *             grad_x = (dt v', grad_tau_hist[t], 0)                     over (dv, u, z)
 *             direct part: g_q <- (d qpos_{t+1} / d qpos_t)' g_q,  g_v <- v'
 *   solve     grad_x -> grad_M, grad_C, grad_J, grad_b, grad_T (and the QP parameters' gradients)
 *   PD mode   grad_T -> base coordinates of qpos and qvel (osc_pd_base_targets_backward's rule)
 *   kinematics grad_M .. grad_b -> qpos, qvel (and the inertial parameters' gradients)
 *   combine   g_q[t] = step-direct + kinematics + PD + grad_qpos_hist[t], added in that order;
 *             g_v[t] likewise
 * Two launches of this header's kernels per tick (the step adjoint; the combine, which also holds
 * the PD adjoint, the tick-ordered sums and the packing of the next tick's base state), next to
 * the recompute's and the two backward passes' own.
 *
 * Frozen envs.  An env is frozen at tick t when status_hist[t] == OSC_SOLVE_NUMERICAL or the
 * recomputed dv holds a non-finite entry -- the forward step's own rule.  Its g_q and g_v pass
 * through the tick unchanged (the forward left its state unchanged), its grad_x is zero, and it
 * adds nothing to a target or parameter gradient at that tick.  An env whose recomputed status is
 * merely not OSC_SOLVE_OK still stepped: its direct state path is differentiated, and the solve's
 * backward passes give it zeros through the solve.  An env with invalid parameters
 * (osc_env_params.h, osc_kin_env_params.h) is frozen at every tick: zeros in every target and
 * parameter gradient, and its state cotangents summed over the slabs in grad_qpos0 / grad_qvel0
 * (the derivative of a state that never moved).
 *
 * Quaternions.  A free or ball joint's quaternion is differentiated through the step's own
 * normalisation, q' = normalise(q * exp(w dt / 2)), exactly as the step computes it; the
 * quaternion block of a state gradient that comes out of the step is orthogonal to q.  At a zero
 * rotation angle the adjoint is the analytic limit (the increment's vector part has slope dt / 2),
 * and below |w dt| = 1e-2 the one coefficient that cancels, (cos(th/2)/2 - sin(th/2)/th) / th^2,
 * is a three-term series.
 *
 * No atomics: one owning lane per output, sums in index or tick order.  An env's gradients are
 * bitwise reproducible and independent of its row and of the batch around it.  Gradients with
 * respect to pos_ref, quat_ref and the gains, and every tick's own grad_T, are
 * osc_batch_rollout_backward_sched's (osc_rollout_schedule.h).  Out of scope: gradients with
 * respect to dt and the mask; the two-model, host-fed and wheel-row entries.
 */
#ifndef OSC_ROLLOUT_BACKWARD_H_
#define OSC_ROLLOUT_BACKWARD_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_backward_env.h"
#include "osc_batch.h"
#include "osc_env_params.h"
#include "osc_kin_backward.h"
#include "osc_kin_env_params.h"
#include "osc_kinematics.h"
#include "osc_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The VJP of osc_batch_integrate (osc_rollout.h).
 *   qpos          [nenv][nq]  the step's input positions (slab t)
 *   qvel_new      [nenv][nv]  the step's OUTPUT velocities (slab t + 1): integratePos used them
 *   status        [nenv] int32, nullable: the status the step was given
 *   qacc          [nenv] rows of nv doubles, row e at qacc + e * qacc_stride (>= nv): the step's
 *                 accelerations, read only for the freeze rule (a non-finite entry)
 *   grad_qpos_new [nenv][nq], grad_qvel_new [nenv][nv]: cotangents of the step's outputs, each
 *                 nullable = zero
 *   grad_qpos [nenv][nq], grad_qvel [nenv][nv], grad_qacc rows of nv at grad_qacc_stride (>= nv):
 *                 the outputs, each nullable = not computed; grad_qpos may alias grad_qpos_new and
 *                 grad_qvel may alias grad_qvel_new (in place)
 * A frozen env (status OSC_SOLVE_NUMERICAL or a non-finite qacc entry) gets grad_qpos =
 * grad_qpos_new, grad_qvel = grad_qvel_new and grad_qacc = 0.  dt may be negative.
 * OSC_ERR_INVALID_ARGUMENT before any launch: a NULL kin, nenv < 0, a non-finite dt, a NULL qpos,
 * qvel_new or qacc, a stride below nv, a misaligned pointer, every output NULL.  nenv == 0: OK. */
int osc_batch_integrate_backward(const osc_kin_model* kin, int32_t nenv, double dt,
                                 const double* qpos, const double* qvel_new, const int32_t* status,
                                 const double* qacc, int64_t qacc_stride,
                                 const double* grad_qpos_new, const double* grad_qvel_new,
                                 double* grad_qpos, double* grad_qvel, double* grad_qacc,
                                 int64_t grad_qacc_stride, void* stream);

/* The VJP of osc_pd_base_targets (osc_producers.h) with respect to the base state.  Only row 0 of
 * the targets depends on the state, so only row 0 of grad_targets is read.
 *   base_quat     [nenv][4], nullable: the producer is linear in the (raw, unnormalised)
 *                 quaternion, so the adjoint does not read it; taken for symmetry with the forward
 *   quat_ref      [nenv][4] if quat_ref_per_env else [4]
 *   gains         host pointer to {kp_lin, kd_lin, kp_ang, kd_ang}
 *   grad_targets  [nenv][ns][6]
 *   grad_base_pos [nenv][3], grad_base_quat [nenv][4], grad_lin_vel [nenv][3], grad_ang_vel
 *                 [nenv][3]: each nullable = not computed
 * OSC_ERR_INVALID_ARGUMENT before any launch: nenv < 0, ns < 1, NULL gains, quat_ref or
 * grad_targets, a misaligned pointer, every output NULL.  nenv == 0: OK. */
int osc_pd_base_targets_backward(int32_t nenv, int32_t ns, const double* base_quat,
                                 const double* quat_ref, int32_t quat_ref_per_env,
                                 const double* gains, const double* grad_targets,
                                 double* grad_base_pos, double* grad_base_quat,
                                 double* grad_lin_vel, double* grad_ang_vel, void* stream);

typedef struct {
  /* ---- the forward call's arguments ---- */
  int32_t nticks;                 /* K >= 0                                                     */
  double dt;                      /* > 0                                                        */
  int32_t target_mode;            /* OSC_ROLLOUT_TARGETS_*                                      */
  const double* T;                /* held mode: [nenv][ns][6]                                   */
  const double* pos_ref;          /* PD mode: as osc_rollout_args (the adjoint does not read it,
                                     the recompute does)                                        */
  int32_t pos_ref_per_env;
  const double* quat_ref;
  int32_t quat_ref_per_env;
  double gains[4];
  const double* contact_mask;     /* [nenv][nc]                                                 */
  /* ---- the forward call's histories: the checkpoints ---- */
  const double* qpos_hist;        /* [K + 1][nenv][nq]                                          */
  const double* qvel_hist;        /* [K + 1][nenv][nv]                                          */
  const int32_t* status_hist;     /* [K][nenv]                                                  */
  /* ---- cotangents, each nullable = zero; a loss on the final state is a cotangent on slab K - */
  const double* grad_qpos_hist;   /* [K + 1][nenv][nq]                                          */
  const double* grad_qvel_hist;   /* [K + 1][nenv][nv]                                          */
  const double* grad_tau_hist;    /* [K][nenv][nu]                                              */
  /* ---- outputs, each nullable = not computed (it leaves the others bitwise unchanged) ---- */
  double* grad_qpos0;             /* [nenv][nq]                                                 */
  double* grad_qvel0;             /* [nenv][nv]                                                 */
  double* grad_T;                 /* [nenv][ns][6], held mode only: the sum over ticks, added in
                                     tick order K-1 .. 0 (starting from zero)                   */
  const osc_env_grads* env_grads;     /* nullable; each field nullable: the same sum per field   */
  const osc_kin_env_grads* kin_grads; /* likewise                                                */
  void* workspace;                /* 16-byte aligned, >= osc_rollout_backward_workspace_bytes;
                                     NULL = stream-ordered scratch for this call                */
  size_t workspace_bytes;
} osc_rollout_backward_args;

/* Device scratch of one rollout backward: one tick's M, C, J, b, T, x, duals and statuses, the
 * cotangents between the stages, the running state adjoints, one tick's target and parameter
 * gradients and the solve's workspace.  It does not grow with nticks. */
int osc_rollout_backward_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                         int32_t nenv, size_t* bytes);

/* The backward pass of osc_batch_rollout (env_params and kin_params NULL) or osc_batch_rollout_env
 * (the forward's blocks; a NULL block or field = the model's values), enqueued on `stream`; never
 * synchronises.  The solve's backward is osc_batch_solve_backward_env when env_params or env_grads
 * is given, osc_batch_solve_backward_data otherwise.  Every argument is checked before the first
 * launch, so an argument error leaves nothing enqueued and every output untouched.
 * OSC_ERR_INVALID_ARGUMENT for: whatever osc_batch_rollout(_env) refuses (NULL handles or args,
 * nenv < 0, nticks < 0, dt <= 0 or non-finite, an unknown target mode, a model with wheel rows,
 * PD-base targets on a tree whose root joint is not free, a missing T / reference / mask, a
 * misaligned parameter pointer); a missing history (qpos_hist, qvel_hist or status_hist NULL with
 * nticks > 0; qpos_hist / qvel_hist are not needed for nticks == 0); grad_T asked in PD mode;
 * every output NULL (an env_grads / kin_grads block with every field NULL counts as NULL); a
 * misaligned pointer; a misaligned or too small workspace.  nenv == 0 is OSC_OK; nticks == 0 is
 * OSC_OK with grad_qpos0 / grad_qvel0 the slab-0 cotangents and zeros in every other output. */
int osc_batch_rollout_backward(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                               const osc_rollout_backward_args* args,
                               const osc_env_params* env_params,
                               const osc_kin_env_params* kin_params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_ROLLOUT_BACKWARD_H_ */
