/*
 * osc_plant_backward.h -- the vector-Jacobian product of the forward dynamics of osc_plant.h, and
 * the backward pass of osc_batch_rollout_plant built on it.  Part of libosc_batch.so; same return
 * codes as osc_batch.h; additive to ABI 4 (every existing entry point and struct is unchanged).
 * All array pointers are DEVICE pointers, env-major, fp64, 8-byte aligned; `stream` is a
 * hipStream_t (NULL = default).
 *
 * Out of scope: gradients with respect to dt and the mask; any ground or contact model; the
 * two-model, host-fed, shim and wheel-row entries; a warm-started recompute.
 * osc_batch_rollout_backward(_sched) itself still differentiates the matched model only.
 */
#ifndef OSC_PLANT_BACKWARD_H_
#define OSC_PLANT_BACKWARD_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_env_params.h"
#include "osc_kin_backward.h"
#include "osc_kin_env_params.h"
#include "osc_plant.h"
#include "osc_rollout_backward.h"
#include "osc_rollout_schedule.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward pass of osc_batch_forward_dynamics, one launch.  With
 *   qacc = M^-1 ( B u + Jc' z + qfrc_applied - C ),   g = grad_qacc,   w = M^-1 g,   nb = nv - nu,
 * and contact row j the row 3 ns - 3 nc + j of J:
 *   grad_M    [nenv][nv][nv]      grad_M[i][k] = -w_i qacc_k: all nv^2 entries, NOT symmetrised
 *                                 (the convention of osc_backward.h, which
 *                                 osc_batch_kinematics_backward consumes)
 *   grad_C    [nenv][nv]          -w
 *   grad_Jc   [nenv][3 nc][nv]    grad_Jc[j][:] = z_j w': COMPACT, the contact rows only
 *   grad_u    [nenv] rows of nu doubles, row e at grad_u + e * grad_u_stride:  w[nb:]
 *   grad_z    [nenv] rows of 3 nc doubles, row e at grad_z + e * grad_z_stride:  Jc w
 *   grad_qfrc [nenv][nv]          w
 * Inputs:
 *   M [nenv][nv][nv], J [nenv][6 ns][nv]: what the forward took
 *   z   the forward's, rows of 3 nc doubles at z + e * z_stride; nullable: the forward had no
 *       contact force, and J, grad_Jc and grad_z must then be NULL as well
 *   qacc [nenv][nv], dense: the forward's RESULT (the right-hand side is not formed again, so C, u
 *       and qfrc_applied are not inputs)
 *   grad_qacc  rows of nv doubles, row e at grad_qacc + e * grad_qacc_stride
 * Every output is nullable (not computed), and a NULL output leaves the others bitwise unchanged.
 * J is read only for grad_z.  M is factored as in the forward: L D L' without pivoting, no
 * refinement step, the same pivot test.
 * A BAD env gets ZEROS, not NaN, in every output, and every other env is unaffected, bitwise; an
 * env's result does not depend on its batch.  An env is bad when it has a pivot <= 0 (or >=
 * 1e120), or a non-finite entry in M, qacc, grad_qacc, z, or the rows of J that were read: the
 * forward gave such an env a NaN qacc row and the rollout's step froze it, so its derivative is 0.
 * Every argument is checked before the launch.  OSC_ERR_INVALID_ARGUMENT: a NULL model, nenv < 0,
 * a model with wheel rows, a missing required pointer (M, qacc, grad_qacc; z with J, grad_Jc or
 * grad_z given; J with grad_z given), a pointer that is not 8-byte aligned, a stride shorter than
 * its row, every output NULL.  nenv == 0 returns OSC_OK. */
int osc_batch_forward_dynamics_backward(const osc_model* model, int32_t nenv, const double* M,
                                        const double* J, const double* z, int64_t z_stride,
                                        const double* qacc, const double* grad_qacc,
                                        int64_t grad_qacc_stride, double* grad_M, double* grad_C,
                                        double* grad_Jc, double* grad_u, int64_t grad_u_stride,
                                        double* grad_z, int64_t grad_z_stride, double* grad_qfrc,
                                        void* stream);

/* The plant of a rollout's backward pass: the forward's osc_rollout_plant inputs, one more
 * cotangent, and the plant's gradients.  Every field is nullable. */
typedef struct {
  const osc_kin_env_params* kin_params;   /* the forward's plant block; NULL = the controller's */
  const double* qfrc_applied;             /* the forward's, held */
  const double* qfrc_applied_seq;         /* the forward's, per tick */
  const double* grad_qacc_hist;           /* [K][nenv][nv] cotangent of qacc_hist, nullable = 0 */
  double* grad_qfrc_applied;              /* [nenv][nv]: sum over ticks, order K-1..0; held only */
  double* grad_qfrc_applied_seq;          /* [K][nenv][nv]: tick t's slab stored; seq only */
  const osc_kin_env_grads* kin_grads;     /* the PLANT's parameter gradients; needs kin_params */
} osc_rollout_plant_backward;

/* osc_rollout_backward_workspace_bytes plus the plant's sections (M_p | C_p | qacc | grad_qacc |
 * grad_M_p | grad_C_p | grad_Jc | grad_qfrc | the plant's kinematics' state adjoints and one
 * tick's parameter gradients).  It does not grow with nticks. */
int osc_rollout_plant_backward_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                               int32_t nenv, size_t* bytes);

/* The backward pass of osc_batch_rollout_plant: osc_batch_rollout_backward_sched (`sched` and
 * `sched_grads` nullable: osc_batch_rollout_backward) through the plant.
 * `plant` NULL enqueues exactly the launches of osc_batch_rollout_backward(_sched); the results
 * are bitwise theirs.  A non-NULL `plant` ALWAYS differentiates the plant path, even with every
 * field NULL (the matched plant of a forward that asked only for qacc_hist).  Per tick, t = K-1..0:
 *   1. the tick is recomputed as without a plant: the controller's kinematics, the tick's inputs,
 *      the cold solve;
 *   2. if plant->kin_params has a non-NULL field, osc_batch_kinematics_env with the plant's
 *      parameters -> M_p, C_p; otherwise the tick's own M, C are the plant's;
 *   3. osc_batch_forward_dynamics -> qacc (the forward's qacc_hist is not an input);
 *   4. the step's adjoint (osc_batch_integrate_backward's kernel) on that qacc, with the forward's
 *      freeze rule: status OSC_SOLVE_NUMERICAL, or a non-finite qacc entry;
 *   5. osc_batch_forward_dynamics_backward's kernel on grad_qacc + grad_qacc_hist[t]: the solve's
 *      cotangent grad_x = (0, grad_tau_hist[t] + w[nb:], Jc w), the plant-side grad_M_p, grad_C_p,
 *      grad_Jc, and w into grad_qfrc_applied_seq[t] or the held sum's term;
 *   6. the solve's backward, unchanged;
 *   7. one flat launch adds grad_Jc to the contact rows of the solve's grad_J and, when the plant
 *      shares the controller's parameters, grad_M_p and grad_C_p to its grad_M and grad_C;
 *   8. osc_batch_kinematics_backward for the controller, as without a plant;
 *   9. with plant parameters, osc_batch_kinematics_backward once more on (grad_M_p, grad_C_p) and
 *      the plant's kin_params -> its state adjoints and its parameter gradients;
 *  10. the combine launch: slab t's adjoints = step-direct + controller kinematics + plant
 *      kinematics + PD + slab cotangent, and the running sums (grad_qfrc_applied and the plant's
 *      kin_grads among them, added in tick order K-1..0 from zero).
 * A frozen env, and an env with invalid plant parameters (its qacc row is NaN), passes its state
 * cotangents through unchanged and gets zeros in every force, target and parameter gradient; no
 * NaN anywhere.  An env whose recomputed status is merely not OK stepped on u, z as given: its
 * plant path is differentiated and the solve's backward gives it zeros.
 * grad_qfrc_applied without a held force is accepted: it is the gradient at qfrc_applied = 0.
 * Every argument is checked before the first launch.  OSC_ERR_INVALID_ARGUMENT, nothing enqueued
 * and every output untouched: what osc_batch_rollout_backward(_sched) refuses (with a plant, the
 * plant's outputs count among "every output NULL"); grad_qfrc_applied together with
 * qfrc_applied_seq, or grad_qfrc_applied_seq without it; kin_grads with a non-NULL field while
 * kin_params is NULL or has every field NULL; a plant pointer that is not 8-byte aligned; with a
 * plant, a workspace smaller than osc_rollout_plant_backward_workspace_bytes. */
int osc_batch_rollout_plant_backward(const osc_model* model, const osc_kin_model* kin,
                                     int32_t nenv, const osc_rollout_backward_args* args,
                                     const osc_rollout_schedule* sched,
                                     const osc_rollout_schedule_grads* sched_grads,
                                     const osc_env_params* env_params,
                                     const osc_kin_env_params* kin_params,
                                     const osc_rollout_plant_backward* plant, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_PLANT_BACKWARD_H_ */
