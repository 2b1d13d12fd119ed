/*
 * osc_plant.h -- forward dynamics, and the closed-loop rollout against a plant that is not the
 * controller's model.  Part of libosc_batch.so; same return codes as osc_batch.h; additive to
 * ABI 4 (every existing entry point and struct is unchanged).  All array pointers are DEVICE
 * pointers, env-major, fp64, 8-byte aligned; `stream` is a hipStream_t (NULL = default).
 *
 * osc_batch_rollout integrates dv = x[0:nv], the acceleration the QP itself chose, so its plant is
 * always the controller's model.  Here the step integrates
 *   qacc = M_p^-1 ( B u + Jc' z + qfrc_applied - C_p )
 * instead: the torques u and contact forces z of the tick's solve applied to a plant with its own
 * mass / COM / armature (M_p, C_p) and pushed by given generalised forces -- the same controller
 * on robots whose true payload it does not know, and push recovery.
 *
 * THE ROLLOUT'S DISCLAIMER STANDS (osc_rollout.h): an idealised rollout, not a simulator.  The
 * contact forces are still whatever the QP chose, applied to the plant as given forces; there is
 * still no ground.
 *
 * Out of scope: gradients through the plant (osc_batch_rollout_backward of a plant rollout would
 * be the matched model's; they are osc_plant_backward.h's: the forward dynamics' vector-Jacobian
 * product and osc_batch_rollout_plant_backward); a wrench on an arbitrary body (the caller forms
 * J' f and passes it as qfrc_applied); contact forces as constraint reactions, or any ground; the
 * two-model grids (osc_mixed.h), the host feeds (osc_host_feed.h) and the controller shim
 * (osc_controller.h); models with wheel rows.
 */
#ifndef OSC_PLANT_H_
#define OSC_PLANT_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_env_params.h"
#include "osc_kin_env_params.h"
#include "osc_kinematics.h"
#include "osc_rollout.h"
#include "osc_rollout_schedule.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward dynamics of every environment, one launch:
 *   qacc[e] = M[e]^-1 ( B u[e] + Jc[e]' z[e] + qfrc_applied[e] - C[e] )
 * with B = [0; I_nu] and Jc the rows [3 ns - 3 nc, 3 ns) of J, as osc_batch_solve's dynamics row
 * defines them.
 *   M [nenv][nv][nv], C [nenv][nv], J [nenv][6 ns][nv]: the layouts osc_batch_solve takes
 *   u   [nenv] rows of nu doubles, row e at u + e * u_stride (doubles; u_stride >= nu)
 *   z   [nenv] rows of 3 nc doubles, row e at z + e * z_stride (z_stride >= 3 nc); nullable: no
 *       contact force, and J may then be NULL too.  A solve's x is passed as (x + nv, nx) and
 *       (x + nv + nu, nx), nx = nv + nu + 3 nc
 *   qfrc_applied [nenv][nv], nullable: MuJoCo's generalised applied force; on a free root, entries
 *       0..2 are a world-frame force at the base origin
 *   qacc [nenv][nv], dense
 * M is factored as L D L' without pivoting and without a refinement step.  An env with a pivot
 * <= 0 (or >= 1e120), or with a non-finite entry in any of its inputs, gets NaN in its whole qacc
 * row; every other env is unaffected, bitwise, and an env's result does not depend on its batch.
 * Every argument is checked before the launch.  OSC_ERR_INVALID_ARGUMENT: a NULL model, nenv < 0,
 * a model with wheel rows, a missing required pointer (J with z given), a pointer that is not
 * 8-byte aligned, a stride shorter than its row.  nenv == 0 returns OSC_OK. */
int osc_batch_forward_dynamics(const osc_model* model, int32_t nenv, const double* M,
                               const double* C, const double* J, const double* u,
                               int64_t u_stride, const double* z, int64_t z_stride,
                               const double* qfrc_applied, double* qacc, void* stream);

typedef struct {
  const osc_kin_env_params* kin_params;  /* the PLANT's mass / COM / armature; NULL = the controller's
                                            own (the rollout's kin_params, or the model's) */
  const double* qfrc_applied;            /* [nenv][nv] held, nullable */
  const double* qfrc_applied_seq;        /* [nticks][nenv][nv], nullable; tick t's slab REPLACES the held one */
  double* qacc_hist;                     /* [nticks][nenv][nv] nullable output: what the step integrated */
} osc_rollout_plant;

/* osc_rollout_workspace_bytes plus the plant's sections (M_p | C_p | qacc). */
int osc_rollout_plant_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                      int32_t nenv, int32_t nticks, size_t* bytes);

/* osc_batch_rollout_sched (`sched` nullable: osc_batch_rollout_env) against a plant.  Per tick:
 *   1. the tick's solve, exactly as without a plant: the controller uses ITS kin_params;
 *   2. if plant->kin_params has a non-NULL field, osc_batch_kinematics_env of the same qpos / qvel
 *      with the plant's parameters -> M_p, C_p (J and b do not depend on them); otherwise the
 *      tick's own M, C are the plant's;
 *   3. osc_batch_forward_dynamics of (M_p, C_p, J, the solve's u and z) and the tick's
 *      qfrc_applied slab -> qacc (straight into qacc_hist[t] when that is given);
 *   4. the rollout's step with qacc in place of dv.
 * An env whose plant parameters are invalid (osc_kin_env_params.h) or whose M_p is not positive
 * definite has a NaN qacc row and stays frozen: state unchanged, bad_ticks = nticks, and no NaN
 * enters a state.  A matched plant (nothing but qacc_hist) reproduces osc_batch_rollout to
 * rounding, not bitwise: M^-1 (B u + Jc' z - C) is dv only up to the solve's own elimination.
 * `plant` NULL, or with every field NULL, enqueues exactly the launches of
 * osc_batch_rollout(_env | _sched); the results are bitwise theirs.
 * Every argument is checked before the first launch.  OSC_ERR_INVALID_ARGUMENT, nothing
 * enqueued: what those entries refuse; a plant pointer that is not 8-byte aligned; with a plant
 * that has a non-NULL field, a workspace smaller than osc_rollout_plant_workspace_bytes. */
int osc_batch_rollout_plant(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                            const osc_rollout_args* args, const osc_rollout_schedule* sched,
                            const osc_env_params* env_params,
                            const osc_kin_env_params* kin_params, const osc_rollout_plant* plant,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_PLANT_H_ */
