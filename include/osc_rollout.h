/*
 * osc_rollout.h -- device-resident closed-loop rollout over the controller's own model.  Part of
 * libosc_batch.so; same return codes as osc_batch.h.  All array pointers are DEVICE pointers,
 * env-major, fp64 unless noted; `stream` is a hipStream_t (NULL = default).
 *
 * The QP's design vector already holds the acceleration the controller's model predicts:
 * dv = x[0:nv], subject to the dynamics row M dv + C = B u + Jc' z.  Integrating it the way
 * MuJoCo's Euler step does closes the loop on that model:
 *   qvel += dt * dv,   then   qpos = mj_integratePos(qpos, qvel, dt)   (semi-implicit Euler)
 * so K ticks of   kinematics -> task targets -> solve -> step   run with every array in HBM: no
 * host synchronisation and no host <-> device traffic between ticks.
 *
 * THIS IS AN IDEALISED ROLLOUT, NOT A SIMULATOR.  There is no ground and no contact detection:
 * the contact mask is an input -- held constant over the rollout here, one per tick with
 * osc_batch_rollout_sched (osc_rollout_schedule.h), which also takes per-tick targets and PD
 * references -- and the contact forces are whatever the QP chose.  It answers "what does this controller do over the next K ticks if its
 * own model is right?" -- a look-ahead primitive and a source of dynamically consistent tick
 * sequences, not a replacement for a physics engine.
 */
#ifndef OSC_ROLLOUT_H_
#define OSC_ROLLOUT_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_kinematics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One semi-implicit Euler step for every environment, in place (the rollout's step kernel alone,
 * for callers who run their own loop):
 *   qvel' = qvel + dt * qacc
 *   qpos' = mj_integratePos(qpos, qvel', dt): free joint position += v dt and quaternion <-
 *           normalise(q * exp(w_body dt / 2)); ball joint the same for its quaternion; hinge and
 *           slide q += qd dt; welded bodies carry no coordinate.  A zero rotation angle takes the
 *           identity increment (no division by the angle).
 *   qacc      [nenv] rows of nv doubles, row e at qacc + e * qacc_stride (doubles; >= nv), so the
 *             dv block of a solve's x is passed as (x, nv + nu + 3 nc)
 *   status    [nenv] int32, nullable: the solve's per-env status
 *   qpos      [nenv][nq], qvel [nenv][nv]: updated in place
 *   bad_ticks [nenv] int32, nullable: incremented for every env whose status is not OSC_SOLVE_OK
 *             or that is frozen (below)
 * An env whose status is OSC_SOLVE_NUMERICAL, or whose qacc holds a non-finite entry, is FROZEN
 * for this step: its qpos and qvel are left exactly as they are, so a NaN never enters a state
 * (and from there the next tick's warm start).  dt may be negative (a step backwards). */
int osc_batch_integrate(const osc_kin_model* kin, int32_t nenv, double dt, const double* qacc,
                        int64_t qacc_stride, const int32_t* status, double* qpos, double* qvel,
                        int32_t* bad_ticks, void* stream);

#define OSC_ROLLOUT_WARM 1u          /* flags: warm-start tick k from tick k - 1                */

#define OSC_ROLLOUT_TARGETS_HELD 0   /* target_mode: T, constant over the rollout               */
#define OSC_ROLLOUT_TARGETS_PD_BASE 1 /* target_mode: osc_pd_base_targets of the current state  */

typedef struct {
  int32_t nticks;                 /* >= 0                                                       */
  double dt;                      /* > 0                                                        */
  uint32_t flags;                 /* OSC_ROLLOUT_WARM: every tick goes through
                                     osc_batch_solve_qpos_warm; the warm state lives in the
                                     workspace and is zero-filled by the call (tick 0 is cold)   */
  int32_t target_mode;            /* OSC_ROLLOUT_TARGETS_*                                      */
  /* held targets */
  const double* T;                /* [nenv][ns][6]                                              */
  /* PD base targets (examples/standing.cc:143-155), recomputed every tick from the state:
   * osc_pd_base_targets with position = qpos[0:3], quaternion = qpos[3:7], linear velocity =
   * qvel[0:3], angular velocity = qvel[3:6]; the tree's root joint must be free */
  const double* pos_ref;          /* [nenv][3] if pos_ref_per_env else [3]                      */
  int32_t pos_ref_per_env;
  const double* quat_ref;         /* [nenv][4] if quat_ref_per_env else [4]                     */
  int32_t quat_ref_per_env;
  double gains[4];                /* {kp_lin, kd_lin, kp_ang, kd_ang}                           */
  const double* contact_mask;     /* [nenv][nc], held constant over the rollout                 */
  double* qpos;                   /* [nenv][nq] in: initial state; out: state after the last tick */
  double* qvel;                   /* [nenv][nv] likewise                                        */
  /* outputs, each nullable; histories are tick-major, one contiguous slab per tick */
  double* tau;                    /* [nenv][nu]               the last tick's torques           */
  double* qpos_hist;              /* [nticks + 1][nenv][nq]   slab 0 = the initial state        */
  double* qvel_hist;              /* [nticks + 1][nenv][nv]                                     */
  double* tau_hist;               /* [nticks][nenv][nu]                                         */
  int32_t* status_hist;           /* [nticks][nenv]           the solve's status per tick       */
  int32_t* bad_ticks;             /* [nenv] zeroed by the call, then counted as
                                     osc_batch_integrate counts                                 */
  void* workspace;                /* 16-byte aligned, >= osc_rollout_workspace_bytes; NULL =
                                     stream-ordered scratch for this call                       */
  size_t workspace_bytes;
} osc_rollout_args;

/* Device scratch of one rollout: the per-tick targets, x, torques, status, the packed base state,
 * the warm state and osc_batch_solve_qpos's workspace.  It does not grow with nticks (the
 * histories are the caller's). */
int osc_rollout_workspace_bytes(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                int32_t nticks, size_t* bytes);

/* nticks ticks of   [targets] -> osc_batch_solve_qpos(_warm) with x -> step   enqueued on
 * `stream`; the call returns once everything is enqueued and never synchronises, captures a
 * graph or copies to the host.  `kin` must describe the same robot as `model` (as
 * osc_batch_solve_qpos).  Every argument is checked before the first launch, so an argument
 * error leaves nothing enqueued.  OSC_ERR_INVALID_ARGUMENT for: NULL handles or args, nenv < 0,
 * nticks < 0, dt <= 0 or non-finite, unknown flags or target mode, a model with wheel rows (its
 * per-env wheel directions are not part of the state), PD-base targets on a tree whose root
 * joint is not free, a missing required pointer, a misaligned or too small workspace.
 * nticks == 0 or nenv == 0 returns OSC_OK, the state untouched; with nticks == 0 slab 0 of the
 * given histories is written and bad_ticks zeroed. */
int osc_batch_rollout(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                      const osc_rollout_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_ROLLOUT_H_ */
