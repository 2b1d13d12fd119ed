/*
 * osc_mixed.h -- the mixed-robot tick (BASELINE configs[4]: a Go2 shard and a WaLTER Sr shard on
 * one GPU) with everything a single-model tick has: warm starts from the previous tick, inputs
 * from joint states, inputs fed from host memory (the reference does all three every tick:
 * unitree_go2/operational_space_controller.h:519-526, 546-573).  Part of libosc_batch.so; same
 * return codes as osc_batch.h; additive to ABI 4 (osc_batch_solve_multi and the single-model
 * host feed are unchanged).
 */
#ifndef OSC_MIXED_H_
#define OSC_MIXED_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_batch.h"
#include "osc_host_feed.h"
#include "osc_kinematics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One model's batch inside osc_batch_tick_multi.  All array pointers are DEVICE pointers with the
 * layouts of osc_batch.h / osc_kinematics.h.  The job takes one of two input forms:
 *   kin == NULL   QP inputs M, C, J, b (osc_batch_solve's; 16-byte aligned)
 *   kin != NULL   joint states qpos, qvel (osc_batch_solve_qpos's; `kin` must be the same robot
 *                 as `model`: equal nv and site count, same device)
 * and is warm-started when warm_state != NULL (osc_batch_solve_warm's buffer and rules: at least
 * osc_warm_state_bytes, read and updated in place; zero-filled = every env cold). */
typedef struct {
  const osc_model* model;
  const osc_kin_model* kin;       /* NULL = QP inputs                                          */
  int32_t nenv;
  const double *M, *C, *J, *b;    /* kin == NULL                                               */
  const double *qpos, *qvel;      /* kin != NULL                                               */
  const double *T, *contact_mask;
  double *tau, *x;                /* x nullable                                                */
  int32_t *status, *iters;        /* nullable                                                  */
  double* warm_state;             /* NULL = cold                                               */
  size_t warm_state_bytes;
  void* workspace;                /* required: osc_workspace_bytes, or                         */
  size_t workspace_bytes;         /* osc_qpos_workspace_bytes with kin                         */
} osc_tick_job;

/* Several models' ticks in one call on one stream.  Every job is checked before anything is
 * launched; a model with wheel rows, a kin of other dimensions or on another device, a warm buffer
 * or workspace that is too small, a misaligned pointer or a job whose model lives on another
 * device than the current one returns OSC_ERR_INVALID_ARGUMENT with nothing enqueued.
 *
 * Exactly {walter_sr, unitree_go2}, both batches within one wavefront per SIMD (the rule of
 * osc_batch_solve_multi) and both models with the refinement on (the default), run as two-model
 * grids: one assembly grid and one interior-point grid over both, WaLTER's wavefronts first; a
 * cold job shares the grid of a warm one, and two joint-state jobs share one kinematics grid.
 * Any other set of jobs runs one after another through osc_batch_solve / _warm / _qpos /
 * _qpos_warm.  Either way each job's results are bitwise those of that single-model call. */
int osc_batch_tick_multi(const osc_tick_job* jobs, int32_t njobs, void* stream);

/* The kinematics of two models in one grid (the front end of two joint-state jobs): each model's
 * M, C, J, b exactly as osc_batch_kinematics writes them.  Model A's wavefronts come first. */
int osc_batch_kinematics_pair(const osc_kin_model* kin_a, int32_t nenv_a, const double* qpos_a,
                              const double* qvel_a, double* M_a, double* C_a, double* J_a,
                              double* b_a, const osc_kin_model* kin_b, int32_t nenv_b,
                              const double* qpos_b, const double* qvel_b, double* M_b, double* C_b,
                              double* J_b, double* b_b, void* stream);

/* ---- the two-model host feed ----
 * osc_host_feed.h's feed over one or two models' batches ("parts").  A slot's pinned input block
 * holds part 0's arrays, then part 1's, and crosses PCIe in ONE H2D copy per tick; one D2H copy
 * brings both parts' tau / status / iters back.  The joint-state form runs both parts' kinematics
 * (one grid) on the copy stream behind the H2D; the solve is osc_batch_tick_multi on the solve
 * stream, so every tick and part is bitwise that call on the same inputs.  OSC_FEED_WARM gives
 * each part its own warm state, carried from tick to tick.
 *
 * osc_host_feed_submit, _timing and _destroy are osc_host_feed.h's and act on the whole feed (the
 * timing's kin_ms / solve_ms cover both parts).  Inputs and outputs are per part, through the
 * two functions below; osc_host_feed_inputs / _wait on a two-part feed return
 * OSC_ERR_INVALID_ARGUMENT.
 *
 * The models and kin handles are borrowed: they must outlive the feed. */
typedef struct {
  const osc_model* model;
  const osc_kin_model* kin;       /* OSC_FEED_JOINT_STATES: required; OSC_FEED_QP: NULL        */
  int32_t nenv;                   /* > 0                                                       */
} osc_feed_part;

/* Create a feed of 1 <= nparts <= 2 parts on the current HIP device.  Every argument the ticks'
 * solves depend on is checked here -- wheel-row models, a kin of other dimensions, a model or kin
 * created on another device than the current one are refused (OSC_ERR_INVALID_ARGUMENT) -- so
 * that osc_host_feed_submit cannot fail on them later. */
int osc_host_feed_create_multi(const osc_feed_part* parts, int32_t nparts, int32_t form,
                               uint32_t flags, int32_t depth, osc_host_feed** out);

/* osc_host_feed_inputs / osc_host_feed_wait for part `part` (0 <= part < nparts) of the feed;
 * `bytes` is the whole slot's block (both parts). */
int osc_host_feed_inputs_part(osc_host_feed* feed, int32_t tick, int32_t part,
                              osc_feed_inputs* in);
int osc_host_feed_wait_part(osc_host_feed* feed, int32_t tick, int32_t part,
                            osc_feed_outputs* out);

#ifdef __cplusplus
}
#endif

#endif /* OSC_MIXED_H_ */
