/*
 * osc_rollout_schedule.h -- inputs that change over the rollout's ticks, and their gradients: a
 * per-tick feed-forward on the targets, a contact-mask schedule (a gait's stance / swing pattern),
 * per-tick PD references (a base trajectory to follow), and in the backward pass the per-tick
 * target gradient and the gradients with respect to the PD references and gains.  Part of
 * libosc_batch.so; same return codes as osc_batch.h; additive to ABI 4: osc_rollout_args and
 * osc_rollout_backward_args keep their layouts, and every existing entry point and kernel is
 * unchanged.  All array pointers are DEVICE pointers, fp64, 8-byte aligned, TICK-MAJOR: one
 * contiguous slab per tick; `stream` is a hipStream_t (NULL = default).
 *
 * The rollout is still idealised (osc_rollout.h): no ground and no contact detection.  The mask
 * is an INPUT, now per tick; nothing here decides when a foot touches down.  dt and the mask get
 * no gradient.  Under OSC_ROLLOUT_WARM an env whose mask differs from the one its warm state was
 * stored with restarts cold (osc_batch.h), so a mask schedule is safe with warm starts.
 *
 * Launches.  A sequence that replaces a held input is a pointer offset per tick: T_seq alone in
 * held mode (args->T NULL), mask_seq and the reference sequences launch nothing.  T_seq ADDED to
 * a held T or to the PD producer's targets is one flat elementwise kernel per tick, a separate
 * IEEE addition of the producer's already rounded value.  The backward's combine
 * kernel (osc_rollout_backward.h) also stores the tick's grad_T and forms the reference and gain
 * adjoints, in the same launch; the recompute's addition is its only extra launch.
 */
#ifndef OSC_ROLLOUT_SCHEDULE_H_
#define OSC_ROLLOUT_SCHEDULE_H_

#include <stddef.h>
#include <stdint.h>

#include "osc_rollout.h"
#include "osc_rollout_backward.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const double* T_seq;        /* [K][nenv][ns][6], nullable.  ADDED to what the target mode
                                 produces: held mode T_t = args->T + T_seq[t] (args->T may then
                                 be NULL = 0); PD mode T_t = osc_pd_base_targets(state_t) +
                                 T_seq[t] (a feed-forward)                                       */
  const double* mask_seq;     /* [K][nenv][nc], nullable: tick t's contact mask (else
                                 args->contact_mask, which may be NULL when this is given)       */
  const double* pos_ref_seq;  /* PD mode: [K][nenv][3] if pos_ref_per_env else [K][3]; nullable:
                                 tick t's reference (else args->pos_ref, likewise)               */
  const double* quat_ref_seq; /* PD mode: likewise with 4                                        */
} osc_rollout_schedule;

/* osc_batch_rollout (env_params and kin_params NULL) or osc_batch_rollout_env with a schedule.
 * Every field of `sched` is nullable; with sched NULL or every field NULL the call is bitwise
 * osc_batch_rollout / osc_batch_rollout_env.  It checks what those check, except that args->T,
 * args->contact_mask, args->pos_ref and args->quat_ref may be NULL when the matching sequence is
 * given (with nticks == 0 every sequence is empty and none of the four is needed), and in addition
 * OSC_ERR_INVALID_ARGUMENT for: a reference sequence in held mode, a misaligned sequence pointer.
 * Every check runs before the first launch.  The workspace is osc_rollout_workspace_bytes (the
 * addition lands in its target slab). */
int osc_batch_rollout_sched(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                            const osc_rollout_args* args, const osc_rollout_schedule* sched,
                            const osc_env_params* env_params, const osc_kin_env_params* kin_params,
                            void* stream);

/* The VJP of osc_pd_base_targets (osc_producers.h) with respect to its references and gains, per
 * env.  Only row 0 of the targets depends on them, so only row 0 of grad_targets is read.
 *   base_pos [nenv][3], base_quat [nenv][4], lin_vel [nenv][3], ang_vel [nenv][3]: the forward's
 *   pos_ref  [nenv][3] if pos_ref_per_env else [3];  quat_ref [nenv][4] if quat_ref_per_env else [4]
 *   gains    host pointer to {kp_lin, kd_lin, kp_ang, kd_ang}
 *   grad_targets  [nenv][ns][6]
 *   grad_pos_ref [nenv][3], grad_quat_ref [nenv][4], grad_gains [nenv][4]: each nullable = not
 *                 computed
 * The outputs are ALWAYS per env, also when the forward's reference is shared: summing a shared
 * reference's or the gains' gradient over the envs is the caller's (no atomics and no cross-env
 * reduction in the library).  One owning lane per output.
 * OSC_ERR_INVALID_ARGUMENT before any launch: nenv < 0, ns < 1, a NULL input (gains included), a
 * misaligned pointer, every output NULL.  nenv == 0: OK. */
int osc_pd_base_targets_backward_params(int32_t nenv, int32_t ns, const double* base_pos,
                                        const double* base_quat, const double* lin_vel,
                                        const double* ang_vel, const double* pos_ref,
                                        int32_t pos_ref_per_env, const double* quat_ref,
                                        int32_t quat_ref_per_env, const double* gains,
                                        const double* grad_targets, double* grad_pos_ref,
                                        double* grad_quat_ref, double* grad_gains, void* stream);

typedef struct {
  double* grad_T_seq;         /* [K][nenv][ns][6]: tick t's grad_T, stored and not summed; an env
                                 frozen at t = zeros.  Held mode: the gradient of T_seq[t] (and of
                                 a per-tick T); PD mode: the feed-forward's gradient             */
  double* grad_pos_ref;       /* [nenv][3]: summed over the ticks in the order K-1 .. 0 from zero
                                 (a held reference, shared or per env)                           */
  double* grad_quat_ref;      /* [nenv][4] likewise                                              */
  double* grad_pos_ref_seq;   /* [K][nenv][3]: per tick, when pos_ref_seq was given              */
  double* grad_quat_ref_seq;  /* [K][nenv][4]                                                    */
  double* grad_gains;         /* [nenv][4]: summed over the ticks in the order K-1 .. 0          */
} osc_rollout_schedule_grads; /* each nullable = not computed                                    */

/* The backward pass of osc_batch_rollout_sched: osc_batch_rollout_backward with the recompute of
 * tick t on mask_seq[t], T_seq[t] and the tick's references, and the outputs of `sgrads` next to
 * those of `bargs`.  sched and sgrads are nullable (both NULL: bitwise
 * osc_batch_rollout_backward).  The frozen-env, invalid-parameter and quaternion rules of
 * osc_rollout_backward.h hold unchanged.  bargs->grad_T (held mode) stays available and equals
 * the tick-ordered sum of grad_T_seq.  An output that is not asked for leaves the others bitwise
 * unchanged.  The mask gets no gradient.
 * OSC_ERR_INVALID_ARGUMENT before any launch, every output untouched: whatever
 * osc_batch_rollout_backward refuses, with a missing T / mask / reference allowed when the
 * matching sequence is given and "every output NULL" counting sgrads' fields; a reference
 * sequence, or a reference or gain gradient, in held mode; grad_pos_ref_seq / grad_quat_ref_seq
 * without the matching forward sequence; grad_pos_ref / grad_quat_ref when the sequence was
 * given; a misaligned pointer.  nticks == 0: zeros in grad_pos_ref, grad_quat_ref and grad_gains
 * (the _seq outputs have no slab). */
int osc_batch_rollout_backward_sched(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                     const osc_rollout_backward_args* bargs,
                                     const osc_rollout_schedule* sched,
                                     const osc_rollout_schedule_grads* sgrads,
                                     const osc_env_params* env_params,
                                     const osc_kin_env_params* kin_params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OSC_ROLLOUT_SCHEDULE_H_ */
