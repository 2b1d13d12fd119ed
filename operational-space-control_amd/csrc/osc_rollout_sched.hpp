// osc_rollout_sched.hpp -- what osc_rollout.hip, osc_rollout_backward.hip and
// osc_rollout_schedule.hip share: the tick loops live in the first two (one loop each for the
// plain and the scheduled entries), the schedule's kernels and entry points in the third.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "osc_plant.h"
#include "osc_rollout_schedule.h"

namespace osc {

// osc_rollout.hip: the forward tick loop behind osc_batch_rollout(_env) (sched NULL) and
// osc_batch_rollout_sched; `plant` (include/osc_plant.h) NULL for all of those
int rollout_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                const osc_rollout_args* args, const osc_rollout_schedule* sched,
                const osc_env_params* ep, const osc_kin_env_params* kp,
                const osc_rollout_plant* plant, void* stream);

// osc_rollout_backward.hip: the backward tick loop behind osc_batch_rollout_backward (sched and
// sgrads NULL: its own combine kernel, untouched) and osc_batch_rollout_backward_sched
int rollout_backward_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                         const osc_rollout_backward_args* args, const osc_rollout_schedule* sched,
                         const osc_rollout_schedule_grads* sgrads, const osc_env_params* ep,
                         const osc_kin_env_params* kp, void* stream);

// out[i] = base[i] + add[i], i < count (out may alias base): the target slab of a scheduled tick
int launch_sched_add(const double* base, const double* add, double* out, long long count,
                     hipStream_t s);

constexpr int kSchedMaxAcc = 11;   // as osc_rollout_backward.hip's kMaxAcc

struct SchedAcc {
  double* acc;         // [nenv][cnt] the running sum
  const double* src;   // [nenv][cnt] this tick's term
  int32_t cnt;
};

// the scheduled combine's arguments: osc_rollout_backward.hip's CombineArgs, then the schedule's
struct SchedCombineArgs {
  int32_t nenv, nq, nv, ns;
  double* gq;                 // [nenv][nq] in: the step's direct part; out: slab t's adjoint
  double* gv;
  const double* kq;           // the kinematics' backward's grad_qpos / grad_qvel
  const double* kv;
  const double* hq;           // slab t of grad_qpos_hist / grad_qvel_hist, nullable
  const double* hv;
  const double* gT;           // this tick's grad_T [nenv][ns][6]; NULL = not formed
  int32_t pd;                 // PD mode: gT reaches the base coordinates
  const double* pos_ref;      // PD mode: tick t's references
  int32_t pos_ref_stride;
  const double* quat_ref;
  int32_t quat_ref_stride;
  double kp_lin, kd_lin, kp_ang, kd_ang;
  const double* pack_qpos;    // PD mode, t > 0: slab t - 1, packed for the producer; else NULL
  const double* pack_qvel;
  double* bpos;
  double* bquat;
  double* blin;
  double* bang;
  int32_t nacc;
  SchedAcc acc[kSchedMaxAcc];
  // ---- the schedule's outputs ----
  double* gT_slab;            // grad_T_seq[t], nullable
  const double* qpos;         // slab t of qpos_hist / qvel_hist: the producer's base state
  const double* qvel;
  double* gpos_ref;           // [nenv][3]; nullable
  double* gquat_ref;          // [nenv][4]; nullable
  double* ggains;             // [nenv][4]; nullable: always added to
  int32_t pos_ref_add;        // 1: gpos_ref is a running sum (a held reference); 0: this tick's slab
  int32_t quat_ref_add;       // likewise gquat_ref
};

int launch_sched_combine(const SchedCombineArgs& a, hipStream_t s);

}  // namespace osc
