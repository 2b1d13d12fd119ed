// osc_rollout_internal.hpp -- what the rollout family's three units share, once each:
// osc_rollout.hip (the step kernel and the forward tick loop), osc_rollout_backward.hip (the step
// adjoint, the combine kernel and the backward tick loop) and osc_rollout_schedule.hip (a tick's
// inputs under a schedule, the PD parameter adjoint, the scheduled entry points).  Here: the
// launch geometry, the small host helpers, the handle check, the per-block joint maps, the PD
// producer's adjoints, the two tick loops' declarations and the resolution of one tick's inputs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "osc_batch.h"
#include "osc_kin_device.hpp"
#include "osc_kinematics.h"
#include "osc_plant.h"
#include "osc_plant_backward.h"
#include "osc_rollout_schedule.h"

namespace osc {

// ---- launch geometry: a 256-thread block owns 16 consecutive envs ----
constexpr int kBlock = 256;
constexpr int kEnvPerBlock = 16;
// every joint has at most one more coordinate than dofs, and there is at most one joint per body
constexpr int kMaxNq = OSC_KIN_MAX_DOFS + OSC_KIN_MAX_BODIES;
constexpr int kParamOut = 11;   // grad_pos_ref 3, grad_quat_ref 4, grad_gains 4
static_assert(kEnvPerBlock * kParamOut <= kBlock, "one owning lane per parameter output");

inline unsigned env_blocks(int32_t nenv) {
  return static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerBlock - 1) / kEnvPerBlock);
}

inline unsigned grid_for(long long n) {   // a grid-stride kernel over n items
  long long b = (n + kBlock - 1) / kBlock;
  if (b > 65535LL * 8) b = 65535LL * 8;
  return static_cast<unsigned>(b < 1 ? 1 : b);
}

inline size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// what every entry checks of the handles: the pair describes one robot (osc_qpos_workspace_bytes
// holds check_pair's nv / ns agreement) and the model has no wheel rows
inline int check_handles(const osc_model* model, const osc_kin_model* kin, osc_model_desc* d) {
  if (!model || !kin) return OSC_ERR_INVALID_ARGUMENT;
  size_t probe = 0;
  const int rc = osc_qpos_workspace_bytes(model, kin, 0, &probe);
  if (rc != OSC_OK) return rc;
  if (osc_model_get_desc(model, d) != OSC_OK) return OSC_ERR_INVALID_ARGUMENT;
  if (d->wheel_rows) return OSC_ERR_INVALID_ARGUMENT;
  return OSC_OK;
}

// ---- per-coordinate and per-dof joint maps of a block, from the kinematics model's tables ----
struct JointMaps {
  int16_t cdof[kMaxNq];             // coordinate -> its dof (quaternion: its first rate)
  int8_t ccomp[kMaxNq];             // coordinate -> quaternion component 0..3, -1 = q += qd dt
  int16_t dcoord[OSC_KIN_MAX_DOFS]; // dof -> its coordinate (a quaternion's rate: its w component)
  int8_t dcomp[OSC_KIN_MAX_DOFS];   // dof -> rate component 0..2 of a quaternion, -1 = scalar
};
static_assert(kMaxNq <= 127, "JointMaps index types");

// (thread `tid` fills body tid's entries; the caller synchronises the block)
__device__ __forceinline__ void build_maps(const osc_kin::KinDev* K, int nbody, int tid,
                                           JointMaps& m) {
  if (tid < nbody) {
    const int jt = K->jtype[tid], qa = K->qadr[tid], da = K->dadr[tid];
    if (jt == OSC_KIN_JOINT_FREE) {
      for (int i = 0; i < 3; ++i) {
        m.cdof[qa + i] = static_cast<int16_t>(da + i);
        m.ccomp[qa + i] = -1;
        m.dcoord[da + i] = static_cast<int16_t>(qa + i);
        m.dcomp[da + i] = -1;
        m.dcoord[da + 3 + i] = static_cast<int16_t>(qa + 3);
        m.dcomp[da + 3 + i] = static_cast<int8_t>(i);
      }
      for (int i = 0; i < 4; ++i) {
        m.cdof[qa + 3 + i] = static_cast<int16_t>(da + 3);
        m.ccomp[qa + 3 + i] = static_cast<int8_t>(i);
      }
    } else if (jt == OSC_KIN_JOINT_BALL) {
      for (int i = 0; i < 4; ++i) {
        m.cdof[qa + i] = static_cast<int16_t>(da);
        m.ccomp[qa + i] = static_cast<int8_t>(i);
      }
      for (int i = 0; i < 3; ++i) {
        m.dcoord[da + i] = static_cast<int16_t>(qa);
        m.dcomp[da + i] = static_cast<int8_t>(i);
      }
    } else if (jt == OSC_KIN_JOINT_HINGE || jt == OSC_KIN_JOINT_SLIDE) {
      m.cdof[qa] = static_cast<int16_t>(da);
      m.ccomp[qa] = -1;
      m.dcoord[da] = static_cast<int16_t>(qa);
      m.dcomp[da] = -1;
    }   // welded: no coordinate
  }
}

// ---- the adjoints of osc_pd_base_targets ----
// Component `comp` of the adjoint of its rotation error vec(q_ref (x) conj(q)) with respect to
// the raw quaternion q; g = kp_ang x the cotangent of T[0][3:6].
__device__ __forceinline__ double pd_quat_adjoint(const double* qr, const double* g, int comp) {
  const double aw = qr[0], ax = qr[1], ay = qr[2], az = qr[3];
  return comp == 0   ? ax * g[0] + ay * g[1] + az * g[2]
         : comp == 1 ? -(aw * g[0] + az * g[1] - ay * g[2])
         : comp == 2 ? -(aw * g[1] - az * g[0] + ax * g[2])
                     : -(aw * g[2] + ay * g[0] - ax * g[1]);
}

// Output j of one env's adjoint with respect to the producer's parameters: 0..2 grad_pos_ref,
// 3..6 grad_quat_ref, 7..10 grad_gains.  t = the cotangent of row 0 of the targets,
//   T[0][0:3] = kp_l (p_ref - p) + kd_l (0 - v),   T[0][3:6] = kp_a vec(q_ref (x) conj(q)) + kd_a (0 - w)
// (osc_producers.hip's expressions for the error terms, so the gains' adjoints weigh bitwise the
// errors the forward scaled).
__device__ __forceinline__ double pd_param_adjoint(int j, const double* t, const double* p,
                                                   const double* q, const double* v,
                                                   const double* w, const double* pr,
                                                   const double* qr, double kp_lin,
                                                   double kp_ang) {
  if (j < 3) return kp_lin * t[j];
  const double bw = q[0], bx = -q[1], by = -q[2], bz = -q[3];
  if (j < 7) {
    const double g0 = kp_ang * t[3], g1 = kp_ang * t[4], g2 = kp_ang * t[5];
    return j == 3   ? bx * g0 + by * g1 + bz * g2
           : j == 4 ? bw * g0 - bz * g1 + by * g2
           : j == 5 ? bz * g0 + bw * g1 - bx * g2
                    : -by * g0 + bx * g1 + bw * g2;
  }
  if (j == 7) return (pr[0] - p[0]) * t[0] + (pr[1] - p[1]) * t[1] + (pr[2] - p[2]) * t[2];
  if (j == 8) return (0.0 - v[0]) * t[0] + (0.0 - v[1]) * t[1] + (0.0 - v[2]) * t[2];
  if (j == 10) return (0.0 - w[0]) * t[3] + (0.0 - w[1]) * t[4] + (0.0 - w[2]) * t[5];
  const double aw = qr[0], ax = qr[1], ay = qr[2], az = qr[3];
  const double rx = aw * bx + ax * bw + ay * bz - az * by;
  const double ry = aw * by - ax * bz + ay * bw + az * bx;
  const double rz = aw * bz + ax * by - ay * bx + az * bw;
  return rx * t[3] + ry * t[4] + rz * t[5];
}

// ---- the tick loops ----
// osc_rollout.hip: behind osc_batch_rollout(_env) (sched and plant NULL), osc_batch_rollout_sched
// (plant NULL) and osc_batch_rollout_plant
int rollout_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                const osc_rollout_args* args, const osc_rollout_schedule* sched,
                const osc_env_params* ep, const osc_kin_env_params* kp,
                const osc_rollout_plant* plant, void* stream);

// osc_rollout_backward.hip: behind osc_batch_rollout_backward (sched, sgrads and plant NULL),
// osc_batch_rollout_backward_sched (plant NULL) and osc_batch_rollout_plant_backward
int rollout_backward_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                         const osc_rollout_backward_args* args, const osc_rollout_schedule* sched,
                         const osc_rollout_schedule_grads* sgrads, const osc_env_params* ep,
                         const osc_kin_env_params* kp, const osc_rollout_plant_backward* plant,
                         void* stream);

// osc_forward_dynamics_backward.hip: osc_batch_forward_dynamics_backward (extras NULL) and, for
// the rollout's backward, the same launch completing the solve's grad_x row.  Not in the C ABI.
struct FdBackwardExtras {
  const double* grad_qacc_add;   // [nenv][nv], nullable: added to grad_qacc (grad_qacc_hist[t])
  const double* grad_tau;        // [nenv][nu], nullable: added to w[nb:] in grad_u (needs grad_u)
  const int32_t* status;         // [nenv], nullable: OSC_SOLVE_NUMERICAL makes the env bad
  double* grad_x_dv;             // nullable: rows of nv zeros at grad_x_dv + e * grad_x_stride
  int64_t grad_x_stride;
};
int forward_dynamics_backward_run(const osc_model* model, int32_t nenv, const double* M,
                                  const double* J, const double* z, int64_t z_stride,
                                  const double* qacc, const double* grad_qacc,
                                  int64_t grad_qacc_stride, double* grad_M, double* grad_C,
                                  double* grad_Jc, double* grad_u, int64_t grad_u_stride,
                                  double* grad_z, int64_t grad_z_stride, double* grad_qfrc,
                                  const FdBackwardExtras* extras, void* stream);

// ---- one tick's inputs (osc_rollout_schedule.hip) ----
// The backward recomputes the forward's tick, so both loops resolve a tick's inputs through
// these two functions.  osc_rollout_args and osc_rollout_backward_args name the held inputs
// alike; each loop copies them into this block.
struct HeldInputs {
  bool pd;                      // OSC_ROLLOUT_TARGETS_PD_BASE
  const double* T;
  const double* contact_mask;
  const double* pos_ref;
  int32_t pos_ref_per_env;
  const double* quat_ref;
  int32_t quat_ref_per_env;
  const double* gains;
};

struct TickInputs {
  const double* T;
  const double* mask;
  const double* pos_ref;        // PD mode: the references the producer read
  const double* quat_ref;
};

// Every input a tick reads is there, held or as a sequence.  (With a schedule and no tick every
// sequence is empty, so nothing can stand in for a held input, and nothing reads one.)
bool tick_inputs_present(const HeldInputs& in, const osc_rollout_schedule* sched, int32_t nticks,
                         int32_t nc);

// Tick t's inputs: a sequence replaces its held input by slab t's pointer; in PD mode
// osc_pd_base_targets of the packed base state (bpos | bquat | blin | bang) is enqueued into
// Tbuf; T_seq[t] is added to the held or produced targets into Tbuf (one launch), or is the
// targets itself when there is nothing to add it to.
int tick_inputs(const HeldInputs& in, const osc_rollout_schedule& sc, int32_t t, int32_t nenv,
                const osc_model_desc& d, const double* bpos, const double* bquat,
                const double* blin, const double* bang, double* Tbuf, void* stream,
                TickInputs* out);

}  // namespace osc
