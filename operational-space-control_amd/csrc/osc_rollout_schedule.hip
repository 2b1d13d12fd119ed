// osc_rollout_schedule.hip -- the scheduled rollout (C-ABI in include/osc_rollout_schedule.h):
// per-tick targets, masks and PD references in the forward, and in the backward the per-tick
// grad_T and the gradients with respect to the PD references and gains.  The tick loops are
// osc_rollout.hip's and osc_rollout_backward.hip's own (osc_rollout_sched.hpp); this unit holds
// the three kernels they need and the entry points.  No existing kernel changes.
//
// The per-tick glue is launch-latency bound (osc_rollout.hip's header), so a scheduled tick adds
// at most ONE small launch to a plain one, and none where a pointer offset does the job:
//   forward   a sequence that replaces a held input (T_seq with args->T NULL, mask_seq, the
//             reference sequences) is tick t's slab pointer.  T_seq added to a held T or to the
//             producer's targets is sched_add_kernel: flat over nenv x ns x 6, consecutive lanes on
//             consecutive doubles.  The producer's value is already rounded and in memory when
//             the addition reads it, and the kernel holds no multiplication, so nothing can
//             contract across the two: the sum is bitwise osc_pd_base_targets followed by one
//             IEEE addition.
//   backward  sched_combine_kernel is osc_rollout_backward.hip's combine kernel -- its statements
//             verbatim, so the state adjoints and the tick-ordered sums round as they do there --
//             and in the same launch stores the tick's grad_T into its slab and forms the
//             reference and gain adjoints from slab t's base state, read from the histories.  Eleven
//             outputs per env (3 + 4 + 4), one owning lane each: 176 lanes of the 256-thread block
//             that owns 16 consecutive envs, as every kernel of the rollout.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "osc_batch.h"
#include "osc_rollout_sched.hpp"
#include "osc_rollout_schedule.h"

namespace {

// the layouts bindings restate (osc_amd/_lib.py; tests/test_rollout_schedule_ref.py)
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_schedule) == 32,
              "osc_rollout_schedule layout");
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_schedule_grads) == 48,
              "osc_rollout_schedule_grads layout");

constexpr int kBlock = 256;
constexpr int kEnvPerBlock = 16;
constexpr int kParamOut = 11;   // grad_pos_ref 3, grad_quat_ref 4, grad_gains 4
static_assert(kEnvPerBlock * kParamOut <= kBlock, "one owning lane per parameter output");

__global__ __launch_bounds__(kBlock) void osc_rollout_sched_add_kernel(
    long long count, const double* base, const double* add, double* out) {
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < count;
       i += static_cast<long long>(gridDim.x) * kBlock)
    out[i] = __dadd_rn(base[i], add[i]);   // out may alias base: each lane reads before it writes
}

// as osc_rollout_backward.hip's: component `comp` of the adjoint of vec(q_ref (x) conj(q)) with
// respect to the raw quaternion q; g = kp_ang x the cotangent of T[0][3:6]
__device__ __forceinline__ double pd_quat_adjoint(const double* qr, const double* g, int comp) {
  const double aw = qr[0], ax = qr[1], ay = qr[2], az = qr[3];
  return comp == 0   ? ax * g[0] + ay * g[1] + az * g[2]
         : comp == 1 ? -(aw * g[0] + az * g[1] - ay * g[2])
         : comp == 2 ? -(aw * g[1] - az * g[0] + ax * g[2])
                     : -(aw * g[2] + ay * g[0] - ax * g[1]);
}

// Output j of one env's adjoint of osc_pd_base_targets with respect to its parameters: 0..2
// grad_pos_ref, 3..6 grad_quat_ref, 7..10 grad_gains.  t = the cotangent of row 0 of the targets,
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

__global__ __launch_bounds__(kBlock) void osc_pd_base_targets_backward_params_kernel(
    int nenv, int ns, const double* __restrict__ pos, const double* __restrict__ quat,
    const double* __restrict__ lin, const double* __restrict__ ang,
    const double* __restrict__ pos_ref, int pos_ref_stride, const double* __restrict__ quat_ref,
    int quat_ref_stride, double kp_lin, double kp_ang, const double* __restrict__ gT,
    double* __restrict__ gpos_ref, double* __restrict__ gquat_ref, double* __restrict__ ggains) {
  const long long total = static_cast<long long>(nenv) * kParamOut;
  for (long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * kBlock) {
    const long long e = idx / kParamOut;
    const int j = static_cast<int>(idx - e * kParamOut);
    double* out = j < 3 ? gpos_ref : j < 7 ? gquat_ref : ggains;
    if (!out) continue;
    const double r = pd_param_adjoint(j, gT + e * 6 * ns, pos + e * 3, quat + e * 4, lin + e * 3,
                                      ang + e * 3, pos_ref + e * pos_ref_stride,
                                      quat_ref + e * quat_ref_stride, kp_lin, kp_ang);
    if (j < 3) out[e * 3 + j] = r;
    else if (j < 7) out[e * 4 + (j - 3)] = r;
    else out[e * 4 + (j - 7)] = r;
  }
}

__global__ __launch_bounds__(kBlock) void osc_rollout_sched_combine_kernel(
    osc::SchedCombineArgs a) {
  const int tid = threadIdx.x;
  const int nq = a.nq, nv = a.nv;
  const long long e0 = static_cast<long long>(blockIdx.x) * kEnvPerBlock;
  const long long left = a.nenv - e0;
  const int ne = left < kEnvPerBlock ? static_cast<int>(left) : kEnvPerBlock;
  const long long trow = 6LL * a.ns;
  const bool pd = a.pd != 0;

  // ---- osc_rollout_combine_kernel's statements ----
  for (int idx = tid; idx < ne * nq; idx += kBlock) {
    const int el = idx / nq, i = idx - el * nq;
    const long long g = e0 * nq + idx, e = e0 + el;
    double v = a.gq[g] + a.kq[g];
    if (pd && i < 7) {   // free root: qpos[0:3] position, qpos[3:7] quaternion
      const double* t = a.gT + e * trow;
      if (i < 3) {
        v += -a.kp_lin * t[i];
      } else {
        const double ga[3] = {a.kp_ang * t[3], a.kp_ang * t[4], a.kp_ang * t[5]};
        v += pd_quat_adjoint(a.quat_ref + e * a.quat_ref_stride, ga, i - 3);
      }
    }
    if (a.hq) v += a.hq[g];
    a.gq[g] = v;
    if (a.pack_qpos && i < 7) {
      const double s = a.pack_qpos[g];
      if (i < 3) a.bpos[e * 3 + i] = s;
      else a.bquat[e * 4 + (i - 3)] = s;
    }
  }
  for (int idx = tid; idx < ne * nv; idx += kBlock) {
    const int el = idx / nv, d = idx - el * nv;
    const long long g = e0 * nv + idx, e = e0 + el;
    double v = a.gv[g] + a.kv[g];
    if (pd && d < 6) v += -(d < 3 ? a.kd_lin : a.kd_ang) * a.gT[e * trow + d];
    if (a.hv) v += a.hv[g];
    a.gv[g] = v;
    if (a.pack_qvel && d < 6) {
      const double s = a.pack_qvel[g];
      if (d < 3) a.blin[e * 3 + d] = s;
      else a.bang[e * 3 + (d - 3)] = s;
    }
  }
  for (int k = 0; k < a.nacc; ++k) {
    const long long cnt = a.acc[k].cnt, base = e0 * cnt;
    for (long long idx = tid; idx < ne * cnt; idx += kBlock)
      a.acc[k].acc[base + idx] += a.acc[k].src[base + idx];
  }

  // ---- the schedule's: tick t's grad_T, stored; the reference and gain adjoints ----
  // (they read gT, the history slab and the references only: nothing written above)
  if (a.gT_slab)
    for (long long idx = tid; idx < ne * trow; idx += kBlock)
      a.gT_slab[e0 * trow + idx] = a.gT[e0 * trow + idx];
  if ((a.gpos_ref || a.gquat_ref || a.ggains) && tid < ne * kParamOut) {
    const int el = tid / kParamOut, j = tid - el * kParamOut;
    const long long e = e0 + el;
    double* out = j < 3 ? a.gpos_ref : j < 7 ? a.gquat_ref : a.ggains;
    if (out) {
      const double* q = a.qpos + e * nq;
      const double* v = a.qvel + e * nv;
      const double r = pd_param_adjoint(j, a.gT + e * trow, q, q + 3, v, v + 3,
                                        a.pos_ref + e * a.pos_ref_stride,
                                        a.quat_ref + e * a.quat_ref_stride, a.kp_lin, a.kp_ang);
      if (j < 3) {
        if (a.pos_ref_add) out[e * 3 + j] += r;
        else out[e * 3 + j] = r;
      } else if (j < 7) {
        if (a.quat_ref_add) out[e * 4 + (j - 3)] += r;
        else out[e * 4 + (j - 3)] = r;
      } else {
        out[e * 4 + (j - 7)] += r;
      }
    }
  }
}

unsigned grid_for(long long n) {
  long long b = (n + kBlock - 1) / kBlock;
  if (b > 65535LL * 8) b = 65535LL * 8;
  return static_cast<unsigned>(b < 1 ? 1 : b);
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

namespace osc {

int launch_sched_add(const double* base, const double* add, double* out, long long count,
                     hipStream_t s) {
  if (count <= 0) return OSC_OK;
  hipLaunchKernelGGL(osc_rollout_sched_add_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, count,
                     base, add, out);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

int launch_sched_combine(const SchedCombineArgs& a, hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(a.nenv) + kEnvPerBlock - 1) /
                                              kEnvPerBlock);
  hipLaunchKernelGGL(osc_rollout_sched_combine_kernel, dim3(nblk), dim3(kBlock), 0, s, a);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

}  // namespace osc

extern "C" int osc_batch_rollout_sched(const osc_model* model, const osc_kin_model* kin,
                                       int32_t nenv, const osc_rollout_args* args,
                                       const osc_rollout_schedule* sched,
                                       const osc_env_params* env_params,
                                       const osc_kin_env_params* kin_params, void* stream) {
  return osc::rollout_run(model, kin, nenv, args, sched, env_params, kin_params, nullptr, stream);
}

extern "C" int osc_pd_base_targets_backward_params(
    int32_t nenv, int32_t ns, const double* base_pos, const double* base_quat,
    const double* lin_vel, const double* ang_vel, const double* pos_ref, int32_t pos_ref_per_env,
    const double* quat_ref, int32_t quat_ref_per_env, const double* gains,
    const double* grad_targets, double* grad_pos_ref, double* grad_quat_ref, double* grad_gains,
    void* stream) {
  if (nenv < 0 || ns < 1 || !gains) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_pos_ref && !grad_quat_ref && !grad_gains) return OSC_ERR_INVALID_ARGUMENT;
  for (const void* p : {static_cast<const void*>(base_pos), static_cast<const void*>(base_quat),
                        static_cast<const void*>(lin_vel), static_cast<const void*>(ang_vel),
                        static_cast<const void*>(pos_ref), static_cast<const void*>(quat_ref),
                        static_cast<const void*>(grad_targets),
                        static_cast<const void*>(grad_pos_ref),
                        static_cast<const void*>(grad_quat_ref),
                        static_cast<const void*>(grad_gains)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  if (!base_pos || !base_quat || !lin_vel || !ang_vel || !pos_ref || !quat_ref || !grad_targets)
    return OSC_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(osc_pd_base_targets_backward_params_kernel,
                     dim3(grid_for(static_cast<long long>(nenv) * kParamOut)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), nenv, ns, base_pos, base_quat, lin_vel,
                     ang_vel, pos_ref, pos_ref_per_env ? 3 : 0, quat_ref, quat_ref_per_env ? 4 : 0,
                     gains[0], gains[2], grad_targets, grad_pos_ref, grad_quat_ref, grad_gains);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

extern "C" int osc_batch_rollout_backward_sched(const osc_model* model, const osc_kin_model* kin,
                                                int32_t nenv,
                                                const osc_rollout_backward_args* bargs,
                                                const osc_rollout_schedule* sched,
                                                const osc_rollout_schedule_grads* sgrads,
                                                const osc_env_params* env_params,
                                                const osc_kin_env_params* kin_params,
                                                void* stream) {
  return osc::rollout_backward_run(model, kin, nenv, bargs, sched, sgrads, env_params, kin_params,
                                   stream);
}
