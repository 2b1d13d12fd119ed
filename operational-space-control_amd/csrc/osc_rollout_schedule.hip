// osc_rollout_schedule.hip -- the scheduled rollout (C-ABI in include/osc_rollout_schedule.h):
// per-tick targets, masks and PD references in the forward, and in the backward the per-tick
// grad_T and the gradients with respect to the PD references and gains.  The tick loops are
// osc_rollout.hip's and osc_rollout_backward.hip's; this unit holds what a schedule adds to them:
// the resolution of one tick's inputs, which both loops call (the backward recomputes the
// forward's tick, so the two must agree bit for bit), the addition kernel it launches, the
// stand-alone PD parameter adjoint and the scheduled entry points.
//
// The per-tick glue is launch-latency bound (osc_rollout.hip's header), so a scheduled tick adds
// at most ONE small launch to a plain one, and none where a pointer offset does the job: a
// sequence that replaces a held input (T_seq with args->T NULL, mask_seq, the reference sequences)
// is tick t's slab pointer.  T_seq added to a held T or to the producer's targets is
// sched_add_kernel: flat over nenv x ns x 6, consecutive lanes on consecutive doubles.  The
// producer's value is already rounded and in memory when the addition reads it, and the kernel
// holds no multiplication, so nothing can contract across the two: the sum is bitwise
// osc_pd_base_targets followed by one IEEE addition.  In the backward the schedule's outputs are
// written by the one combine kernel (osc_rollout_backward.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "osc_batch.h"
#include "osc_producers.h"
#include "osc_rollout_internal.hpp"
#include "osc_rollout_schedule.h"

namespace {

// the layouts bindings restate (osc_amd/_lib.py; tests/test_rollout_schedule_ref.py)
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_schedule) == 32,
              "osc_rollout_schedule layout");
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_schedule_grads) == 48,
              "osc_rollout_schedule_grads layout");

using namespace osc;   // osc_rollout_internal.hpp's geometry, helpers and adjoints

__global__ __launch_bounds__(kBlock) void osc_rollout_sched_add_kernel(
    long long count, const double* base, const double* add, double* out) {
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < count;
       i += static_cast<long long>(gridDim.x) * kBlock)
    out[i] = __dadd_rn(base[i], add[i]);   // out may alias base: each lane reads before it writes
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

int launch_sched_add(const double* base, const double* add, double* out, long long count,
                     hipStream_t s) {
  if (count <= 0) return OSC_OK;
  hipLaunchKernelGGL(osc_rollout_sched_add_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, count,
                     base, add, out);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

}  // namespace

bool osc::tick_inputs_present(const HeldInputs& in, const osc_rollout_schedule* sched,
                              int32_t nticks, int32_t nc) {
  if (sched && nticks <= 0) return true;
  const osc_rollout_schedule sc = sched ? *sched : osc_rollout_schedule{};
  if (nc > 0 && !in.contact_mask && !sc.mask_seq) return false;
  return in.pd ? (in.pos_ref || sc.pos_ref_seq) && (in.quat_ref || sc.quat_ref_seq)
               : in.T || sc.T_seq;
}

int osc::tick_inputs(const HeldInputs& in, const osc_rollout_schedule& sc, int32_t t,
                     int32_t nenv, const osc_model_desc& d, const double* bpos,
                     const double* bquat, const double* blin, const double* bang, double* Tbuf,
                     void* stream, TickInputs* out) {
  const size_t n = static_cast<size_t>(nenv), s6 = 6 * static_cast<size_t>(d.ns);
  out->T = in.T;
  out->mask = sc.mask_seq ? sc.mask_seq + n * d.nc * t : in.contact_mask;
  out->pos_ref =
      sc.pos_ref_seq ? sc.pos_ref_seq + (in.pos_ref_per_env ? n * 3 : 3) * t : in.pos_ref;
  out->quat_ref =
      sc.quat_ref_seq ? sc.quat_ref_seq + (in.quat_ref_per_env ? n * 4 : 4) * t : in.quat_ref;
  if (in.pd) {
    const int rc = osc_pd_base_targets(nenv, d.ns, bpos, bquat, blin, bang, out->pos_ref,
                                       in.pos_ref_per_env, out->quat_ref, in.quat_ref_per_env,
                                       in.gains, Tbuf, stream);
    if (rc != OSC_OK) return rc;
    out->T = Tbuf;
  }
  if (sc.T_seq) {   // T_t = T + T_seq[t]; nothing to add to: the slab itself
    const double* add = sc.T_seq + n * s6 * t;
    if (!out->T) {
      out->T = add;
    } else {
      const int rc = launch_sched_add(out->T, add, Tbuf, static_cast<long long>(n * s6),
                                      static_cast<hipStream_t>(stream));
      if (rc != OSC_OK) return rc;
      out->T = Tbuf;
    }
  }
  return OSC_OK;
}

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
                                   nullptr, stream);
}
