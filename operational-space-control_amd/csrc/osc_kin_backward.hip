// osc_kin_backward.hip -- vector-Jacobian product of the batched kinematics for gfx950 (MI355X):
// d L / d (qpos, qvel, mass_scale, com_offset, armature_scale) from the cotangents of M, C, J, b
// and site_xpos (C-ABI: include/osc_kin_backward.h; the per-stage adjoints: osc_kin_backward.hpp).
//
// Stateless: a wavefront recomputes the forward of its envs with the forward's own device
// functions (osc_kin_device.hpp), then runs the stages in reverse with an adjoint block next to
// each env's forward state in LDS.  Mapping as the forward's: one 16-lane row per env, up to four
// envs per wavefront.  The LDS per env is twice the forward's, so the host picks the envs per
// workgroup from the model: four while 4 x 2 x EnvLayout.size doubles and the staged tables fit
// 64 KB (Go2, WaLTER), else two (the table limits: 16 bodies, 32 dofs, 32 sites), else one; a
// workgroup is launched with 16 lanes per env it holds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "osc_batch.h"
#include "osc_kin_backward.h"
#include "osc_kin_backward.hpp"
#include "osc_kin_env_params.h"
#include "osc_kin_model.hpp"
#include "osc_kinematics.h"

namespace {

using namespace osc_kin;

struct KinGradPtrs {
  double* qpos;             // [nenv][nq]
  double* qvel;             // [nenv][nv]
  double* mass_scale;       // [nenv][nbody]
  double* com_offset;       // [nenv][nbody][3]
  double* armature_scale;   // [nenv][nv]
};

struct KinCotPtrs {
  const double* M;
  const double* C;
  const double* J;
  const double* b;
  const double* x;
};

// blockDim.x = 16 x (envs per workgroup); dynamic LDS = envs x 2 x EnvLayout.size doubles.
__global__ __launch_bounds__(kKinWave) void osc_kinematics_backward_kernel(
    const KinDev* __restrict__ Kg, int nenv, const double* __restrict__ qpos,
    const double* __restrict__ qvel, KinEnvPtrs ep, KinCotPtrs cot, KinGradPtrs out) {
  extern __shared__ __attribute__((aligned(16))) double kin_sm[];
  __shared__ __attribute__((aligned(16))) KinDev sK;
  constexpr int kRow = kKinRow;
  {
    const uint4* src = reinterpret_cast<const uint4*>(Kg);
    uint4* dst = reinterpret_cast<uint4*>(&sK);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(KinDev) / 16); i += blockDim.x)
      dst[i] = src[i];
  }
  wave_sync();
  const KinDev* K = &sK;
  const int epw = static_cast<int>(blockDim.x) / kRow;
  const int lane = threadIdx.x;
  const int row = lane / kRow, l = lane % kRow;
  const int env_raw = static_cast<int>(blockIdx.x) * epw + row;
  const bool valid = env_raw < nenv;
  const int env = valid ? env_raw : nenv - 1;   // tail rows recompute the last env, store nothing
  const int nq = K->nq, nv = K->nv, nb = K->nbody, ns = K->nsite;
  const EnvLayout lay(nq, nv, nb, ns);
  double* E = kin_sm + static_cast<size_t>(row) * 2 * lay.size;
  double* A = E + lay.size;
  const size_t e = static_cast<size_t>(env);

  for (int i = l; i < nq; i += kRow) E[lay.q + i] = qpos[e * nq + i];
  for (int i = l; i < nv; i += kRow) E[lay.q + nq + i] = qvel[e * nv + i];
  wave_sync();

  // this lane's parameters of the row's env and the row's validity (the forward's rule)
  double ms = 1.0, dc[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  if (l < nb) {
    const size_t eb = e * nb + l;
    if (ep.mass_scale) {
      ms = ep.mass_scale[eb];
      bad = !(ms > 0.0) || !isfinite(ms);
    }
    if (ep.com_offset)
      for (int i = 0; i < 3; ++i) {
        dc[i] = ep.com_offset[eb * 3 + i];
        bad = bad || !isfinite(dc[i]);
      }
  }
  if (ep.armature_scale)
    for (int c = l; c < nv; c += kRow) {
      const double as = ep.armature_scale[e * nv + c];
      bad = bad || !(as >= 0.0) || !isfinite(as);
    }
  const bool env_bad = ((__ballot(bad) >> (row * kRow)) & 0xffffull) != 0;

  // ---- the forward, recomputed: stages 1 .. 4 (5 and 6 are products of the dof slots) ----
  kin_forward<true>(K, E, lay, l, ms, dc);
  kin_backward(K, E, lay, l);
  for (int d = l; d < nv; d += kRow) (void)kin_dof(K, E, lay, d);
  for (int k = l; k < ns; k += kRow) {
    double bp[3], br[3];
    kin_site(K, E, lay, k, bp, br);
  }
  wave_sync();

  KinCot g;
  g.M = cot.M ? cot.M + e * nv * nv : nullptr;
  g.C = cot.C ? cot.C + e * nv : nullptr;
  g.J = cot.J ? cot.J + e * 6 * ns * nv : nullptr;
  g.b = cot.b ? cot.b + e * 6 * ns : nullptr;
  g.x = cot.x ? cot.x + e * ns * 3 : nullptr;

  // ---- stages 6', 5' (lane = dof, then lane = site) ----
  for (int c = l; c < nv; c += kRow) {
    const double gd = kinb_dof_seed(K, E, A, lay, c, g);
    if (valid && out.armature_scale)
      out.armature_scale[e * nv + c] = env_bad ? 0.0 : gd * K->dof_arm[c];
  }
  for (int k = l; k < ns; k += kRow) kinb_site_seed(K, E, A, lay, k, g);
  wave_sync();
  // ---- stages 4', 3' (lane = body) ----
  if (l < nb) kinb_body_seed(K, E, A, lay, l, g);
  wave_sync();
  // ---- stage 2' ----
  kinb_composite(K, A, lay, l);
  // ---- body_dynamics' ----
  if (l < nb) {
    double g_ms, g_dc[3];
    kinb_dynamics(K, E, A, lay, l, ms, dc, &g_ms, g_dc);
    if (valid && out.mass_scale) out.mass_scale[e * nb + l] = env_bad ? 0.0 : g_ms;
    if (valid && out.com_offset)
      for (int i = 0; i < 3; ++i) out.com_offset[(e * nb + l) * 3 + i] = env_bad ? 0.0 : g_dc[i];
  }
  wave_sync();
  // ---- stage 1' ----
  kinb_tree(K, E, A, lay, l);
  // ---- stores ----
  if (valid && out.qpos)
    for (int i = l; i < nq; i += kRow) out.qpos[e * nq + i] = env_bad ? 0.0 : A[lay.q + i];
  if (valid && out.qvel)
    for (int i = l; i < nv; i += kRow) out.qvel[e * nv + i] = env_bad ? 0.0 : A[lay.q + nq + i];
}

constexpr size_t kLdsBudget = 64 * 1024;

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int osc_batch_kinematics_backward(
    const osc_kin_model* kin, int32_t nenv, const double* qpos, const double* qvel,
    const osc_kin_env_params* kin_params, const double* grad_M, const double* grad_C,
    const double* grad_J, const double* grad_b, const double* grad_site_xpos, double* grad_qpos,
    double* grad_qvel, const osc_kin_env_grads* kin_grads, void* stream) {
  // ---- every check before the launch; none of them reads the model ----
  if (!kin || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  KinEnvPtrs ep{nullptr, nullptr, nullptr};
  if (kin_params) ep = {kin_params->mass_scale, kin_params->com_offset, kin_params->armature_scale};
  KinGradPtrs out{grad_qpos, grad_qvel, nullptr, nullptr, nullptr};
  if (kin_grads) {
    out.mass_scale = kin_grads->mass_scale;
    out.com_offset = kin_grads->com_offset;
    out.armature_scale = kin_grads->armature_scale;
  }
  for (const void* p : {static_cast<const void*>(qpos), static_cast<const void*>(qvel),
                        static_cast<const void*>(ep.mass_scale),
                        static_cast<const void*>(ep.com_offset),
                        static_cast<const void*>(ep.armature_scale),
                        static_cast<const void*>(grad_M), static_cast<const void*>(grad_C),
                        static_cast<const void*>(grad_J), static_cast<const void*>(grad_b),
                        static_cast<const void*>(grad_site_xpos),
                        static_cast<const void*>(out.qpos), static_cast<const void*>(out.qvel),
                        static_cast<const void*>(out.mass_scale),
                        static_cast<const void*>(out.com_offset),
                        static_cast<const void*>(out.armature_scale)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;   // (as the forward: an empty batch has no arrays to look at)
  if (!qpos || !qvel) return OSC_ERR_INVALID_ARGUMENT;
  if (!out.qpos && !out.qvel && !out.mass_scale && !out.com_offset && !out.armature_scale)
    return OSC_ERR_INVALID_ARGUMENT;
  const KinDev& k = kin->host;
  const EnvLayout lay(k.nq, k.nv, k.nbody, k.nsite);
  const size_t per_env = sizeof(double) * 2 * static_cast<size_t>(lay.size);
  int epw = kKinEnvPerWave;
  while (epw > 1 && epw * per_env + sizeof(KinDev) > kLdsBudget) epw /= 2;
  if (epw * per_env + sizeof(KinDev) > kLdsBudget) return OSC_ERR_INVALID_ARGUMENT;
  const unsigned nblk = static_cast<unsigned>((nenv + epw - 1) / epw);
  const KinCotPtrs cot{grad_M, grad_C, grad_J, grad_b, grad_site_xpos};
  hipLaunchKernelGGL(osc_kinematics_backward_kernel, dim3(nblk), dim3(kKinRow * epw),
                     epw * per_env, static_cast<hipStream_t>(stream), kin->dev, nenv, qpos, qvel,
                     ep, cot, out);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}
