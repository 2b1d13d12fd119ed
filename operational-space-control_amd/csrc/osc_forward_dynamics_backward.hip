// osc_forward_dynamics_backward.hip -- vector-Jacobian product of the forward dynamics (C-ABI in
// include/osc_plant_backward.h, osc_batch_forward_dynamics_backward).  With
//   qacc = M^-1 (B u + Jc' z + qfrc - C),   g = dL/dqacc,   w = M^-1 g   (M symmetric):
//   dL/dM[i][k] = -w_i qacc_k      dL/dC = -w      dL/dqfrc = w      dL/du = w[nb:]
//   dL/dJc[j][:] = z_j w'          dL/dz = Jc w
// qacc is the forward's result, so the right-hand side is never formed again: C, u and qfrc are
// not inputs, and z and Jc are read only for the two outputs that hold them.
//
// Layout: the forward's (osc_forward_dynamics.hip).  FOUR envs per wavefront, one 16-lane DPP row
// each; lane l holds columns l and l + 16 of M (WaLTER's 14 x 14 padded with identity columns to
// the two-slot layout's 17) and entries l and l + 16 of g; ldl_rows / ldl_solve_rows factor and
// solve, with the forward's pivot test and 1 / D threshold.  w, qacc and z then go through the
// row's LDS block, and every output has ONE owning lane per entry: the vectors from the lane that
// holds the entry, Jc w from the lane of contact row j (and j + 16), the nv x nv and 3 nc x nv
// outer products as 8-byte stores with consecutive lanes on consecutive doubles.  Nothing crosses
// a row, there are no atomics and no scratch, so an env's outputs are bitwise independent of its
// batch, and a NULL output only skips its own stores.
//
// A bad env -- a pivot <= 0 (a tiny 1 / D), or a non-finite entry in M (it reaches a pivot or w),
// qacc, g, z, or the contact rows of J when dL/dz reads them -- gets ZEROS in every output: the
// forward gave it a NaN qacc row, the rollout's step froze it, and its derivative is zero.  The
// flag is one row_max over the row's 16 lanes, taken before the first store.
//
// The rollout's backward (osc_rollout_backward.hip) launches the same kernel with FdBackwardExtras
// (osc_rollout_internal.hpp; not in the C ABI): a second cotangent added to g (grad_qacc_hist's
// slab), the tick's status (OSC_SOLVE_NUMERICAL froze the env: bad), and the completion of the
// solve's grad_x row -- zeros in its dv part and grad_tau added to w[nb:] -- so that the row costs
// no launch of its own.  With every extra NULL the instructions on the values are the entry's.
//
// Traffic per env: M, qacc, g once (+ z, + the 3 nc contact rows of J for dL/dz); the outputs once.
#include <hip/hip_runtime.h>

#include "osc_internal.hpp"
#include "osc_ipm_ldl.hpp"
#include "osc_plant_backward.h"
#include "osc_rollout_internal.hpp"

namespace osc {

// the forward's threshold on 1 / D (osc_forward_dynamics.hip, kFdDinvMin)
constexpr double kFdBwDinvMin = 1e-120;

// LDS per env (doubles): 1 / D of the factorisation | w | qacc | z
template <class D>
struct FdBwLayout {
  static constexpr int I_DINV = 0;
  static constexpr int I_W = 2 * kRow;
  static constexpr int I_Q = I_W + even(D::NV);
  static constexpr int I_Z = I_Q + even(D::NV);
  static constexpr int IL = I_Z + even(D::NZ);
};

template <class D>
__global__ __launch_bounds__(kWave) void osc_forward_dynamics_backward_kernel(
    int nenv, const double* __restrict__ gM, const double* __restrict__ gJ,
    const double* __restrict__ gz, long long z_stride, const double* __restrict__ gqacc,
    const double* __restrict__ gg, long long g_stride, double* __restrict__ oM,
    double* __restrict__ oC, double* __restrict__ oJc, double* __restrict__ ou,
    long long ou_stride, double* __restrict__ oz, long long oz_stride, double* __restrict__ of,
    const double* __restrict__ gg2, const double* __restrict__ gtau,
    const int32_t* __restrict__ gstatus, double* __restrict__ ox, long long ox_stride) {
  constexpr int NV = D::NV, NU = D::NU, NB = D::NB, NZ = D::NZ, S = D::S;
  constexpr int R0 = 3 * D::NS - NZ;                 // the first contact row of J
  constexpr int NM = NV > kRow ? NV : kRow + 1;      // columns of M's factorisation
  constexpr int NZT = (NZ + kRow - 1) / kRow;        // contact rows per lane
  using LY = FdBwLayout<D>;
  static_assert(!D::WH, "no wheel rows");
  static_assert(NV <= 2 * kRow, "two column slots per lane");
  __shared__ double smem[kEnvPerWave * LY::IL];
  const int lane = static_cast<int>(threadIdx.x), l = lane & (kRow - 1);
  const long long env = static_cast<long long>(blockIdx.x) * kEnvPerWave + (lane >> 4);
  const bool valid = env < nenv;
  const size_t e = static_cast<size_t>(valid ? env : nenv - 1);   // (loads stay in bounds)
  double* B = smem + (lane >> 4) * LY::IL;
  double *sDinv = B + LY::I_DINV, *sW = B + LY::I_W, *sQ = B + LY::I_Q, *sZ = B + LY::I_Z;

  // the lane's two columns / entries; past the end a copy of the last one (never stored)
  const int jm0 = l < NV ? l : NV - 1, j1 = l + kRow < NM ? l + kRow : NM - 1,
            jm1 = j1 < NV ? j1 : NV - 1;

  // ---- M: row i across the lanes of the row, consecutive 8-byte loads ----
  const double* Me = gM + e * (NV * NV);
  double m0[NM], m1[NM];
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i < NV) {
      m0[i] = l < NV ? Me[i * NV + jm0] : 0.0;
      m1[i] = j1 < NV ? Me[i * NV + jm1] : 0.0;
    } else {
      m0[i] = i == l ? 1.0 : 0.0;
      m1[i] = i == j1 ? 1.0 : 0.0;
    }
  }

  // ---- the cotangent g and the forward's qacc, entries jm0 and jm1; z, contact rows l, l + 16 ----
  double r0 = gg[e * g_stride + jm0], r1 = gg[e * g_stride + jm1];
  const double q0 = gqacc[e * NV + jm0], q1 = gqacc[e * NV + jm1];
  if (gg2 != nullptr) {
    r0 += gg2[e * NV + jm0];
    r1 += gg2[e * NV + jm1];
  }
  bool bad = !isfinite(r0) || !isfinite(r1) || !isfinite(q0) || !isfinite(q1);
  if (gstatus != nullptr) bad = bad || gstatus[e] == OSC_SOLVE_NUMERICAL;
  r0 = l < NV ? r0 : 0.0;       // the identity columns' entries
  r1 = j1 < NV ? r1 : 0.0;
  if (l < NV) sQ[l] = q0;
  if (l + kRow < NV) sQ[l + kRow] = q1;
  if (gz != nullptr) {
    const double* z = gz + e * z_stride;
#pragma unroll
    for (int t = 0; t < NZT; ++t) {
      const int j = l + kRow * t;
      if (j < NZ) {
        const double zj = z[j];
        bad = bad || !isfinite(zj);
        sZ[j] = zj;
      }
    }
  }

  // ---- M = L D L' in registers, then w = M^-1 g by the two triangular solves ----
  double dinv0, dinv1;
  ldl_rows<NM, false>(m0, m1, sDinv, l, dinv0, dinv1, 0.0, 0.0, 0.0);
  bad = bad || !(dinv0 > kFdBwDinvMin) || !(dinv1 > kFdBwDinvMin);
  ldl_solve_rows<NM>(m0, m1, dinv0, dinv1, r0, r1, l);
  bad = bad || (l < NV && !isfinite(r0)) || (l + kRow < NV && !isfinite(r1));
  if (l < NV) sW[l] = r0;
  if (l + kRow < NV) sW[l + kRow] = r1;
  wave_sync();

  // ---- dL/dz = Jc w: contact row j on lane j % 16 ----
  double jw[NZT] = {};
  if (oz != nullptr) {
    const double* Jc = gJ + e * (S * NV) + R0 * NV;
#pragma unroll
    for (int t = 0; t < NZT; ++t) {
      const int j = l + kRow * t, jj = j < NZ ? j : NZ - 1;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NV; ++k) acc = fma(Jc[jj * NV + k], sW[k], acc);
      bad = bad || !isfinite(acc);
      jw[t] = acc;
    }
  }

  // ---- one flag per env: any lane of the row ----
  const bool ok = row_max(bad ? 1.0 : 0.0) == 0.0;
  if (!valid) return;

  // ---- the vectors, from the lane that holds the entry ----
  const double w0 = ok ? r0 : 0.0, w1 = ok ? r1 : 0.0;
  if (oC) {
    if (l < NV) oC[e * NV + l] = ok ? -r0 : 0.0;
    if (l + kRow < NV) oC[e * NV + l + kRow] = ok ? -r1 : 0.0;
  }
  if (of) {
    if (l < NV) of[e * NV + l] = w0;
    if (l + kRow < NV) of[e * NV + l + kRow] = w1;
  }
  if (ou) {
    double* u = ou + e * ou_stride;
    double t0 = 0.0, t1 = 0.0;   // the rollout's grad_tau slab; a bad env's row stays zero
    if (gtau != nullptr && ok) {
      if (l >= NB && l < NV) t0 = gtau[e * NU + l - NB];
      if (l + kRow >= NB && l + kRow < NV) t1 = gtau[e * NU + l + kRow - NB];
    }
    if (l >= NB && l < NV) u[l - NB] = gtau ? t0 + w0 : w0;
    if (l + kRow >= NB && l + kRow < NV) u[l + kRow - NB] = gtau ? t1 + w1 : w1;
  }
  if (ox) {   // the dv part of the rollout's grad_x row: the plant's step does not read dv
    if (l < NV) ox[e * ox_stride + l] = 0.0;
    if (l + kRow < NV) ox[e * ox_stride + l + kRow] = 0.0;
  }
  if (oz) {
    double* z = oz + e * oz_stride;
#pragma unroll
    for (int t = 0; t < NZT; ++t) {
      const int j = l + kRow * t;
      if (j < NZ) z[j] = ok ? jw[t] : 0.0;
    }
  }

  // ---- the outer products, consecutive lanes on consecutive doubles ----
  if (oM) {
    double* o = oM + e * (NV * NV);
#pragma unroll 1
    for (int p = l; p < NV * NV; p += kRow) {
      const int i = p / NV, k = p - i * NV;
      o[p] = ok ? -(sW[i] * sQ[k]) : 0.0;
    }
  }
  if (oJc) {
    double* o = oJc + e * (NZ * NV);
#pragma unroll 1
    for (int p = l; p < NZ * NV; p += kRow) {
      const int j = p / NV, k = p - j * NV;
      o[p] = ok ? sZ[j] * sW[k] : 0.0;
    }
  }
}

namespace {

template <class D>
int launch_forward_dynamics_backward(int32_t nenv, const double* M, const double* J,
                                     const double* z, int64_t z_stride, const double* qacc,
                                     const double* g, int64_t g_stride, double* oM, double* oC,
                                     double* oJc, double* ou, int64_t ou_stride, double* oz,
                                     int64_t oz_stride, double* of, const FdBackwardExtras& ex,
                                     hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerWave - 1) /
                                              kEnvPerWave);
  hipLaunchKernelGGL(osc_forward_dynamics_backward_kernel<D>, dim3(nblk), dim3(kWave), 0, s, nenv,
                     M, J, z, static_cast<long long>(z_stride), qacc, g,
                     static_cast<long long>(g_stride), oM, oC, oJc, ou,
                     static_cast<long long>(ou_stride), oz, static_cast<long long>(oz_stride), of,
                     ex.grad_qacc_add, ex.grad_tau, ex.status, ex.grad_x_dv,
                     static_cast<long long>(ex.grad_x_stride));
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace
}  // namespace osc

extern "C" int osc_batch_forward_dynamics_backward(
    const osc_model* model, int32_t nenv, const double* M, const double* J, const double* z,
    int64_t z_stride, const double* qacc, const double* grad_qacc, int64_t grad_qacc_stride,
    double* grad_M, double* grad_C, double* grad_Jc, double* grad_u, int64_t grad_u_stride,
    double* grad_z, int64_t grad_z_stride, double* grad_qfrc, void* stream) {
  return osc::forward_dynamics_backward_run(model, nenv, M, J, z, z_stride, qacc, grad_qacc,
                                            grad_qacc_stride, grad_M, grad_C, grad_Jc, grad_u,
                                            grad_u_stride, grad_z, grad_z_stride, grad_qfrc,
                                            nullptr, stream);
}

int osc::forward_dynamics_backward_run(
    const osc_model* model, int32_t nenv, const double* M, const double* J, const double* z,
    int64_t z_stride, const double* qacc, const double* grad_qacc, int64_t grad_qacc_stride,
    double* grad_M, double* grad_C, double* grad_Jc, double* grad_u, int64_t grad_u_stride,
    double* grad_z, int64_t grad_z_stride, double* grad_qfrc, const FdBackwardExtras* extras,
    void* stream) {
  using namespace osc;
  const FdBackwardExtras ex = extras ? *extras : FdBackwardExtras{};
  // ---- every check before the launch ----
  if (!model || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (model->kid != K_GO2 && model->kid != K_WALTER) return OSC_ERR_INVALID_ARGUMENT;   // wheel rows
  if (nenv == 0) return OSC_OK;
  if (!M || !qacc || !grad_qacc) return OSC_ERR_INVALID_ARGUMENT;
  if (!z && (J || grad_Jc || grad_z)) return OSC_ERR_INVALID_ARGUMENT;
  if (grad_z && !J) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_M && !grad_C && !grad_Jc && !grad_u && !grad_z && !grad_qfrc)
    return OSC_ERR_INVALID_ARGUMENT;
  if (misaligned8(M) || misaligned8(J) || misaligned8(z) || misaligned8(qacc) ||
      misaligned8(grad_qacc) || misaligned8(grad_M) || misaligned8(grad_C) ||
      misaligned8(grad_Jc) || misaligned8(grad_u) || misaligned8(grad_z) ||
      misaligned8(grad_qfrc) || misaligned8(ex.grad_qacc_add) || misaligned8(ex.grad_tau) ||
      misaligned8(ex.grad_x_dv) || (reinterpret_cast<uintptr_t>(ex.status) & 3u) != 0)
    return OSC_ERR_INVALID_ARGUMENT;
  if ((ex.grad_tau && !grad_u) || (ex.grad_x_dv && ex.grad_x_stride < model->desc.nv))
    return OSC_ERR_INVALID_ARGUMENT;
  const int nv = model->desc.nv, nu = model->desc.nu, nz = 3 * model->desc.nc;
  if (grad_qacc_stride < nv || (z && z_stride < nz) || (grad_u && grad_u_stride < nu) ||
      (grad_z && grad_z_stride < nz))
    return OSC_ERR_INVALID_ARGUMENT;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != model->device) return OSC_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return model->kid == K_GO2
             ? launch_forward_dynamics_backward<Go2>(
                   nenv, M, J, z, z_stride, qacc, grad_qacc, grad_qacc_stride, grad_M, grad_C,
                   grad_Jc, grad_u, grad_u_stride, grad_z, grad_z_stride, grad_qfrc, ex, s)
             : launch_forward_dynamics_backward<Walter>(
                   nenv, M, J, z, z_stride, qacc, grad_qacc, grad_qacc_stride, grad_M, grad_C,
                   grad_Jc, grad_u, grad_u_stride, grad_z, grad_z_stride, grad_qfrc, ex, s);
}
