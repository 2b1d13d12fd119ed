// osc_forward_dynamics.hip -- forward dynamics of every env (C-ABI in include/osc_plant.h,
// osc_batch_forward_dynamics): qacc = M^-1 (B u + Jc' z + qfrc_applied - C), the plant's
// acceleration under the torques and contact forces of a solve.
//
// Layout: the interior point's, as osc_backward_data.hip uses it for M.  FOUR envs per wavefront,
// one 16-lane DPP row each; lane l holds columns l and l + 16 of M (WaLTER's 14 x 14 padded with
// identity columns to the two-slot layout's 17), ldl_rows / ldl_solve_rows of osc_ipm_ldl.hpp
// factor and solve.  Lane l forms right-hand-side entries l and l + 16 itself: u by index, the
// 3 nc rows of Jc with consecutive lanes on consecutive doubles.  Nothing crosses a row and there
// are no atomics, so an env's result is bitwise independent of its batch.
//
// No refinement step: cond(M) <= 1.4e3 on the shipped models, where the unpivoted LDL' is as
// close to an extended-precision solve as a pivoted LU.  An env with a pivot
// <= 0, or with a non-finite input, gets a NaN row: a replaced pivot shows as a tiny 1 / D, a
// non-finite M reaches a pivot, and a non-finite right-hand side or result is seen directly.
//
// Traffic per env: M, C, the 3 nc contact rows of J, u, z, qfrc once; qacc once (Go2: 4.9 KB).
#include <hip/hip_runtime.h>

#include "osc_internal.hpp"
#include "osc_ipm_ldl.hpp"
#include "osc_plant.h"

namespace osc {

// 1 / D below this: the pivot was not above 0 (ldl_rows made it 1e128) or is out of any mass
// matrix's range; NaN (a non-finite pivot) fails the comparison as well
constexpr double kFdDinvMin = 1e-120;

template <class D>
__global__ __launch_bounds__(kWave) void osc_forward_dynamics_kernel(
    int nenv, const double* __restrict__ gM, const double* __restrict__ gC,
    const double* __restrict__ gJ, const double* __restrict__ gu, long long u_stride,
    const double* __restrict__ gz, long long z_stride, const double* __restrict__ gf,
    double* __restrict__ qacc) {
  constexpr int NV = D::NV, NU = D::NU, NB = D::NB, NZ = D::NZ, S = D::S;
  constexpr int R0 = 3 * D::NS - NZ;                 // the first contact row of J
  constexpr int NM = NV > kRow ? NV : kRow + 1;      // columns of M's factorisation
  static_assert(!D::WH, "no wheel rows");
  static_assert(NV <= 2 * kRow, "two column slots per lane");
  __shared__ double smem[kEnvPerWave * 2 * kRow];    // 1 / D of each row's factorisation
  const int lane = static_cast<int>(threadIdx.x), l = lane & (kRow - 1);
  const long long env = static_cast<long long>(blockIdx.x) * kEnvPerWave + (lane >> 4);
  const bool valid = env < nenv;
  const size_t e = static_cast<size_t>(valid ? env : nenv - 1);   // (loads stay in bounds)
  double* sDinv = smem + (lane >> 4) * (2 * kRow);

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

  // ---- the right-hand side B u + Jc' z + qfrc - C, entries jm0 and jm1 ----
  double r0 = 0.0, r1 = 0.0;
  if (gz != nullptr) {
    const double* z = gz + e * z_stride;
    const double* Jc = gJ + e * (S * NV) + R0 * NV;
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
      const double zk = z[k];
      r0 = fma(Jc[k * NV + jm0], zk, r0);
      r1 = fma(Jc[k * NV + jm1], zk, r1);
    }
  }
  {
    const double* u = gu + e * u_stride;
    if (jm0 >= NB) r0 += u[jm0 - NB];
    if (jm1 >= NB) r1 += u[jm1 - NB];
    if (gf != nullptr) {
      r0 += gf[e * NV + jm0];
      r1 += gf[e * NV + jm1];
    }
    r0 -= gC[e * NV + jm0];
    r1 -= gC[e * NV + jm1];
  }
  bool bad = !isfinite(r0) || !isfinite(r1);
  r0 = l < NV ? r0 : 0.0;       // the identity columns' entries
  r1 = j1 < NV ? r1 : 0.0;

  // ---- M = L D L' in registers, then the two triangular solves ----
  double dinv0, dinv1;
  ldl_rows<NM, false>(m0, m1, sDinv, l, dinv0, dinv1, 0.0, 0.0, 0.0);
  bad = bad || !(dinv0 > kFdDinvMin) || !(dinv1 > kFdDinvMin);
  ldl_solve_rows<NM>(m0, m1, dinv0, dinv1, r0, r1, l);
  bad = bad || (l < NV && !isfinite(r0)) || (l + kRow < NV && !isfinite(r1));

  // ---- one flag per env: any lane of the row ----
  const bool row_bad = row_max(bad ? 1.0 : 0.0) != 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (valid) {
    if (l < NV) qacc[e * NV + l] = row_bad ? nan : r0;
    if (l + kRow < NV) qacc[e * NV + l + kRow] = row_bad ? nan : r1;
  }
}

namespace {

template <class D>
int launch_forward_dynamics(int32_t nenv, const double* M, const double* C, const double* J,
                            const double* u, int64_t u_stride, const double* z, int64_t z_stride,
                            const double* f, double* qacc, hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerWave - 1) /
                                              kEnvPerWave);
  hipLaunchKernelGGL(osc_forward_dynamics_kernel<D>, dim3(nblk), dim3(kWave), 0, s, nenv, M, C, J,
                     u, static_cast<long long>(u_stride), z, static_cast<long long>(z_stride), f,
                     qacc);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace
}  // namespace osc

extern "C" int osc_batch_forward_dynamics(const osc_model* model, int32_t nenv, const double* M,
                                          const double* C, const double* J, const double* u,
                                          int64_t u_stride, const double* z, int64_t z_stride,
                                          const double* qfrc_applied, double* qacc, void* stream) {
  using namespace osc;
  // ---- every check before the launch ----
  if (!model || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (model->kid != K_GO2 && model->kid != K_WALTER) return OSC_ERR_INVALID_ARGUMENT;   // wheel rows
  if (nenv == 0) return OSC_OK;
  if (!M || !C || !u || !qacc || (z && !J)) return OSC_ERR_INVALID_ARGUMENT;
  if (misaligned8(M) || misaligned8(C) || misaligned8(J) || misaligned8(u) || misaligned8(z) ||
      misaligned8(qfrc_applied) || misaligned8(qacc))
    return OSC_ERR_INVALID_ARGUMENT;
  if (u_stride < model->desc.nu || (z && z_stride < 3 * model->desc.nc))
    return OSC_ERR_INVALID_ARGUMENT;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != model->device) return OSC_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return model->kid == K_GO2
             ? launch_forward_dynamics<Go2>(nenv, M, C, J, u, u_stride, z, z_stride, qfrc_applied,
                                            qacc, s)
             : launch_forward_dynamics<Walter>(nenv, M, C, J, u, u_stride, z, z_stride,
                                               qfrc_applied, qacc, s);
}
