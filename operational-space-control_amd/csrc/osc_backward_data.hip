// osc_backward_data.hip -- backward pass of the batched solve with respect to the dynamics inputs
// (C-ABI in include/osc_backward.h, osc_batch_solve_backward_data): dL/dM, dL/dC, dL/dJ, the
// per-row weight gradient, and dL/dT, dL/db, of every env from dL/dx.
//
// Per env, after the w / v stage of the first backward entry (osc_backward_wv.hpp: w = -dx_(u,z),
// v = X_y w = -dx_dv), with dv*, z* from x, nu = y[0:nv] and g_dv = dL/dx[0:nv]:
//   dnu = -M^-1 (g_dv - H_dv v)             LDL^T of M in registers, a column per lane and slot
//   Jv = J v,  e = J dv* + b - t            one pass over J, a task row per lane and slot
//   dL/dC = dnu,   dL/dM[i][k] = dnu_i dv*_k - nu_i v_k
//   dL/dJ[r][:] = -2 W_r (Jv_r dv*' + e_r v')  (- z*_j dnu' + w_z,j nu' on contact row j)
//   dL/dw_row[r] = -2 Jv_r e_r,   dL/db = -2 W Jv,   dL/dT = +2 W Jv re-laid out.
// The numpy model of this formulation (tests/backward_data_ref.projector_adjoint_data) is within
// the 1e-5 contract of the full-space reference without a refinement step of the M solve (its
// error is v's, not the solve's), so there is none.
//
// Layout: FOUR envs per wavefront, one 16-lane row each, as the first entry; nothing crosses a row
// and there are no atomics, so an env's outputs are bitwise independent of its batch.  dL/dT and
// dL/db come from the same instruction sequence as the first entry's and are bitwise its results.
// dL/dM, dL/dC and dL/dJ leave as 16-byte stores, consecutive lanes on consecutive pairs (the row
// lengths nv are even); the per-row vectors as 8-byte stores from the lane that owns the row.
// Traffic per env on top of the first entry's: M, x, b, T once; the outputs once.  The kernel
// runs one wavefront per SIMD with the AGPRs as spill space (no scratch).
#include "osc_backward.h"

#include "osc_backward_wv.hpp"

namespace osc {

// LDS per env (doubles): the w / v stage's block, then this unit's
template <class D>
struct BwDataLayout {
  static constexpr int I_VV = BwLayout<D>::IL;               // v
  static constexpr int I_DN = I_VV + even(D::NV);            // dnu
  static constexpr int I_DV = I_DN + even(D::NV);            // dv*
  static constexpr int I_NU = I_DV + even(D::NV);            // nu
  static constexpr int I_A = I_NU + even(D::NV);             // -2 W_r Jv_r per task row
  static constexpr int I_B = I_A + even(D::S);               // -2 W_r e_r per task row
  static constexpr int I_C = I_B + even(D::S);               // -z*_j per contact row
  static constexpr int I_D = I_C + even(D::NZ);              // w_z,j per contact row
  static constexpr int IL = I_D + even(D::NZ);
};

// One wavefront per SIMD for both models, the AGPRs as spill space: the w / v stage alone fills the
// 256 VGPRs of a two-wave budget (osc_backward.hip), and with this kernel's tail behind it Go2's
// spills 128 bytes per lane to scratch there.
template <class D>
__global__ __launch_bounds__(kWave, 1) void osc_backward_data_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gM,
    const double* __restrict__ gJ, const double* __restrict__ gbias,
    const double* __restrict__ gtgt, const double* __restrict__ gmask,
    const double* __restrict__ gxs, const double* __restrict__ gy,
    const int32_t* __restrict__ gstatus, const double* __restrict__ ggx,
    const double* __restrict__ ws, double* __restrict__ oM, double* __restrict__ oC,
    double* __restrict__ oJ, double* __restrict__ oW, double* __restrict__ gT,
    double* __restrict__ gb) {
  constexpr int NV = D::NV, NU = D::NU, NC = D::NC, NS = D::NS, NY = D::NY, NZ = D::NZ,
                NX = D::NX, S = D::S;
  constexpr int NROW = NV + 4 * NC + NX, R0 = 3 * NS - NZ;   // R0: the first contact row of J
  constexpr int NT = (NV + kRow - 1) / kRow;                 // dv-space slots per lane
  constexpr int NM = NV > kRow ? NV : kRow + 1;              // columns of M's factorisation
  using LY = BwLayout<D>;
  using LD = BwDataLayout<D>;
  static_assert(!D::WH, "no wheel rows");
  static_assert(NV % 2 == 0 && NT <= 2, "16-byte output pairs; two dv-space slots per lane");
  __shared__ double smem[kEnvPerWave * LD::IL];
  const int lane = static_cast<int>(threadIdx.x), l = lane & (kRow - 1);
  const long long env = static_cast<long long>(blockIdx.x) * kEnvPerWave + (lane >> 4);
  const bool valid = env < nenv;
  const size_t e = static_cast<size_t>(valid ? env : nenv - 1);   // (loads stay in bounds)
  const bool ok = valid && gstatus[e] == OSC_SOLVE_OK;
  double* B = smem + (lane >> 4) * LD::IL;
  double *sV = B + LY::I_V, *sH = B + LY::I_H, *sDinv = B + LY::I_DINV;
  double *sVv = B + LD::I_VV, *sDn = B + LD::I_DN, *sDv = B + LD::I_DV,
         *sNu = B + LD::I_NU, *sA = B + LD::I_A, *sB = B + LD::I_B, *sC = B + LD::I_C,
         *sD = B + LD::I_D;
  const double* wenv = ws + e * D::WS;
  const double* yy = gy + e * NROW;
  const double* gx = ggx + e * NX;

  // ---- the active set, K and its LDL^T, w and v = X_y w (osc_backward_wv.hpp) ----
  double v[NV], w0, w1;   // v whole in every lane of the row
  bw_solve_wv<D>(P, l, B, wenv, yy, gx, gmask + e * NC, v, w0, w1);
  const double* xs = gxs + e * NX;
  const double* J = gJ + e * (S * NV);

  // ---- H_dv v (a row per lane), v, w, dv* and nu into LDS ----
  const double* Hd = wenv + D::W_HD;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = l + kRow * t, ii = i < NV ? i : NV - 1;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc = fma(Hd[ii * NV + k], v[k], acc);
    if (i < NV) {
      sH[i] = acc;
      sDv[i] = xs[i];
      sNu[i] = yy[i];
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) sVv[i] = v[i];   // (every lane of the row holds the same v)
  sV[l] = w0;
  if (l + kRow < NY) sV[l + kRow] = w1;
  wave_sync();

  // ---- dnu = M^-1 (H_dv v - g_dv): M = L D L' in registers, lane l holding columns l and l + 16
  // (ldl_rows, the factorisation of K above; its two-slot layout wants more than 16 columns, so
  // WaLTER's 14 x 14 M is padded with identity columns to 17), then the two triangular solves.  An
  // M that is not positive definite failed the forward solve: its pivots are replaced, its
  // garbage stays in the env's row and its outputs are zeroed below ----
  {
    const int jm0 = l < NV ? l : NV - 1, j1 = l + kRow < NM ? l + kRow : NM - 1,
              jm1 = j1 < NV ? j1 : NV - 1;
    const double* Me = gM + e * (NV * NV);
    double m0[NM], m1[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      if (i < NV) {   // (row i of M across the lanes of the row: consecutive 8-byte loads)
        m0[i] = l < NV ? Me[i * NV + jm0] : 0.0;
        m1[i] = j1 < NV ? Me[i * NV + jm1] : 0.0;
      } else {
        m0[i] = i == l ? 1.0 : 0.0;
        m1[i] = i == j1 ? 1.0 : 0.0;
      }
    }
    double dg0 = 0.0, dg1 = 0.0;
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      dg0 = i == l ? m0[i] : dg0;
      dg1 = i == j1 ? m1[i] : dg1;
    }
    double dinv0, dinv1;
    ldl_rows<NM, false>(m0, m1, sDinv, l, dinv0, dinv1, 1e-13 * dg0, 1e-13 * dg1, 0.0);
    wave_sync();
    double r0 = l < NV ? sH[jm0] - gx[jm0] : 0.0, r1 = j1 < NV ? sH[jm1] - gx[jm1] : 0.0;
    ldl_solve_rows<NM>(m0, m1, dinv0, dinv1, r0, r1, l);
    if (l < NV) sDn[l] = r0;
    if (l + kRow < NV) sDn[l + kRow] = r1;
  }
  wave_sync();

  // ---- one pass over J: Jv and J dv* of task rows l, l + 16, ...; dL/db, dL/dT, dL/dw_row ----
  const double* bb = gbias + e * S;
  const double* tt = gtgt + e * S;
#pragma unroll
  for (int t = 0; t < (S + kRow - 1) / kRow; ++t) {
    const int s = l + kRow * t, ss = s < S ? s : S - 1;
    const double2* jr = reinterpret_cast<const double2*>(J + ss * NV);
    double acc = 0.0, acd = 0.0;
#pragma unroll
    for (int k = 0; k < NV / 2; ++k) {
      const double2 jj = jr[k];
      acc = fma(jj.x, v[2 * k], acc);
      acc = fma(jj.y, v[2 * k + 1], acc);
      acd = fma(jj.x, sDv[2 * k], acd);
      acd = fma(jj.y, sDv[2 * k + 1], acd);
    }
    const int sr = ss < 3 * NS ? ss : ss - 3 * NS;
    const int ti = (sr / 3) * 6 + (ss < 3 * NS ? 0 : 3) + sr % 3;   // T's entry of task row ss
    const double wr = P->w_row[ss];
    const double er = acd + bb[ss] - tt[ti];
    const double q = ok ? 2.0 * wr * acc : 0.0;   // a failed env: all-zero gradients
    if (s < S) {
      sA[s] = -2.0 * wr * acc;
      sB[s] = -2.0 * wr * er;
    }
    if (valid && s < S) {
      if (gb) gb[e * S + s] = -q;
      if (gT) gT[e * S + ti] = q;
      if (oW) oW[e * S + s] = ok ? -2.0 * acc * er : 0.0;
    }
  }
#pragma unroll
  for (int t = 0; t < (NZ + kRow - 1) / kRow; ++t) {
    const int j = l + kRow * t;
    if (j < NZ) {
      sC[j] = -xs[NV + NU + j];
      sD[j] = sV[NU + j];
    }
  }
  wave_sync();

  // ---- the matrix outputs, 16 bytes per lane, consecutive lanes on consecutive pairs ----
  if (valid) {
    if (oC) {
      double2* o2 = reinterpret_cast<double2*>(oC + e * NV);
      if (l < NV / 2)
        o2[l] = ok ? make_double2(sDn[2 * l], sDn[2 * l + 1]) : make_double2(0.0, 0.0);
    }
    if (oM) {
      double2* o2 = reinterpret_cast<double2*>(oM + e * (NV * NV));
#pragma unroll 1
      for (int p = l; p < NV * NV / 2; p += kRow) {
        const int i = (2 * p) / NV, k = 2 * p - i * NV;
        const double dn = sDn[i], nu = sNu[i];
        const double m0 = fma(-nu, sVv[k], dn * sDv[k]);
        const double m1 = fma(-nu, sVv[k + 1], dn * sDv[k + 1]);
        o2[p] = ok ? make_double2(m0, m1) : make_double2(0.0, 0.0);
      }
    }
    if (oJ) {
      double2* o2 = reinterpret_cast<double2*>(oJ + e * (S * NV));
#pragma unroll 1
      for (int p = l; p < S * NV / 2; p += kRow) {
        const int rr = (2 * p) / NV, k = 2 * p - rr * NV;
        const bool ct = rr >= R0 && rr < R0 + NZ;
        const int jc = ct ? rr - R0 : 0;
        const double a = sA[rr], b = sB[rr], c = ct ? sC[jc] : 0.0, d = ct ? sD[jc] : 0.0;
        const double j0 = fma(d, sNu[k], fma(c, sDn[k], fma(b, sVv[k], a * sDv[k])));
        const double j1 =
            fma(d, sNu[k + 1], fma(c, sDn[k + 1], fma(b, sVv[k + 1], a * sDv[k + 1])));
        o2[p] = ok ? make_double2(j0, j1) : make_double2(0.0, 0.0);
      }
    }
  }
}

namespace {

template <class D>
int launch_backward_data(const osc_model* model, int32_t nenv, const double* M, const double* J,
                         const double* b, const double* T, const double* mask, const double* x,
                         const double* y, const int32_t* status, const double* gx, double* oM,
                         double* oC, double* oJ, double* oW, double* gT, double* gb,
                         const double* ws, hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerWave - 1) /
                                              kEnvPerWave);
  hipLaunchKernelGGL(osc_backward_data_kernel<D>, dim3(nblk), dim3(kWave), 0, s, model->dparams,
                     nenv, M, J, b, T, mask, x, y, status, gx, ws, oM, oC, oJ, oW, gT, gb);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace
}  // namespace osc

extern "C" int osc_batch_solve_backward_data(
    const osc_model* model, int32_t nenv, const double* M, const double* J, const double* b,
    const double* T, const double* contact_mask, const double* x, const double* y,
    const int32_t* status, const double* grad_x, double* grad_M, double* grad_C, double* grad_J,
    double* grad_wrow, double* grad_T, double* grad_b, const void* workspace,
    size_t workspace_bytes, void* stream) {
  using namespace osc;
  // ---- every check before the launch ----
  if (!model || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (model->kid != K_GO2 && model->kid != K_WALTER) return OSC_ERR_INVALID_ARGUMENT;   // wheel rows
  if (nenv == 0) return OSC_OK;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != model->device) return OSC_ERR_INVALID_ARGUMENT;
  if (!M || !J || !b || !T || !contact_mask || !x || !y || !status || !grad_x || !workspace)
    return OSC_ERR_INVALID_ARGUMENT;
  // J is read, and grad_M, grad_C and grad_J are written, 16 bytes at a time; M (read 8 bytes at
  // a time here), the mask and the workspace as the forward call takes them
  if (misaligned(M, 16) || misaligned(J, 16) || misaligned(contact_mask, 16) ||
      misaligned(workspace, 16) || misaligned(grad_M, 16) || misaligned(grad_C, 16) ||
      misaligned(grad_J, 16) || misaligned(b, 8) || misaligned(T, 8) || misaligned(x, 8) ||
      misaligned(y, 8) || misaligned(grad_x, 8) || misaligned(grad_wrow, 8) ||
      misaligned(grad_T, 8) || misaligned(grad_b, 8) || misaligned(status, 4))
    return OSC_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < ws_layout(model->kid, nenv).total) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_M && !grad_C && !grad_J && !grad_wrow && !grad_T && !grad_b) return OSC_OK;
  const double* ws = static_cast<const double*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return model->kid == K_GO2
             ? launch_backward_data<Go2>(model, nenv, M, J, b, T, contact_mask, x, y, status,
                                         grad_x, grad_M, grad_C, grad_J, grad_wrow, grad_T,
                                         grad_b, ws, s)
             : launch_backward_data<Walter>(model, nenv, M, J, b, T, contact_mask, x, y, status,
                                            grad_x, grad_M, grad_C, grad_J, grad_wrow, grad_T,
                                            grad_b, ws, s);
}
