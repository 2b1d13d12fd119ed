// osc_backward.hip -- backward pass of the batched solve (C-ABI in include/osc_backward.h):
// dL/dT and dL/db of every env from dL/dx, by one equality-constrained solve with the reduced
// Hessian the forward call left in its workspace.
//
// Per env, with y' = (u, z), dv = X_y y' + X_c, P the orthogonal projector onto the null space of
// the active rows and K = P Hr P + (I - P):
//   r = P ((g_u, g_z) + X_y' g_dv),   w = P K^-1 r,   one refinement step
//   w += P K^-1 (r - P (X_y'(H_dv (X_y w)) + D w))   (the residual never goes through Hr),
//   v = X_y w,  q = 2 W (J v),  dL/db = -q,  dL/dT = +q re-laid out.
// P is block diagonal -- 1 or 0 per torque, a 3 x 3 projector per contact from Gram-Schmidt of its
// active rows' normals with a rank test (an unloaded foot sits at the pyramid apex: five active
// rows on three forces) -- so K is positive definite and of the interior point's size whatever is
// active, and the kernel reuses that kernel's layout and linear algebra (osc_ipm_ldl.hpp): FOUR
// envs per wavefront, one 16-lane DPP row each, lane l holding columns l and l + 16 of K, the
// LDL^T and the triangular solves broadcasting inside the row by DPP.  Nothing crosses a row, so
// an env's result does not depend on its neighbours (a failed env's NaNs stay in its row, and its
// outputs are zeroed), and there are no atomics: results are bitwise reproducible.
//
// Traffic per env: J once for the final product (each lane walks whole rows, 16 bytes per load),
// Hr three times over for P Hr P's column combinations (each lane reads the up to three Hr
// columns of its contact's block; the repeats hit the cache), X_y four times (r, X_y w twice, the
// residual), H_dv once.  No scratch.
#include "osc_backward.h"

#include "osc_backward_wv.hpp"

namespace osc {

// Two waves per SIMD for the 24-column system (Go2: 256 VGPRs, no scratch).  WaLTER's 32 columns
// are 128 VGPRs of K alone and spill at that budget (68 bytes per lane of scratch), so, like its
// interior point, it runs one wave per SIMD with the AGPRs as spill space (256 + 24, no scratch).
template <class D>
__global__ __launch_bounds__(kWave, D::NY > 24 ? 1 : 2) void osc_backward_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gJ,
    const double* __restrict__ gmask, const double* __restrict__ gy,
    const int32_t* __restrict__ gstatus, const double* __restrict__ ggx,
    const double* __restrict__ ws, double* __restrict__ gT, double* __restrict__ gb) {
  constexpr int NV = D::NV, NC = D::NC, NS = D::NS, NX = D::NX, S = D::S;
  constexpr int NROW = NV + 4 * NC + NX;
  using LY = BwLayout<D>;
  static_assert(!D::WH, "no wheel rows");
  __shared__ double smem[kEnvPerWave * LY::IL];
  const int lane = static_cast<int>(threadIdx.x), l = lane & (kRow - 1);
  const long long env = static_cast<long long>(blockIdx.x) * kEnvPerWave + (lane >> 4);
  const bool valid = env < nenv;
  const size_t e = static_cast<size_t>(valid ? env : nenv - 1);   // (loads stay in bounds)
  const bool ok = valid && gstatus[e] == OSC_SOLVE_OK;
  const double* J = gJ + e * (S * NV);

  // ---- the active set, K and its LDL^T, w and v = X_y w (osc_backward_wv.hpp) ----
  double v[NV], w0, w1;   // v whole in every lane of the row
  bw_solve_wv<D>(P, l, smem + (lane >> 4) * LY::IL, ws + e * D::WS, gy + e * NROW, ggx + e * NX,
                 gmask + e * NC, v, w0, w1);

  // ---- q = 2 W (J v): task rows l, l + 16, ... of this lane; dL/db = -q, dL/dT = +q ----
#pragma unroll
  for (int t = 0; t < (S + kRow - 1) / kRow; ++t) {
    const int s = l + kRow * t, ss = s < S ? s : S - 1;
    const double2* jr = reinterpret_cast<const double2*>(J + ss * NV);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NV / 2; ++k) {
      const double2 jj = jr[k];
      acc = fma(jj.x, v[2 * k], acc);
      acc = fma(jj.y, v[2 * k + 1], acc);
    }
    const double q = ok ? 2.0 * P->w_row[ss] * acc : 0.0;   // a failed env: all-zero gradients
    if (valid && s < S) {
      if (gb) gb[e * S + s] = -q;
      if (gT) {
        const int sr = s < 3 * NS ? s : s - 3 * NS;
        gT[e * S + (sr / 3) * 6 + (s < 3 * NS ? 0 : 3) + sr % 3] = q;
      }
    }
  }
}

namespace {

template <class D>
int launch_backward(const osc_model* model, int32_t nenv, const double* J, const double* mask,
                    const double* y, const int32_t* status, const double* gx, double* gT,
                    double* gb, const double* ws, hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerWave - 1) /
                                              kEnvPerWave);
  hipLaunchKernelGGL(osc_backward_kernel<D>, dim3(nblk), dim3(kWave), 0, s, model->dparams, nenv,
                     J, mask, y, status, gx, ws, gT, gb);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace
}  // namespace osc

extern "C" int osc_batch_solve_backward(const osc_model* model, int32_t nenv, const double* J,
                                        const double* contact_mask, const double* y,
                                        const int32_t* status, const double* grad_x,
                                        double* grad_T, double* grad_b, const void* workspace,
                                        size_t workspace_bytes, void* stream) {
  using namespace osc;
  // ---- every check before the launch ----
  if (!model || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (model->kid != K_GO2 && model->kid != K_WALTER) return OSC_ERR_INVALID_ARGUMENT;   // wheel rows
  if (nenv == 0) return OSC_OK;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != model->device) return OSC_ERR_INVALID_ARGUMENT;
  if (!J || !contact_mask || !y || !status || !grad_x || !workspace)
    return OSC_ERR_INVALID_ARGUMENT;
  // J is read 16 bytes at a time; the mask and the workspace as the forward call takes them
  if (misaligned(J, 16) || misaligned(contact_mask, 16) || misaligned(workspace, 16) ||
      misaligned(y, 8) || misaligned(grad_x, 8) || misaligned(grad_T, 8) ||
      misaligned(grad_b, 8) || misaligned(status, 4))
    return OSC_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < ws_layout(model->kid, nenv).total) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_T && !grad_b) return OSC_OK;
  const double* ws = static_cast<const double*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return model->kid == K_GO2
             ? launch_backward<Go2>(model, nenv, J, contact_mask, y, status, grad_x, grad_T,
                                    grad_b, ws, s)
             : launch_backward<Walter>(model, nenv, J, contact_mask, y, status, grad_x, grad_T,
                                       grad_b, ws, s);
}
