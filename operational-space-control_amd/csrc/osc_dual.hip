// osc_dual.hip -- kernel 3, the dual solution of the reference's QP (optional output,
// osc_solve_extras.y): OsqpSolver::dual_solution, unitree_go2/operational_space_controller.h:
// 534-535.
#include "osc_internal.hpp"
#include "osc_wave_sum.hpp"

namespace osc {

// ============================ kernel 3: dual solution (optional output) ======================
// The reference's OsqpSolver::dual_solution (operational_space_controller.h:534-535) over its rows
// A = [Aeq; Aineq; I_n] (osc.h:483-497; with wheel rows Aeq = [dynamics; wheel rows]) in OSQP's
// sign convention (H x + f + A'y = 0, y >= 0 on an active upper bound, <= 0 on a lower one),
// recovered from the returned design vector x = (dv, u, z) by stationarity:
//   dynamics rows  nu = -M^-1 (H_dv dv + f_dv + E'nu_w)             (the dv block)
//   wheel rows     nu_w by least squares on stationarity itself (below; the interior point's W_NU
//                  is not read: it exists only where the refinement was kept, and the active-set
//                  fallback's envs have none -- ADVICE r5)
//   u box rows     nu_a - 2 (w_tau + w_reg) u                        (the u block)
//   contact k      r_k = 2 w_reg z_k - Jc_k'nu must be balanced by its active rows: the pyramid
//                  rows, fz >= 0, fz <= big_number (a tiny non-negative least squares over the
//                  active rows, every subset of at most three -- Caratheodory -- tried: the apex,
//                  where five rows are active on three forces, has non-unique multipliers);
//                  fx, fy have no bounds (y = 0); a contact off the ground (l = u = 0) takes -r_k.
// A design vector that is not optimal shows up as a residual of the z block, a u-box multiplier of
// the wrong sign or one on an inactive bound -- the KKT certificate of tests/test_gpu_wheels.py.
// One 64-lane wavefront per env; M is factored in LDS (left-looking Cholesky, lane = row).
template <class D>
// (two waves per SIMD at least: with the serial solves' loops rolled the wheel model's kernel
// needs 124 VGPRs, four waves per SIMD -- it ran one per SIMD at 256 + 28 fully unrolled,
// 2,048 envs in two rounds of waves: 206 -> 155 us, the inner loops unrolled by four 149 us,
// bitwise, profiles/r05/dual/r05du{4,5}_*)
__global__ __launch_bounds__(kWave, 2) void osc_dual_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gM,
    const double* __restrict__ gJ, const double* __restrict__ gmask,
    const double* __restrict__ gwd, const double* __restrict__ ws, const double* __restrict__ gx,
    double* __restrict__ gy) {
  constexpr bool ENV = false;
  const EnvPtrs EP{};
#include "osc_dual_body.hpp"
}

// the _env entry points' dual kernel: the same body with the env's own parameters (a kernel of
// its own: osc_dual_kernel keeps its name, arguments and code)
template <class D>
__global__ __launch_bounds__(kWave, 2) void osc_dual_env_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gM,
    const double* __restrict__ gJ, const double* __restrict__ gmask,
    const double* __restrict__ ws, const double* __restrict__ gx, double* __restrict__ gy,
    EnvPtrs EP) {
  constexpr bool ENV = true;
  const double* __restrict__ gwd = nullptr;   // (wheel directions: no wheel-row model here)
#include "osc_dual_body.hpp"
}

template <class D>
void launch_dual_env(const LaunchArgs& a) {
  hipLaunchKernelGGL(osc_dual_env_kernel<D>, dim3(static_cast<unsigned>(a.nenv)), dim3(kWave), 0,
                     a.s, a.model->dparams, a.nenv, a.M, a.J, a.mask, a.ws, a.x, a.y, a.ep);
}

template <class D>
void launch_dual(const LaunchArgs& a) {
  hipLaunchKernelGGL(osc_dual_kernel<D>, dim3(static_cast<unsigned>(a.nenv)), dim3(kWave), 0, a.s,
                     a.model->dparams, a.nenv, a.M, a.J, a.mask, a.wdir, a.ws, a.x, a.y);
}

template void launch_dual<Go2>(const LaunchArgs&);
template void launch_dual<Walter>(const LaunchArgs&);
template void launch_dual<WalterW>(const LaunchArgs&);
template void launch_dual_env<Go2>(const LaunchArgs&);
template void launch_dual_env<Walter>(const LaunchArgs&);

}  // namespace osc
