// osc_multi.hip -- the two-model grids of osc_batch_solve_multi (BASELINE configs[4]: a Go2 shard
// and a WaLTER Sr shard on one GPU): ONE assembly grid (osc_setup_pair_kernel) and ONE
// interior-point grid (osc_ipm_pair_kernel) over both models, the slower model's wavefronts first.
// And those of osc_batch_tick_multi (include/osc_mixed.h): the warm-started interior-point grid
// (osc_ipm_pair_warm_kernel) and the joint-state front end (osc_kinematics_pair_kernel).
#include <algorithm>

#include "osc_ipm.hpp"
#include "osc_kin_model.hpp"
#include "osc_setup.hpp"

namespace osc {

namespace {
template <class DA, class DB>
void launch_pair(const osc_batch_job& a, const osc_batch_job& b, hipStream_t s) {
  // (the fix-up pass reads each env's status: the caller's array, else the workspace's scratch
  // after the per-env blocks, as launch_t places it)
  auto args = [](const osc_batch_job& j, int ws_doubles) {
    PairArgs p;
    p.P = j.model->dparams;
    p.nenv = j.nenv;
    p.M = j.M; p.C = j.C; p.J = j.J; p.b = j.b; p.T = j.T; p.mask = j.contact_mask;
    p.ws = static_cast<double*>(j.workspace);
    p.tau = j.tau; p.x = j.x; p.iters = j.iters;
    p.status = j.status ? j.status
                        : reinterpret_cast<int32_t*>(p.ws + static_cast<size_t>(ws_doubles) * j.nenv);
    return p;
  };
  const PairArgs A = args(a, DA::WS), B = args(b, DB::WS);
  hipLaunchKernelGGL((osc_setup_pair_kernel<DA, DB>),
                     dim3(static_cast<unsigned>(a.nenv + b.nenv)), dim3(kWave), 0, s, A, B);
  const unsigned nb = static_cast<unsigned>((a.nenv + kEnvPerWave - 1) / kEnvPerWave +
                                            (b.nenv + kEnvPerWave - 1) / kEnvPerWave);
  // one-wave interior point of both models with the refinement in the same wavefront
  // (then the cold fix-up pass over the envs the solve left not OK, as launch_ipm's entries do)
  if (a.model->refine || b.model->refine) {
    hipLaunchKernelGGL((osc_ipm_pair_kernel<DA, DB, kRfFused>), dim3(nb), dim3(kWave), 0, s, A, B,
                       0);
    hipLaunchKernelGGL((osc_ipm_pair_kernel<DA, DB, kRfFused>), dim3(nb), dim3(kWave), 0, s, A, B,
                       1);
  } else {
    hipLaunchKernelGGL((osc_ipm_pair_kernel<DA, DB>), dim3(nb), dim3(kWave), 0, s, A, B, 0);
  }
}
}  // namespace

void launch_pair_walter_go2(const osc_batch_job& w, const osc_batch_job& g, hipStream_t s) {
  launch_pair<Walter, Go2>(w, g, s);
}

// ---- the two-model tick (osc_batch_tick_multi, include/osc_mixed.h) ----

// Two models' warm-started interior point in one grid, the refinement fused: the warm twin of
// osc_ipm_pair_kernel<DA, DB, kRfFused> (same LDS, same blocks-by-model dispatch).  WA / WB say
// which model's job carries a warm state; the other one's wavefronts run the cold body in the same
// grid, so each job is bitwise its own single-model call.  flags bit 2: the cold fix-up pass in
// the same launch, each wavefront right after its own solve, as osc_ipm_kernel runs it (four
// inlined bodies: 256 VGPRs + 236 AGPRs and no scratch, as the solo warm kernels; the SGPR
// spills go to VGPR lanes).  -DOSC_PAIR_WARM_TWO_LAUNCHES builds the other form, the fix-up pass
// as a second launch (flags bit 0) like the cold pair's: also without scratch, measured 1 %
// slower at 4,096 + 4,096 envs (DESIGN.md §8 has both forms' resource numbers and times).
template <class D, bool W>
__device__ __forceinline__ void pair_tick_body(const PairArgs& a, int blk, int flags, double* sm) {
  ipm_block<D, true, W, kRfFused, kCpNone, false, true>(a.P, blk, a.nenv, a.mask, a.ws, a.tau, a.x,
                                                        a.status, a.iters, W ? a.warm : nullptr,
                                                        flags & 1, sm);
#ifndef OSC_PAIR_WARM_TWO_LAUNCHES
  if (flags & 4) {   // (its statuses are the wavefront's own stores: a workgroup-scope fence)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    ipm_block<D, true, W, kRfFused, kCpNone, false, true>(a.P, blk, a.nenv, a.mask, a.ws, a.tau,
                                                          a.x, a.status, a.iters,
                                                          W ? a.warm : nullptr, 1, sm);
  }
#endif
}

template <class DA, class DB, bool WA, bool WB>
__global__ __launch_bounds__(kWave, 1) void osc_ipm_pair_warm_kernel(PairArgs A, PairArgs B,
                                                                     int flags) {
  static_assert(WA || WB, "the cold pair is osc_ipm_pair_kernel");
  __shared__ __attribute__((aligned(16))) double
      sm[cmax(ipm_lds_doubles<DA, true, kRfFused>(), ipm_lds_doubles<DB, true, kRfFused>())];
  const int nbA = (A.nenv + kEnvPerWave - 1) / kEnvPerWave;
  const int blk = static_cast<int>(blockIdx.x);
  if (blk < nbA) pair_tick_body<DA, WA>(A, blk, flags, sm);
  else pair_tick_body<DB, WB>(B, blk - nbA, flags, sm);
}

// Two models' kinematics in one grid: blocks [0, ceil(A.nenv / 4)) are model A's wavefronts, the
// rest model B's; each block stages its own model's tables.  Dynamic LDS: the larger of the two
// models' 4 * EnvLayout.size doubles.
struct KinPairArgs {
  const osc_kin::KinDev* K;
  int nenv;
  const double *qpos, *qvel;
  double *M, *C, *J, *b;
};
extern __shared__ __attribute__((aligned(16))) double osc_kin_pair_sm[];
__global__ __launch_bounds__(kWave) void osc_kinematics_pair_kernel(KinPairArgs A, KinPairArgs B) {
  __shared__ __attribute__((aligned(16))) osc_kin::KinDev sK;
  const int nbA = (A.nenv + kEnvPerWave - 1) / kEnvPerWave;
  const int blk = static_cast<int>(blockIdx.x);
  if (blk < nbA)
    osc_kin::kin_block(A.K, &sK, osc_kin_pair_sm, blk, A.nenv, A.qpos, A.qvel, A.M, A.C, A.J, A.b,
                       nullptr);
  else
    osc_kin::kin_block(B.K, &sK, osc_kin_pair_sm, blk - nbA, B.nenv, B.qpos, B.qvel, B.M, B.C, B.J,
                       B.b, nullptr);
}

void launch_kin_pair(const PairTick& a, const PairTick& b, hipStream_t s) {
  static_assert(osc_kin::kKinWave == kWave && osc_kin::kKinEnvPerWave == kEnvPerWave, "one layout");
  auto args = [](const PairTick& j) {
    return KinPairArgs{j.kin->dev, j.nenv, j.qpos, j.qvel, j.M, j.C, j.J, j.b};
  };
  auto lds = [](const PairTick& j) {
    const osc_kin::KinDev& k = j.kin->host;
    return sizeof(double) * static_cast<size_t>(osc_kin::EnvLayout(k.nq, k.nv, k.nbody, k.nsite).size) *
           kEnvPerWave;
  };
  const unsigned nb = static_cast<unsigned>((a.nenv + kEnvPerWave - 1) / kEnvPerWave +
                                            (b.nenv + kEnvPerWave - 1) / kEnvPerWave);
  hipLaunchKernelGGL(osc_kinematics_pair_kernel, dim3(nb), dim3(kWave), std::max(lds(a), lds(b)), s,
                     args(a), args(b));
}

namespace {
template <class DA, class DB>
void launch_pair_tick(const PairTick& a, const PairTick& b, hipStream_t s) {
  auto args = [](const PairTick& j, int ws_doubles) {
    PairArgs p;
    p.P = j.model->dparams;
    p.nenv = j.nenv;
    p.M = j.M; p.C = j.C; p.J = j.J; p.b = j.b; p.T = j.T; p.mask = j.mask;
    p.ws = j.ws;
    p.tau = j.tau; p.x = j.x; p.iters = j.iters;
    // (the fix-up pass reads each env's status: the caller's array, else scratch, as launch_t)
    p.status = j.status ? j.status
                        : reinterpret_cast<int32_t*>(p.ws + static_cast<size_t>(ws_doubles) * j.nenv);
    p.warm = j.warm;
    return p;
  };
  const PairArgs A = args(a, DA::WS), B = args(b, DB::WS);
  // joint states: both models' kinematics in one grid (a lone joint-state job's ran before this)
  if (a.kin != nullptr && b.kin != nullptr) launch_kin_pair(a, b, s);
  hipLaunchKernelGGL((osc_setup_pair_kernel<DA, DB>),
                     dim3(static_cast<unsigned>(a.nenv + b.nenv)), dim3(kWave), 0, s, A, B);
  const unsigned nb = static_cast<unsigned>((a.nenv + kEnvPerWave - 1) / kEnvPerWave +
                                            (b.nenv + kEnvPerWave - 1) / kEnvPerWave);
  // the solve and the cold fix-up pass over the envs it left not OK (a warm job's in its warm
  // kernel: it writes the re-solved envs' warm state): one launch with a warm job, two launches
  // for two cold jobs, as osc_batch_solve_multi
  auto pass = [&](int flags) {
    if (A.warm && B.warm)
      hipLaunchKernelGGL((osc_ipm_pair_warm_kernel<DA, DB, true, true>), dim3(nb), dim3(kWave), 0,
                         s, A, B, flags);
    else if (A.warm)
      hipLaunchKernelGGL((osc_ipm_pair_warm_kernel<DA, DB, true, false>), dim3(nb), dim3(kWave), 0,
                         s, A, B, flags);
    else if (B.warm)
      hipLaunchKernelGGL((osc_ipm_pair_warm_kernel<DA, DB, false, true>), dim3(nb), dim3(kWave), 0,
                         s, A, B, flags);
    else
      hipLaunchKernelGGL((osc_ipm_pair_kernel<DA, DB, kRfFused>), dim3(nb), dim3(kWave), 0, s, A,
                         B, flags);
  };
#ifndef OSC_PAIR_WARM_TWO_LAUNCHES
  if (A.warm || B.warm) {
    pass(4);
    return;
  }
#endif
  pass(0);
  pass(1);
}
}  // namespace

void launch_pair_tick_walter_go2(const PairTick& w, const PairTick& g, hipStream_t s) {
  launch_pair_tick<Walter, Go2>(w, g, s);
}

}  // namespace osc
