// osc_ipm_launch.hpp -- the interior point's __global__ wrappers around ipm_block (osc_ipm.hpp,
// which includes this file last) and launch_ipm, the pass sequence of one call.
#pragma once

namespace osc {

template <class D, bool SMALL, bool WARM, int RF = kRfNone>
#ifndef OSC_LARGE_WAVES
#define OSC_LARGE_WAVES 2
#endif
__global__ __launch_bounds__(kWave, SMALL ? 1 : OSC_LARGE_WAVES) void osc_ipm_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus, int32_t* __restrict__ giters, double* __restrict__ gwarm,
    int flags) {
  // one-wave variant: four workgroups per CU (160 KB of LDS), never five.  (The opt-in wheel
  // rows' Schur blocks take it to 53 KB per wave: three per CU)
  static_assert(!SMALL || ipm_lds_doubles<D, SMALL, RF>() * 8 <= 160 * 1024 / (D::WH ? 3 : 4),
                "IPM LDS");
  static_assert(ipm_lds_doubles<D, SMALL, RF>() * 8 <= 64 * 1024, "IPM LDS per workgroup");
  __shared__ __attribute__((aligned(16))) double sm[ipm_lds_doubles<D, SMALL, RF>()];
  // flags bit 2 (warm-started, refinement fused): the cold fix-up pass runs in the same launch,
  // each wavefront right after its own warm pass (its statuses are its own global stores: the
  // fence makes them visible to its lanes) -- the separate fix-up launch, 1,024 wavefronts that
  // mostly exit at once, cost 4.2 us of a 139 us Go2 4,096 warm tick
  ipm_block<D, SMALL, WARM, RF>(P, static_cast<int>(blockIdx.x), nenv, gmask, ws, gtau, gx,
                                gstatus, giters, gwarm, flags & 3, sm);
  if constexpr (WARM || RF == kRfFused) {
    if (flags & 4) {   // (a second inlined body: a loop over both passes spilled 180 B per lane)
      // the statuses it reads are this wavefront's own stores: a workgroup-scope fence (their
      // completion) is enough -- a device-scope __threadfence() wrote the L2 back in every
      // wavefront, +15-18 % at 8,192 / 65,536 envs where two waves share each SIMD
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      ipm_block<D, SMALL, WARM, RF>(P, static_cast<int>(blockIdx.x), nenv, gmask, ws, gtau, gx,
                                    gstatus, giters, gwarm, (flags & 2) | 1, sm);
    }
  }
}

// The cold fused solve split in two passes for lockstep compaction (ParkArgs): CP = kCpPark
// over every env's wavefront, then CP = kCpResume over the parked envs, packed.
template <class D, bool SMALL, int CP>
__global__ __launch_bounds__(kWave, SMALL ? 1 : 2) void osc_ipm_compact_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus, int32_t* __restrict__ giters, int flags, ParkArgs PA) {
  __shared__ __attribute__((aligned(16))) double sm[ipm_lds_doubles<D, SMALL, kRfFused>()];
  ipm_block<D, SMALL, false, kRfFused, CP>(P, static_cast<int>(blockIdx.x), nenv, gmask, ws, gtau,
                                           gx, gstatus, giters, nullptr, flags, sm, PA);
}

// The full-space refinement pass (torque coordinates): the same body with the interior-point
// loop compiled out, started from the result the interior point left in W_SOL, so its extra
// state never weighs on the interior point's register allocation.
template <class D, bool SMALL>
__global__ __launch_bounds__(kWave, SMALL ? 1 : 2) void osc_refine_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus) {
  __shared__ __attribute__((aligned(16))) double sm[ipm_lds_doubles<D, SMALL, kRfOnly>()];
  ipm_block<D, SMALL, false, kRfOnly>(P, static_cast<int>(blockIdx.x), nenv, gmask, ws, gtau, gx,
                                   gstatus, nullptr, nullptr, 0, sm);
}

// The _env entry points' kernels (include/osc_env_params.h): osc_ipm_kernel's and
// osc_refine_kernel's bodies with ipm_block's ENV on and the per-env arrays by value.  Kernels of
// their own, so the ones above keep their names, arguments and code.
template <class D, bool SMALL, bool WARM, int RF>
__global__ __launch_bounds__(kWave, SMALL ? 1 : OSC_LARGE_WAVES) void osc_ipm_env_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus, int32_t* __restrict__ giters, double* __restrict__ gwarm,
    int flags, EnvPtrs EP) {
  static_assert(!D::WH, "per-env parameters: no wheel rows");
  __shared__ __attribute__((aligned(16))) double sm[ipm_lds_doubles<D, SMALL, RF>()];
  ipm_block<D, SMALL, WARM, RF, kCpNone, true>(P, static_cast<int>(blockIdx.x), nenv, gmask, ws,
                                               gtau, gx, gstatus, giters, gwarm, flags & 3, sm,
                                               ParkArgs{}, EP);
  if constexpr (WARM || RF == kRfFused) {
    if (flags & 4) {   // the cold fix-up pass in the same launch (osc_ipm_kernel)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      ipm_block<D, SMALL, WARM, RF, kCpNone, true>(P, static_cast<int>(blockIdx.x), nenv, gmask,
                                                   ws, gtau, gx, gstatus, giters, gwarm,
                                                   (flags & 2) | 1, sm, ParkArgs{}, EP);
    }
  }
}
template <class D, bool SMALL>
__global__ __launch_bounds__(kWave, SMALL ? 1 : 2) void osc_refine_env_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus, EnvPtrs EP) {
  __shared__ __attribute__((aligned(16))) double sm[ipm_lds_doubles<D, SMALL, kRfOnly>()];
  ipm_block<D, SMALL, false, kRfOnly, kCpNone, true>(P, static_cast<int>(blockIdx.x), nenv, gmask,
                                                     ws, gtau, gx, gstatus, nullptr, nullptr, 0, sm,
                                                     ParkArgs{}, EP);
}

// Two models' interior point in one grid, one wavefront per SIMD (the one-wave variant of both):
// blocks [0, nbA) are model A's wavefronts, the rest model B's.  The dispatcher hands out blocks
// in order, so with the slower model first the faster model's wavefronts fill the SIMDs that
// the first model's early finishers free (its iteration-count tail) -- two grids on two streams
// instead split the SIMDs between the models and each pays its own tail.
template <class DA, class DB, int RF = kRfNone>
__global__ __launch_bounds__(kWave, 1) void osc_ipm_pair_kernel(PairArgs A, PairArgs B, int flags) {
  __shared__ __attribute__((aligned(16))) double
      sm[cmax(ipm_lds_doubles<DA, true, RF>(), ipm_lds_doubles<DB, true, RF>())];
  const int nbA = (A.nenv + kEnvPerWave - 1) / kEnvPerWave;
  const int blk = static_cast<int>(blockIdx.x);
  // (flags bit 0: the cold fix-up pass over the envs left not OK, launched after the solve when
  // refinement is fused -- a second launch: a second inlined body per model spills, launch_pair)
  if (blk < nbA)
    ipm_block<DA, true, false, RF, kCpNone, false, true>(A.P, blk, A.nenv, A.mask, A.ws, A.tau, A.x,
                                                         A.status, A.iters, nullptr, flags & 1, sm);
  else
    ipm_block<DB, true, false, RF, kCpNone, false, true>(B.P, blk - nbA, B.nenv, B.mask, B.ws, B.tau,
                                                         B.x, B.status, B.iters, nullptr, flags & 1,
                                                         sm);
}

// One launch of osc_ipm_kernel<D, SMALL, WARM, RF> over the call's wavefronts.  Everything but
// `flags` (the kernel's: bit 0 the fix-up pass, bit 1 the duals, bit 2 both passes in one launch)
// comes from the call's arguments; a cold kernel takes no warm state.
template <class D, bool SMALL, bool WARM, int RF>
void ipm_launch(const LaunchArgs& a, unsigned nb, int flags) {
  hipLaunchKernelGGL((osc_ipm_kernel<D, SMALL, WARM, RF>), dim3(nb), dim3(kWave), 0, a.s,
                     a.model->dparams, a.nenv, a.mask, a.ws, a.tau, a.x, a.status, a.iters,
                     WARM ? a.warm : nullptr, flags);
}
template <class D, bool SMALL, int CP>
void ipm_compact_launch(const LaunchArgs& a, unsigned nb, int flags, const ParkArgs& pa) {
  hipLaunchKernelGGL((osc_ipm_compact_kernel<D, SMALL, CP>), dim3(nb), dim3(kWave), 0, a.s,
                     a.model->dparams, a.nenv, a.mask, a.ws, a.tau, a.x, a.status, a.iters, flags,
                     pa);
}
// f(std::bool_constant<small>{}): the runtime choice between the one-wave and the two-wave
// variant as the template argument the kernels take
template <class F>
void with_small(bool small, F&& f) {
  if (small) f(std::true_type{});
  else f(std::false_type{});
}

// ---- launch_ipm: the interior-point passes of one call (after the assembly) ----
// All wavefronts resident at once (<= one per SIMD): the latency-optimised variant (one wave per
// SIMD, Hr in LDS where it fits); otherwise the two-waves-per-SIMD variant.
template <class D>
void launch_ipm(const LaunchArgs& a) {
  const osc_model* model = a.model;
  const int32_t nenv = a.nenv;
  const unsigned nb = static_cast<unsigned>((nenv + kEnvPerWave - 1) / kEnvPerWave);
  const int flags = a.y != nullptr ? 2 : 0;   // hand the multipliers to the dual kernel
  if constexpr (D::WH) {
    // wheel rows: the one-wave solve with the refinement fused; warm-started: the warm pass, then
    // (same launch) the cold fix-up pass in the wavefronts holding an env the warm start left
    // unconverged (the per-env status: the caller's array, else scratch -- launch_t).  The fused entries then run
    // the active-set fallback over the envs the interior point left unconverged (launch_gi).
    if (a.warm == nullptr) ipm_launch<D, true, false, kRfFused>(a, nb, flags);
    else ipm_launch<D, true, true, kRfFused>(a, nb, flags | 4);
  } else {
    // A warm-started solve is followed by a cold fix-up pass over the wavefronts that hold an
    // env the warm start did not bring to convergence (per-env status: launch_t).
    const bool small = nenv <= model->small_batch_max;
    // Every cold solve runs the refinement in the same wavefront (kRfFused), and so does the
    // one-wave warm solve; warm past one wave per SIMD the fused two-wave kernel spills (Go2
    // 65,536 warm 50.0 -> 44.5 M solves/s), so that case keeps the separate refinement pass.
    const bool fused = a.warm == nullptr && model->refine;
    const bool fused_warm = small && a.warm != nullptr && model->refine;
    // Lockstep compaction: more wavefronts than SIMDs, so the SIMD time the lockstep tail costs
    // is time other wavefronts could use (ParkArgs; bitwise the single pass's results)
    // (from four rounds of wavefronts per SIMD: at two, WaLTER configs[3] -- 8,192 tumbling envs,
    // masks redrawn -- is 4 % slower with it, 17.0 vs 17.7 M solves/s; at eight, 32,768, 3 %
    // faster: profiles/r03ze_*)
    const bool compact = fused && model->park_it > 0 &&
                         nenv >= kParkMinRounds * model->resident_envs &&
                         static_cast<size_t>(nenv) * D::WS < (size_t{1} << 32);
    if (a.warm == nullptr && compact) {
      const WsLayout wl = ws_layout(model->kid, nenv);
      char* base = reinterpret_cast<char*>(a.ws);
      ParkArgs pa;
      pa.park = reinterpret_cast<double*>(base + wl.park);
      pa.list = reinterpret_cast<int32_t*>(base + wl.list);
      pa.count = reinterpret_cast<int32_t*>(base + wl.count);
      pa.park_it = model->park_it;
      (void)hipMemsetAsync(pa.count, 0, sizeof(int32_t), a.s);
      with_small(small, [&](auto S) {
        constexpr bool SMALL = decltype(S)::value;
        ipm_compact_launch<D, SMALL, kCpPark>(a, nb, flags, pa);
        ipm_compact_launch<D, SMALL, kCpResume>(a, nb, flags, pa);
      });
      // the cold fix-up pass the one-launch solves run in their own launch (an env left not OK
      // re-solved cold to mu <= 1e-12): here a third launch, whose wavefronts without such an
      // env exit at once (round 5 census: 3 WaLTER envs in 1.6 M stalled at max_iter here)
      with_small(small, [&](auto S) {
        ipm_launch<D, decltype(S)::value, false, kRfFused>(a, nb, (flags & 2) | 1);
      });
    } else if (a.warm == nullptr) {
      // every env the interior point or the refinement leaves not OK (MAX_ITER, UNREFINED,
      // non-finite) is re-solved cold to mu <= 1e-12 by its own wavefront in the same launch, as
      // the warm entries do (round 5's census: ~1 such env per 600,000 joint-state envs; only
      // the wavefronts holding one run the second pass)
      with_small(small, [&](auto S) {
        constexpr bool SMALL = decltype(S)::value;
        if (fused) ipm_launch<D, SMALL, false, kRfFused>(a, nb, flags | 4);
        else ipm_launch<D, SMALL, false, kRfNone>(a, nb, flags);
      });
    } else if (fused_warm) {
      // warm-started: the refinement runs in the same wavefront too, in the warm pass for the
      // envs the warm start converged and in the cold fix-up pass (same launch) for the ones it
      // redoes
      ipm_launch<D, true, true, kRfFused>(a, nb, 4);
    } else {
      // warm past one wave per SIMD (or without the refinement): the warm pass, the separate
      // refinement pass, then the cold fix-up pass over every env not OK by then -- MAX_ITER,
      // non-finite, and an env whose refinement found no KKT point, UNREFINED.  The
      // fix-up pass runs the refinement in its own wavefront (the fused two-wave warm kernel: it
      // spills, but only the wavefronts holding such an env execute it).
      auto warm_pass = [&](int fl) {
        with_small(small, [&](auto S) {
          ipm_launch<D, decltype(S)::value, true, kRfNone>(a, nb, fl);
        });
      };
      warm_pass(0);
      if (model->refine) {
        hipLaunchKernelGGL((osc_refine_kernel<D, false>), dim3(nb), dim3(kWave), 0, a.s,
                           model->dparams, nenv, a.mask, a.ws, a.tau, a.x, a.status);
        ipm_launch<D, false, true, kRfFused>(a, nb, 1);
      } else {
        warm_pass(1);
      }
    }
  }
}

// ---- launch_ipm_env: launch_ipm's pass sequence with the per-env kernels ----
// (models with the refinement on and no wheel rows: the entries refuse the others.)  No lockstep
// compaction: its park and resume kernels have no per-env variant -- the results are bitwise the
// single pass's (tests/test_gpu_stages.py), only the throughput of cold batches from kParkMinRounds
// rounds of wavefronts per SIMD differs.
template <class D, bool SMALL, bool WARM, int RF>
void ipm_env_launch(const LaunchArgs& a, unsigned nb, int flags) {
  hipLaunchKernelGGL((osc_ipm_env_kernel<D, SMALL, WARM, RF>), dim3(nb), dim3(kWave), 0, a.s,
                     a.model->dparams, a.nenv, a.mask, a.ws, a.tau, a.x, a.status, a.iters,
                     WARM ? a.warm : nullptr, flags, a.ep);
}
template <class D>
void launch_ipm_env(const LaunchArgs& a) {
  const unsigned nb = static_cast<unsigned>((a.nenv + kEnvPerWave - 1) / kEnvPerWave);
  const int flags = a.y != nullptr ? 2 : 0;
  const bool small = a.nenv <= a.model->small_batch_max;
  if (a.warm == nullptr) {          // cold: refinement and fix-up pass fused, one launch
    with_small(small, [&](auto S) {
      ipm_env_launch<D, decltype(S)::value, false, kRfFused>(a, nb, flags | 4);
    });
  } else if (small) {               // warm, one wave per SIMD: the same
    ipm_env_launch<D, true, true, kRfFused>(a, nb, 4);
  } else {                          // warm past it: warm pass, refinement pass, cold fix-up pass
    ipm_env_launch<D, false, true, kRfNone>(a, nb, 0);
    hipLaunchKernelGGL((osc_refine_env_kernel<D, false>), dim3(nb), dim3(kWave), 0, a.s,
                       a.model->dparams, a.nenv, a.mask, a.ws, a.tau, a.x, a.status, a.ep);
    ipm_env_launch<D, false, true, kRfFused>(a, nb, 1);
  }
}

}  // namespace osc
