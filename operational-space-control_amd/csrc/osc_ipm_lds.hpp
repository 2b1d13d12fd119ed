// osc_ipm_lds.hpp -- what one interior-point wavefront keeps in LDS, by kernel variant: the
// refinement's and the wheel rows' blocks, the refinement modes, where Hr lives, and the doubles a
// wavefront asks for.  Part of osc_ipm.hpp.
#pragma once
#include "osc_internal.hpp"

namespace osc {

// LDS doubles of one IPM wavefront.  The one-wave variant must run ONE wavefront per SIMD: when
// its registers would allow two, the LDS request (> 160 KB / 5 per workgroup) is what keeps the
// dispatcher from stacking a fifth and sixth workgroup on some CUs while others idle (Go2 in
// torque coordinates: 26 KB of LDS, 255 VGPRs -> IPM 144 -> 158 us at 4,096 envs until padded).
// The refinement pass (REFINE) streams Hr from L2 and keeps instead each env's [X | H_dv | f_dv]
// block of the workspace in LDS (RefineLds).
template <class D>
struct RefineLds {
  static constexpr int X = 0;
  static constexpr int HD = D::NV * D::NY1P;
  static constexpr int GD = HD + D::NV * D::NV;
  static constexpr int SIZE = GD + even(D::NV);   // = W_SOL - W_X in the workspace
};
// Refinement modes of the IPM body: none (the interior point alone, handing its result to
// osc_refine_kernel through W_SOL: warm-started solves past one wave per SIMD, whose fused kernel
// spills, and models created with osc_model_tuning.refine_steps = 0), the refinement pass alone
// (osc_refine_kernel), or both in one wavefront (every cold solve and the one-wave warm solve:
// no hand-off, no second launch).
constexpr int kRfNone = 0, kRfOnly = 1, kRfFused = 2;
// Full-space refinement without wheel rows: rounds of active-set changes, and
// steps per round at most (each env stops at its own convergence, at least refine_steps)
// (kRefineRounds, kRefineMaxSteps: osc_device.hpp -- the host clamps refine_steps to the latter)
template <class D, bool SMALL, int RF>
constexpr bool ipm_hrl() {   // Hr kept in LDS across the interior point's iterations
  return SMALL && RF != kRfOnly && hr_fits_lds<D>();
}
// Two-wave variant (round 6): Hr's first column slot -- columns 0..15, every row
// (NY x 16 doubles per env) -- is staged into LDS once per solve, and only the second slot's
// columns are read from the workspace each iteration, as ROWS 16..NY-1 of Hr (Hr is stored exactly
// symmetric, so row j = column j bitwise): per-lane contiguous 16-byte loads over a contiguous
// (NY - 16) x NY block.  At 8,192 Go2 envs every Hr re-read used to miss L2 (37.7 MB of Hr against
// 8 x 4 MB of L2: 7x the algorithmic bytes); the streamed part is now 1.5 KB per env (12 MB).
// LDS: 246 + 384 doubles per env, 20.2 KB per wave -- eight waves per CU in 160 KB.
template <class D, bool SMALL, int RF>
constexpr bool ipm_hrh() {
  return !SMALL && !D::WH && RF != kRfOnly && D::NY > kRow &&
         (IpmLayout<D, false>::IL + D::NY * kRow) * 8 * kEnvPerWave * 8 <= 160 * 1024;
}
template <class D, bool SMALL, int RF>
constexpr int hrh_lds_extra() { return ipm_hrh<D, SMALL, RF>() ? D::NY * kRow : 0; }
// LDS doubles per env beyond the interior point's layout: the refinement's [X | H_dv | f_dv]
// block, except that a fused pass with Hr in LDS moves X into Hr's region once the first K_A is
// assembled (registers hold it from then on) and only keeps [H_dv | f_dv] apart.
// WH: the wheel rows' LDS block of an env: the rotation T (T[i][k] at i * TST + k; odd stride:
// lanes reading a row of T or a column hit distinct banks), the Q row each column of T carries
// (-1: free), q1 per Q row, a staging vector for the rotations, and the rows' multipliers.
template <class D>
struct WheelLds {
  static constexpr int NW = D::NW, NY = D::NY, TST = NY + 1;
  static constexpr int T = 0;
  static constexpr int PIN = even(NY * TST);
  static constexpr int Q1 = PIN + even(NY);
  static constexpr int ROT = Q1 + even(NW);
  static constexpr int NUV = ROT + even(NY);
  static constexpr int SIZE = NUV + even(NW);
};
template <class D, bool SMALL, int RF>
constexpr int refine_lds_extra() {
  if constexpr (D::WH && RF == kRfFused) return WheelLds<D>::SIZE;   // (reads [X | ..] from L2)
  else if constexpr (RF == kRfNone) return 0;
  else if constexpr (RF == kRfFused && !SMALL) return 0;   // reads [X | H_dv | f_dv] from L2
  else if constexpr (RF == kRfFused && ipm_hrl<D, SMALL, RF>())   // (DMA: whole 1 KB rows)
    return (((RefineLds<D>::SIZE - RefineLds<D>::HD) / 2 + kWave - 1) / kWave) * kWave * 2;
  else return RefineLds<D>::SIZE;
}
// Two-wave variant, measured and not adopted: capping the waves resident per CU so
// each XCD's Hr working set fits its L2 (slower: the eighth wave per CU hides issue latency), and
// Hr's upper triangle packed in LDS (2.5 % slower: at full occupancy the Hr loads' latency is
// already hidden, and the packed addressing costs issue slots).
template <class D, bool SMALL, int RF = kRfNone>
constexpr int ipm_lds_doubles() {
  constexpr int il = IpmLayout<D, ipm_hrl<D, SMALL, RF>()>::IL + refine_lds_extra<D, SMALL, RF>() +
                     hrh_lds_extra<D, SMALL, RF>();
  return SMALL ? cmax(kEnvPerWave * il, 160 * 1024 / 5 / 8 + 2) : kEnvPerWave * il;
}

}  // namespace osc
