// osc_ipm_ldl.hpp -- the interior point's dense linear algebra on one 16-lane DPP row per env: the
// row dot products, the LDL^T of the Newton matrix held one column per lane in two slots, and the
// triangular solves with its factor.  Part of osc_ipm.hpp; the only includer of the
// generated one-statement forms (osc_ipm_asm.hpp).
#pragma once
#include "osc_internal.hpp"
#include "osc_ipm_asm.hpp"

namespace osc {

// ============================ kernel 2: interior point, 4 env / wave ========================

// a += bcast_K(src) * ma;  b += bcast_K(src) * mb  (one broadcast source, two slots).
// NOP = true guards a source that a VALU instruction may have written just before.
template <int K, bool NOP>
__device__ __forceinline__ void fmac_bcast2(double& a, double& b, double src, double ma, double mb) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\t"
                 "v_fmac_f64_dpp %0, %2, %3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
                 : "+v"(a), "+v"(b) : "v"(src), "v"(ma), "v"(mb), "n"(K));
  else
    asm volatile("v_fmac_f64_dpp %0, %2, %3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
                 : "+v"(a), "+v"(b) : "v"(src), "v"(ma), "v"(mb), "n"(K));
}

template <int N>
__device__ __forceinline__ void dot_rows(double& a, double& b, double x0, double x1,
                                         const double (&ma)[N], const double (&mb)[N]) {
  double a2 = 0.0, b2 = 0.0;                // two chains: no back-to-back dependent f64 ops
  if constexpr (N == 24 || N == 32) {       // one asm statement (osc_ipm_asm.hpp): no s_nop per pair
    dot_rows_asm<N>(a, b, a2, b2, x0, x1, ma, mb);
    a += a2;
    b += b2;
    return;
  }
  static_for<0, N>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    if constexpr (i % 2 == 0)
      fmac_bcast2<i % kRow, i % kRow == 0>(a, b, i < kRow ? x0 : x1, ma[i], mb[i]);
    else
      fmac_bcast2<i % kRow, false>(a2, b2, i < kRow ? x0 : x1, ma[i], mb[i]);
  });
  a += a2;
  b += b2;
}

// LDL^T of an N x N symmetric matrix held one column per lane in two slots: lane l of a row
// holds column l in c0 and column l+16 in c1.  Right-looking; at step k every lane j > k
// applies  c_j[i] -= L[i][k] L[j][k] D_k  for i > k with the pivot column entry c_k[i]
// broadcast by DPP straight into the FMA.  On exit (for slot column j):
//   c[i], i > j : -L[i][j] D[j] / D[i]  (column j of L, unscaled, times -1/D_i: backward solve)
//   c[i], i < j : -L[j][i]              (row j of L: forward solve)
//   c[j]        : -1
//   dinv0, dinv1: 1 / D[j]
// thr0, thr1: 1e-13 x the original diagonal (Cholesky-infinity test: a pivot not above it
// becomes 1e128).  sdinv: 2 x 16 doubles of LDS for this row: every lane writes 1/D_k at step k
// (one ds_write instead of a lane select), each lane reads its own two back at the end.
// Slot-1 lanes past N (N < 32) hold a copy of column N-1 (the caller loads jj1 = N-1 there);
// they are left unmasked while column N-1 is still active, so they stay an exact mirror of it --
// finite, and never a broadcast source.
// Look-ahead: pivot k+1's test, broadcast, reciprocal and scaling are issued right after step k's
// first trailing FMA pair (which finalises column k+1's entry), so their dependent chain overlaps
// the rest of step k's FMAs instead of stalling between the steps (bitwise the same factor;
// profiles/r04f_ab_ldl_lookahead.jsonl: Go2 4,096 0.1737 -> 0.1721 ms per solve, 65,536 1.782 ->
// 1.762, WaLTER 4,096 0.2804 -> 0.2758).
// (Fusing pass 0's forward elimination into the factorisation -- the right-hand side formed
// first, its step k riding along the factor's -- measured within noise: Go2 4,096 0.1739 vs
// 0.1718 ms per solve, 65,536 1.760 vs 1.748, WaLTER 4,096 0.2754 vs 0.2768, and not bitwise;
// profiles/r04k/ab_fwd_fused.jsonl.)
// ASM: the scheduled one-statement form (osc_ipm_asm.hpp) -- it claims 12 VGPRs of its own, which
// the one-wave kernels (512 registers with the AGPRs) have to spare and the two-wave ones do not
// (their spills grow 12 -> 52 bytes per lane), so those keep the per-pivot form.
// du: the torque rows' diagonal terms of G'DG (lane q's column q < NU, 0 on the other lanes),
// added to each pivot where it is taken (round 6: the diagonal of K enters the factorisation only
// as its pivots, so the same K as adding du to c0[l] up front -- which took a lane select per torque
// column every iteration -- up to the rounding of the pivots' sums)
// An empty asm that "rewrites" columns I.. of both slots (ldl_rows: orders their last VALU writes)
template <int I, int N>
__device__ __forceinline__ void touch_cols(double (&c0)[N], double (&c1)[N]) {
  asm volatile("" : "+v"(c0[I]), "+v"(c1[I]));
  if constexpr (I + 1 < N) touch_cols<I + 1, N>(c0, c1);
}
template <int N, bool ASM = true>
__device__ __forceinline__ void ldl_rows(double (&c0)[N], double (&c1)[N], double* sdinv, int l,
                                         double& dinv0, double& dinv1, double thr0, double thr1,
                                         double du) {
  // pivot k's preparation: -> (t0, t1) = -L[lane][k] for the lanes still to be eliminated
  auto prep = [&](auto kc, double& t0, double& t1) {
    constexpr int k = decltype(kc)::value;
    constexpr int s = k / kRow, kl = k % kRow;
    // the lanes l > k, compared ahead of the guarded broadcast: its three wait states lie between
    // the mask's write and the selects below (osc_device.hpp lane_gt)
    const unsigned long long gt = lane_gt<kl>(l);
    const double own = (s == 0) ? c0[k] + du : c1[k];
    const double dk = bcast_guarded<kl>(own > ((s == 0) ? thr0 : thr1) ? own : 1e128);
    const double inv = recip1(dk);
    sdinv[k] = inv;
    c0[k] = -c0[k] * inv;
    c1[k] = -c1[k] * inv;
    // (in slot 1 the mirror lanes past N keep their multipliers too and so stay exact copies of
    // column N - 1)
    if constexpr (k < kRow) {
      t0 = keep_mask(gt, c0[k]);
      t1 = c1[k];
    } else {
      t0 = 0.0;   // (no lane of slot 0 lies past pivot k >= 16; not read: upd)
      t1 = keep_mask(gt, c1[k]);
    }
  };
  // one trailing FMA pair of step k, row i (NOP: the DPP source was written just before)
  auto upd = [&](auto kc, auto ic, double t0, double t1) {
    constexpr int k = decltype(kc)::value, i = decltype(ic)::value;
    constexpr int s = k / kRow, kl = k % kRow;
    constexpr bool nop = (i == k + 1) && (k >= 1) && (i == N - 1);
    if constexpr (s == 0) {
      fmac_bcast<kl, nop>(c1[i], c0[i], t1);
      if constexpr (k < kRow - 1) fmac_bcast_self<kl>(c0[i], t0);
    } else {
      fmac_bcast_self<kl, nop>(c1[i], t1);
    }
  };
  if constexpr (ASM && (N == 24 || N == 32)) {
    // one scheduled asm statement (tools/gen_ipm_asm.py -> osc_ipm_asm.hpp): the same
    // instructions on the same values, pivot k+1's preparation interleaved with pivot k's FMAs
    // so that the FMAs are the wait states (no s_nop, no asm-boundary padding)
    const unsigned addr = static_cast<unsigned>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) double*)sdinv));
    ldl_asm<N>(c0, c1, thr0, thr1, l, addr, du);
    wave_sync();
    dinv0 = sdinv[l];
    dinv1 = sdinv[(l + kRow < N) ? l + kRow : N - 1];
    return;
  }
  // Step 0's DPP reads take columns the caller's C++ just wrote (K = Hr + G'DG): every column goes
  // through an empty asm first and then one s_nop 1, so no schedule can put a column's VALU write
  // within the DPP read's two wait states (tests/test_asm_hazards.py; LLVM's ILP scheduler did).
  touch_cols<0, N>(c0, c1);
  asm volatile("s_nop 1");
  double ta0, ta1;
  prep(std::integral_constant<int, 0>{}, ta0, ta1);
  static_for<0, N>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    double tb0 = 0.0, tb1 = 0.0;
    if constexpr (k + 1 < N) {
      upd(kc, std::integral_constant<int, k + 1>{}, ta0, ta1);
      prep(std::integral_constant<int, k + 1>{}, tb0, tb1);
    }
    static_for<k + 2, N>([&](auto ic) { upd(kc, ic, ta0, ta1); });
    ta0 = tb0;
    ta1 = tb1;
  });
  wave_sync();
  dinv0 = sdinv[l];
  dinv1 = sdinv[(l + kRow < N) ? l + kRow : N - 1];
}

// Solve K x = r with the factor above; r0 (var l), r1 (var l+16) in, x out.  Every lane of
// the row is updated at every step (no lane masks): a lane whose value is already final saves
// it at its own pivot step and may take garbage afterwards.  The factor's row k is pre-scaled
// by -1/D_k (ldl_rows), so each step is the pivot's broadcast straight into the FMAs -- no
// multiply in the dependency chain (Go2 4,096: 0.183 -> 0.178 ms per solve;
// profiles/r03_ab_ldl_prescale.txt):
//   forward   z = L^-1 r             a_j += a_k * (-L[j][k])
//   backward  in D-scaled form       a_j += a_k * (-L[k][j] D_j / D_k),  x_j = a_j / D_j
// The other slot's FMA goes first: the own slot's FMA rewrites the pivot lane (c[k] = -1 there).
// (Masking each FMA to the lanes it may change through EXEC instead of saving was measured
// slower: 0.186 ms -- the EXEC writes cost more than the two v_cndmask they replace.)
// (ldl_fwd_rows / ldl_bwd_rows: the two halves, for callers that act on z in between.)
template <int N>
__device__ __forceinline__ void ldl_fwd_rows(const double (&c0)[N], const double (&c1)[N],
                                             double dinv0, double dinv1,
                                             double& a0, double& a1, int l) {
  double z0 = 0.0, z1 = 0.0;                // z_j, saved at step j
  if constexpr (N == 24 || N == 32) {       // one asm statement (osc_ipm_asm.hpp), bitwise the same
    ldl_fwd_asm<N>(c0, c1, a0, a1, z0, z1, l);
    a0 = z0;
    a1 = z1;
    return;
  }
  // step k + 1's lane mask is compared ahead of step k's selects, which with step k's FMAs are
  // its wait states (osc_device.hpp lane_eq); the selects are the DPP read's wait states
  unsigned long long m = lane_eq<0, 1>(l);
  static_for<0, N>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    constexpr int s = k / kRow, kl = k % kRow;
    unsigned long long mn = m;
    if constexpr (k + 1 < N) mn = lane_eq<(k + 1) % kRow>(l);
    if constexpr (s == 0) {
      z0 = sel_mask(m, a0, z0);
      const double p = a0;
      fmac_bcast<kl>(a1, p, c1[k]);
      if constexpr (k < kRow - 1) fmac_bcast<kl>(a0, p, c0[k]);
    } else {
      z1 = sel_mask(m, a1, z1);
      const double p = a1;
      fmac_bcast<kl>(a1, p, c1[k]);
    }
    m = mn;
  });
  a0 = z0;
  a1 = z1;
}
template <int N>
__device__ __forceinline__ void ldl_bwd_rows(const double (&c0)[N], const double (&c1)[N],
                                             double dinv0, double dinv1,
                                             double& a0, double& a1, int l) {
  double x0 = 0.0, x1 = 0.0;                // D-scaled x_j, saved at step j
  if constexpr (N == 24 || N == 32) {
    ldl_bwd_asm<N>(c0, c1, a0, a1, x0, x1, l);
    a0 = x0 * dinv0;
    a1 = x1 * dinv1;
    return;
  }
  unsigned long long m = lane_eq<(N - 1) % kRow, 1>(l);   // masks a step ahead, as in ldl_fwd_rows
  static_for<0, N>([&](auto kc) {
    constexpr int k = N - 1 - decltype(kc)::value;
    constexpr int s = k / kRow, kl = k % kRow;
    unsigned long long mn = m;
    if constexpr (k >= 1) mn = lane_eq<(k - 1) % kRow>(l);
    if constexpr (s == 0) {
      x0 = sel_mask(m, a0, x0);
      const double p = a0;
      if constexpr (k >= 1) fmac_bcast<kl>(a0, p, c0[k]);
    } else {
      x1 = sel_mask(m, a1, x1);
      const double p = a1;
      fmac_bcast<kl>(a0, p, c0[k]);
      if constexpr (k > kRow) fmac_bcast<kl>(a1, p, c1[k]);
    }
    m = mn;
  });
  a0 = x0 * dinv0;
  a1 = x1 * dinv1;
}
template <int N>
__device__ __forceinline__ void ldl_solve_rows(const double (&c0)[N], const double (&c1)[N],
                                               double dinv0, double dinv1,
                                               double& a0, double& a1, int l) {
  ldl_fwd_rows<N>(c0, c1, dinv0, dinv1, a0, a1, l);
  ldl_bwd_rows<N>(c0, c1, dinv0, dinv1, a0, a1, l);
}

}  // namespace osc
