// osc_ipm_wheel.hpp -- the wheel no-slip rows (D::WH) of the interior point and its refinement.
// Wheel no-slip rows (WH): Q [y; 1] = 0, orthonormal rows (setup_env).  The Newton systems of
// the interior point and the refinement are solved in y^ = T'y, T = [rows of Q | null-space
// basis] (setup_env): K^ = H^ + sum_r D_r (T'g_r)(T'g_r)' assembled from the rows g_r of G one
// original coordinate at a time (no cancellation of large entries), the coordinates along Q's
// rows pinned (identity rows, step = -(Q y + q1): the rows hold after every step).  The
// iterate itself stays in y coordinates.  (An earlier Schur-complement treatment of the rows on
// K's factor lost the Newton steps' accuracy next to nearly dependent active rows: DESIGN.md §3.)
// Everything here is called only from `if constexpr` branches of a D::WH kernel.  Part of
// osc_ipm.hpp.
#pragma once
#include "osc_ipm_lds.hpp"
#include "osc_ipm_rows.hpp"

namespace osc {

// The wheel rows' LDS block of an env (WheelLds) and this lane's slots: pinned?  (the Q row's q1
// for the residual)
struct WheelRot {
  double *T, *Pin, *Q1, *Rot, *Nu;
  bool pin0 = false, pin1 = false;
  double q10 = 0.0, q11 = 0.0;
};
template <class D>
__device__ __forceinline__ WheelRot wheel_rot(double* base) {
  using WL = WheelLds<D>;
  WheelRot W;
  W.T = base + WL::T;
  W.Pin = base + WL::PIN;
  W.Q1 = base + WL::Q1;
  W.Rot = base + WL::ROT;
  W.Nu = base + WL::NUV;
  return W;
}

template <class D>
__device__ __forceinline__ void rot_load_pins(WheelRot& W, const RowLane& L) {
  const double p0v = W.Pin[L.j0], p1v = W.Pin[L.jj1];
  W.pin0 = p0v != -1.0;
  W.pin1 = L.v1 && p1v != -1.0;
  W.q10 = p0v >= 0.0 ? W.Q1[static_cast<int>(p0v)] : 0.0;
  W.q11 = (L.v1 && p1v >= 0.0) ? W.Q1[static_cast<int>(p1v)] : 0.0;
}
// T'v and T v for a y-space vector held in the lane slots (staged through W.Rot)
template <class D>
__device__ __forceinline__ void rot_in(const WheelRot& W, const RowLane& L, double v0, double v1v,
                                       double& o0, double& o1) {
  constexpr int NY = D::NY, TST = WheelLds<D>::TST;
  const int j0 = L.j0, j1 = L.j1, jj1 = L.jj1;
  wave_sync();
  W.Rot[j0] = v0;
  if (L.v1) W.Rot[j1] = v1v;
  wave_sync();
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int i = 0; i < NY; ++i) {
    const double r = W.Rot[i];
    a0 = fma(W.T[i * TST + j0], r, a0);
    a1 = fma(W.T[i * TST + jj1], r, a1);
  }
  o0 = a0;
  o1 = a1;
  wave_sync();
}
template <class D>
__device__ __forceinline__ void rot_out(const WheelRot& W, const RowLane& L, double v0, double v1v,
                                        double& o0, double& o1) {
  constexpr int NY = D::NY, TST = WheelLds<D>::TST;
  const int j0 = L.j0, j1 = L.j1, jj1 = L.jj1;
  wave_sync();
  W.Rot[j0] = v0;
  if (L.v1) W.Rot[j1] = v1v;
  wave_sync();
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = 0; k < NY; ++k) {
    const double r = W.Rot[k];
    a0 = fma(W.T[j0 * TST + k], r, a0);
    a1 = fma(W.T[jj1 * TST + k], r, a1);
  }
  o0 = a0;
  o1 = a1;
  wave_sync();
}

// WH: c0 / c1 hold H^'s columns j0, jj1; add T'(G'DG)T from sDr (D per row slot) one original
// coordinate i at a time -- column j gains coef_i(j) T[i][:], coef_i(j) = (G'DG)[i][:] T[:][j]
// (torque rows: diagonal; a contact's rows: its 3 x 3 block) -- then pin Q's coordinates.
// Returns the assembled diagonal entries (the pivot threshold's reference).
template <class D>
__device__ __forceinline__ void assemble_rot(const WheelRot& W, const RowLane& L, const double* sDr,
                                             double (&c0)[D::NY], double (&c1)[D::NY],
                                             double& dg0r, double& dg1r) {
  constexpr int NY = D::NY, NU = D::NU, NC = D::NC, TST = WheelLds<D>::TST;
  const int j0 = L.j0, jj1 = L.jj1;
  // K^ columns j0, jj1 += T' (B T)[:, j] with B = G'DG (diagonal on u, a 3 x 3 block per
  // contact), one row i of T at a time: a = (B T)[i, j] from the lane's own entries of T, then
  // c[m] += a T[i][m] with T[i][m] broadcast from the lane that owns column m
  // (v_fmac_f64_dpp row_newbcast) -- each lane reads its own two entries of row i instead of
  // the whole row from LDS (the per-iteration product of the wheel rows: NY^3 per env)
  auto rank1 = [&](double a0, double a1, double t0, double t1) __attribute__((always_inline)) {
    static_for<0, kRow>([&](auto K) __attribute__((always_inline)) {
      constexpr int k = decltype(K)::value;
      if constexpr (k < NY) {
        fmac_bcast<k, k == 0>(c0[k], t0, a0);
        fmac_bcast<k>(c1[k], t0, a1);
      }
      if constexpr (k + kRow < NY) {
        fmac_bcast<k, k == 0>(c0[k + kRow], t1, a0);
        fmac_bcast<k>(c1[k + kRow], t1, a1);
      }
    });
  };
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const double d = sDr[2 * i] + sDr[2 * i + 1];
    const double t0 = W.T[i * TST + j0], t1 = W.T[i * TST + jj1];
    rank1(d * t0, d * t1, t0, t1);
  }
  static_for<0, NC>([&](auto Kc) __attribute__((always_inline)) {
    constexpr int k = decltype(Kc)::value, zb = NU + 3 * k;
    double t0r[3], t1r[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      t0r[r] = W.T[(zb + r) * TST + j0];
      t1r[r] = W.T[(zb + r) * TST + jj1];
    }
    static_for<0, 3>([&](auto Ci) __attribute__((always_inline)) {
      constexpr int ci = decltype(Ci)::value;
      double b0, b1, b2;   // row ci of contact k's block (symmetric: its column ci)
      contact_col<D>(L.mu_f, sDr, k, ci, b0, b1, b2);
      const double a0 = b0 * t0r[0] + b1 * t0r[1] + b2 * t0r[2];
      const double a1 = b0 * t1r[0] + b1 * t1r[1] + b2 * t1r[2];
      rank1(a0, a1, t0r[ci], t1r[ci]);
    });
  });
  double d0 = 0.0, d1 = 0.0;
#pragma unroll
  for (int m = 0; m < NY; ++m) {
    const bool pm = W.Pin[m] != -1.0;
    c0[m] = W.pin0 ? ((m == j0) ? 1.0 : 0.0) : (pm ? 0.0 : c0[m]);
    c1[m] = W.pin1 ? ((m == jj1) ? 1.0 : 0.0) : (pm ? 0.0 : c1[m]);
    d0 = (m == j0) ? c0[m] : d0;
    d1 = (m == jj1) ? c1[m] : d1;
  }
  dg0r = d0;
  dg1r = d1;
}

// WH with the duals requested: the wheel rows' multipliers (W_NU; the refinement's where it is
// kept, else the interior point's centre) -- a diagnostic of the workspace since round 4: the
// dual kernel recovers every multiplier, the wheel rows' included, from the design vector.
// (w = L' nu: the multipliers of the rows [V X | V x0 - vs] before their orthonormalisation,
// which the dual kernel maps back to E's rows; every lane of the env's row takes part)
template <class D>
__device__ __forceinline__ void put_wheel_duals(const double* ws, int env, int l,
                                                bool want_dual, bool write_out, double nu) {
  constexpr int NW = D::NW;
  if (want_dual) {
    const double* Lw = ws + static_cast<size_t>(env) * D::WS + D::W_WL;
    const int lc = l < NW ? l : 0;
    double acc = 0.0;
    static_for<0, NW>([&](auto W) {
      constexpr int w = decltype(W)::value;
      acc = fma(Lw[w * NW + lc], bcast_guarded<w>(nu), acc);
    });
    if (write_out && l < NW)
      const_cast<double*>(ws)[static_cast<size_t>(env) * D::WS + D::W_NU + l] = acc;
  }
}

}  // namespace osc
