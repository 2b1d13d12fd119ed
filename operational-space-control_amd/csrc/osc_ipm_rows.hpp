// osc_ipm_rows.hpp -- the reduced QP's inequality rows G y <= h as one 16-lane row of the interior
// point sees them: the products G v and G'w and the contact blocks of G'DG (which rows a lane
// holds, and their bounds, is set up by ipm_block itself: osc_ipm.hpp).  G is never stored: row
// r is a torque bound +-y_q (r < 2 NU) or one of a contact's six rows (four friction-pyramid
// sides, -fz <= -lb, fz <= ub), recomputed from r.
// Part of osc_ipm.hpp.
#pragma once
#include "osc_internal.hpp"

namespace osc {

// What a lane of an env's row needs to address the rows and the variables: its index l in the row
// (inequality rows r = l + 16 t), its variable slots j = l + 16 s -- j0, and j1 where it exists
// (v1; jj1 = a valid stand-in otherwise) -- and, for a slot that is a contact force, its contact
// jk (-1: a torque) and component jc; mu_f: the friction coefficient of the pyramid rows.
struct RowLane {
  int l, j0, j1, jj1;
  bool v1;
  int jk0, jc0, jk1, jc1;
  double mu_f;
};

// (G v)_r for all row slots at once, branch-free, every read issued first (one-wave variant):
// torque rows read y_q, contact rows read their contact's three force entries.
template <class D>
__device__ __forceinline__ void Gv_all(const RowLane& L, const bool (&act)[D::NRL],
                                       const double* v, double (&out)[D::NRL]) {
  constexpr int NU = D::NU, MI = D::MI, NRL = D::NRL;
  const int l = L.l;
  const double mu_f = L.mu_f;
  double uq[NRL], f0[NRL], f1[NRL], f2[NRL];
#pragma unroll
  for (int t = 0; t < NRL; ++t) {
    const int r = l + kRow * t;
    const int q = (r < 2 * NU) ? (r >> 1) : 0;
    const int k = (r >= 2 * NU && r < MI) ? (r - 2 * NU) / 6 : 0;
    uq[t] = v[q];
    f0[t] = v[NU + 3 * k];
    f1[t] = v[NU + 3 * k + 1];
    f2[t] = v[NU + 3 * k + 2];
  }
#pragma unroll
  for (int t = 0; t < NRL; ++t) {
    const int r = l + kRow * t;
    const int rt = (r - 2 * NU) % 6;
    const double sx = (rt & 1) ? -1.0 : 1.0, sy = (rt >= 2) ? -1.0 : 1.0;
    double pyr = sx * f0[t] + sy * f1[t] - mu_f * f2[t];
    in_vgpr(pyr);   // (computed on every lane, not behind a branch on the row's kind)
    double crow = (rt < 4) ? pyr : ((rt == 4) ? -f2[t] : f2[t]);
    in_vgpr(crow);
    double trow = (r & 1) ? -uq[t] : uq[t];
    in_vgpr(trow);   // (or its read sinks behind a branch on act[t], and is waited for alone)
    out[t] = !act[t] ? 0.0 : ((r < 2 * NU) ? trow : crow);
  }
}
// (G v)_r for row slot t
template <class D>
__device__ __forceinline__ double Gv(const RowLane& L, const bool (&act)[D::NRL], const double* v,
                                     int t) {
  constexpr int NU = D::NU;
  const double mu_f = L.mu_f;
  if (!act[t]) return 0.0;
  const int r = L.l + kRow * t;
  if (r < 2 * NU) {
    const double uq = v[r >> 1];
    return (r & 1) ? -uq : uq;
  }
  const int k = (r - 2 * NU) / 6, rt = (r - 2 * NU) % 6;
  const int z0 = NU + 3 * k;
  if (rt < 4) {
    const double sx = (rt & 1) ? -1.0 : 1.0, sy = (rt >= 2) ? -1.0 : 1.0;
    return sx * v[z0] + sy * v[z0 + 1] - mu_f * v[z0 + 2];
  }
  return (rt == 4) ? -v[z0 + 2] : v[z0 + 2];
}

// (G' w)_j for both variable slots of this lane, w row-space in LDS (inactive rows hold 0).
// All reads are issued before the arithmetic (one wait, not one per torque row); the contact
// part is branch-free: each lane reads its contact's six rows (16-byte pairs) and keeps the
// combination of its component jc.
template <class D, bool SMALL>
__device__ __forceinline__ double contact_term(double mu_f, const double* w, int jk, int jc) {
  constexpr int NU = D::NU;
  const double* wk = w + 2 * NU + 6 * (jk >= 0 ? jk : 0);
  const double2 a = *reinterpret_cast<const double2*>(wk);
  const double2 b = *reinterpret_cast<const double2*>(wk + 2);
  const double2 c = *reinterpret_cast<const double2*>(wk + 4);
  if constexpr (SMALL) {
    // one chain for the three components, its signs picked per lane: the same operations in
    // the same order as v0 / v1 / v2 below (x - y is x + (-y), bit for bit), less than half of
    // them issued, and no branch on the lane's component
    const double t1 = (jc == 0) ? -a.y : a.y;
    const double t2 = (jc == 1) ? -b.x : b.x;
    const double t3 = (jc == 2) ? b.y : -b.y;
    double q = ((a.x + t1) + t2) + t3;
    double fz = fma(-mu_f, q, -c.x) + c.y;
    in_vgpr(q);
    in_vgpr(fz);
    const double v = (jc == 2) ? fz : q;
    return jk >= 0 ? v : 0.0;
  }
  const double v0 = a.x - a.y + b.x - b.y;
  const double v1 = a.x + a.y - b.x - b.y;
  const double v2 = -mu_f * (a.x + a.y + b.x + b.y) - c.x + c.y;
  const double v = (jc == 0) ? v0 : ((jc == 1) ? v1 : v2);
  return jk >= 0 ? v : 0.0;
}
template <class D, bool SMALL>
__device__ __forceinline__ void GTw2(const RowLane& L, const double* w, double& r0, double& r1) {
  constexpr int NU = D::NU;
  const int j0 = L.j0;
  // torque rows +-e_q: lane j0 < NU picks up w[2 j0] - w[2 j0 + 1]; slot j1 >= 16 > NU is a
  // contact variable
  const double2 p = *reinterpret_cast<const double2*>(w + 2 * (j0 < NU ? j0 : 0));
  const double k0 = contact_term<D, SMALL>(L.mu_f, w, L.jk0, L.jc0),
               k1 = contact_term<D, SMALL>(L.mu_f, w, L.jk1, L.jc1);
  r0 = (j0 < NU ? p.x - p.y : 0.0) + k0;
  r1 = k1;
}

// contact block column (B[0..2][jc]) of var slot in contact jk, from D = lambda/s (sDr)
template <class D>
__device__ __forceinline__ void contact_col(double mu_f, const double* sDr, int jk, int jc,
                                            double& v0, double& v1_, double& v2) {
  constexpr int NU = D::NU;
  const double* dk = sDr + 2 * NU + 6 * jk;
  const double s4 = dk[0] + dk[1] + dk[2] + dk[3];
  const double sxy = dk[0] - dk[1] - dk[2] + dk[3];
  const double sx = dk[0] - dk[1] + dk[2] - dk[3];
  const double sy = dk[0] + dk[1] - dk[2] - dk[3];
  const double b00 = s4, b11 = s4, b01 = sxy, b02 = -mu_f * sx, b12 = -mu_f * sy,
               b22 = mu_f * mu_f * s4 + dk[4] + dk[5];
  v0 = (jc == 0) ? b00 : (jc == 1) ? b01 : b02;
  v1_ = (jc == 0) ? b01 : (jc == 1) ? b11 : b12;
  v2 = (jc == 0) ? b02 : (jc == 1) ? b12 : b22;
}

// G'DG's contact blocks into K's columns (c0 / c1), row by row (round 6): the rows of contact k
// are NU + 3k .. NU + 3k + 2, and the lanes whose column lies in contact k form a compile-time lane
// range of each slot -- so each row takes its entry (a, b or cc by the row's component) masked
// to that range, and rows no lane of a slot reaches are not touched.  (It was a select per row
// of all 12 contact rows against the lane's runtime contact index, behind a branch per slot.)
template <class D>
__device__ __forceinline__ void add_contact_blocks(const RowLane& L, const double* sDr,
                                                   double (&c0)[D::NY], double (&c1)[D::NY],
                                                   double& dg0, double& dg1) {
  constexpr int NU = D::NU, NC = D::NC;
  const int jk0 = L.jk0, jc0 = L.jc0, jk1 = L.jk1, jc1 = L.jc1;
  double a0, b0, e0, a1, b1, e1;
  contact_col<D>(L.mu_f, sDr, jk0 >= 0 ? jk0 : 0, jc0, a0, b0, e0);
  contact_col<D>(L.mu_f, sDr, jk1 >= 0 ? jk1 : 0, jc1, a1, b1, e1);
  dg0 += jk0 >= 0 ? ((jc0 == 0) ? a0 : (jc0 == 1) ? b0 : e0) : 0.0;
  dg1 += jk1 >= 0 ? ((jc1 == 0) ? a1 : (jc1 == 1) ? b1 : e1) : 0.0;
  static_for<0, NC>([&](auto Kc) __attribute__((always_inline)) {
    constexpr int k = decltype(Kc)::value, r0 = NU + 3 * k;
    constexpr unsigned m0 = r0 <= kRow - 1 ? lanes_from(r0, r0 + 2) : 0u;   // slot 0: lane = row
    constexpr unsigned m1 = lanes_from(r0 - kRow, r0 + 2 - kRow);           // slot 1: row - 16
    if constexpr (m0 != 0u) {
      const unsigned long long m = mask_here<rows_mask(m0)>();
      c0[r0] += keep_m(m, a0);
      c0[r0 + 1] += keep_m(m, b0);
      c0[r0 + 2] += keep_m(m, e0);
    }
    if constexpr (m1 != 0u) {
      const unsigned long long m = mask_here<rows_mask(m1)>();
      c1[r0] += keep_m(m, a1);
      c1[r0 + 1] += keep_m(m, b1);
      c1[r0 + 2] += keep_m(m, e1);
    }
  });
}

}  // namespace osc
