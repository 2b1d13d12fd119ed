// osc_backward_wv.hpp -- the w / v stage of the backward pass, shared by the two
// backward units (osc_backward.hip: dL/dT, dL/db; osc_backward_data.hip: dL/dM, dL/dC, dL/dJ and
// the row weights as well): the active set -> the projector P, K = P Hr P + (I - P), its LDL^T,
// w = P K^-1 P r with one refinement step through the factored form, and v = X_y w.  Four envs per
// wavefront, one 16-lane DPP row each; the layout and the linear algebra are the interior point's
// (osc_ipm_ldl.hpp).
#pragma once
#include "osc_internal.hpp"
#include "osc_ipm_ldl.hpp"

namespace osc {

constexpr int kBwRefine = 1;       // refinement steps (5e-6 -> 5e-9 on WaLTER)
constexpr double kBwActive = 1e-6; // torque row active: |y| above this x (1 + largest multiplier)
constexpr double kBwRank = 1e-12;  // a normal is dependent: remainder^2 below this x length^2

// LDS per env (doubles)
template <class D>
struct BwLayout {
  static constexpr int PU = even(D::NU);
  static constexpr int I_P = 0;                        // torque factors | 6 per contact (upper)
  static constexpr int I_V = I_P + PU + 6 * D::NC;     // a y-space vector
  static constexpr int I_H = I_V + 2 * kRow;           // a dv-space vector
  static constexpr int I_DINV = I_H + even(D::NV);     // 1 / D of the factorisation
  static constexpr int IL = I_DINV + 2 * kRow;
};

// One column slot of a lane: its column j of K lies in the block of columns k[0..2] (a torque: j
// three times) with P's entries pc[t] = P[k[t]][j]; dd[t] = (I - P)[a + t][j].
struct BwCol {
  int a;
  int k[3];
  double pc[3], dd[3];
};

template <class D>
__device__ __forceinline__ BwCol bw_col(int j, const double* sP) {
  constexpr int NU = D::NU, PU = BwLayout<D>::PU;
  BwCol c;
  const bool tq = j < NU;
  const int ct = tq ? 0 : (j - NU) / 3, m = tq ? 0 : (j - NU) - 3 * ct;
  c.a = tq ? j : NU + 3 * ct;
  const double* pp = sP + PU + 6 * ct;
  const double pt = sP[tq ? j : 0];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int lo = m < t ? m : t, hi = m < t ? t : m;
    const double pv = pp[lo * (5 - lo) / 2 + hi];
    c.pc[t] = tq ? (t == 0 ? pt : 0.0) : pv;
    c.k[t] = tq ? j : c.a + t;
    c.dd[t] = (m == t ? 1.0 : 0.0) - c.pc[t];
  }
  return c;
}

// One env's w / v stage, run by the 16 lanes of its row (l: the lane in the row).  B: the env's
// BwLayout block of LDS; wenv, yy, gx, mask: the env's workspace block, duals, dL/dx and contact
// mask.  On return v = X_y w is whole in every lane and (w0, w1) are the lane's entries of w
// (columns l and l + 16; the second a mirror of column NY - 1 past NY).
// EXT = true (osc_backward_env.hip, the per-env parameter gradients): the pyramid normals take
// ext->mu, the env's friction, instead of the model's, and ext->r0 / r1 return the lane's entries of
// r~ = (g_u, g_z) + X_y' g_dv BEFORE the projection.  EXT = false compiles none of it.
struct BwExt {
  double mu, r0, r1;
};
template <class D, bool EXT = false>
__device__ __forceinline__ void bw_solve_wv(const DevParams* __restrict__ P, int l, double* B,
                                            const double* __restrict__ wenv,
                                            const double* __restrict__ yy,
                                            const double* __restrict__ gx,
                                            const double* __restrict__ mask,
                                            double (&v)[D::NV], double& w0, double& w1,
                                            BwExt* ext = nullptr) {
  constexpr int NV = D::NV, NU = D::NU, NC = D::NC, NY = D::NY, NY1P = D::NY1P;
  constexpr int Y_PYR = NV, Y_U = NV + 4 * NC + NV, Y_Z = Y_U + NU;
  using LY = BwLayout<D>;
  double *sP = B + LY::I_P, *sV = B + LY::I_V, *sH = B + LY::I_H, *sDinv = B + LY::I_DINV;

  // ---- the active set -> P: lane q < NU its torque's factor, lane c < NC contact c's block ----
  {
    const int cq = l < NC ? l : NC - 1;
    const bool on = mask[cq] != 0.0;
    double py[4], yz[3];
#pragma unroll
    for (int r = 0; r < 4; ++r) py[r] = yy[Y_PYR + 4 * cq + r];
#pragma unroll
    for (int c = 0; c < 3; ++c) yz[c] = yy[Y_Z + 3 * cq + c];
    const double yu = yy[Y_U + (l < NU ? l : NU - 1)];
    double mc = fmax(fmax(fabs(py[0]), fabs(py[1])), fmax(fabs(py[2]), fabs(py[3])));
    mc = fmax(mc, fmax(fabs(yz[0]), fmax(fabs(yz[1]), fabs(yz[2]))));
    const double big = row_max(fmax(l < NU ? fabs(yu) : 0.0, (l < NC && on) ? mc : 0.0));
    if (l < NU) sP[l] = fabs(yu) > kBwActive * (1.0 + big) ? 0.0 : 1.0;

    // Gram-Schmidt of the active normals, each orthogonalised twice against the basis so far
    double q0x = 0.0, q0y = 0.0, q0z = 0.0, q1x = 0.0, q1y = 0.0, q1z = 0.0, q2x = 0.0, q2y = 0.0,
           q2z = 0.0;
    int nq = 0;
    auto add = [&](double ax, double ay, double az, bool act) {
      double ux = ax, uy = ay, uz = az;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        double d = q0x * ux + q0y * uy + q0z * uz;
        ux -= d * q0x, uy -= d * q0y, uz -= d * q0z;
        d = q1x * ux + q1y * uy + q1z * uz;
        ux -= d * q1x, uy -= d * q1y, uz -= d * q1z;
        d = q2x * ux + q2y * uy + q2z * uz;
        ux -= d * q2x, uy -= d * q2y, uz -= d * q2z;
      }
      const double nn = ux * ux + uy * uy + uz * uz;
      const bool take = act && nq < 3 && nn > kBwRank * (ax * ax + ay * ay + az * az);
      const double inv = 1.0 / sqrt(take ? nn : 1.0);
      ux *= inv, uy *= inv, uz *= inv;
      const bool t0 = take && nq == 0, t1 = take && nq == 1, t2 = take && nq == 2;
      q0x = t0 ? ux : q0x, q0y = t0 ? uy : q0y, q0z = t0 ? uz : q0z;
      q1x = t1 ? ux : q1x, q1y = t1 ? uy : q1y, q1z = t1 ? uz : q1z;
      q2x = t2 ? ux : q2x, q2y = t2 ? uy : q2y, q2z = t2 ? uz : q2z;
      nq += take ? 1 : 0;
    };
    double mu = P->mu;
    if constexpr (EXT) mu = ext->mu;
    add(1.0, 1.0, -mu, py[0] > 0.0);     // the pyramid rows in Aineq's order
    add(-1.0, 1.0, -mu, py[1] > 0.0);
    add(1.0, -1.0, -mu, py[2] > 0.0);
    add(-1.0, -1.0, -mu, py[3] > 0.0);
    add(1.0, 0.0, 0.0, yz[0] != 0.0);    // the box rows of fx, fy, fz
    add(0.0, 1.0, 0.0, yz[1] != 0.0);
    add(0.0, 0.0, 1.0, yz[2] != 0.0);
    const double keep = on ? 1.0 : 0.0;  // mask == 0: all three forces fixed
    if (l < NC) {
      double* pp = sP + LY::PU + 6 * l;
      pp[0] = keep * (1.0 - q0x * q0x - q1x * q1x - q2x * q2x);
      pp[1] = keep * (-q0x * q0y - q1x * q1y - q2x * q2y);
      pp[2] = keep * (-q0x * q0z - q1x * q1z - q2x * q2z);
      pp[3] = keep * (1.0 - q0y * q0y - q1y * q1y - q2y * q2y);
      pp[4] = keep * (-q0y * q0z - q1y * q1z - q2y * q2z);
      pp[5] = keep * (1.0 - q0z * q0z - q1z * q1z - q2z * q2z);
    }
  }
  wave_sync();

  // variable slots of this lane: j = l + 16 s (past NY: a mirror of column NY - 1, ldl_rows)
  const int j0 = l, j1 = l + kRow;
  const bool has1 = j1 < NY;
  const int jj1 = has1 ? j1 : NY - 1;
  const BwCol C0 = bw_col<D>(j0, sP), C1 = bw_col<D>(jj1, sP);

  // ---- K = P Hr P + (I - P): the column combinations (Hr P) straight from the workspace ... ----
  const double* hr = wenv + D::W_HR;
  double c0[NY], c1[NY];
#pragma unroll
  for (int i = 0; i < NY; ++i) {
    c0[i] = fma(C0.pc[2], hr[hr_off<D>(i, C0.k[2])],
                fma(C0.pc[1], hr[hr_off<D>(i, C0.k[1])], C0.pc[0] * hr[hr_off<D>(i, C0.k[0])]));
    c1[i] = fma(C1.pc[2], hr[hr_off<D>(i, C1.k[2])],
                fma(C1.pc[1], hr[hr_off<D>(i, C1.k[1])], C1.pc[0] * hr[hr_off<D>(i, C1.k[0])]));
  }
  // ... then the row combinations, inside each lane's registers
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const double p = sP[i];
    c0[i] *= p;
    c1[i] *= p;
  }
  static_for<0, NC>([&](auto cc) {
    constexpr int a = NU + 3 * decltype(cc)::value;
    const double* pp = sP + LY::PU + 6 * decltype(cc)::value;
    const double p00 = pp[0], p01 = pp[1], p02 = pp[2], p11 = pp[3], p12 = pp[4], p22 = pp[5];
    const double x0 = c0[a], x1 = c0[a + 1], x2 = c0[a + 2];
    c0[a] = fma(p02, x2, fma(p01, x1, p00 * x0));
    c0[a + 1] = fma(p12, x2, fma(p11, x1, p01 * x0));
    c0[a + 2] = fma(p22, x2, fma(p12, x1, p02 * x0));
    const double z0 = c1[a], z1 = c1[a + 1], z2 = c1[a + 2];
    c1[a] = fma(p02, z2, fma(p01, z1, p00 * z0));
    c1[a + 1] = fma(p12, z2, fma(p11, z1, p01 * z0));
    c1[a + 2] = fma(p22, z2, fma(p12, z1, p02 * z0));
  });
  double dg0 = 0.0, dg1 = 0.0;   // K's diagonal entries of the lane's columns
#pragma unroll
  for (int i = 0; i < NY; ++i) {
    const int t0 = i - C0.a, t1 = i - C1.a;
    c0[i] += t0 == 0 ? C0.dd[0] : t0 == 1 ? C0.dd[1] : t0 == 2 ? C0.dd[2] : 0.0;
    c1[i] += t1 == 0 ? C1.dd[0] : t1 == 1 ? C1.dd[1] : t1 == 2 ? C1.dd[2] : 0.0;
    dg0 = i == j0 ? c0[i] : dg0;
    dg1 = i == jj1 ? c1[i] : dg1;
  }
  wave_sync();
  double dinv0, dinv1;
  ldl_rows<NY, true>(c0, c1, sDinv, l, dinv0, dinv1, 1e-13 * dg0, 1e-13 * dg1, 0.0);
  wave_sync();

  // a <- P a for a y-space vector held one entry per column slot
  auto apply_p = [&](double& a0, double& a1) {
    sV[j0] = a0;
    if (has1) sV[j1] = a1;
    wave_sync();
    a0 = fma(C0.pc[2], sV[C0.k[2]], fma(C0.pc[1], sV[C0.k[1]], C0.pc[0] * sV[C0.k[0]]));
    a1 = fma(C1.pc[2], sV[C1.k[2]], fma(C1.pc[1], sV[C1.k[1]], C1.pc[0] * sV[C1.k[0]]));
    wave_sync();
  };

  // ---- r = P ((g_u, g_z) + X_y' g_dv) ----
  const double* X = wenv + D::W_X;
  double r0 = gx[NV + j0], r1 = gx[NV + jj1];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double g = gx[i];
    r0 = fma(X[i * NY1P + j0], g, r0);
    r1 = fma(X[i * NY1P + jj1], g, r1);
  }
  if constexpr (EXT) ext->r0 = r0, ext->r1 = r1;
  apply_p(r0, r1);

  // ---- w = P K^-1 r, refined through the factored form ----
  w0 = r0, w1 = r1;
  ldl_solve_rows<NY>(c0, c1, dinv0, dinv1, w0, w1, l);
  apply_p(w0, w1);
  auto x_times_w = [&]() {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      v[i] = row_sum(fma(X[i * NY1P + j0], w0, has1 ? X[i * NY1P + jj1] * w1 : 0.0));
  };
  const double wu = 2.0 * (P->w_torque + P->w_reg), wz = 2.0 * P->w_reg;
  const double* Hd = wenv + D::W_HD;
#pragma unroll 1
  for (int it = 0; it < kBwRefine; ++it) {
    x_times_w();
#pragma unroll
    for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) {   // H_dv v, a row per lane
      const int i = l + kRow * t, ii = i < NV ? i : NV - 1;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NV; ++k) acc = fma(Hd[ii * NV + k], v[k], acc);
      if (i < NV) sH[i] = acc;
    }
    wave_sync();
    double t0 = (j0 < NU ? wu : wz) * w0, t1 = (jj1 < NU ? wu : wz) * w1;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const double h = sH[i];
      t0 = fma(X[i * NY1P + j0], h, t0);
      t1 = fma(X[i * NY1P + jj1], h, t1);
    }
    wave_sync();
    apply_p(t0, t1);
    double d0 = r0 - t0, d1 = r1 - t1;
    ldl_solve_rows<NY>(c0, c1, dinv0, dinv1, d0, d1, l);
    apply_p(d0, d1);
    w0 += d0;
    w1 += d1;
  }
  x_times_w();
}

}  // namespace osc
