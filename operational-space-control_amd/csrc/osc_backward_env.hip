// osc_backward_env.hip -- backward pass of the batched solve with per-env parameters (C-ABI in
// include/osc_backward_env.h, osc_batch_solve_backward_env): the six outputs of
// osc_backward_data.hip with the env's own friction and task weights read where the model's were,
// and the gradients of the seven per-env fields.
//
// Per env, after the w / v stage (osc_backward_wv.hpp with EXT: the env's mu in the pyramid
// normals, r~ kept before the projection):
//   rho = X_y'(H_dv v) + D w - r~          the refinement step's product, once more, unprojected
//   torque row j (lane j < NU): -rho_j to u_ub or u_lb by the multiplier's sign, if active
//   contact c (lane c < NC): the Gram-Schmidt of its active rows again, this time keeping the
//     triangular factor R (G = R Q, Q's rows orthonormal) and which rows were kept, then
//     R' dnu = Q rho_c by back substitution; mu, fz_lb, fz_ub from dnu, nu, fz*, w_fz and the mask
//   the per-env scalars: lane 0 adds the contacts' terms in order
// then osc_backward_data.hip's stages line by line (the solve with M, the pass over J, the matrix
// outputs; W_r from the env's weights), and the site weights' gradients as ordered three-row sums of
// the row-weight gradient.  The two halves are compile-time switches of one body -- DATA: the solve
// with M, the pass over J, the six data outputs and the site weights' gradients; PAR: rho and the
// gradients of mu and the bounds -- and the entry launches the variant that holds what the call
// asks for, so that a call without parameter gradients runs code of osc_backward_data.hip's size
// and a call for mu / bound gradients alone skips the solve with M and the pass over J.
//
// Layout: FOUR envs per wavefront, one 16-lane row each, nothing crossing a row, no atomics -- as
// the two other backward units.  ENV = true: the per-env arrays travel by value and are read where
// they are used; ENV = false compiles none of those reads.
#include "osc_backward_env.h"

#include "osc_backward_wv.hpp"

namespace osc {

// the gradients' device arrays (osc_env_grads), by value
struct EnvGradPtrs {
  double *mu, *u_lb, *u_ub, *fz_lb, *fz_ub, *w_pos, *w_rot;
};

// LDS per env (doubles): the w / v stage's block, osc_backward_data.hip's, then this unit's
template <class D>
struct BwEnvLayout {
  static constexpr int I_VV = BwLayout<D>::IL;               // v
  static constexpr int I_DN = I_VV + even(D::NV);            // dnu
  static constexpr int I_DV = I_DN + even(D::NV);            // dv*
  static constexpr int I_NU = I_DV + even(D::NV);            // nu
  static constexpr int I_A = I_NU + even(D::NV);             // -2 W_r Jv_r per task row
  static constexpr int I_B = I_A + even(D::S);               // -2 W_r e_r per task row
  static constexpr int I_C = I_B + even(D::S);               // -z*_j per contact row
  static constexpr int I_D = I_C + even(D::NZ);              // w_z,j per contact row
  static constexpr int I_RHO = I_D + even(D::NZ);            // rho, a y-space vector
  static constexpr int I_CT = I_RHO + 2 * kRow;              // (dmu, dfz_lb, dfz_ub) per contact
  static constexpr int I_WR = I_CT + even(3 * D::NC);        // dL/dw_row per task row
  static constexpr int IL = I_WR + even(D::S);
};

// One wavefront per SIMD, the AGPRs as spill space, as osc_backward_data_kernel.
template <class D, bool ENV, bool DATA, bool PAR>
__global__ __launch_bounds__(kWave, 1) void osc_backward_env_kernel(
    const DevParams* __restrict__ P, int nenv, const double* __restrict__ gM,
    const double* __restrict__ gJ, const double* __restrict__ gbias,
    const double* __restrict__ gtgt, const double* __restrict__ gmask,
    const double* __restrict__ gxs, const double* __restrict__ gy,
    const int32_t* __restrict__ gstatus, const double* __restrict__ ggx,
    const double* __restrict__ ws, double* __restrict__ oM, double* __restrict__ oC,
    double* __restrict__ oJ, double* __restrict__ oW, double* __restrict__ gT,
    double* __restrict__ gb, EnvPtrs EP, EnvGradPtrs G) {
  constexpr int NV = D::NV, NU = D::NU, NC = D::NC, NS = D::NS, NY = D::NY, NZ = D::NZ,
                NX = D::NX, S = D::S, NY1P = D::NY1P;
  constexpr int NROW = NV + 4 * NC + NX, R0 = 3 * NS - NZ;   // R0: the first contact row of J
  constexpr int Y_PYR = NV, Y_U = NV + 4 * NC + NV, Y_Z = Y_U + NU;
  constexpr int NT = (NV + kRow - 1) / kRow;                 // dv-space slots per lane
  constexpr int NM = NV > kRow ? NV : kRow + 1;              // columns of M's factorisation
  using LY = BwLayout<D>;
  using LD = BwEnvLayout<D>;
  static_assert(!D::WH, "no wheel rows");
  static_assert(NV % 2 == 0 && NT <= 2, "16-byte output pairs; two dv-space slots per lane");
  __shared__ double smem[kEnvPerWave * LD::IL];
  const int lane = static_cast<int>(threadIdx.x), l = lane & (kRow - 1);
  const long long env = static_cast<long long>(blockIdx.x) * kEnvPerWave + (lane >> 4);
  const bool valid = env < nenv;
  const size_t e = static_cast<size_t>(valid ? env : nenv - 1);   // (loads stay in bounds)
  const bool ok = valid && gstatus[e] == OSC_SOLVE_OK;
  double* B = smem + (lane >> 4) * LD::IL;
  double *sP = B + LY::I_P, *sV = B + LY::I_V, *sH = B + LY::I_H, *sDinv = B + LY::I_DINV;
  double *sVv = B + LD::I_VV, *sDn = B + LD::I_DN, *sDv = B + LD::I_DV,
         *sNu = B + LD::I_NU, *sA = B + LD::I_A, *sB = B + LD::I_B, *sC = B + LD::I_C,
         *sD = B + LD::I_D, *sR = B + LD::I_RHO, *sCt = B + LD::I_CT, *sWr = B + LD::I_WR;
  const double* wenv = ws + e * D::WS;
  const double* yy = gy + e * NROW;
  const double* gx = ggx + e * NX;
  const double* mask = gmask + e * NC;
  static_assert(DATA || PAR, "something to compute");

  // the model's value of each per-env quantity, or (ENV) this env's: read where it is used
  auto env_mu = [&]() -> double {
    if constexpr (ENV) return EP.mu ? EP.mu[e] : P->mu;
    return P->mu;
  };
  auto env_ulb = [&](int q) -> double {
    if constexpr (ENV) return EP.u_lb ? EP.u_lb[e * NU + q] : P->u_lb[q];
    return P->u_lb[q];
  };
  auto env_uub = [&](int q) -> double {
    if constexpr (ENV) return EP.u_ub ? EP.u_ub[e * NU + q] : P->u_ub[q];
    return P->u_ub[q];
  };
  auto env_zlb = [&]() -> double {
    if constexpr (ENV) return EP.fz_lb ? EP.fz_lb[e] : P->z_lb[2];
    return P->z_lb[2];
  };
  auto env_wrow = [&](int r) -> double {   // task row r: site (r mod 3 ns) / 3 of [w_pos | w_rot]
    if constexpr (ENV) {
      const double* a = r < 3 * NS ? EP.w_pos : EP.w_rot;
      return a ? a[e * NS + (r < 3 * NS ? r : r - 3 * NS) / 3] : P->w_row[r];
    }
    return P->w_row[r];
  };

  // ---- the active set, K and its LDL^T, w and v = X_y w (osc_backward_wv.hpp) ----
  double v[NV], w0, w1;   // v whole in every lane of the row
  BwExt ext;
  ext.mu = env_mu();
  bw_solve_wv<D, true>(P, l, B, wenv, yy, gx, mask, v, w0, w1, &ext);
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

  // ---- the parameter gradients of mu and the bounds ----
  if constexpr (PAR) {
    // rho = X_y'(H_dv v) + D w - r~: the adjoint multipliers of the active rows, stacked
    {
      const int j0 = l, j1 = l + kRow, jj1 = j1 < NY ? j1 : NY - 1;
      const double wu = 2.0 * (P->w_torque + P->w_reg), wz = 2.0 * P->w_reg;
      const double* X = wenv + D::W_X;
      double t0 = (j0 < NU ? wu : wz) * w0, t1 = (jj1 < NU ? wu : wz) * w1;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const double h = sH[i];
        t0 = fma(X[i * NY1P + j0], h, t0);
        t1 = fma(X[i * NY1P + jj1], h, t1);
      }
      sR[j0] = t0 - ext.r0;
      if (j1 < NY) sR[j1] = t1 - ext.r1;
    }
    wave_sync();

    // torque rows: lane q < NU; the row's activity is the projector's factor (0 = active)
    {
      const int q = l < NU ? l : NU - 1;
      const bool act = ok && sP[q] == 0.0;
      const bool up = yy[Y_U + q] > 0.0;
      const double thr = P->inf_thresh, g = -sR[q];
      const bool has_ub = fabs(env_uub(q)) < thr, has_lb = fabs(env_ulb(q)) < thr;
      if (valid && l < NU) {
        if (G.u_ub) G.u_ub[e * NU + l] = (act && up && has_ub) ? g : 0.0;
        if (G.u_lb) G.u_lb[e * NU + l] = (act && !up && has_lb) ? g : 0.0;
      }
    }

    // contacts: lane c < NC
    {
      const int cq = l < NC ? l : NC - 1;
      const double m = mask[cq];
      const bool on = m != 0.0;
      double py[4], yz[3];
#pragma unroll
      for (int r = 0; r < 4; ++r) py[r] = yy[Y_PYR + 4 * cq + r];
#pragma unroll
      for (int c = 0; c < 3; ++c) yz[c] = yy[Y_Z + 3 * cq + c];
      // the w / v stage's Gram-Schmidt, keeping G = R Q: row k of the kept rows is
      // sum_j<k R[k][j] q_j + R[k][k] q_k; kd_k its kind (0 a pyramid row, 1 the fz box row, 2 none
      // or another) and pn_k a pyramid row's multiplier
      double q0x = 0.0, q0y = 0.0, q0z = 0.0, q1x = 0.0, q1y = 0.0, q1z = 0.0, q2x = 0.0, q2y = 0.0,
             q2z = 0.0;
      double R00 = 1.0, R10 = 0.0, R11 = 1.0, R20 = 0.0, R21 = 0.0, R22 = 1.0;
      double pn0 = 0.0, pn1 = 0.0, pn2 = 0.0;
      int kd0 = 2, kd1 = 2, kd2 = 2, nq = 0;
      auto add = [&](double ax, double ay, double az, bool act, int kind, double mult) {
        double ux = ax, uy = ay, uz = az, c0 = 0.0, c1 = 0.0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          double d = q0x * ux + q0y * uy + q0z * uz;
          ux -= d * q0x, uy -= d * q0y, uz -= d * q0z;
          c0 += d;
          d = q1x * ux + q1y * uy + q1z * uz;
          ux -= d * q1x, uy -= d * q1y, uz -= d * q1z;
          c1 += d;
          d = q2x * ux + q2y * uy + q2z * uz;
          ux -= d * q2x, uy -= d * q2y, uz -= d * q2z;
        }
        const double nn = ux * ux + uy * uy + uz * uz;
        const bool take = act && nq < 3 && nn > kBwRank * (ax * ax + ay * ay + az * az);
        const double len = sqrt(take ? nn : 1.0), inv = 1.0 / len;
        ux *= inv, uy *= inv, uz *= inv;
        const bool t0 = take && nq == 0, t1 = take && nq == 1, t2 = take && nq == 2;
        q0x = t0 ? ux : q0x, q0y = t0 ? uy : q0y, q0z = t0 ? uz : q0z;
        q1x = t1 ? ux : q1x, q1y = t1 ? uy : q1y, q1z = t1 ? uz : q1z;
        q2x = t2 ? ux : q2x, q2y = t2 ? uy : q2y, q2z = t2 ? uz : q2z;
        R00 = t0 ? len : R00, kd0 = t0 ? kind : kd0, pn0 = t0 ? mult : pn0;
        R10 = t1 ? c0 : R10, R11 = t1 ? len : R11, kd1 = t1 ? kind : kd1, pn1 = t1 ? mult : pn1;
        R20 = t2 ? c0 : R20, R21 = t2 ? c1 : R21, R22 = t2 ? len : R22, kd2 = t2 ? kind : kd2,
        pn2 = t2 ? mult : pn2;
        nq += take ? 1 : 0;
      };
      const double mu = ext.mu;
      add(1.0, 1.0, -mu, py[0] > 0.0, 0, py[0]);    // the pyramid rows in Aineq's order
      add(-1.0, 1.0, -mu, py[1] > 0.0, 0, py[1]);
      add(1.0, -1.0, -mu, py[2] > 0.0, 0, py[2]);
      add(-1.0, -1.0, -mu, py[3] > 0.0, 0, py[3]);
      add(1.0, 0.0, 0.0, yz[0] != 0.0, 2, 0.0);     // the box rows of fx, fy, fz
      add(0.0, 1.0, 0.0, yz[1] != 0.0, 2, 0.0);
      add(0.0, 0.0, 1.0, yz[2] != 0.0, 1, 0.0);
      // R' dnu = Q rho_c (an empty slot: q = 0, R[k][k] = 1, so dnu = 0)
      const double rx = sR[NU + 3 * cq], ry = sR[NU + 3 * cq + 1], rz = sR[NU + 3 * cq + 2];
      const double b0 = q0x * rx + q0y * ry + q0z * rz, b1 = q1x * rx + q1y * ry + q1z * rz,
                   b2 = q2x * rx + q2y * ry + q2z * rz;
      const double d2 = b2 / R22;
      const double d1 = (b1 - d2 * R21) / R11;
      const double d0 = (b0 - d1 * R10 - d2 * R20) / R00;
      const double fzs = xs[NV + NU + 3 * cq + 2], wfz = sV[NU + 3 * cq + 2];
      auto pyr_term = [&](int kd, double nu, double dn) -> double {   // -dnu_r fz* + nu_r w_fz
        return kd == 0 ? fma(nu, wfz, -dn * fzs) : 0.0;
      };
      const double dmu = pyr_term(kd0, pn0, d0) + pyr_term(kd1, pn1, d1) + pyr_term(kd2, pn2, d2);
      const double dfz = kd0 == 1 ? d0 : kd1 == 1 ? d1 : kd2 == 1 ? d2 : 0.0;
      const double gfz = -dfz * m;
      // (the left derivative at the pyramid's apex: an active lower row at fz_lb mask = 0 gives 0)
      const bool lo = yz[2] < 0.0 && env_zlb() * m != 0.0;
      if (l < NC) {
        sCt[3 * l] = on ? dmu : 0.0;
        sCt[3 * l + 1] = (on && lo) ? gfz : 0.0;
        sCt[3 * l + 2] = (on && yz[2] > 0.0) ? gfz : 0.0;
      }
    }
    wave_sync();
    if (valid && l == 0) {   // the env's sums over its contacts, in order
      double smu = 0.0, slb = 0.0, sub = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        smu += sCt[3 * c];
        slb += sCt[3 * c + 1];
        sub += sCt[3 * c + 2];
      }
      if (G.mu) G.mu[e] = ok ? smu : 0.0;
      if (G.fz_lb) G.fz_lb[e] = ok ? slb : 0.0;
      if (G.fz_ub) G.fz_ub[e] = ok ? sub : 0.0;
    }
  }
  if constexpr (!DATA) return;

  // ---- dnu = M^-1 (H_dv v - g_dv): osc_backward_data.hip's solve ----
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
    const double wr = env_wrow(ss);
    const double er = acd + bb[ss] - tt[ti];
    const double q = ok ? 2.0 * wr * acc : 0.0;   // a failed env: all-zero gradients
    const double gw = ok ? -2.0 * acc * er : 0.0;
    if (s < S) {
      sA[s] = -2.0 * wr * acc;
      sB[s] = -2.0 * wr * er;
      sWr[s] = gw;
    }
    if (valid && s < S) {
      if (gb) gb[e * S + s] = -q;
      if (gT) gT[e * S + ti] = q;
      if (oW) oW[e * S + s] = gw;
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

  // ---- the site weights: the ordered sums of their three rows ----
#pragma unroll
  for (int t = 0; t < (NS + kRow - 1) / kRow; ++t) {
    const int s = l + kRow * t;
    if (valid && s < NS) {
      if (G.w_pos) G.w_pos[e * NS + s] = (sWr[3 * s] + sWr[3 * s + 1]) + sWr[3 * s + 2];
      if (G.w_rot)
        G.w_rot[e * NS + s] =
            (sWr[3 * NS + 3 * s] + sWr[3 * NS + 3 * s + 1]) + sWr[3 * NS + 3 * s + 2];
    }
  }

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

struct BwEnvArgs {
  const double *M, *J, *b, *T, *mask, *x, *y, *gx, *ws;
  const int32_t* status;
  double *oM, *oC, *oJ, *oW, *gT, *gb;
  EnvPtrs ep;
  EnvGradPtrs g;
};

template <class D, bool ENV, bool DATA, bool PAR>
int launch_variant(const osc_model* model, int32_t nenv, const BwEnvArgs& a, hipStream_t s) {
  const unsigned nblk = static_cast<unsigned>((static_cast<long long>(nenv) + kEnvPerWave - 1) /
                                              kEnvPerWave);
  hipLaunchKernelGGL((osc_backward_env_kernel<D, ENV, DATA, PAR>), dim3(nblk), dim3(kWave), 0, s,
                     model->dparams, nenv, a.M, a.J, a.b, a.T, a.mask, a.x, a.y, a.status, a.gx,
                     a.ws, a.oM, a.oC, a.oJ, a.oW, a.gT, a.gb, a.ep, a.g);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

// data: a data output or a site-weight gradient is asked for (the weights' need the pass over J);
// par: a gradient of mu or of a bound
template <class D, bool ENV>
int launch_backward_env(const osc_model* model, int32_t nenv, const BwEnvArgs& a, bool data,
                        bool par, hipStream_t s) {
  if (data && par) return launch_variant<D, ENV, true, true>(model, nenv, a, s);
  return data ? launch_variant<D, ENV, true, false>(model, nenv, a, s)
              : launch_variant<D, ENV, false, true>(model, nenv, a, s);
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace
}  // namespace osc

extern "C" int osc_batch_solve_backward_env(
    const osc_model* model, int32_t nenv, const double* M, const double* J, const double* b,
    const double* T, const double* contact_mask, const osc_env_params* env_params,
    const double* x, const double* y, const int32_t* status, const double* grad_x, double* grad_M,
    double* grad_C, double* grad_J, double* grad_wrow, double* grad_T, double* grad_b,
    const osc_env_grads* grads, const void* workspace, size_t workspace_bytes, void* stream) {
  using namespace osc;
  // ---- every check before the launch ----
  if (!model || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (model->kid != K_GO2 && model->kid != K_WALTER) return OSC_ERR_INVALID_ARGUMENT;   // wheel rows
  if (!model->refine) return OSC_ERR_INVALID_ARGUMENT;   // (as the forward _env entries)
  const EnvPtrs ep = env_params ? EnvPtrs{env_params->mu, env_params->u_lb, env_params->u_ub,
                                          env_params->fz_lb, env_params->fz_ub, env_params->w_pos,
                                          env_params->w_rot}
                                : EnvPtrs{};
  const EnvGradPtrs g = grads ? EnvGradPtrs{grads->mu, grads->u_lb, grads->u_ub, grads->fz_lb,
                                            grads->fz_ub, grads->w_pos, grads->w_rot}
                              : EnvGradPtrs{};
  for (const void* p : {static_cast<const void*>(ep.mu), static_cast<const void*>(ep.u_lb),
                        static_cast<const void*>(ep.u_ub), static_cast<const void*>(ep.fz_lb),
                        static_cast<const void*>(ep.fz_ub), static_cast<const void*>(ep.w_pos),
                        static_cast<const void*>(ep.w_rot), static_cast<const void*>(g.mu),
                        static_cast<const void*>(g.u_lb), static_cast<const void*>(g.u_ub),
                        static_cast<const void*>(g.fz_lb), static_cast<const void*>(g.fz_ub),
                        static_cast<const void*>(g.w_pos), static_cast<const void*>(g.w_rot)})
    if (misaligned(p, 8)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != model->device) return OSC_ERR_INVALID_ARGUMENT;
  if (!M || !J || !b || !T || !contact_mask || !x || !y || !status || !grad_x || !workspace)
    return OSC_ERR_INVALID_ARGUMENT;
  // (alignments as osc_batch_solve_backward_data)
  if (misaligned(M, 16) || misaligned(J, 16) || misaligned(contact_mask, 16) ||
      misaligned(workspace, 16) || misaligned(grad_M, 16) || misaligned(grad_C, 16) ||
      misaligned(grad_J, 16) || misaligned(b, 8) || misaligned(T, 8) || misaligned(x, 8) ||
      misaligned(y, 8) || misaligned(grad_x, 8) || misaligned(grad_wrow, 8) ||
      misaligned(grad_T, 8) || misaligned(grad_b, 8) || misaligned(status, 4))
    return OSC_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < ws_layout(model->kid, nenv).total) return OSC_ERR_INVALID_ARGUMENT;
  const bool data = grad_M || grad_C || grad_J || grad_wrow || grad_T || grad_b || g.w_pos ||
                    g.w_rot;
  const bool par = g.mu || g.u_lb || g.u_ub || g.fz_lb || g.fz_ub;
  if (!data && !par) return OSC_OK;
  const BwEnvArgs a{M, J, b, T, contact_mask, x, y, grad_x,
                    static_cast<const double*>(workspace), status, grad_M, grad_C, grad_J,
                    grad_wrow, grad_T, grad_b, ep, g};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool env = ep.mu || ep.u_lb || ep.u_ub || ep.fz_lb || ep.fz_ub || ep.w_pos || ep.w_rot;
  if (model->kid == K_GO2)
    return env ? launch_backward_env<Go2, true>(model, nenv, a, data, par, s)
               : launch_backward_env<Go2, false>(model, nenv, a, data, par, s);
  return env ? launch_backward_env<Walter, true>(model, nenv, a, data, par, s)
             : launch_backward_env<Walter, false>(model, nenv, a, data, par, s);
}
