// osc_kin_backward.hpp -- device code of the kinematics kernel's vector-Jacobian product
// (include/osc_kin_backward.h; the forward: osc_kin_device.hpp, formulation in osc_kinematics.hip's
// header).  The forward stages are recomputed by the forward's own device functions, unedited; the
// functions here are their adjoints, one per stage, run in reverse order by
// osc_kinematics_backward_kernel (osc_kin_backward.hip).
//
// Next to an env's forward state E (EnvLayout) lies an adjoint block A of the same layout:
//   A + lay.q      d L / d qpos (nq) | d L / d qvel (nv)
//   A + lay.body   per body, the B_* offsets: adjoints of R, x, w, v_O, al, a_O and of the
//                  composite (m, h, I_O) and force f
//   A + lay.dof    per dof: adjoints of S (6) | F (6)
//   A + lay.site   per site: grad_J's part of the adjoint of its position
// Every slot has one owning lane per phase (lane = dof, then lane = body), phases are separated
// by wave barriers, and sums over sites / dofs / children run in index order inside the owning
// lane: no atomics, and an env's result does not depend on its row or on the batch around it.
#pragma once
#include "osc_kin_device.hpp"

namespace osc_kin {

// Cotangents of one env (each nullable = zero), already offset to the env.
struct KinCot {
  const double* M;   // [nv][nv]
  const double* C;   // [nv]
  const double* J;   // [6 ns][nv]
  const double* b;   // [6 ns]
  const double* x;   // [ns][3]
};

// a += s x t  (a . (s x t) bookkeeping lives at the call sites)
__device__ __forceinline__ void cross_acc(const double* s, const double* t, double* a) {
  a[0] += s[1] * t[2] - s[2] * t[1];
  a[1] += s[2] * t[0] - s[0] * t[2];
  a[2] += s[0] * t[1] - s[1] * t[0];
}

// Adjoint of (n, f) = inertia_mul(m, h, IO, w, v): given gn, gf accumulates into gm, gh, gIO
// (packed xx yy zz xy xz yz: each off-diagonal scalar sits at two matrix positions), gw, gv.
__device__ __forceinline__ void inertia_mul_adj(double m, const double* h, const double* IO,
                                                const double* w, const double* v,
                                                const double* gn, const double* gf, double* gm,
                                                double* gh, double* gIO, double* gw, double* gv) {
  gw[0] += IO[0] * gn[0] + IO[3] * gn[1] + IO[4] * gn[2];
  gw[1] += IO[3] * gn[0] + IO[1] * gn[1] + IO[5] * gn[2];
  gw[2] += IO[4] * gn[0] + IO[5] * gn[1] + IO[2] * gn[2];
  gIO[0] += gn[0] * w[0];
  gIO[1] += gn[1] * w[1];
  gIO[2] += gn[2] * w[2];
  gIO[3] += gn[0] * w[1] + gn[1] * w[0];
  gIO[4] += gn[0] * w[2] + gn[2] * w[0];
  gIO[5] += gn[1] * w[2] + gn[2] * w[1];
  cross_acc(v, gn, gh);    // gn . (h x v) = h . (v x gn)
  cross_acc(gn, h, gv);    //              = v . (gn x h)
  *gm += gf[0] * v[0] + gf[1] * v[1] + gf[2] * v[2];
  for (int k = 0; k < 3; ++k) gv[k] += m * gf[k];
  cross_acc(gf, w, gh);    // -gf . (h x w) = h . (gf x w)
  cross_acc(h, gf, gw);    //               = w . (h x gf)
}

// Adjoint of R = quat2mat(q / |q|) with respect to the raw q: gq[0..3] (orthogonal to q).
__device__ __forceinline__ void quat_adj(const double* q, const double* gR, double* gq) {
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
  double g[4];
  g[0] = 2 * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
  g[1] = 2 * (y * gR[1] + z * gR[2] + y * gR[3] - 2 * x * gR[4] - w * gR[5] + z * gR[6] +
              w * gR[7] - 2 * x * gR[8]);
  g[2] = 2 * (-2 * y * gR[0] + x * gR[1] + w * gR[2] + x * gR[3] + z * gR[5] - w * gR[6] +
              z * gR[7] - 2 * y * gR[8]);
  g[3] = 2 * (-2 * z * gR[0] - w * gR[1] + x * gR[2] + w * gR[3] - 2 * z * gR[4] + y * gR[5] +
              x * gR[6] + y * gR[7]);
  const double dot = w * g[0] + x * g[1] + y * g[2] + z * g[3];
  gq[0] = inv * (g[0] - w * dot);
  gq[1] = inv * (g[1] - x * dot);
  gq[2] = inv * (g[2] - y * dot);
  gq[3] = inv * (g[3] - z * dot);
}

// Stages 6' and 5' for dof c (lane = dof): the adjoints of S_c and F_c from grad_J and grad_M into
// the dof's adjoint slot.  M_ij and M_ji (i < j) are one product S_i . F_j, so its cotangent is
// grad_M[i][j] + grad_M[j][i]; dof c sums over its related partners itself, in index order.
// Returns grad_M[c][c] (the armature's cotangent).
__device__ __forceinline__ double kinb_dof_seed(const KinDev* K, const double* E, double* A,
                                                const EnvLayout& lay, int c, const KinCot& g) {
  const int nv = K->nv, ns = K->nsite;
  double gS[6] = {0, 0, 0, 0, 0, 0}, gF[6] = {0, 0, 0, 0, 0, 0};
  double gdiag = 0.0;
  if (g.J) {
    // (selects, not branches: the loop stays uniform over the row's lanes and its loads can be
    // issued ahead; a column that is not an ancestor dof of the site has no gradient)
    for (int k = 0; k < ns; ++k) {
      const bool r = (K->site_dofmask[k] >> c) & 1u;
      const double* xk = E + lay.site + 3 * k;
      double gp[3], gr[3];
      for (int t = 0; t < 3; ++t) {
        const double p0 = g.J[(3 * k + t) * nv + c], r0 = g.J[(3 * ns + 3 * k + t) * nv + c];
        gp[t] = r ? p0 : 0.0;
        gr[t] = r ? r0 : 0.0;
      }
      // Jp = S.v + S.w x xk, Jr = S.w
      for (int t = 0; t < 3; ++t) {
        gS[t] += gr[t];
        gS[3 + t] += gp[t];
      }
      cross_acc(xk, gp, gS);   // gp . (w x xk) = w . (xk x gp)
    }
  }
  if (g.M) {
    const uint32_t rel = K->dof_relmask[c];
    for (int t = 0; t < nv; ++t) {
      const double* Dt = E + lay.dof + kDofStride * t;
      const double row = g.M[c * nv + t], col = g.M[t * nv + c];
      const double gm = ((rel >> t) & 1u) ? (t == c ? row : row + col) : 0.0;
      gdiag = (t == c) ? gm : gdiag;
      const double gs = (t >= c) ? gm : 0.0, gf = (t <= c) ? gm : 0.0;
      for (int i = 0; i < 6; ++i) {
        gS[i] = fma(gs, Dt[6 + i], gS[i]);
        gF[i] = fma(gf, Dt[i], gF[i]);
      }
    }
  }
  double* Ad = A + lay.dof + kDofStride * c;
  for (int i = 0; i < 6; ++i) {
    Ad[i] = gS[i];
    Ad[6 + i] = gF[i];
  }
  return gdiag;
}

// Stage 6' for site k (lane = site): grad_J's part of the site position's adjoint, through
// Jp_c = S_c.v + S_c.w x xk over the site's ancestor dofs c, into the site's adjoint slot.
__device__ __forceinline__ void kinb_site_seed(const KinDev* K, const double* E, double* A,
                                               const EnvLayout& lay, int k, const KinCot& g) {
  const int nv = K->nv;
  double gx[3] = {0, 0, 0};
  if (g.J) {
    const uint32_t rel = K->site_dofmask[k];
    for (int c = 0; c < nv; ++c) {
      const bool r = (rel >> c) & 1u;
      const double* Sc = E + lay.dof + kDofStride * c;
      double gp[3];
      for (int t = 0; t < 3; ++t) {
        const double p0 = g.J[(3 * k + t) * nv + c];
        gp[t] = r ? p0 : 0.0;
      }
      cross_acc(gp, Sc, gx);                // gp . (w x xk) = xk . (gp x w)
    }
  }
  for (int t = 0; t < 3; ++t) A[lay.site + 3 * k + t] = gx[t];
}

// Stages 4' and 3' for body b (lane = body): every adjoint of the body that does not come through
// the tree -- its sites' (grad_b, grad_site_xpos, and grad_J through the site position) and its
// own dofs' (S, F = Ic S, C = S . f) -- written to the body's adjoint slot: frame adjoints at
// B_R .. B_AO, composite adjoints at B_M .. B_F.
__device__ __forceinline__ void kinb_body_seed(const KinDev* K, const double* E, double* A,
                                               const EnvLayout& lay, int b, const KinCot& g) {
  const int ns = K->nsite;
  const double* B = E + lay.body + kBodyStride * b;
  double a[kBodyStride];
  for (int i = 0; i < kBodyStride; ++i) a[i] = 0.0;
  // ---- sites: b as the Jacobian body (w, v_O, al, a_O) and as the point's body (R, x) ----
  for (int k = 0; k < ns; ++k) {
    const bool jac = K->site_jac[k] == b, pt = K->site_body[k] == b;
    if (!jac && !pt) continue;
    const double* xk = E + lay.site + 3 * k;
    const double* Bj = E + lay.body + kBodyStride * K->site_jac[k];
    double gx[3] = {0, 0, 0};
    if (g.b) {
      const double gp[3] = {g.b[3 * k], g.b[3 * k + 1], g.b[3 * k + 2]};
      const double w[3] = {Bj[B_W], Bj[B_W + 1], Bj[B_W + 2]};
      const double al[3] = {Bj[B_AL], Bj[B_AL + 1], Bj[B_AL + 2]};
      // bp = a_O + al x xk + w x vx, vx = v_O + w x xk;  br = al
      double wx[3], vx[3], gvx[3];
      cross(w, xk, wx);
      for (int i = 0; i < 3; ++i) vx[i] = Bj[B_VO + i] + wx[i];
      cross(gp, w, gvx);                    // gp . (w x vx) = vx . (gp x w)
      if (jac) {
        for (int i = 0; i < 3; ++i) {
          a[B_AO + i] += gp[i];
          a[B_AL + i] += g.b[3 * ns + 3 * k + i];
          a[B_VO + i] += gvx[i];
        }
        cross_acc(xk, gp, a + B_AL);        // gp . (al x xk) = al . (xk x gp)
        cross_acc(vx, gp, a + B_W);         // gp . (w x vx) = w . (vx x gp)
        cross_acc(xk, gvx, a + B_W);        // gvx . (w x xk) = w . (xk x gvx)
      }
      if (pt) {
        cross_acc(gp, al, gx);              // gp . (al x xk) = xk . (gp x al)
        cross_acc(gvx, w, gx);              // gvx . (w x xk) = xk . (gvx x w)
      }
    }
    if (pt) {
      if (g.x)
        for (int i = 0; i < 3; ++i) gx[i] += g.x[3 * k + i];
      for (int i = 0; i < 3; ++i) gx[i] += A[lay.site + 3 * k + i];   // grad_J's (kinb_site_seed)
      // xk = x + R sp
      const double* sp = K->site_pos[k];
      for (int i = 0; i < 3; ++i) {
        a[B_X + i] += gx[i];
        for (int j = 0; j < 3; ++j) a[B_R + 3 * i + j] += gx[i] * sp[j];
      }
    }
  }
  // ---- the body's own dofs ----
  const int jt = K->jtype[b];
  const int nd = jt == OSC_KIN_JOINT_FREE ? 6 : jt == OSC_KIN_JOINT_BALL ? 3
               : (jt == OSC_KIN_JOINT_HINGE || jt == OSC_KIN_JOINT_SLIDE) ? 1 : 0;
  for (int k = 0; k < nd; ++k) {
    const int d = K->dadr[b] + k;
    const double* Dd = E + lay.dof + kDofStride * d;
    const double* Ad = A + lay.dof + kDofStride * d;
    double S[6], gS[6], gF[6];
    for (int i = 0; i < 6; ++i) {
      S[i] = Dd[i];
      gS[i] = Ad[i];
      gF[i] = Ad[6 + i];
    }
    if (g.C) {   // C_d = S . f (composite force)
      const double gc = g.C[d];
      for (int i = 0; i < 6; ++i) {
        gS[i] = fma(gc, B[B_F + i], gS[i]);
        a[B_F + i] = fma(gc, S[i], a[B_F + i]);
      }
    }
    // F = Ic S (the composite inertia at B_M, B_H, B_IO)
    inertia_mul_adj(B[B_M], B + B_H, B + B_IO, S, S + 3, gF, gF + 3, a + B_M, a + B_H, a + B_IO,
                    gS, gS + 3);
    // S -> R, x
    if (jt == OSC_KIN_JOINT_FREE) {
      if (k >= 3) {   // S = (a, x x a), a = R e_(k-3)
        const double av[3] = {B[B_R + k - 3], B[B_R + 3 + k - 3], B[B_R + 6 + k - 3]};
        double ga[3] = {gS[0], gS[1], gS[2]};
        cross_acc(gS + 3, B + B_X, ga);     // gv . (x x a) = a . (gv x x)
        cross_acc(av, gS + 3, a + B_X);     //              = x . (a x gv)
        for (int i = 0; i < 3; ++i)   // (a select, not a dynamic index: `a` stays in registers)
          for (int j = 0; j < 3; ++j) a[B_R + 3 * i + j] += (j == k - 3) ? ga[i] : 0.0;
      }
    } else if (jt == OSC_KIN_JOINT_SLIDE) {   // S = (0, R u)
      const double* u = K->axis[b];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[B_R + 3 * i + j] += gS[3 + i] * u[j];
    } else {   // S = (a, pa x a), a = R u or R e_k, pa = x + R jp
      const double* u = K->axis[b];
      const double* jp = K->jpos[b];
      const bool ball = jt == OSC_KIN_JOINT_BALL;
      double av[3], pa[3];
      for (int i = 0; i < 3; ++i) {
        av[i] = ball ? B[B_R + 3 * i + k]
                     : B[B_R + 3 * i] * u[0] + B[B_R + 3 * i + 1] * u[1] + B[B_R + 3 * i + 2] * u[2];
        pa[i] = B[B_X + i] + B[B_R + 3 * i] * jp[0] + B[B_R + 3 * i + 1] * jp[1] +
                B[B_R + 3 * i + 2] * jp[2];
      }
      double ga[3] = {gS[0], gS[1], gS[2]}, gpa[3] = {0, 0, 0};
      cross_acc(gS + 3, pa, ga);
      cross_acc(av, gS + 3, gpa);
      for (int i = 0; i < 3; ++i) {
        a[B_X + i] += gpa[i];
        for (int j = 0; j < 3; ++j) {
          a[B_R + 3 * i + j] += gpa[i] * jp[j];
          a[B_R + 3 * i + j] += ga[i] * (ball ? (j == k ? 1.0 : 0.0) : u[j]);
        }
      }
    }
  }
  double* Ab = A + lay.body + kBodyStride * b;
  for (int i = 0; i < kBodyStride; ++i) Ab[i] = a[i];
}

// Stage 2': a body's own (m, h, I_O, f) enters the composite of every ancestor-or-self, so its
// adjoint is the sum of theirs: top-down by level, own plus the parent's total (lane = body l).
__device__ __forceinline__ void kinb_composite(const KinDev* K, double* A, const EnvLayout& lay,
                                               int l) {
  const int nb = K->nbody, nd = K->ndepth;
  const int my_depth = (l < nb) ? K->depth[l] : -1;
  for (int L = 1; L < nd; ++L) {
    if (my_depth == L) {
      double* Ab = A + lay.body + kBodyStride * l;
      const double* Ap = A + lay.body + kBodyStride * K->parent[l];
      for (int i = B_M; i < kBodyStride; ++i) Ab[i] += Ap[i];
    }
    wave_sync();
  }
}

// body_dynamics' for body b (lane = body): the adjoints of the body's own (m, h, I_O) and RNEA
// force at B_M .. B_F go into its frame adjoints at B_R .. B_AO; returns the gradients of the
// body's mass scale (m gm + sum ib gIb) and COM offset (R' gc).  The own inertia is recomputed
// (the forward state holds the composite by now).  ms, dc: the env's parameters of this body.
__device__ __forceinline__ void kinb_dynamics(const KinDev* K, const double* E, double* A,
                                              const EnvLayout& lay, int b, double ms,
                                              const double* dc, double* g_ms, double* g_dc) {
  const double* B = E + lay.body + kBodyStride * b;
  double* Ab = A + lay.body + kBodyStride * b;
  double R[9], x[3], w[3], vo[3], al[3], ag[3];
  for (int i = 0; i < 9; ++i) R[i] = B[B_R + i];
  for (int i = 0; i < 3; ++i) {
    x[i] = B[B_X + i]; w[i] = B[B_W + i]; vo[i] = B[B_VO + i];
    al[i] = B[B_AL + i]; ag[i] = B[B_AO + i] - K->gravity[i];
  }
  const double m0 = K->mass[b], m = ms * m0;
  double ip[3], ib[6];
  for (int i = 0; i < 3; ++i) ip[i] = K->ipos[b][i] + dc[i];
  for (int i = 0; i < 6; ++i) ib[i] = ms * K->ib[b][i];
  double c[3];
  for (int i = 0; i < 3; ++i) c[i] = x[i] + R[3 * i] * ip[0] + R[3 * i + 1] * ip[1] + R[3 * i + 2] * ip[2];
  const double Ibf[9] = {ib[0], ib[3], ib[4], ib[3], ib[1], ib[5], ib[4], ib[5], ib[2]};
  double RI[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      RI[3 * i + j] = R[3 * i] * Ibf[j] + R[3 * i + 1] * Ibf[3 + j] + R[3 * i + 2] * Ibf[6 + j];
  auto rir = [&](int i, int j) {
    return RI[3 * i] * R[3 * j] + RI[3 * i + 1] * R[3 * j + 1] + RI[3 * i + 2] * R[3 * j + 2];
  };
  const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  double IO[6], h[3];
  IO[0] = rir(0, 0) + m * (cc - c[0] * c[0]);
  IO[1] = rir(1, 1) + m * (cc - c[1] * c[1]);
  IO[2] = rir(2, 2) + m * (cc - c[2] * c[2]);
  IO[3] = rir(0, 1) - m * c[0] * c[1];
  IO[4] = rir(0, 2) - m * c[0] * c[2];
  IO[5] = rir(1, 2) - m * c[1] * c[2];
  for (int i = 0; i < 3; ++i) h[i] = m * c[i];
  double n1[3], f1[3], ln[3], lf[3];
  inertia_mul(m, h, IO, al, ag, n1, f1);
  inertia_mul(m, h, IO, w, vo, ln, lf);
  (void)n1; (void)f1;

  double gm = Ab[B_M], gh[3], gIO[6], gFn[3], gFf[3];
  for (int i = 0; i < 3; ++i) {
    gh[i] = Ab[B_H + i];
    gFn[i] = Ab[B_F + i];
    gFf[i] = Ab[B_F + 3 + i];
  }
  for (int i = 0; i < 6; ++i) gIO[i] = Ab[B_IO + i];
  double gw[3] = {0, 0, 0}, gvo[3] = {0, 0, 0}, gal[3] = {0, 0, 0}, gao[3] = {0, 0, 0};
  double gln[3] = {0, 0, 0}, glf[3] = {0, 0, 0};
  // Fn = n1 + w x ln + vo x lf, Ff = f1 + w x lf
  cross_acc(ln, gFn, gw);
  cross_acc(gFn, w, gln);
  cross_acc(lf, gFn, gvo);
  cross_acc(gFn, vo, glf);
  cross_acc(lf, gFf, gw);
  cross_acc(gFf, w, glf);
  inertia_mul_adj(m, h, IO, al, ag, gFn, gFf, &gm, gh, gIO, gal, gao);
  inertia_mul_adj(m, h, IO, w, vo, gln, glf, &gm, gh, gIO, gw, gvo);
  // h = m c
  double gc[3];
  gm += gh[0] * c[0] + gh[1] * c[1] + gh[2] * c[2];
  for (int i = 0; i < 3; ++i) gc[i] = m * gh[i];
  // I_O = R Ib R' + m (|c|^2 I - c c')
  gm += gIO[0] * (cc - c[0] * c[0]) + gIO[1] * (cc - c[1] * c[1]) + gIO[2] * (cc - c[2] * c[2]) -
        gIO[3] * c[0] * c[1] - gIO[4] * c[0] * c[2] - gIO[5] * c[1] * c[2];
  const double tr = gIO[0] + gIO[1] + gIO[2];
  gc[0] += m * (2 * (tr - gIO[0]) * c[0] - gIO[3] * c[1] - gIO[4] * c[2]);
  gc[1] += m * (2 * (tr - gIO[1]) * c[1] - gIO[3] * c[0] - gIO[5] * c[2]);
  gc[2] += m * (2 * (tr - gIO[2]) * c[2] - gIO[4] * c[0] - gIO[5] * c[1]);
  // sum_p gIO_p (R Ib R')_p = tr(W R Ib R'), W symmetric with the off-diagonals halved
  const double W[9] = {gIO[0], 0.5 * gIO[3], 0.5 * gIO[4], 0.5 * gIO[3], gIO[1], 0.5 * gIO[5],
                       0.5 * gIO[4], 0.5 * gIO[5], gIO[2]};
  double gR[9], WR[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      gR[3 * i + j] = 2 * (W[3 * i] * RI[j] + W[3 * i + 1] * RI[3 + j] + W[3 * i + 2] * RI[6 + j]);
      WR[3 * i + j] = W[3 * i] * R[j] + W[3 * i + 1] * R[3 + j] + W[3 * i + 2] * R[6 + j];
    }
  auto rwr = [&](int i, int j) {   // (R' W R)_ij
    return R[i] * WR[j] + R[3 + i] * WR[3 + j] + R[6 + i] * WR[6 + j];
  };
  const double* ib0 = K->ib[b];
  *g_ms = m0 * gm + ib0[0] * rwr(0, 0) + ib0[1] * rwr(1, 1) + ib0[2] * rwr(2, 2) +
          2 * (ib0[3] * rwr(0, 1) + ib0[4] * rwr(0, 2) + ib0[5] * rwr(1, 2));
  // c = x + R ip
  for (int j = 0; j < 3; ++j) g_dc[j] = R[j] * gc[0] + R[3 + j] * gc[1] + R[6 + j] * gc[2];
  for (int i = 0; i < 3; ++i) {
    Ab[B_X + i] += gc[i];
    Ab[B_W + i] += gw[i];
    Ab[B_VO + i] += gvo[i];
    Ab[B_AL + i] += gal[i];
    Ab[B_AO + i] += gao[i];
    for (int j = 0; j < 3; ++j) Ab[B_R + 3 * i + j] += gR[3 * i + j] + gc[i] * ip[j];
  }
}

// body_forward' for body b: its total frame adjoints (own slot plus what its children pushed into
// theirs) go to its qpos / qvel entries (A + lay.q) and to its parent: the push overwrites the
// body's own slot B_R .. B_AO, which the parent's lane sums one level later.  s, c: the hinge's
// sin / cos, as the forward takes them.
__device__ __forceinline__ void kinb_body(const KinDev* K, const double* E, double* A,
                                          const EnvLayout& lay, int b, double s, double c) {
  double* Ab = A + lay.body + kBodyStride * b;
  double gR[9], gx[3], gw[3], gvo[3], gal[3], gao[3];
  for (int i = 0; i < 9; ++i) gR[i] = Ab[B_R + i];
  for (int i = 0; i < 3; ++i) {
    gx[i] = Ab[B_X + i]; gw[i] = Ab[B_W + i]; gvo[i] = Ab[B_VO + i];
    gal[i] = Ab[B_AL + i]; gao[i] = Ab[B_AO + i];
  }
  for (int ch = K->first_child[b]; ch >= 0; ch = K->next_sibling[ch]) {
    const double* Ac = A + lay.body + kBodyStride * ch;
    for (int i = 0; i < 9; ++i) gR[i] += Ac[B_R + i];
    for (int i = 0; i < 3; ++i) {
      gx[i] += Ac[B_X + i]; gw[i] += Ac[B_W + i]; gvo[i] += Ac[B_VO + i];
      gal[i] += Ac[B_AL + i]; gao[i] += Ac[B_AO + i];
    }
  }
  const int jt = K->jtype[b];
  const double* q = E + lay.q;
  const double* qd = E + lay.q + K->nq;
  double* gq = A + lay.q;
  double* gqd = A + lay.q + K->nq;
  const double* B = E + lay.body + kBodyStride * b;
  if (jt == OSC_KIN_JOINT_FREE) {
    const int qa = K->qadr[b], da = K->dadr[b];
    const double x[3] = {B[B_X], B[B_X + 1], B[B_X + 2]};
    const double w[3] = {B[B_W], B[B_W + 1], B[B_W + 2]};
    const double v[3] = {qd[da], qd[da + 1], qd[da + 2]};
    const double wl[3] = {qd[da + 3], qd[da + 4], qd[da + 5]};
    // w = R wl, v_O = v + x x w, al = 0, a_O = v x w
    double gv[3] = {gvo[0], gvo[1], gvo[2]};
    cross_acc(w, gao, gv);      // gao . (v x w) = v . (w x gao)
    cross_acc(gao, v, gw);      //               = w . (gao x v)
    cross_acc(w, gvo, gx);      // gvo . (x x w) = x . (w x gvo)
    cross_acc(gvo, x, gw);      //               = w . (gvo x x)
    for (int j = 0; j < 3; ++j) {
      gqd[da + j] = gv[j];
      gqd[da + 3 + j] = B[B_R + j] * gw[0] + B[B_R + 3 + j] * gw[1] + B[B_R + 6 + j] * gw[2];
      gq[qa + j] = gx[j];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gR[3 * i + j] += gw[i] * wl[j];
    quat_adj(q + qa + 3, gR, gq + qa + 3);
    return;
  }
  const int p = K->parent[b];
  double pR[9], px[3], pw[3], pvo[3];
  if (p >= 0) {
    const double* P = E + lay.body + kBodyStride * p;
    for (int i = 0; i < 9; ++i) pR[i] = P[B_R + i];
    for (int i = 0; i < 3; ++i) { px[i] = P[B_X + i]; pw[i] = P[B_W + i]; pvo[i] = P[B_VO + i]; }
  } else {
    for (int i = 0; i < 9; ++i) pR[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) px[i] = pw[i] = pvo[i] = 0.0;
  }
  const double* rq = K->rq[b];
  const double* bp = K->pos[b];
  const double* u = K->axis[b];
  const double* jp = K->jpos[b];
  double Rb[9], x0[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      Rb[3 * i + j] = pR[3 * i] * rq[j] + pR[3 * i + 1] * rq[3 + j] + pR[3 * i + 2] * rq[6 + j];
    x0[i] = px[i] + pR[3 * i] * bp[0] + pR[3 * i + 1] * bp[1] + pR[3 * i + 2] * bp[2];
  }
  // the parent's adjoints, and those of Rb and x0 = px + pR bp
  double gpw[3] = {gw[0], gw[1], gw[2]}, gpvo[3] = {gvo[0], gvo[1], gvo[2]};
  double gRb[9], gx0[3];
  if (jt == OSC_KIN_JOINT_HINGE || jt == OSC_KIN_JOINT_BALL) {
    const bool ball = jt == OSC_KIN_JOINT_BALL;
    double anc[3], Ra[9], av[3], wj[3], vj[3];
    for (int i = 0; i < 3; ++i)
      anc[i] = x0[i] + Rb[3 * i] * jp[0] + Rb[3 * i + 1] * jp[1] + Rb[3 * i + 2] * jp[2];
    double wl[3] = {0, 0, 0}, qv = 0.0;
    if (ball) {
      const int qa = K->qadr[b], da = K->dadr[b];
      double qw = q[qa], qx = q[qa + 1], qy = q[qa + 2], qz = q[qa + 3];
      const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
      qw *= inv; qx *= inv; qy *= inv; qz *= inv;
      Ra[0] = 1 - 2 * (qy * qy + qz * qz); Ra[1] = 2 * (qx * qy - qw * qz); Ra[2] = 2 * (qx * qz + qw * qy);
      Ra[3] = 2 * (qx * qy + qw * qz); Ra[4] = 1 - 2 * (qx * qx + qz * qz); Ra[5] = 2 * (qy * qz - qw * qx);
      Ra[6] = 2 * (qx * qz - qw * qy); Ra[7] = 2 * (qy * qz + qw * qx); Ra[8] = 1 - 2 * (qx * qx + qy * qy);
      for (int i = 0; i < 3; ++i) wl[i] = qd[da + i];
      for (int i = 0; i < 3; ++i)
        wj[i] = B[B_R + 3 * i] * wl[0] + B[B_R + 3 * i + 1] * wl[1] + B[B_R + 3 * i + 2] * wl[2];
    } else {
      const double t = 1.0 - c;
      Ra[0] = c + t * u[0] * u[0]; Ra[1] = t * u[0] * u[1] - s * u[2]; Ra[2] = t * u[0] * u[2] + s * u[1];
      Ra[3] = t * u[0] * u[1] + s * u[2]; Ra[4] = c + t * u[1] * u[1]; Ra[5] = t * u[1] * u[2] - s * u[0];
      Ra[6] = t * u[0] * u[2] - s * u[1]; Ra[7] = t * u[1] * u[2] + s * u[0]; Ra[8] = c + t * u[2] * u[2];
      qv = qd[K->dadr[b]];
      for (int i = 0; i < 3; ++i) {
        av[i] = Rb[3 * i] * u[0] + Rb[3 * i + 1] * u[1] + Rb[3 * i + 2] * u[2];
        wj[i] = av[i] * qv;
      }
    }
    cross(anc, wj, vj);
    // w = pw + wj, v_O = pvo + vj, al = pal + pw x wj, a_O = pao + pw x vj + pvo x wj
    double gwj[3] = {gw[0], gw[1], gw[2]}, gvj[3] = {gvo[0], gvo[1], gvo[2]};
    cross_acc(vj, gao, gpw);
    cross_acc(gao, pw, gvj);
    cross_acc(wj, gao, gpvo);
    cross_acc(gao, pvo, gwj);
    cross_acc(wj, gal, gpw);
    cross_acc(gal, pw, gwj);
    // vj = anc x wj
    double ganc[3] = {gx[0], gx[1], gx[2]};   // x = anc - R jp
    cross_acc(wj, gvj, ganc);
    cross_acc(gvj, anc, gwj);
    for (int i = 0; i < 9; ++i) gRb[i] = 0.0;
    if (ball) {   // wj = R wl
      const int da = K->dadr[b];
      for (int j = 0; j < 3; ++j)
        gqd[da + j] = B[B_R + j] * gwj[0] + B[B_R + 3 + j] * gwj[1] + B[B_R + 6 + j] * gwj[2];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) gR[3 * i + j] += gwj[i] * wl[j];
    } else {      // wj = (Rb u) qv
      gqd[K->dadr[b]] = gwj[0] * av[0] + gwj[1] * av[1] + gwj[2] * av[2];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) gRb[3 * i + j] += qv * gwj[i] * u[j];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gR[3 * i + j] -= gx[i] * jp[j];
    // R = Rb Ra
    double gRa[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        gRb[3 * i + j] += gR[3 * i] * Ra[3 * j] + gR[3 * i + 1] * Ra[3 * j + 1] +
                          gR[3 * i + 2] * Ra[3 * j + 2];
        gRa[3 * i + j] = Rb[i] * gR[j] + Rb[3 + i] * gR[3 + j] + Rb[6 + i] * gR[6 + j];
      }
    // anc = x0 + Rb jp
    for (int i = 0; i < 3; ++i) {
      gx0[i] = ganc[i];
      for (int j = 0; j < 3; ++j) gRb[3 * i + j] += ganc[i] * jp[j];
    }
    if (ball) {
      quat_adj(q + K->qadr[b], gRa, gq + K->qadr[b]);
    } else {   // Ra = c I + s [u]x + (1 - c) u u'
      const double gs = -gRa[1] * u[2] + gRa[2] * u[1] + gRa[3] * u[2] - gRa[5] * u[0] -
                        gRa[6] * u[1] + gRa[7] * u[0];
      double gcs = 0.0;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) gcs += gRa[3 * i + j] * ((i == j ? 1.0 : 0.0) - u[i] * u[j]);
      gq[K->qadr[b]] = gs * c - gcs * s;
    }
  } else if (jt == OSC_KIN_JOINT_SLIDE) {
    // a = Rb u: x = x0 + a q, vj = a qd, R = Rb, w = pw, v_O = pvo + vj, al = pal,
    // a_O = pao + pw x vj
    const double qv = q[K->qadr[b]], qdv = qd[K->dadr[b]];
    double av[3], vj[3];
    for (int i = 0; i < 3; ++i) {
      av[i] = Rb[3 * i] * u[0] + Rb[3 * i + 1] * u[1] + Rb[3 * i + 2] * u[2];
      vj[i] = av[i] * qdv;
    }
    double gvj[3] = {gvo[0], gvo[1], gvo[2]};
    cross_acc(vj, gao, gpw);
    cross_acc(gao, pw, gvj);
    gqd[K->dadr[b]] = gvj[0] * av[0] + gvj[1] * av[1] + gvj[2] * av[2];
    gq[K->qadr[b]] = gx[0] * av[0] + gx[1] * av[1] + gx[2] * av[2];
    for (int i = 0; i < 3; ++i) {
      const double ga = qdv * gvj[i] + qv * gx[i];
      gx0[i] = gx[i];
      for (int j = 0; j < 3; ++j) gRb[3 * i + j] = gR[3 * i + j] + ga * u[j];
    }
  } else {   // welded
    for (int i = 0; i < 9; ++i) gRb[i] = gR[i];
    for (int i = 0; i < 3; ++i) gx0[i] = gx[i];
  }
  // Rb = pR rq, x0 = px + pR bp: the push to the parent
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      Ab[B_R + 3 * i + j] = gRb[3 * i] * rq[3 * j] + gRb[3 * i + 1] * rq[3 * j + 1] +
                            gRb[3 * i + 2] * rq[3 * j + 2] + gx0[i] * bp[j];
    Ab[B_X + i] = gx0[i];
    Ab[B_W + i] = gpw[i];
    Ab[B_VO + i] = gpvo[i];
    Ab[B_AL + i] = gal[i];
    Ab[B_AO + i] = gao[i];
  }
}

// Stage 1': level by level, deepest first (lane = body l).
__device__ __forceinline__ void kinb_tree(const KinDev* K, const double* E, double* A,
                                          const EnvLayout& lay, int l) {
  const int nb = K->nbody, nd = K->ndepth;
  const int my_depth = (l < nb) ? K->depth[l] : -1;
  double sn = 0.0, cs = 1.0;
  if (l < nb && K->jtype[l] == OSC_KIN_JOINT_HINGE) sincos(E[lay.q + K->qadr[l]], &sn, &cs);
  for (int L = nd - 1; L >= 0; --L) {
    if (my_depth == L) kinb_body(K, E, A, lay, l, sn, cs);
    wave_sync();
  }
}

}  // namespace osc_kin
