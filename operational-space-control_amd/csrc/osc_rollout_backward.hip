// osc_rollout_backward.hip -- backward pass of the closed-loop rollout (C-ABI and the formulation
// in include/osc_rollout_backward.h): for t = K-1 .. 0 the tick is recomputed from history slab t
// and differentiated by the library's single-tick backward passes; this unit adds the adjoint of
// the semi-implicit Euler step, the adjoint of the PD base-target producer and the tick-to-tick
// reduction.  One tick loop serves the plain and the scheduled entries
// (include/osc_rollout_schedule.h); the tick's inputs are resolved by osc::tick_inputs, as in the
// forward's loop.
//
// Two kernels of this unit run per tick, both with the step kernel's mapping (a 256-thread block
// owns 16 consecutive envs and walks them with a flat env x coordinate index; what is per env
// rather than per coordinate goes through LDS; joint types and addresses come from the kinematics
// model's device tables, turned into the per-block JointMaps of osc_rollout_internal.hpp):
//   step adjoint  g_q, g_v of slab t + 1  ->  grad_x = (dt v', grad_tau, 0) for the solve's backward
//                 and, in place, the step's direct part of slab t's adjoints.  A quaternion's four
//                 lanes each need all four cotangent components, the old quaternion and the three
//                 rates (staged in LDS, as the forward stages the states), and so do the three
//                 lanes of its rates: every one of those seven lanes recomputes the quaternion's
//                 adjoint and keeps its own output -- one owning lane per output, no atomics.
//   combine       g[t] = step-direct + kinematics (+ the plant's kinematics, osc_plant_backward.h)
//                 + PD + cotangent of slab t, in that order; the
//                 tick-ordered sums of the target and parameter gradients; in PD mode the packed
//                 base state of slab t - 1 for the next tick's producer call.  The same launch
//                 writes what a scheduled call asks for, each behind a NULL check: tick t's
//                 grad_T into its slab, and the reference and gain adjoints from slab t's base
//                 state -- eleven outputs per env (3 + 4 + 4), one owning lane each, 176 lanes
//                 of the block.  No atomics, no LDS.
// Both move about a KB per env and are launch-latency bound, as the forward's step kernel is.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "osc_backward.h"
#include "osc_batch.h"
#include "osc_kin_device.hpp"
#include "osc_kin_model.hpp"
#include "osc_producers.h"
#include "osc_qpos.hpp"
#include "osc_rollout_backward.h"
#include "osc_rollout_internal.hpp"

namespace {

using namespace osc;   // osc_rollout_internal.hpp's geometry, helpers, joint maps and adjoints
using osc_kin::KinDev;

// the layout bindings restate (osc_amd/_lib.py OscRolloutBackwardArgs)
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_backward_args) == 208,
              "osc_rollout_backward_args layout");

// grad_T, seven osc_env_grads fields, three osc_kin_env_grads fields; with a plant
// (osc_plant_backward.h) its held grad_qfrc_applied and its own three osc_kin_env_grads fields
constexpr int kMaxAcc = 15;

static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_plant_backward) == 56,
              "osc_rollout_plant_backward layout");

// a (x) b, quaternions (w, x, y, z)
__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// The adjoint of osc_rollout.hip's quat_step, q' = normalise(q (x) d(w dt)), d = (cos(th/2),
// sin(th/2) r / th), r = w dt, th = |r|: from the cotangent g of q', gq = dL/dq and gw = dL/dw.
//   p = q (x) d, n = |p|:   gp = (g - q' (q'.g)) / n      (so gq below is orthogonal to q)
//   gq = gp (x) conj(d),    gd = conj(q) (x) gp           (the product is bilinear)
//   d_w = cos(th/2), d_v = A r with A = sin(th/2)/th:
//   gr = -A/2 gd_w r + A gd_v + B (r.gd_v) r,   B = (cos(th/2)/2 - A) / th^2,   gw = dt gr
// At th == 0 the forward takes d = (1, 0); its analytic limit is A = 1/2, B = -1/24.  B's
// numerator cancels as th -> 0, so below th = 1e-2 it is the series -1/24 + th^2/960 -
// th^4/107520 (next term th^6/1.5e7 x 1e-12: below rounding).
__device__ __forceinline__ void quat_step_adjoint(const double* q, const double* w, double dt,
                                                  const double* g, double* gq, double* gw) {
  const double r[3] = {w[0] * dt, w[1] * dt, w[2] * dt};
  const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const double th = sqrt(th2);
  double c = 1.0, A = 0.5, B = -1.0 / 24.0;
  double d[4] = {1.0, 0.0, 0.0, 0.0};
  if (th != 0.0) {
    double s;
    sincos(0.5 * th, &s, &c);
    A = s / th;
    d[0] = c;
    d[1] = s * r[0] / th;   // the forward's own expressions: p below is the forward's, bitwise
    d[2] = s * r[1] / th;
    d[3] = s * r[2] / th;
    B = th < 1e-2 ? -1.0 / 24.0 + th2 * (1.0 / 960.0 - th2 * (1.0 / 107520.0))
                  : (0.5 * c - A) / th2;
  }
  double p[4];
  quat_mul(q, d, p);
  const double n = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
  const double qn[4] = {p[0] / n, p[1] / n, p[2] / n, p[3] / n};
  const double dot = qn[0] * g[0] + qn[1] * g[1] + qn[2] * g[2] + qn[3] * g[3];
  const double gp[4] = {(g[0] - qn[0] * dot) / n, (g[1] - qn[1] * dot) / n,
                        (g[2] - qn[2] * dot) / n, (g[3] - qn[3] * dot) / n};
  const double dc[4] = {d[0], -d[1], -d[2], -d[3]};
  const double qc[4] = {q[0], -q[1], -q[2], -q[3]};
  double gd[4];
  quat_mul(gp, dc, gq);
  quat_mul(qc, gp, gd);
  const double rg = r[0] * gd[1] + r[1] * gd[2] + r[2] * gd[3];
  const double k = B * rg - 0.5 * A * gd[0];
  gw[0] = dt * (A * gd[1] + k * r[0]);
  gw[1] = dt * (A * gd[2] + k * r[1]);
  gw[2] = dt * (A * gd[3] + k * r[2]);
}

struct StepAdjArgs {
  const KinDev* K;
  int32_t nenv, nq, nv, nbody;
  double dt;
  const double* qpos;        // [nenv][nq] the step's input positions
  const double* qvel_new;    // [nenv][nv] the step's output velocities
  const int32_t* status;     // nullable
  const double* qacc;        // rows of nv at qacc_stride: the freeze rule only
  int64_t qacc_stride;
  const double* gq_new;      // nullable = zero; may alias gq
  const double* gv_new;      // nullable = zero; may alias gv
  double* gq;                // nullable
  double* gv;                // nullable
  double* gacc;              // nullable; rows at gacc_stride
  int64_t gacc_stride;
  int32_t ntail;             // columns nv .. nv + ntail of a gacc row are written too (the rollout's
  int32_t nu;                // grad_x): the first nu from gtau (NULL or a frozen env = 0), 0 after
  const double* gtau;        // [nenv][nu], nullable
};

__global__ __launch_bounds__(kBlock) void osc_rollout_step_adjoint_kernel(StepAdjArgs a) {
  __shared__ double sq[kEnvPerBlock * kMaxNq];             // the block's qpos rows (slab t)
  __shared__ double sg[kEnvPerBlock * kMaxNq];             // cotangents of the new qpos rows
  __shared__ double sv[kEnvPerBlock * OSC_KIN_MAX_DOFS];   // the new qvel rows
  __shared__ JointMaps maps;
  __shared__ int32_t sfrozen[kEnvPerBlock];
  const int tid = threadIdx.x;
  const int nq = a.nq, nv = a.nv;
  const long long e0 = static_cast<long long>(blockIdx.x) * kEnvPerBlock;
  const long long left = a.nenv - e0;
  const int ne = left < kEnvPerBlock ? static_cast<int>(left) : kEnvPerBlock;
  const double dt = a.dt;

  build_maps(a.K, a.nbody, tid, maps);
  if (tid < kEnvPerBlock)
    sfrozen[tid] = (a.status && tid < ne) ? (a.status[e0 + tid] == OSC_SOLVE_NUMERICAL ? 1 : 0) : 0;
  __syncthreads();

  for (int idx = tid; idx < ne * nv; idx += kBlock) {
    const int el = idx / nv, d = idx - el * nv;
    if (!isfinite(a.qacc[(e0 + el) * a.qacc_stride + d])) sfrozen[el] = 1;   // same 1 from any lane
    sv[idx] = a.qvel_new[e0 * nv + idx];
  }
  for (int idx = tid; idx < ne * nq; idx += kBlock) {
    sq[idx] = a.qpos[e0 * nq + idx];
    sg[idx] = a.gq_new ? a.gq_new[e0 * nq + idx] : 0.0;
  }
  __syncthreads();   // from here gq_new is in LDS: gq may alias it

  // v' = g_v + (d qpos' / d qvel')' g_q;  grad_qvel = v',  grad_qacc = dt v'
  for (int idx = tid; idx < ne * nv; idx += kBlock) {
    const int el = idx / nv, d = idx - el * nv;
    const long long g = e0 * nv + idx;
    double vb = a.gv_new ? a.gv_new[g] : 0.0;
    const bool live = !sfrozen[el];
    if (live) {
      const int comp = maps.dcomp[d], co = maps.dcoord[d];
      if (comp < 0) {
        vb = fma(dt, sg[el * nq + co], vb);
      } else {
        double gq4[4], gw[3];
        quat_step_adjoint(sq + el * nq + co, sv + el * nv + (d - comp), dt, sg + el * nq + co, gq4,
                          gw);
        vb += comp == 0 ? gw[0] : comp == 1 ? gw[1] : gw[2];
      }
    }
    if (a.gv) a.gv[g] = vb;
    if (a.gacc) a.gacc[(e0 + el) * a.gacc_stride + d] = live ? dt * vb : 0.0;
  }
  if (a.gacc)
    for (int idx = tid; idx < ne * a.ntail; idx += kBlock) {
      const int el = idx / a.ntail, j = idx - el * a.ntail;
      double v = 0.0;
      if (j < a.nu && a.gtau && !sfrozen[el]) v = a.gtau[(e0 + el) * a.nu + j];
      a.gacc[(e0 + el) * a.gacc_stride + nv + j] = v;
    }
  // grad_qpos = (d qpos' / d qpos)' g_q
  if (a.gq)
    for (int idx = tid; idx < ne * nq; idx += kBlock) {
      const int el = idx / nq, i = idx - el * nq;
      double gi = sg[idx];
      const int comp = maps.ccomp[i];
      if (comp >= 0 && !sfrozen[el]) {
        double gq4[4], gw[3];
        quat_step_adjoint(sq + el * nq + (i - comp), sv + el * nv + maps.cdof[i], dt,
                          sg + el * nq + (i - comp), gq4, gw);
        gi = comp == 0 ? gq4[0] : comp == 1 ? gq4[1] : comp == 2 ? gq4[2] : gq4[3];
      }
      a.gq[e0 * nq + idx] = gi;
    }
}

struct CombineAcc {
  double* acc;         // [nenv][cnt] the running sum
  const double* src;   // [nenv][cnt] this tick's term
  int32_t cnt;
};

struct CombineArgs {
  int32_t nenv, nq, nv, ns;
  double* gq;                 // [nenv][nq] in: the step's direct part; out: slab t's adjoint
  double* gv;
  const double* kq;           // the kinematics' backward's grad_qpos / grad_qvel
  const double* kv;
  const double* kq2;          // the PLANT's kinematics' backward's (osc_plant_backward.h), nullable
  const double* kv2;
  const double* hq;           // slab t of grad_qpos_hist / grad_qvel_hist, nullable
  const double* hv;
  const double* gT;           // this tick's grad_T [nenv][ns][6]; NULL = not formed
  int32_t pd;                 // PD mode: gT reaches the base coordinates
  const double* pos_ref;      // PD mode: tick t's references
  int32_t pos_ref_stride;
  const double* quat_ref;
  int32_t quat_ref_stride;
  double kp_lin, kd_lin, kp_ang, kd_ang;
  const double* pack_qpos;    // PD mode, t > 0: slab t - 1, packed for the producer; else NULL
  const double* pack_qvel;
  double* bpos;
  double* bquat;
  double* blin;
  double* bang;
  int32_t nacc;
  CombineAcc acc[kMaxAcc];
  // ---- the schedule's outputs (osc_rollout_schedule_grads), all NULL for the plain entry ----
  double* gT_slab;            // grad_T_seq[t], nullable
  const double* qpos;         // slab t of qpos_hist / qvel_hist: the producer's base state
  const double* qvel;
  double* gpos_ref;           // [nenv][3]; nullable
  double* gquat_ref;          // [nenv][4]; nullable
  double* ggains;             // [nenv][4]; nullable: always added to
  int32_t pos_ref_add;        // 1: gpos_ref is a running sum (a held reference); 0: this tick's slab
  int32_t quat_ref_add;       // likewise gquat_ref
};

__global__ __launch_bounds__(kBlock) void osc_rollout_combine_kernel(CombineArgs a) {
  const int tid = threadIdx.x;
  const int nq = a.nq, nv = a.nv;
  const long long e0 = static_cast<long long>(blockIdx.x) * kEnvPerBlock;
  const long long left = a.nenv - e0;
  const int ne = left < kEnvPerBlock ? static_cast<int>(left) : kEnvPerBlock;
  const long long trow = 6LL * a.ns;
  const bool pd = a.pd != 0;

  // ---- slab t's state adjoints, the tick-ordered sums, the next tick's packed base state ----
  for (int idx = tid; idx < ne * nq; idx += kBlock) {
    const int el = idx / nq, i = idx - el * nq;
    const long long g = e0 * nq + idx, e = e0 + el;
    double v = a.gq[g] + a.kq[g];
    if (a.kq2) v += a.kq2[g];
    if (pd && i < 7) {   // free root: qpos[0:3] position, qpos[3:7] quaternion
      const double* t = a.gT + e * trow;
      if (i < 3) {
        v += -a.kp_lin * t[i];
      } else {
        const double ga[3] = {a.kp_ang * t[3], a.kp_ang * t[4], a.kp_ang * t[5]};
        v += pd_quat_adjoint(a.quat_ref + e * a.quat_ref_stride, ga, i - 3);
      }
    }
    if (a.hq) v += a.hq[g];
    a.gq[g] = v;
    if (a.pack_qpos && i < 7) {
      const double s = a.pack_qpos[g];
      if (i < 3) a.bpos[e * 3 + i] = s;
      else a.bquat[e * 4 + (i - 3)] = s;
    }
  }
  for (int idx = tid; idx < ne * nv; idx += kBlock) {
    const int el = idx / nv, d = idx - el * nv;
    const long long g = e0 * nv + idx, e = e0 + el;
    double v = a.gv[g] + a.kv[g];
    if (a.kv2) v += a.kv2[g];
    if (pd && d < 6) v += -(d < 3 ? a.kd_lin : a.kd_ang) * a.gT[e * trow + d];
    if (a.hv) v += a.hv[g];
    a.gv[g] = v;
    if (a.pack_qvel && d < 6) {
      const double s = a.pack_qvel[g];
      if (d < 3) a.blin[e * 3 + d] = s;
      else a.bang[e * 3 + (d - 3)] = s;
    }
  }
  for (int k = 0; k < a.nacc; ++k) {
    const long long cnt = a.acc[k].cnt, base = e0 * cnt;
    for (long long idx = tid; idx < ne * cnt; idx += kBlock)
      a.acc[k].acc[base + idx] += a.acc[k].src[base + idx];
  }

  // ---- the schedule's: tick t's grad_T, stored; the reference and gain adjoints ----
  // (they read gT, the history slab and the references only: nothing written above)
  if (a.gT_slab)
    for (long long idx = tid; idx < ne * trow; idx += kBlock)
      a.gT_slab[e0 * trow + idx] = a.gT[e0 * trow + idx];
  if ((a.gpos_ref || a.gquat_ref || a.ggains) && tid < ne * kParamOut) {
    const int el = tid / kParamOut, j = tid - el * kParamOut;
    const long long e = e0 + el;
    double* out = j < 3 ? a.gpos_ref : j < 7 ? a.gquat_ref : a.ggains;
    if (out) {
      const double* q = a.qpos + e * nq;
      const double* v = a.qvel + e * nv;
      const double r = pd_param_adjoint(j, a.gT + e * trow, q, q + 3, v, v + 3,
                                        a.pos_ref + e * a.pos_ref_stride,
                                        a.quat_ref + e * a.quat_ref_stride, a.kp_lin, a.kp_ang);
      if (j < 3) {
        if (a.pos_ref_add) out[e * 3 + j] += r;
        else out[e * 3 + j] = r;
      } else if (j < 7) {
        if (a.quat_ref_add) out[e * 4 + (j - 3)] += r;
        else out[e * 4 + (j - 3)] = r;
      } else {
        out[e * 4 + (j - 7)] += r;
      }
    }
  }
}

// The plant's cotangents into the solve's (osc_plant_backward.h, step 7), one flat launch: per env
// grad_Jc onto the contact rows [r0, r0 + nz) of gJ and, when the plant shares the controller's
// parameters (gMp non-NULL), grad_M_p onto gM and grad_C_p onto gC.  One owning thread per entry.
__global__ __launch_bounds__(kBlock) void osc_rollout_plant_route_kernel(
    long long nenv, int nv, int srows, int r0, int nz, const double* __restrict__ gJc,
    double* __restrict__ gJ, const double* __restrict__ gMp, double* __restrict__ gM,
    const double* __restrict__ gCp, double* __restrict__ gC) {
  const long long nj = static_cast<long long>(nz) * nv, nm = static_cast<long long>(nv) * nv;
  const long long per = nj + (gMp ? nm + nv : 0), total = nenv * per;
  for (long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * kBlock) {
    const long long e = idx / per;
    long long r = idx - e * per;
    if (r < nj) {
      gJ[e * srows * nv + static_cast<long long>(r0) * nv + r] += gJc[e * nj + r];
    } else if ((r -= nj) < nm) {
      gM[e * nm + r] += gMp[e * nm + r];
    } else {
      r -= nm;
      gC[e * nv + r] += gCp[e * nv + r];
    }
  }
}

// the base state of one history slab, packed for osc_pd_base_targets (the last tick's; every
// other tick's is packed by the combine kernel of the tick after it)
__global__ __launch_bounds__(kBlock) void osc_rollout_pack_base_kernel(
    int nenv, int nq, int nv, const double* __restrict__ qpos, const double* __restrict__ qvel,
    double* __restrict__ bpos, double* __restrict__ bquat, double* __restrict__ blin,
    double* __restrict__ bang) {
  const long long total = static_cast<long long>(nenv) * 13;
  for (long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
       idx += static_cast<long long>(gridDim.x) * kBlock) {
    const long long e = idx / 13;
    const int i = static_cast<int>(idx - e * 13);
    if (i < 3) bpos[e * 3 + i] = qpos[e * nq + i];
    else if (i < 7) bquat[e * 4 + (i - 3)] = qpos[e * nq + i];
    else if (i < 10) blin[e * 3 + (i - 7)] = qvel[e * nv + (i - 7)];
    else bang[e * 3 + (i - 10)] = qvel[e * nv + (i - 7)];
  }
}

__global__ __launch_bounds__(kBlock) void osc_pd_base_targets_backward_kernel(
    int nenv, int ns, const double* __restrict__ quat_ref, int quat_ref_stride, double kp_lin,
    double kd_lin, double kp_ang, double kd_ang, const double* __restrict__ gT,
    double* __restrict__ gpos, double* __restrict__ gquat, double* __restrict__ glin,
    double* __restrict__ gang) {
  for (long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; e < nenv;
       e += static_cast<long long>(gridDim.x) * kBlock) {
    const double* t = gT + e * 6 * ns;
    const double ga[3] = {kp_ang * t[3], kp_ang * t[4], kp_ang * t[5]};
    for (int i = 0; i < 3; ++i) {
      if (gpos) gpos[e * 3 + i] = -kp_lin * t[i];
      if (glin) glin[e * 3 + i] = -kd_lin * t[i];
      if (gang) gang[e * 3 + i] = -kd_ang * t[3 + i];
    }
    if (gquat)
      for (int i = 0; i < 4; ++i)
        gquat[e * 4 + i] = pd_quat_adjoint(quat_ref + e * quat_ref_stride, ga, i);
  }
}

int launch_step_adjoint(const StepAdjArgs& a, hipStream_t s) {
  if (a.nq > kMaxNq || a.nv > OSC_KIN_MAX_DOFS || a.nbody > OSC_KIN_MAX_BODIES)
    return OSC_ERR_INVALID_ARGUMENT;   // the kernel's LDS rows (build_tables cannot produce these)
  hipLaunchKernelGGL(osc_rollout_step_adjoint_kernel, dim3(env_blocks(a.nenv)), dim3(kBlock), 0, s,
                     a);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

constexpr int kEnvFields = 7, kKinFields = 3;
static_assert(1 + kEnvFields + kKinFields + 1 + kKinFields <= kMaxAcc,
              "CombineArgs holds every running sum");

struct BackwardWorkspace {   // sections, each 256-B aligned (byte offsets)
  size_t M, C, J, b, T, x, y, tau, status, gx, gM, gC, gJ, gb, gT, gq, gv, kq, kv, bpos, bquat,
      blin, bang, eg[kEnvFields], kg[kKinFields], qp, qp_bytes, total;
  size_t eg_cnt[kEnvFields], kg_cnt[kKinFields];
  int rc;
  BackwardWorkspace(const osc_model* model, const osc_kin_model* kin, const osc_model_desc& d,
                    int32_t nenv) {
    const KinDev& k = kin->host;
    const size_t n = static_cast<size_t>(nenv), dbl = sizeof(double);
    const size_t nv = d.nv, s6 = 6 * static_cast<size_t>(d.ns), nx = nv + d.nu + 3 * d.nc;
    int32_t rows = 0;
    rc = osc_dual_rows(model, &rows);
    size_t off = 0;
    auto take = [&](size_t bytes) {
      const size_t at = off;
      off += align256(bytes);
      return at;
    };
    M = take(dbl * n * nv * nv);
    C = take(dbl * n * nv);
    J = take(dbl * n * s6 * nv);
    b = take(dbl * n * s6);
    T = take(dbl * n * s6);
    x = take(dbl * n * nx);
    y = take(dbl * n * static_cast<size_t>(rows));
    tau = take(dbl * n * d.nu);
    status = take(sizeof(int32_t) * n);
    gx = take(dbl * n * nx);
    gM = take(dbl * n * nv * nv);
    gC = take(dbl * n * nv);
    gJ = take(dbl * n * s6 * nv);
    gb = take(dbl * n * s6);
    gT = take(dbl * n * s6);
    gq = take(dbl * n * k.nq);
    gv = take(dbl * n * nv);
    kq = take(dbl * n * k.nq);
    kv = take(dbl * n * nv);
    bpos = take(dbl * n * 3);
    bquat = take(dbl * n * 4);
    blin = take(dbl * n * 3);
    bang = take(dbl * n * 3);
    // osc_env_grads' fields in order: mu, u_lb, u_ub, fz_lb, fz_ub, w_pos, w_rot
    const size_t ec[kEnvFields] = {1, static_cast<size_t>(d.nu), static_cast<size_t>(d.nu), 1, 1,
                                   static_cast<size_t>(d.ns), static_cast<size_t>(d.ns)};
    for (int i = 0; i < kEnvFields; ++i) {
      eg_cnt[i] = ec[i];
      eg[i] = take(dbl * n * ec[i]);
    }
    // osc_kin_env_grads': mass_scale, com_offset, armature_scale
    const size_t kc[kKinFields] = {static_cast<size_t>(k.nbody), 3 * static_cast<size_t>(k.nbody),
                                   nv};
    for (int i = 0; i < kKinFields; ++i) {
      kg_cnt[i] = kc[i];
      kg[i] = take(dbl * n * kc[i]);
    }
    qp = off;
    qp_bytes = 0;
    if (rc == OSC_OK) rc = osc_workspace_bytes(model, nenv, &qp_bytes);
    total = qp + align256(qp_bytes);
  }
};

// The plant's sections behind the backward's own (include/osc_plant_backward.h), each 256-B
// aligned: the plant's M_p | C_p, the recomputed qacc, the step's grad_qacc, the forward dynamics'
// grad_M_p | grad_C_p | grad_Jc | grad_qfrc, the plant's kinematics' state adjoints and one tick's
// plant parameter gradients.
struct PlantBackwardWorkspace {
  size_t mp, cp, qacc, gacc, gmp, gcp, gjc, gf, kq, kv, kg[kKinFields], total;
  PlantBackwardWorkspace(const BackwardWorkspace& L, const KinDev& k, const osc_model_desc& d,
                         int32_t nenv) {
    const size_t n = static_cast<size_t>(nenv), dbl = sizeof(double), nv = d.nv;
    size_t off = L.total;
    auto take = [&](size_t bytes) {
      const size_t at = off;
      off += align256(bytes);
      return at;
    };
    mp = take(dbl * n * nv * nv);
    cp = take(dbl * n * nv);
    qacc = take(dbl * n * nv);
    gacc = take(dbl * n * nv);
    gmp = take(dbl * n * nv * nv);
    gcp = take(dbl * n * nv);
    gjc = take(dbl * n * 3 * d.nc * nv);
    gf = take(dbl * n * nv);
    kq = take(dbl * n * k.nq);
    kv = take(dbl * n * nv);
    for (int i = 0; i < kKinFields; ++i) kg[i] = take(dbl * n * L.kg_cnt[i]);
    total = off;
  }
};

}  // namespace

extern "C" int osc_batch_integrate_backward(const osc_kin_model* kin, int32_t nenv, double dt,
                                            const double* qpos, const double* qvel_new,
                                            const int32_t* status, const double* qacc,
                                            int64_t qacc_stride, const double* grad_qpos_new,
                                            const double* grad_qvel_new, double* grad_qpos,
                                            double* grad_qvel, double* grad_qacc,
                                            int64_t grad_qacc_stride, void* stream) {
  if (!kin || nenv < 0 || !std::isfinite(dt)) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_qpos && !grad_qvel && !grad_qacc) return OSC_ERR_INVALID_ARGUMENT;
  for (const void* p : {static_cast<const void*>(qpos), static_cast<const void*>(qvel_new),
                        static_cast<const void*>(qacc), static_cast<const void*>(grad_qpos_new),
                        static_cast<const void*>(grad_qvel_new),
                        static_cast<const void*>(grad_qpos), static_cast<const void*>(grad_qvel),
                        static_cast<const void*>(grad_qacc)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(status) & 3u) != 0) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  if (!qpos || !qvel_new || !qacc || qacc_stride < kin->host.nv) return OSC_ERR_INVALID_ARGUMENT;
  if (grad_qacc && grad_qacc_stride < kin->host.nv) return OSC_ERR_INVALID_ARGUMENT;
  StepAdjArgs a{};
  a.K = kin->dev;
  a.nenv = nenv;
  a.nq = kin->host.nq;
  a.nv = kin->host.nv;
  a.nbody = kin->host.nbody;
  a.dt = dt;
  a.qpos = qpos;
  a.qvel_new = qvel_new;
  a.status = status;
  a.qacc = qacc;
  a.qacc_stride = qacc_stride;
  a.gq_new = grad_qpos_new;
  a.gv_new = grad_qvel_new;
  a.gq = grad_qpos;
  a.gv = grad_qvel;
  a.gacc = grad_qacc;
  a.gacc_stride = grad_qacc_stride;
  return launch_step_adjoint(a, static_cast<hipStream_t>(stream));
}

extern "C" int osc_pd_base_targets_backward(int32_t nenv, int32_t ns, const double* base_quat,
                                            const double* quat_ref, int32_t quat_ref_per_env,
                                            const double* gains, const double* grad_targets,
                                            double* grad_base_pos, double* grad_base_quat,
                                            double* grad_lin_vel, double* grad_ang_vel,
                                            void* stream) {
  if (nenv < 0 || ns < 1 || !gains) return OSC_ERR_INVALID_ARGUMENT;
  if (!grad_base_pos && !grad_base_quat && !grad_lin_vel && !grad_ang_vel)
    return OSC_ERR_INVALID_ARGUMENT;
  for (const void* p : {static_cast<const void*>(base_quat), static_cast<const void*>(quat_ref),
                        static_cast<const void*>(grad_targets),
                        static_cast<const void*>(grad_base_pos),
                        static_cast<const void*>(grad_base_quat),
                        static_cast<const void*>(grad_lin_vel),
                        static_cast<const void*>(grad_ang_vel)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  if (!quat_ref || !grad_targets) return OSC_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(osc_pd_base_targets_backward_kernel, dim3(grid_for(nenv)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), nenv, ns, quat_ref,
                     quat_ref_per_env ? 4 : 0, gains[0], gains[1], gains[2], gains[3], grad_targets,
                     grad_base_pos, grad_base_quat, grad_lin_vel, grad_ang_vel);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

extern "C" int osc_rollout_backward_workspace_bytes(const osc_model* model,
                                                    const osc_kin_model* kin, int32_t nenv,
                                                    size_t* bytes) {
  if (!bytes || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  osc_model_desc d;
  const int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  const BackwardWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  *bytes = L.total;
  return OSC_OK;
}

extern "C" int osc_batch_rollout_backward(const osc_model* model, const osc_kin_model* kin,
                                          int32_t nenv, const osc_rollout_backward_args* args,
                                          const osc_env_params* ep, const osc_kin_env_params* kp,
                                          void* stream) {
  return osc::rollout_backward_run(model, kin, nenv, args, nullptr, nullptr, ep, kp, nullptr,
                                   stream);
}

// ---- the backward pass through a plant (include/osc_plant_backward.h) ----

extern "C" int osc_rollout_plant_backward_workspace_bytes(const osc_model* model,
                                                          const osc_kin_model* kin, int32_t nenv,
                                                          size_t* bytes) {
  if (!bytes || nenv < 0) return OSC_ERR_INVALID_ARGUMENT;
  osc_model_desc d;
  const int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  const BackwardWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  *bytes = PlantBackwardWorkspace(L, kin->host, d, nenv).total;
  return OSC_OK;
}

extern "C" int osc_batch_rollout_plant_backward(
    const osc_model* model, const osc_kin_model* kin, int32_t nenv,
    const osc_rollout_backward_args* args, const osc_rollout_schedule* sched,
    const osc_rollout_schedule_grads* sched_grads, const osc_env_params* env_params,
    const osc_kin_env_params* kin_params, const osc_rollout_plant_backward* plant, void* stream) {
  return osc::rollout_backward_run(model, kin, nenv, args, sched, sched_grads, env_params,
                                   kin_params, plant, stream);
}

// osc_batch_rollout_backward (sched and sgrads NULL) and osc_batch_rollout_backward_sched
// (osc_rollout_schedule.h): the recompute of tick t on the schedule's slabs, and the schedule's
// gradients out of the same combine launch
int osc::rollout_backward_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                              const osc_rollout_backward_args* args,
                              const osc_rollout_schedule* sched,
                              const osc_rollout_schedule_grads* sgrads, const osc_env_params* ep,
                              const osc_kin_env_params* kp,
                              const osc_rollout_plant_backward* plant, void* stream) {
  // ---- every check before the first launch ----
  osc_model_desc d;
  int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  if (!args || nenv < 0 || args->nticks < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (!(args->dt > 0.0) || !std::isfinite(args->dt)) return OSC_ERR_INVALID_ARGUMENT;
  const bool pd = args->target_mode == OSC_ROLLOUT_TARGETS_PD_BASE;
  if (!pd && args->target_mode != OSC_ROLLOUT_TARGETS_HELD) return OSC_ERR_INVALID_ARGUMENT;
  const KinDev& k = kin->host;
  if (pd && (k.jtype[0] != OSC_KIN_JOINT_FREE || k.parent[0] != -1))
    return OSC_ERR_INVALID_ARGUMENT;
  // which parameter gradients are asked for
  double* eg_out[kEnvFields] = {};
  double* kg_out[kKinFields] = {};
  bool any_eg = false, any_kg = false;
  if (args->env_grads) {
    const osc_env_grads& g = *args->env_grads;
    double* f[kEnvFields] = {g.mu, g.u_lb, g.u_ub, g.fz_lb, g.fz_ub, g.w_pos, g.w_rot};
    for (int i = 0; i < kEnvFields; ++i) {
      eg_out[i] = f[i];
      any_eg = any_eg || f[i] != nullptr;
      if (!aligned8(f[i])) return OSC_ERR_INVALID_ARGUMENT;
    }
  }
  if (args->kin_grads) {
    const osc_kin_env_grads& g = *args->kin_grads;
    double* f[kKinFields] = {g.mass_scale, g.com_offset, g.armature_scale};
    for (int i = 0; i < kKinFields; ++i) {
      kg_out[i] = f[i];
      any_kg = any_kg || f[i] != nullptr;
      if (!aligned8(f[i])) return OSC_ERR_INVALID_ARGUMENT;
    }
  }
  const bool env_bwd = ep != nullptr || any_eg;   // the solve's backward with per-env parameters
  if (env_bwd) {
    const osc_env_params none{};
    if (!osc::env_tick_ok(model, ep ? ep : &none, nullptr)) return OSC_ERR_INVALID_ARGUMENT;
  }
  if (kp != nullptr)
    for (const double* a : {kp->mass_scale, kp->com_offset, kp->armature_scale})
      if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
  if (pd && args->grad_T) return OSC_ERR_INVALID_ARGUMENT;
  const osc_rollout_schedule sc = sched ? *sched : osc_rollout_schedule{};
  const osc_rollout_schedule_grads sg = sgrads ? *sgrads : osc_rollout_schedule_grads{};
  const bool any_sg = sg.grad_T_seq || sg.grad_pos_ref || sg.grad_quat_ref ||
                      sg.grad_pos_ref_seq || sg.grad_quat_ref_seq || sg.grad_gains;
  if (!pd && (sc.pos_ref_seq || sc.quat_ref_seq || sg.grad_pos_ref || sg.grad_quat_ref ||
              sg.grad_pos_ref_seq || sg.grad_quat_ref_seq || sg.grad_gains))
    return OSC_ERR_INVALID_ARGUMENT;
  if ((sg.grad_pos_ref_seq && !sc.pos_ref_seq) || (sg.grad_quat_ref_seq && !sc.quat_ref_seq) ||
      (sg.grad_pos_ref && sc.pos_ref_seq) || (sg.grad_quat_ref && sc.quat_ref_seq))
    return OSC_ERR_INVALID_ARGUMENT;
  for (const void* p :
       {static_cast<const void*>(sc.T_seq), static_cast<const void*>(sc.mask_seq),
        static_cast<const void*>(sc.pos_ref_seq), static_cast<const void*>(sc.quat_ref_seq),
        static_cast<const void*>(sg.grad_T_seq), static_cast<const void*>(sg.grad_pos_ref),
        static_cast<const void*>(sg.grad_quat_ref), static_cast<const void*>(sg.grad_pos_ref_seq),
        static_cast<const void*>(sg.grad_quat_ref_seq), static_cast<const void*>(sg.grad_gains)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  // ---- the plant (osc_plant_backward.h): NULL = every branch below takes its old side ----
  const bool with_plant = plant != nullptr;
  const osc_kin_env_params* pkp = with_plant ? plant->kin_params : nullptr;
  const bool plant_kin =
      pkp != nullptr && (pkp->mass_scale || pkp->com_offset || pkp->armature_scale);
  double* pkg_out[kKinFields] = {};
  bool any_pkg = false;
  if (with_plant) {
    for (const void* p : {static_cast<const void*>(plant->qfrc_applied),
                          static_cast<const void*>(plant->qfrc_applied_seq),
                          static_cast<const void*>(plant->grad_qacc_hist),
                          static_cast<const void*>(plant->grad_qfrc_applied),
                          static_cast<const void*>(plant->grad_qfrc_applied_seq)})
      if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
    if (pkp != nullptr)
      for (const double* a : {pkp->mass_scale, pkp->com_offset, pkp->armature_scale})
        if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
    if (plant->kin_grads) {
      const osc_kin_env_grads& g = *plant->kin_grads;
      double* f[kKinFields] = {g.mass_scale, g.com_offset, g.armature_scale};
      for (int i = 0; i < kKinFields; ++i) {
        pkg_out[i] = f[i];
        any_pkg = any_pkg || f[i] != nullptr;
        if (!aligned8(f[i])) return OSC_ERR_INVALID_ARGUMENT;
      }
    }
    if (any_pkg && !plant_kin) return OSC_ERR_INVALID_ARGUMENT;
    if (plant->grad_qfrc_applied && plant->qfrc_applied_seq) return OSC_ERR_INVALID_ARGUMENT;
    if (plant->grad_qfrc_applied_seq && !plant->qfrc_applied_seq) return OSC_ERR_INVALID_ARGUMENT;
    // (the forward dynamics and its backward refuse a model with wheel rows: check_handles did)
  }
  const bool any_pl =
      with_plant && (plant->grad_qfrc_applied || plant->grad_qfrc_applied_seq || any_pkg);
  if (!args->grad_qpos0 && !args->grad_qvel0 && !args->grad_T && !any_eg && !any_kg && !any_sg &&
      !any_pl)
    return OSC_ERR_INVALID_ARGUMENT;
  for (const void* p :
       {static_cast<const void*>(args->T), static_cast<const void*>(args->pos_ref),
        static_cast<const void*>(args->quat_ref), static_cast<const void*>(args->contact_mask),
        static_cast<const void*>(args->qpos_hist), static_cast<const void*>(args->qvel_hist),
        static_cast<const void*>(args->grad_qpos_hist),
        static_cast<const void*>(args->grad_qvel_hist),
        static_cast<const void*>(args->grad_tau_hist), static_cast<const void*>(args->grad_qpos0),
        static_cast<const void*>(args->grad_qvel0), static_cast<const void*>(args->grad_T)})
    if (!aligned8(p)) return OSC_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(args->status_hist) & 3u) != 0) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  const int32_t nticks = args->nticks;
  const HeldInputs held{pd, args->T, args->contact_mask, args->pos_ref, args->pos_ref_per_env,
                        args->quat_ref, args->quat_ref_per_env, args->gains};
  if (!tick_inputs_present(held, sched, nticks, d.nc)) return OSC_ERR_INVALID_ARGUMENT;
  if (nticks > 0 && (!args->qpos_hist || !args->qvel_hist || !args->status_hist))
    return OSC_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(args->workspace) & 15u) != 0) return OSC_ERR_INVALID_ARGUMENT;
  const BackwardWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  const PlantBackwardWorkspace LP(L, k, d, nenv);   // (offsets only; used with a plant alone)
  const size_t ws_total = with_plant ? LP.total : L.total;
  if (args->workspace && args->workspace_bytes < ws_total) return OSC_ERR_INVALID_ARGUMENT;
  if (k.nq > kMaxNq || k.nv > OSC_KIN_MAX_DOFS || k.nbody > OSC_KIN_MAX_BODIES)
    return OSC_ERR_INVALID_ARGUMENT;

  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(nenv), dbl = sizeof(double);
  const size_t nq = k.nq, nv = k.nv, nu = d.nu, s6 = 6 * static_cast<size_t>(d.ns);
  const size_t nx = nv + nu + 3 * static_cast<size_t>(d.nc);
  auto ok = [](hipError_t e) { return e == hipSuccess ? OSC_OK : OSC_ERR_DEVICE; };

  // the sums start from zero; with no tick they are the result
  if (args->grad_T) rc = ok(hipMemsetAsync(args->grad_T, 0, dbl * n * s6, s));
  for (int i = 0; i < kEnvFields && rc == OSC_OK; ++i)
    if (eg_out[i]) rc = ok(hipMemsetAsync(eg_out[i], 0, dbl * n * L.eg_cnt[i], s));
  for (int i = 0; i < kKinFields && rc == OSC_OK; ++i)
    if (kg_out[i]) rc = ok(hipMemsetAsync(kg_out[i], 0, dbl * n * L.kg_cnt[i], s));
  if (rc == OSC_OK && sg.grad_pos_ref) rc = ok(hipMemsetAsync(sg.grad_pos_ref, 0, dbl * n * 3, s));
  if (rc == OSC_OK && sg.grad_quat_ref) rc = ok(hipMemsetAsync(sg.grad_quat_ref, 0, dbl * n * 4, s));
  if (rc == OSC_OK && sg.grad_gains) rc = ok(hipMemsetAsync(sg.grad_gains, 0, dbl * n * 4, s));
  if (rc == OSC_OK && with_plant && plant->grad_qfrc_applied)
    rc = ok(hipMemsetAsync(plant->grad_qfrc_applied, 0, dbl * n * nv, s));
  for (int i = 0; i < kKinFields && rc == OSC_OK; ++i)
    if (pkg_out[i]) rc = ok(hipMemsetAsync(pkg_out[i], 0, dbl * n * L.kg_cnt[i], s));
  if (rc != OSC_OK) return rc;

  auto seed = [&](double* out, const double* hist, size_t row) {   // slab nticks' cotangent
    if (!out) return OSC_OK;
    if (hist)
      return ok(hipMemcpyAsync(out, hist + n * row * nticks, dbl * n * row,
                               hipMemcpyDeviceToDevice, s));
    return ok(hipMemsetAsync(out, 0, dbl * n * row, s));
  };
  if (nticks == 0) {
    rc = seed(args->grad_qpos0, args->grad_qpos_hist, nq);
    if (rc == OSC_OK) rc = seed(args->grad_qvel0, args->grad_qvel_hist, nv);
    return rc;
  }

  char* base = static_cast<char*>(args->workspace);
  bool owned = false;
  if (base == nullptr) {
    if (hipMallocAsync(reinterpret_cast<void**>(&base), ws_total, s) != hipSuccess)
      return OSC_ERR_DEVICE;
    owned = true;
  }
  auto dptr = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  double *M = dptr(L.M), *C = dptr(L.C), *J = dptr(L.J), *b = dptr(L.b), *x = dptr(L.x);
  double *gq = dptr(L.gq), *gv = dptr(L.gv);
  int32_t* status = reinterpret_cast<int32_t*>(base + L.status);
  const bool want_gT = pd || args->grad_T != nullptr || sg.grad_T_seq != nullptr;

  // this tick's parameter gradients land in the workspace, the combine kernel adds them on
  osc_env_grads eg_tick{};
  osc_kin_env_grads kg_tick{};
  {
    double** ef[kEnvFields] = {&eg_tick.mu, &eg_tick.u_lb, &eg_tick.u_ub, &eg_tick.fz_lb,
                               &eg_tick.fz_ub, &eg_tick.w_pos, &eg_tick.w_rot};
    for (int i = 0; i < kEnvFields; ++i) *ef[i] = eg_out[i] ? dptr(L.eg[i]) : nullptr;
    double** kf[kKinFields] = {&kg_tick.mass_scale, &kg_tick.com_offset, &kg_tick.armature_scale};
    for (int i = 0; i < kKinFields; ++i) *kf[i] = kg_out[i] ? dptr(L.kg[i]) : nullptr;
  }
  osc_kin_env_grads pkg_tick{};   // the plant's
  {
    double** kf[kKinFields] = {&pkg_tick.mass_scale, &pkg_tick.com_offset,
                               &pkg_tick.armature_scale};
    for (int i = 0; i < kKinFields; ++i) *kf[i] = pkg_out[i] ? dptr(LP.kg[i]) : nullptr;
  }

  rc = seed(gq, args->grad_qpos_hist, nq);
  if (rc == OSC_OK) rc = seed(gv, args->grad_qvel_hist, nv);
  if (rc == OSC_OK && pd) {   // the last tick's base state
    hipLaunchKernelGGL(osc_rollout_pack_base_kernel, dim3(grid_for(13LL * nenv)), dim3(kBlock), 0,
                       s, nenv, static_cast<int>(nq), static_cast<int>(nv),
                       args->qpos_hist + n * nq * (nticks - 1),
                       args->qvel_hist + n * nv * (nticks - 1), dptr(L.bpos), dptr(L.bquat),
                       dptr(L.blin), dptr(L.bang));
    rc = ok(hipGetLastError());
  }

  for (int32_t t = nticks - 1; t >= 0 && rc == OSC_OK; --t) {
    const double* qpos = args->qpos_hist + n * nq * t;
    const double* qvel = args->qvel_hist + n * nv * t;
    // ---- recompute the tick from slab t: kinematics, targets, the cold solve with duals ----
    rc = kp ? osc_batch_kinematics_env(kin, nenv, qpos, qvel, kp, M, C, J, b, nullptr, stream)
            : osc_batch_kinematics(kin, nenv, qpos, qvel, M, C, J, b, nullptr, stream);
    if (rc != OSC_OK) break;
    TickInputs in;
    rc = tick_inputs(held, sc, t, nenv, d, dptr(L.bpos), dptr(L.bquat), dptr(L.blin), dptr(L.bang),
                     dptr(L.T), stream, &in);
    if (rc != OSC_OK) break;
    const double* T = in.T;
    const double* mask = in.mask;
    osc_solve_extras ex{};
    ex.y = dptr(L.y);
    rc = ep ? osc_batch_solve_env(model, nenv, M, C, J, b, T, mask, ep, &ex,
                                  dptr(L.tau), x, status, nullptr, base + L.qp, L.qp_bytes, stream)
            : osc_batch_solve_ex(model, nenv, M, C, J, b, T, mask, &ex, dptr(L.tau),
                                 x, status, nullptr, base + L.qp, L.qp_bytes, stream);
    if (rc != OSC_OK) break;
    // ---- with a plant: its M_p, C_p (its own parameters) or the tick's, then its qacc ----
    const double* Mp = M;
    if (with_plant) {
      const double* Cp = C;
      if (plant_kin) {
        // (the kernel wants J and b too; they land in the gJ / gb sections, which the solve's
        // backward overwrites later, so that an env with invalid PLANT parameters keeps the
        // controller's J and b for its solve's backward)
        rc = osc_batch_kinematics_env(kin, nenv, qpos, qvel, pkp, dptr(LP.mp), dptr(LP.cp),
                                      dptr(L.gJ), dptr(L.gb), nullptr, stream);
        if (rc != OSC_OK) break;
        Mp = dptr(LP.mp);
        Cp = dptr(LP.cp);
      }
      const double* qfrc = plant->qfrc_applied_seq ? plant->qfrc_applied_seq + n * nv * t
                                                   : plant->qfrc_applied;
      rc = osc_batch_forward_dynamics(model, nenv, Mp, Cp, J, x + nv, static_cast<int64_t>(nx),
                                      x + nv + nu, static_cast<int64_t>(nx), qfrc, dptr(LP.qacc),
                                      stream);
      if (rc != OSC_OK) break;
    }
    // ---- the step's adjoint: grad_x, and the direct part of slab t's adjoints in place ----
    StepAdjArgs a{};
    a.K = kin->dev;
    a.nenv = nenv;
    a.nq = k.nq;
    a.nv = k.nv;
    a.nbody = k.nbody;
    a.dt = args->dt;
    a.qpos = qpos;
    a.qvel_new = args->qvel_hist + n * nv * (t + 1);
    a.status = args->status_hist + n * t;
    a.qacc = x;   // dv = x[0:nv]
    a.qacc_stride = static_cast<int64_t>(nx);
    a.gq_new = gq;
    a.gv_new = gv;
    a.gq = gq;
    a.gv = gv;
    a.gacc = dptr(L.gx);
    a.gacc_stride = static_cast<int64_t>(nx);
    a.ntail = static_cast<int32_t>(nx - nv);
    a.nu = d.nu;
    a.gtau = args->grad_tau_hist ? args->grad_tau_hist + n * nu * t : nullptr;
    if (with_plant) {   // the step integrated qacc; grad_qacc goes to a buffer of its own, and the
      a.qacc = dptr(LP.qacc);   // forward dynamics' backward writes the whole grad_x row
      a.qacc_stride = static_cast<int64_t>(nv);
      a.gacc = dptr(LP.gacc);
      a.gacc_stride = static_cast<int64_t>(nv);
      a.ntail = 0;
      a.gtau = nullptr;
    }
    rc = launch_step_adjoint(a, s);
    if (rc != OSC_OK) break;
    if (with_plant) {
      // grad_x = (0, grad_tau_hist[t] + w[nb:], Jc w); the plant-side cotangents; w itself into
      // grad_qfrc_applied_seq[t] or the held sum's term
      FdBackwardExtras ex{};
      ex.grad_qacc_add = plant->grad_qacc_hist ? plant->grad_qacc_hist + n * nv * t : nullptr;
      ex.grad_tau = args->grad_tau_hist ? args->grad_tau_hist + n * nu * t : nullptr;
      ex.status = args->status_hist + n * t;
      ex.grad_x_dv = dptr(L.gx);
      ex.grad_x_stride = static_cast<int64_t>(nx);
      double* gf = plant->grad_qfrc_applied_seq ? plant->grad_qfrc_applied_seq + n * nv * t
                   : plant->grad_qfrc_applied   ? dptr(LP.gf)
                                                : nullptr;
      rc = forward_dynamics_backward_run(
          model, nenv, Mp, J, x + nv + nu, static_cast<int64_t>(nx), dptr(LP.qacc), dptr(LP.gacc),
          static_cast<int64_t>(nv), dptr(LP.gmp), dptr(LP.gcp), dptr(LP.gjc), dptr(L.gx) + nv,
          static_cast<int64_t>(nx), dptr(L.gx) + nv + nu, static_cast<int64_t>(nx), gf, &ex,
          stream);
      if (rc != OSC_OK) break;
    }
    // ---- the solve's backward, then the kinematics' ----
    double* gT = want_gT ? dptr(L.gT) : nullptr;
    rc = env_bwd ? osc_batch_solve_backward_env(model, nenv, M, J, b, T, mask, ep, x,
                                                dptr(L.y), status, dptr(L.gx), dptr(L.gM),
                                                dptr(L.gC), dptr(L.gJ), nullptr, gT, dptr(L.gb),
                                                any_eg ? &eg_tick : nullptr, base + L.qp,
                                                L.qp_bytes, stream)
                 : osc_batch_solve_backward_data(model, nenv, M, J, b, T, mask, x,
                                                 dptr(L.y), status, dptr(L.gx), dptr(L.gM),
                                                 dptr(L.gC), dptr(L.gJ), nullptr, gT, dptr(L.gb),
                                                 base + L.qp, L.qp_bytes, stream);
    if (rc != OSC_OK) break;
    if (with_plant) {   // the plant's cotangents onto the solve's (they were formed before it ran)
      const long long per = 3LL * d.nc * nv + (plant_kin ? 0 : nv * nv + nv);
      hipLaunchKernelGGL(osc_rollout_plant_route_kernel, dim3(grid_for(per * nenv)), dim3(kBlock),
                         0, s, static_cast<long long>(nenv), static_cast<int>(nv),
                         static_cast<int>(s6), 3 * d.ns - 3 * d.nc, 3 * d.nc, dptr(LP.gjc),
                         dptr(L.gJ), plant_kin ? nullptr : dptr(LP.gmp), dptr(L.gM),
                         plant_kin ? nullptr : dptr(LP.gcp), dptr(L.gC));
      rc = ok(hipGetLastError());
      if (rc != OSC_OK) break;
    }
    rc = osc_batch_kinematics_backward(kin, nenv, qpos, qvel, kp, dptr(L.gM), dptr(L.gC),
                                       dptr(L.gJ), dptr(L.gb), nullptr, dptr(L.kq), dptr(L.kv),
                                       any_kg ? &kg_tick : nullptr, stream);
    if (rc != OSC_OK) break;
    if (plant_kin) {   // the plant's own parameters: its state adjoints and parameter gradients
      rc = osc_batch_kinematics_backward(kin, nenv, qpos, qvel, pkp, dptr(LP.gmp), dptr(LP.gcp),
                                         nullptr, nullptr, nullptr, dptr(LP.kq), dptr(LP.kv),
                                         any_pkg ? &pkg_tick : nullptr, stream);
      if (rc != OSC_OK) break;
    }
    // ---- combine: slab t's adjoints, the tick-ordered sums, the next tick's base state ----
    // (the plain entry has no schedule gradient: sg's pointers are NULL, and so are c's)
    CombineArgs c{};
    c.nenv = nenv;
    c.nq = k.nq;
    c.nv = k.nv;
    c.ns = d.ns;
    c.gq = gq;
    c.gv = gv;
    c.kq = dptr(L.kq);
    c.kv = dptr(L.kv);
    c.hq = args->grad_qpos_hist ? args->grad_qpos_hist + n * nq * t : nullptr;
    c.hv = args->grad_qvel_hist ? args->grad_qvel_hist + n * nv * t : nullptr;
    c.gT = gT;
    if (pd) {
      c.pd = 1;
      c.pos_ref = in.pos_ref;
      c.pos_ref_stride = args->pos_ref_per_env ? 3 : 0;
      c.quat_ref = in.quat_ref;
      c.quat_ref_stride = args->quat_ref_per_env ? 4 : 0;
      c.kp_lin = args->gains[0];
      c.kd_lin = args->gains[1];
      c.kp_ang = args->gains[2];
      c.kd_ang = args->gains[3];
      if (t > 0) {
        c.pack_qpos = args->qpos_hist + n * nq * (t - 1);
        c.pack_qvel = args->qvel_hist + n * nv * (t - 1);
        c.bpos = dptr(L.bpos);
        c.bquat = dptr(L.bquat);
        c.blin = dptr(L.blin);
        c.bang = dptr(L.bang);
      }
      c.qpos = qpos;
      c.qvel = qvel;
      c.gpos_ref = sg.grad_pos_ref_seq ? sg.grad_pos_ref_seq + n * 3 * t : sg.grad_pos_ref;
      c.pos_ref_add = sg.grad_pos_ref_seq ? 0 : 1;
      c.gquat_ref = sg.grad_quat_ref_seq ? sg.grad_quat_ref_seq + n * 4 * t : sg.grad_quat_ref;
      c.quat_ref_add = sg.grad_quat_ref_seq ? 0 : 1;
      c.ggains = sg.grad_gains;
    }
    c.gT_slab = sg.grad_T_seq ? sg.grad_T_seq + n * s6 * t : nullptr;
    if (args->grad_T) c.acc[c.nacc++] = CombineAcc{args->grad_T, gT, static_cast<int32_t>(s6)};
    for (int i = 0; i < kEnvFields; ++i)
      if (eg_out[i])
        c.acc[c.nacc++] =
            CombineAcc{eg_out[i], dptr(L.eg[i]), static_cast<int32_t>(L.eg_cnt[i])};
    for (int i = 0; i < kKinFields; ++i)
      if (kg_out[i])
        c.acc[c.nacc++] =
            CombineAcc{kg_out[i], dptr(L.kg[i]), static_cast<int32_t>(L.kg_cnt[i])};
    if (plant_kin) {
      c.kq2 = dptr(LP.kq);
      c.kv2 = dptr(LP.kv);
    }
    if (with_plant && plant->grad_qfrc_applied)
      c.acc[c.nacc++] =
          CombineAcc{plant->grad_qfrc_applied, dptr(LP.gf), static_cast<int32_t>(nv)};
    for (int i = 0; i < kKinFields; ++i)
      if (pkg_out[i])
        c.acc[c.nacc++] =
            CombineAcc{pkg_out[i], dptr(LP.kg[i]), static_cast<int32_t>(L.kg_cnt[i])};
    hipLaunchKernelGGL(osc_rollout_combine_kernel, dim3(env_blocks(nenv)), dim3(kBlock), 0, s, c);
    rc = ok(hipGetLastError());
  }
  if (rc == OSC_OK && args->grad_qpos0)
    rc = ok(hipMemcpyAsync(args->grad_qpos0, gq, dbl * n * nq, hipMemcpyDeviceToDevice, s));
  if (rc == OSC_OK && args->grad_qvel0)
    rc = ok(hipMemcpyAsync(args->grad_qvel0, gv, dbl * n * nv, hipMemcpyDeviceToDevice, s));
  if (owned) (void)hipFreeAsync(base, s);
  return rc;
}
