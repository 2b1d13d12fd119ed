// osc_rollout.hip -- device-resident closed-loop rollout over the controller's own model (C-ABI in
// include/osc_rollout.h): per tick   [PD targets] -> osc_batch_solve_qpos(_warm) with x -> step,
// where the step integrates the acceleration the QP chose, dv = x[0:nv], the way MuJoCo's Euler
// step does (qvel += dt qacc, then mj_integratePos with the new velocity).  An idealised rollout,
// not a simulator: no ground, no contact detection, the contact mask held constant.
//
// The step kernel is the whole per-tick glue in ONE launch: velocity update, position update
// (quaternion joints included), freezing of envs whose solve failed, the tick's history slabs and
// the packed base state osc_pd_base_targets reads.  One env moves ~0.6 KB (Go2: nq 19, nv 18), so
// 4,096 envs are ~2.5 MB: the kernel is launch-latency bound, and several small launches between
// a ~20 us kinematics kernel and the solve would cost more than the work itself.
//
// Mapping: a 256-thread block owns 16 consecutive envs, whose qpos / qvel / history rows are
// contiguous in every env-major array, and walks them with a FLAT index over env x coordinate, so
// consecutive lanes touch consecutive doubles (qacc, read out of x, is contiguous per env row).
// The block's states pass through LDS (<= 10 KB) because two things are per env, not per
// coordinate: the freeze decision (any non-finite qacc entry) and a quaternion's update, which
// needs its four components and three rates; the four lanes of a quaternion each compute the
// rotation and store their own component.  Joint types and addresses come from the kinematics
// model's device tables (jtype, qadr, dadr), turned into the per-block JointMaps
// (osc_rollout_internal.hpp) the step adjoint uses too.
//
// The PD targets themselves are produced by the osc_pd_base_targets kernel from the packed base
// state the step writes (one more small launch per tick in PD mode): its result is then bitwise
// the producer's by construction.  A tick's targets, mask and references come from
// osc::tick_inputs (osc_rollout_schedule.hip), which the backward's recompute calls as well.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "osc_batch.h"
#include "osc_kin_device.hpp"
#include "osc_kin_env_params.h"
#include "osc_kin_model.hpp"
#include "osc_kinematics.h"
#include "osc_plant.h"
#include "osc_producers.h"
#include "osc_qpos.hpp"
#include "osc_rollout.h"
#include "osc_rollout_internal.hpp"

namespace {

using namespace osc;   // osc_rollout_internal.hpp's geometry, helpers and joint maps
using osc_kin::KinDev;

// the layout bindings restate (osc_amd/_lib.py OscRolloutArgs; tests/test_rollout_ref.py)
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_args) == 184, "osc_rollout_args layout");
static_assert(sizeof(void*) != 8 || sizeof(osc_rollout_plant) == 32, "osc_rollout_plant layout");

struct StepArgs {
  const KinDev* K;
  int32_t nenv, nq, nv, nbody, nu;
  double dt;
  const double* qacc;        // NULL: no step (the rollout's prologue: slab 0, packed base state)
  int64_t qacc_stride;
  const int32_t* status;     // nullable
  double* qpos;
  double* qvel;
  int32_t* bad_ticks;        // nullable
  const double* tau;         // read only for tau_hist
  double* qpos_hist;         // this tick's slabs, each nullable
  double* qvel_hist;
  double* tau_hist;
  double* base_pos;          // packed base state [nenv][3 | 4 | 3 | 3], all four or none
  double* base_quat;
  double* base_lin;
  double* base_ang;
};

// q * exp(w dt / 2), normalised (mju_quatIntegrate with a body-frame rate w).
__device__ __forceinline__ void quat_step(const double* q, const double* w, double dt,
                                          double* out) {
  const double rx = w[0] * dt, ry = w[1] * dt, rz = w[2] * dt;
  const double th = sqrt(rx * rx + ry * ry + rz * rz);
  double dw = 1.0, dx = 0.0, dy = 0.0, dz = 0.0;   // zero angle: the identity increment
  if (th != 0.0) {
    double s, c;
    sincos(0.5 * th, &s, &c);
    dw = c;
    dx = s * rx / th;
    dy = s * ry / th;
    dz = s * rz / th;
  }
  const double w0 = q[0], x0 = q[1], y0 = q[2], z0 = q[3];
  const double nw = w0 * dw - x0 * dx - y0 * dy - z0 * dz;
  const double nx = w0 * dx + x0 * dw + y0 * dz - z0 * dy;
  const double ny = w0 * dy - x0 * dz + y0 * dw + z0 * dx;
  const double nz = w0 * dz + x0 * dy - y0 * dx + z0 * dw;
  const double n = sqrt(nw * nw + nx * nx + ny * ny + nz * nz);
  out[0] = nw / n;
  out[1] = nx / n;
  out[2] = ny / n;
  out[3] = nz / n;
}

__global__ __launch_bounds__(kBlock) void osc_rollout_step_kernel(StepArgs a) {
  __shared__ double sq[kEnvPerBlock * kMaxNq];              // the block's qpos rows (old)
  __shared__ double sv[kEnvPerBlock * OSC_KIN_MAX_DOFS];    // qacc, then the new qvel rows
  __shared__ JointMaps maps;          // (the coordinate -> dof half is what the step reads)
  __shared__ int32_t sfrozen[kEnvPerBlock];
  const int tid = threadIdx.x;
  const int nq = a.nq, nv = a.nv, nu = a.nu;
  const long long e0 = static_cast<long long>(blockIdx.x) * kEnvPerBlock;
  const long long left = a.nenv - e0;
  const int ne = left < kEnvPerBlock ? static_cast<int>(left) : kEnvPerBlock;
  const bool step = a.qacc != nullptr;
  const double dt = a.dt;

  build_maps(a.K, a.nbody, tid, maps);
  if (tid < kEnvPerBlock)
    sfrozen[tid] = (step && a.status && tid < ne)
                       ? (a.status[e0 + tid] == OSC_SOLVE_NUMERICAL ? 1 : 0) : 0;
  __syncthreads();

  // qacc rows -> LDS; a non-finite entry freezes its env
  if (step) {
    for (int idx = tid; idx < ne * nv; idx += kBlock) {
      const int el = idx / nv, d = idx - el * nv;
      const double acc = a.qacc[(e0 + el) * a.qacc_stride + d];
      sv[idx] = acc;
      if (!isfinite(acc)) sfrozen[el] = 1;   // several lanes may store the same 1
    }
  }
  for (int idx = tid; idx < ne * nq; idx += kBlock) sq[idx] = a.qpos[e0 * nq + idx];
  __syncthreads();

  // qvel' = qvel + dt qacc (the same lane wrote sv[idx] above)
  for (int idx = tid; idx < ne * nv; idx += kBlock) {
    const int el = idx / nv, d = idx - el * nv;
    const long long g = e0 * nv + idx;
    const double v = a.qvel[g];
    double vn = v;
    if (step && !sfrozen[el]) {
      vn = fma(dt, sv[idx], v);
      a.qvel[g] = vn;
    }
    sv[idx] = vn;
    if (a.qvel_hist) a.qvel_hist[g] = vn;
    if (a.base_lin && d < 6) {
      if (d < 3) a.base_lin[(e0 + el) * 3 + d] = vn;
      else a.base_ang[(e0 + el) * 3 + (d - 3)] = vn;
    }
  }
  if (step && a.bad_ticks && tid < ne) {
    const bool bad = sfrozen[tid] || (a.status && a.status[e0 + tid] != OSC_SOLVE_OK);
    if (bad) a.bad_ticks[e0 + tid] += 1;
  }
  if (a.tau_hist)
    for (int idx = tid; idx < ne * nu; idx += kBlock)
      a.tau_hist[e0 * nu + idx] = a.tau[e0 * nu + idx];
  __syncthreads();

  // qpos' = integratePos(qpos, qvel', dt)
  for (int idx = tid; idx < ne * nq; idx += kBlock) {
    const int el = idx / nq, i = idx - el * nq;
    const long long g = e0 * nq + idx;
    double qn = sq[idx];
    if (step && !sfrozen[el]) {
      const double* v = sv + el * nv;
      const int comp = maps.ccomp[i], dof = maps.cdof[i];
      if (comp < 0) {
        qn = fma(v[dof], dt, qn);
      } else {
        double r[4];
        quat_step(sq + el * nq + (i - comp), v + dof, dt, r);
        qn = comp == 0 ? r[0] : comp == 1 ? r[1] : comp == 2 ? r[2] : r[3];
      }
      a.qpos[g] = qn;
    }
    if (a.qpos_hist) a.qpos_hist[g] = qn;
    if (a.base_pos && i < 7) {   // free root: qpos[0:3] position, qpos[3:7] quaternion
      if (i < 3) a.base_pos[(e0 + el) * 3 + i] = qn;
      else a.base_quat[(e0 + el) * 4 + (i - 3)] = qn;
    }
  }
}

int launch_step(const StepArgs& a, hipStream_t s) {
  if (a.nq > kMaxNq || a.nv > OSC_KIN_MAX_DOFS || a.nbody > OSC_KIN_MAX_BODIES)
    return OSC_ERR_INVALID_ARGUMENT;   // the kernel's LDS rows (build_tables cannot produce these)
  hipLaunchKernelGGL(osc_rollout_step_kernel, dim3(env_blocks(a.nenv)), dim3(kBlock), 0, s, a);
  return hipGetLastError() == hipSuccess ? OSC_OK : OSC_ERR_DEVICE;
}

StepArgs step_args(const osc_kin_model* kin, int32_t nenv) {
  StepArgs a{};
  a.K = kin->dev;
  a.nenv = nenv;
  a.nq = kin->host.nq;
  a.nv = kin->host.nv;
  a.nbody = kin->host.nbody;
  return a;
}

struct RolloutWorkspace {   // sections, each 256-B aligned
  size_t T, x, tau, status, bpos, bquat, blin, bang, warm, warm_bytes, qp, qp_bytes, total;
  int rc;
  RolloutWorkspace(const osc_model* model, const osc_kin_model* kin, const osc_model_desc& d,
                   int32_t nenv) {
    const size_t n = static_cast<size_t>(nenv), dbl = sizeof(double);
    T = 0;
    x = T + align256(dbl * n * d.ns * 6);
    tau = x + align256(dbl * n * (d.nv + d.nu + 3 * d.nc));
    status = tau + align256(dbl * n * d.nu);
    bpos = status + align256(sizeof(int32_t) * n);
    bquat = bpos + align256(dbl * n * 3);
    blin = bquat + align256(dbl * n * 4);
    bang = blin + align256(dbl * n * 3);
    warm = bang + align256(dbl * n * 3);
    warm_bytes = qp_bytes = 0;
    rc = osc_warm_state_bytes(model, nenv, &warm_bytes);
    qp = warm + align256(warm_bytes);
    if (rc == OSC_OK) rc = osc_qpos_workspace_bytes(model, kin, nenv, &qp_bytes);
    total = qp + align256(qp_bytes);
  }
};

// The plant's sections behind the rollout's own (include/osc_plant.h): M_p | C_p of the plant's
// kinematics and the qacc the step integrates, each 256-B aligned.
struct PlantWorkspace {
  size_t mp, cp, qacc, total;
  PlantWorkspace(const RolloutWorkspace& L, const osc_model_desc& d, int32_t nenv) {
    const size_t n = static_cast<size_t>(nenv), dbl = sizeof(double);
    mp = L.total;
    cp = mp + align256(dbl * n * d.nv * d.nv);
    qacc = cp + align256(dbl * n * d.nv);
    total = qacc + align256(dbl * n * d.nv);
  }
};

bool plant_active(const osc_rollout_plant* p) {
  return p != nullptr && (p->kin_params || p->qfrc_applied || p->qfrc_applied_seq || p->qacc_hist);
}

}  // namespace

extern "C" int osc_batch_integrate(const osc_kin_model* kin, int32_t nenv, double dt,
                                   const double* qacc, int64_t qacc_stride, const int32_t* status,
                                   double* qpos, double* qvel, int32_t* bad_ticks, void* stream) {
  if (!kin || nenv < 0 || !std::isfinite(dt)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  if (!qacc || !qpos || !qvel || qacc_stride < kin->host.nv) return OSC_ERR_INVALID_ARGUMENT;
  StepArgs a = step_args(kin, nenv);
  a.dt = dt;
  a.qacc = qacc;
  a.qacc_stride = qacc_stride;
  a.status = status;
  a.qpos = qpos;
  a.qvel = qvel;
  a.bad_ticks = bad_ticks;
  return launch_step(a, static_cast<hipStream_t>(stream));
}

extern "C" int osc_rollout_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                           int32_t nenv, int32_t nticks, size_t* bytes) {
  if (!bytes || nenv < 0 || nticks < 0) return OSC_ERR_INVALID_ARGUMENT;
  osc_model_desc d;
  const int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  const RolloutWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  *bytes = L.total;
  return OSC_OK;
}

// osc_batch_rollout (both blocks NULL: every tick through osc_batch_solve_qpos(_warm)),
// osc_batch_rollout_env (every tick through osc_batch_solve_qpos_env, the blocks held constant)
// and, with a schedule, osc_batch_rollout_sched (osc_rollout_schedule.h): a sequence replaces its
// held input by tick t's slab pointer, and T_seq is added to the tick's targets in the T slab.
// With a plant that has a non-NULL field (osc_batch_rollout_plant, include/osc_plant.h) the step
// integrates the plant's forward dynamics of the solve's u and z instead of dv.
int osc::rollout_run(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                     const osc_rollout_args* args, const osc_rollout_schedule* sched,
                     const osc_env_params* ep, const osc_kin_env_params* kp,
                     const osc_rollout_plant* plant, void* stream) {
  // ---- every check before the first launch ----
  osc_model_desc d;
  int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  const bool env = ep != nullptr || kp != nullptr;
  if (ep != nullptr && !osc::env_tick_ok(model, ep, nullptr)) return OSC_ERR_INVALID_ARGUMENT;
  if (kp != nullptr)
    for (const double* a : {kp->mass_scale, kp->com_offset, kp->armature_scale})
      if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
  const bool with_plant = plant_active(plant);
  const osc_kin_env_params* pkp = with_plant ? plant->kin_params : nullptr;
  // the plant's kinematics runs when its parameters differ from the controller's (the fused
  // diagnostic tick leaves no M, C, J in the workspace: there it always runs)
#ifdef OSC_FUSED_TICK
  const bool plant_kin = with_plant;
#else
  const bool plant_kin = pkp != nullptr && (pkp->mass_scale || pkp->com_offset || pkp->armature_scale);
#endif
  if (with_plant) {
    for (const double* a : {plant->qfrc_applied, plant->qfrc_applied_seq,
                            static_cast<const double*>(plant->qacc_hist)})
      if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
    if (pkp != nullptr)
      for (const double* a : {pkp->mass_scale, pkp->com_offset, pkp->armature_scale})
        if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
    // (the forward dynamics' own check of the model, with nothing to launch)
    rc = osc_batch_forward_dynamics(model, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                    nullptr, nullptr, nullptr);
    if (rc != OSC_OK) return rc;
  }
  if (!args || nenv < 0 || args->nticks < 0) return OSC_ERR_INVALID_ARGUMENT;
  if (!(args->dt > 0.0) || !std::isfinite(args->dt)) return OSC_ERR_INVALID_ARGUMENT;
  if (args->flags & ~OSC_ROLLOUT_WARM) return OSC_ERR_INVALID_ARGUMENT;
  const bool warm = (args->flags & OSC_ROLLOUT_WARM) != 0;
  const bool pd = args->target_mode == OSC_ROLLOUT_TARGETS_PD_BASE;
  if (!pd && args->target_mode != OSC_ROLLOUT_TARGETS_HELD) return OSC_ERR_INVALID_ARGUMENT;
  const KinDev& k = kin->host;
  if (pd && (k.jtype[0] != OSC_KIN_JOINT_FREE || k.parent[0] != -1))
    return OSC_ERR_INVALID_ARGUMENT;
  const osc_rollout_schedule sc = sched ? *sched : osc_rollout_schedule{};
  if (!pd && (sc.pos_ref_seq || sc.quat_ref_seq)) return OSC_ERR_INVALID_ARGUMENT;
  for (const double* a : {sc.T_seq, sc.mask_seq, sc.pos_ref_seq, sc.quat_ref_seq})
    if (!aligned8(a)) return OSC_ERR_INVALID_ARGUMENT;
  if (nenv == 0) return OSC_OK;
  if (!args->qpos || !args->qvel) return OSC_ERR_INVALID_ARGUMENT;
  const HeldInputs held{pd, args->T, args->contact_mask, args->pos_ref, args->pos_ref_per_env,
                        args->quat_ref, args->quat_ref_per_env, args->gains};
  if (!tick_inputs_present(held, sched, args->nticks, d.nc)) return OSC_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(args->workspace) & 15u) != 0) return OSC_ERR_INVALID_ARGUMENT;
  const RolloutWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  const PlantWorkspace LP(L, d, nenv);
  const size_t ws_total = with_plant ? LP.total : L.total;
  if (args->workspace && args->workspace_bytes < ws_total) return OSC_ERR_INVALID_ARGUMENT;

  hipStream_t s = static_cast<hipStream_t>(stream);
  const int32_t nticks = args->nticks;
  const size_t n = static_cast<size_t>(nenv);
  const size_t nx = static_cast<size_t>(d.nv + d.nu + 3 * d.nc);
  char* base = static_cast<char*>(args->workspace);
  bool owned = false;
  if (base == nullptr && nticks > 0) {
    if (hipMallocAsync(reinterpret_cast<void**>(&base), ws_total, s) != hipSuccess)
      return OSC_ERR_DEVICE;
    owned = true;
  }
  auto dptr = [&](size_t off) { return base ? reinterpret_cast<double*>(base + off) : nullptr; };
  double* Tbuf = dptr(L.T);
  double* x = dptr(L.x);
  double* tau = args->tau ? args->tau : dptr(L.tau);
  int32_t* status_ws = base ? reinterpret_cast<int32_t*>(base + L.status) : nullptr;
  double* wstate = dptr(L.warm);
  const bool pack = pd && nticks > 0;   // the producer reads the packed base state

  // ---- prologue: zero-fills, slab 0 of the histories, tick 0's packed base state ----
  if (args->bad_ticks &&
      hipMemsetAsync(args->bad_ticks, 0, sizeof(int32_t) * n, s) != hipSuccess)
    rc = OSC_ERR_DEVICE;
  if (rc == OSC_OK && warm && nticks > 0 &&
      hipMemsetAsync(wstate, 0, L.warm_bytes, s) != hipSuccess)
    rc = OSC_ERR_DEVICE;
  if (rc == OSC_OK && (args->qpos_hist || args->qvel_hist || pack)) {
    StepArgs a = step_args(kin, nenv);
    a.qpos = args->qpos;
    a.qvel = args->qvel;
    a.qpos_hist = args->qpos_hist;
    a.qvel_hist = args->qvel_hist;
    if (pack) {
      a.base_pos = dptr(L.bpos);
      a.base_quat = dptr(L.bquat);
      a.base_lin = dptr(L.blin);
      a.base_ang = dptr(L.bang);
    }
    rc = launch_step(a, s);
  }

  // ---- ticks ----
  for (int32_t t = 0; t < nticks && rc == OSC_OK; ++t) {
    TickInputs in;
    rc = tick_inputs(held, sc, t, nenv, d, dptr(L.bpos), dptr(L.bquat), dptr(L.blin), dptr(L.bang),
                     Tbuf, stream, &in);
    if (rc != OSC_OK) break;
    const double* T = in.T;
    const double* mask = in.mask;
    int32_t* status = args->status_hist ? args->status_hist + n * t : status_ws;
    if (env)
      rc = osc_batch_solve_qpos_env(model, kin, nenv, args->qpos, args->qvel, T, mask,
                                    ep, kp, nullptr, tau, x, status, nullptr,
                                    warm ? wstate : nullptr, warm ? L.warm_bytes : 0, base + L.qp,
                                    L.qp_bytes, stream);
    else
      rc = warm ? osc_batch_solve_qpos_warm(model, kin, nenv, args->qpos, args->qvel, T,
                                            mask, tau, x, status, nullptr, wstate,
                                            L.warm_bytes, base + L.qp, L.qp_bytes, stream)
                : osc_batch_solve_qpos(model, kin, nenv, args->qpos, args->qvel, T,
                                       mask, tau, x, status, nullptr, base + L.qp,
                                       L.qp_bytes, stream);
    if (rc != OSC_OK) break;
    const double* qacc = x;   // dv = x[0:nv]
    int64_t qacc_stride = static_cast<int64_t>(nx);
    if (with_plant) {
      // the tick's own M, C, J (the solve reads them, const, and leaves them as the kinematics
      // wrote them); J and b do not depend on the inertial parameters, so the plant's kinematics
      // rewrites them with the same bits
      const osc_kin::QposWorkspace Q(model, k, nenv);
      const double* Mp = dptr(L.qp + Q.m);
      const double* Cp = dptr(L.qp + Q.c);
      if (plant_kin) {
        rc = osc_batch_kinematics_env(kin, nenv, args->qpos, args->qvel, pkp, dptr(LP.mp),
                                      dptr(LP.cp), dptr(L.qp + Q.j), dptr(L.qp + Q.b), nullptr,
                                      stream);
        if (rc != OSC_OK) break;
        Mp = dptr(LP.mp);
        Cp = dptr(LP.cp);
      }
      const double* qfrc = plant->qfrc_applied_seq ? plant->qfrc_applied_seq + n * d.nv * t
                                                   : plant->qfrc_applied;
      double* out = plant->qacc_hist ? plant->qacc_hist + n * d.nv * t : dptr(LP.qacc);
      rc = osc_batch_forward_dynamics(model, nenv, Mp, Cp, dptr(L.qp + Q.j), x + d.nv,
                                      static_cast<int64_t>(nx), x + d.nv + d.nu,
                                      static_cast<int64_t>(nx), qfrc, out, stream);
      if (rc != OSC_OK) break;
      qacc = out;
      qacc_stride = d.nv;
    }
    StepArgs a = step_args(kin, nenv);
    a.nu = d.nu;
    a.dt = args->dt;
    a.qacc = qacc;
    a.qacc_stride = qacc_stride;
    a.status = status;
    a.qpos = args->qpos;
    a.qvel = args->qvel;
    a.bad_ticks = args->bad_ticks;
    a.tau = tau;
    a.qpos_hist = args->qpos_hist ? args->qpos_hist + n * k.nq * (t + 1) : nullptr;
    a.qvel_hist = args->qvel_hist ? args->qvel_hist + n * k.nv * (t + 1) : nullptr;
    a.tau_hist = args->tau_hist ? args->tau_hist + n * d.nu * t : nullptr;
    if (pd && t + 1 < nticks) {
      a.base_pos = dptr(L.bpos);
      a.base_quat = dptr(L.bquat);
      a.base_lin = dptr(L.blin);
      a.base_ang = dptr(L.bang);
    }
    rc = launch_step(a, s);
  }
  if (owned) (void)hipFreeAsync(base, s);
  return rc;
}

extern "C" int osc_batch_rollout(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                 const osc_rollout_args* args, void* stream) {
  return osc::rollout_run(model, kin, nenv, args, nullptr, nullptr, nullptr, nullptr, stream);
}

// (the tick's workspace is osc_qpos_env_workspace_bytes, which is osc_qpos_workspace_bytes: one
// layout for both rollouts)
extern "C" int osc_rollout_env_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                               int32_t nenv, int32_t nticks, size_t* bytes) {
  return osc_rollout_workspace_bytes(model, kin, nenv, nticks, bytes);
}

extern "C" int osc_batch_rollout_env(const osc_model* model, const osc_kin_model* kin, int32_t nenv,
                                     const osc_rollout_args* args, const osc_env_params* env_params,
                                     const osc_kin_env_params* kin_params, void* stream) {
  return osc::rollout_run(model, kin, nenv, args, nullptr, env_params, kin_params, nullptr, stream);
}

// ---- the rollout against a plant (include/osc_plant.h) ----

extern "C" int osc_rollout_plant_workspace_bytes(const osc_model* model, const osc_kin_model* kin,
                                                 int32_t nenv, int32_t nticks, size_t* bytes) {
  if (!bytes || nenv < 0 || nticks < 0) return OSC_ERR_INVALID_ARGUMENT;
  osc_model_desc d;
  const int rc = check_handles(model, kin, &d);
  if (rc != OSC_OK) return rc;
  const RolloutWorkspace L(model, kin, d, nenv);
  if (L.rc != OSC_OK) return L.rc;
  *bytes = PlantWorkspace(L, d, nenv).total;
  return OSC_OK;
}

extern "C" int osc_batch_rollout_plant(const osc_model* model, const osc_kin_model* kin,
                                       int32_t nenv, const osc_rollout_args* args,
                                       const osc_rollout_schedule* sched,
                                       const osc_env_params* env_params,
                                       const osc_kin_env_params* kin_params,
                                       const osc_rollout_plant* plant, void* stream) {
  return osc::rollout_run(model, kin, nenv, args, sched, env_params, kin_params, plant, stream);
}
