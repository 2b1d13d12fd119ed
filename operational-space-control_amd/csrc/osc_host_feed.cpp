// osc_host_feed.cpp -- the host-fed batched control tick (include/osc_host_feed.h, SURVEY.md
// §8(e)): pinned host slots -> one H2D copy per tick -> the batched solve -> D2H of the torques,
// pipelined over `depth` slots on three HIP streams.  Host code over the public C-ABI only
// (osc_batch_kinematics, osc_batch_solve(_warm)); the reference it replaces is the
// per-tick hand-off of unitree_go2/operational_space_controller.h:546-573 (State and targets in
// host memory under the mutex, the solve, the torque copy back).
// A feed holds one model's batch (osc_host_feed_create) or two models' (osc_host_feed_create_multi,
// include/osc_mixed.h: the parts share every slot's blocks, copies and streams, and the solve is
// osc_batch_tick_multi).
#include "osc_host_feed.h"
#include "osc_mixed.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

namespace {

constexpr size_t kAlign = 256;   // every array of a slot starts on a 256-B boundary
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

enum Ev { kH2dBeg, kH2dEnd, kKinEnd, kSolveBeg, kSolveEnd, kD2hBeg, kD2hEnd, kNumEv };

struct Slot {
  char* h_in = nullptr;        // pinned
  char* d_in = nullptr;        // HBM
  char* h_out = nullptr;       // pinned
  char* d_out = nullptr;       // HBM
  char* d_kin = nullptr;       // HBM: joint-state form, the kinematics' M, C, J, b of this slot
  hipEvent_t ev[kNumEv] = {};
  int32_t tick = -1;           // last tick submitted into this slot
};

}  // namespace

namespace {
constexpr int kMaxParts = 2;

// One model's share of the feed: its arrays' byte offsets inside the slot's blocks (a second
// part's follow the first's), its solve workspace and warm state.
struct Part {
  const osc_model* model = nullptr;
  const osc_kin_model* kin = nullptr;
  int32_t nenv = 0;
  int32_t nv = 0, nu = 0, nc = 0, ns = 0, nq = 0;
  // byte offsets of the arrays inside a slot's input block: M C J b | qpos qvel, then T mask
  size_t off_M = 0, off_C = 0, off_J = 0, off_b = 0, off_qpos = 0, off_qvel = 0, off_T = 0,
         off_mask = 0;
  size_t off_tau = 0, off_status = 0, off_iters = 0;
  size_t kin_M = 0, kin_C = 0, kin_J = 0, kin_b = 0;   // joint-state form
  void* ws = nullptr;
  size_t ws_bytes = 0;
  double* warm = nullptr;
  size_t warm_bytes = 0;
};
}  // namespace

struct osc_host_feed {
  int32_t nparts = 0;
  Part part[kMaxParts];
  int32_t form = 0, depth = 0, device = 0;
  uint32_t flags = 0;
  size_t in_bytes = 0, out_bytes = 0, kin_bytes = 0;   // a slot's blocks, every part's arrays
  Slot slot[OSC_FEED_MAX_DEPTH];
  hipStream_t s_h2d = nullptr, s_solve = nullptr, s_d2h = nullptr;
  int32_t next = 0;            // next tick to submit
  bool failed = false;         // a submit failed part-way: the pipeline state is undefined
};

namespace {

void release(osc_host_feed* f) {
  for (auto& s : f->slot) {
    for (auto& e : s.ev)
      if (e) (void)hipEventDestroy(e);
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.d_kin) (void)hipFree(s.d_kin);
  }
  for (hipStream_t st : {f->s_h2d, f->s_solve, f->s_d2h})
    if (st) (void)hipStreamDestroy(st);
  for (auto& p : f->part) {
    if (p.ws) (void)hipFree(p.ws);
    if (p.warm) (void)hipFree(p.warm);
  }
  delete f;
}

bool ok(hipError_t e) { return e == hipSuccess; }

}  // namespace

namespace {
int feed_create(const osc_feed_part* parts, int32_t nparts, int32_t form, uint32_t flags,
                int32_t depth, bool check_jobs, osc_host_feed** out) {
  if (!out) return OSC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!parts || nparts < 1 || nparts > kMaxParts || depth < 1 || depth > OSC_FEED_MAX_DEPTH ||
      (flags & ~OSC_FEED_WARM) != 0 || (form != OSC_FEED_QP && form != OSC_FEED_JOINT_STATES))
    return OSC_ERR_INVALID_ARGUMENT;
  osc_model_desc d[kMaxParts];
  for (int i = 0; i < nparts; ++i) {
    const osc_feed_part& p = parts[i];
    if (!p.model || p.nenv <= 0) return OSC_ERR_INVALID_ARGUMENT;
    if (form == OSC_FEED_QP ? p.kin != nullptr : p.kin == nullptr) return OSC_ERR_INVALID_ARGUMENT;
    if (osc_model_get_desc(p.model, &d[i]) != OSC_OK) return OSC_ERR_INVALID_ARGUMENT;
    if (d[i].wheel_rows) return OSC_ERR_INVALID_ARGUMENT;   // (per-env wheel directions: no form has them)
  }
  osc_host_feed* f = new (std::nothrow) osc_host_feed;
  if (!f) return OSC_ERR_DEVICE;
  f->nparts = nparts;
  f->form = form;
  f->flags = flags;
  f->depth = depth;
  (void)hipGetDevice(&f->device);
  const size_t e8 = sizeof(double);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes);
    return at;
  };
  for (int i = 0; i < nparts; ++i) {
    Part& p = f->part[i];
    p.model = parts[i].model;
    p.kin = parts[i].kin;
    p.nenv = parts[i].nenv;
    p.nv = d[i].nv;
    p.nu = d[i].nu;
    p.nc = d[i].nc;
    p.ns = d[i].ns;
  }
  for (int i = 0; i < nparts; ++i) {   // the input block: part 0's arrays, then part 1's
    Part& p = f->part[i];
    const size_t n = static_cast<size_t>(p.nenv);
    if (form == OSC_FEED_QP) {
      p.off_M = take(n * p.nv * p.nv * e8);
      p.off_C = take(n * p.nv * e8);
      p.off_J = take(n * 6 * p.ns * p.nv * e8);
      p.off_b = take(n * 6 * p.ns * e8);
    } else {
      int32_t knv = 0, kns = 0;
      if (osc_kin_model_dims(p.kin, &p.nq, &knv, &kns) != OSC_OK || knv != p.nv || kns != p.ns) {
        release(f);
        return OSC_ERR_INVALID_ARGUMENT;
      }
      p.off_qpos = take(n * p.nq * e8);
      p.off_qvel = take(n * p.nv * e8);
    }
    p.off_T = take(n * p.ns * 6 * e8);
    p.off_mask = take(n * p.nc * e8);
  }
  f->in_bytes = o;
  o = 0;
  for (int i = 0; i < nparts; ++i) {
    Part& p = f->part[i];
    const size_t n = static_cast<size_t>(p.nenv);
    p.off_tau = take(n * p.nu * e8);
    p.off_status = take(n * sizeof(int32_t));
    p.off_iters = take(n * sizeof(int32_t));
  }
  f->out_bytes = o;
  if (form == OSC_FEED_JOINT_STATES) {
    o = 0;
    for (int i = 0; i < nparts; ++i) {
      Part& p = f->part[i];
      const size_t n = static_cast<size_t>(p.nenv);
      p.kin_M = take(n * p.nv * p.nv * e8);
      p.kin_C = take(n * p.nv * e8);
      p.kin_J = take(n * 6 * p.ns * p.nv * e8);
      p.kin_b = take(n * 6 * p.ns * e8);
    }
    f->kin_bytes = o;
  }

  int rc = OSC_ERR_DEVICE;
  bool good =
      ok(hipStreamCreateWithFlags(&f->s_h2d, hipStreamNonBlocking)) &&
      ok(hipStreamCreateWithFlags(&f->s_solve, hipStreamNonBlocking)) &&
      ok(hipStreamCreateWithFlags(&f->s_d2h, hipStreamNonBlocking));
  for (int i = 0; good && i < depth; ++i) {
    Slot& s = f->slot[i];
    good = ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_in), f->in_bytes, hipHostMallocDefault)) &&
           ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_out), f->out_bytes, hipHostMallocDefault)) &&
           ok(hipMalloc(reinterpret_cast<void**>(&s.d_in), f->in_bytes)) &&
           ok(hipMalloc(reinterpret_cast<void**>(&s.d_out), f->out_bytes)) &&
           (f->kin_bytes == 0 || ok(hipMalloc(reinterpret_cast<void**>(&s.d_kin), f->kin_bytes)));
    for (int e = 0; good && e < kNumEv; ++e) good = ok(hipEventCreate(&s.ev[e]));
    if (good) {   // zero host inputs: a tick submitted without being written solves a defined QP
      std::memset(s.h_in, 0, f->in_bytes);
      std::memset(s.h_out, 0, f->out_bytes);
    }
  }
  for (int i = 0; good && i < nparts; ++i) {
    Part& p = f->part[i];
    // (the joint-state form runs the kinematics itself, into the slot's d_kin: the solve's
    // workspace is osc_batch_solve's)
    good = osc_workspace_bytes(p.model, p.nenv, &p.ws_bytes) == OSC_OK;
    good = good && ok(hipMalloc(&p.ws, p.ws_bytes));
    if (good && (flags & OSC_FEED_WARM)) {
      good = osc_warm_state_bytes(p.model, p.nenv, &p.warm_bytes) == OSC_OK &&
             ok(hipMalloc(reinterpret_cast<void**>(&p.warm), p.warm_bytes)) &&
             ok(hipMemset(p.warm, 0, p.warm_bytes));   // every env cold on its first tick
    }
  }
  if (good && check_jobs) {
    // osc_host_feed_create_multi: what osc_batch_tick_multi would refuse on every submit is
    // refused once here (an empty call: nenv 0 launches nothing but still checks each model, its
    // device and its kin); the buffers are the feed's own, sized and aligned above.
    osc_tick_job jobs[kMaxParts] = {};
    for (int i = 0; i < nparts; ++i) {
      jobs[i].model = f->part[i].model;
      jobs[i].kin = f->part[i].kin;
    }
    rc = osc_batch_tick_multi(jobs, nparts, nullptr);
    good = rc == OSC_OK;
  }
  if (!good) {
    release(f);
    return rc;
  }
  *out = f;
  return OSC_OK;
}
}  // namespace

extern "C" int osc_host_feed_create(const osc_model* model, const osc_kin_model* kin,
                                    int32_t nenv, int32_t form, uint32_t flags, int32_t depth,
                                    osc_host_feed** out) {
  const osc_feed_part part{model, kin, nenv};
  return feed_create(&part, 1, form, flags, depth, false, out);
}

extern "C" int osc_host_feed_create_multi(const osc_feed_part* parts, int32_t nparts, int32_t form,
                                          uint32_t flags, int32_t depth, osc_host_feed** out) {
  return feed_create(parts, nparts, form, flags, depth, true, out);
}

extern "C" int osc_host_feed_destroy(osc_host_feed* f) {
  if (!f) return OSC_ERR_INVALID_ARGUMENT;
  // drain every stream before freeing what they use
  for (hipStream_t st : {f->s_h2d, f->s_solve, f->s_d2h})
    if (st) (void)hipStreamSynchronize(st);
  release(f);
  return OSC_OK;
}

extern "C" int osc_host_feed_inputs_part(osc_host_feed* f, int32_t tick, int32_t part,
                                         osc_feed_inputs* in) {
  if (!f || !in || tick != f->next || part < 0 || part >= f->nparts)
    return OSC_ERR_INVALID_ARGUMENT;
  if (f->failed) return OSC_ERR_DEVICE;
  const Part& p = f->part[part];
  Slot& s = f->slot[tick % f->depth];
  // the slot's pinned inputs are free once its previous H2D copy has completed
  if (s.tick >= 0 && !ok(hipEventSynchronize(s.ev[kH2dEnd]))) return OSC_ERR_DEVICE;
  std::memset(in, 0, sizeof(*in));
  auto at = [&](size_t off) { return reinterpret_cast<double*>(s.h_in + off); };
  if (f->form == OSC_FEED_QP) {
    in->M = at(p.off_M);
    in->C = at(p.off_C);
    in->J = at(p.off_J);
    in->b = at(p.off_b);
  } else {
    in->qpos = at(p.off_qpos);
    in->qvel = at(p.off_qvel);
  }
  in->T = at(p.off_T);
  in->contact_mask = at(p.off_mask);
  in->bytes = f->in_bytes;
  return OSC_OK;
}

extern "C" int osc_host_feed_inputs(osc_host_feed* f, int32_t tick, osc_feed_inputs* in) {
  if (!f || f->nparts != 1) return OSC_ERR_INVALID_ARGUMENT;   // (two parts: _inputs_part)
  return osc_host_feed_inputs_part(f, tick, 0, in);
}

namespace {
int submit_tick(osc_host_feed* f, int32_t tick);
}  // namespace

extern "C" int osc_host_feed_submit(osc_host_feed* f, int32_t tick) {
  if (!f || tick != f->next) return OSC_ERR_INVALID_ARGUMENT;
  if (f->failed) return OSC_ERR_DEVICE;
  int cur = -1;
  if (!ok(hipGetDevice(&cur)) || cur != f->device) return OSC_ERR_INVALID_ARGUMENT;
  // anything failing past this point leaves part of the tick enqueued: the feed refuses every
  // further tick (sticky OSC_ERR_DEVICE) and is only good for osc_host_feed_destroy
  const int rc = submit_tick(f, tick);
  if (rc != OSC_OK) f->failed = true;
  return rc;
}

namespace {
int submit_tick(osc_host_feed* f, int32_t tick) {
  Slot& s = f->slot[tick % f->depth];
  const bool reuse = s.tick >= 0;
  // H2D: the device inputs of this slot are free once the solve of tick - depth has read them
  if (reuse && !ok(hipStreamWaitEvent(f->s_h2d, s.ev[kSolveEnd], 0))) return OSC_ERR_DEVICE;
  if (!ok(hipEventRecord(s.ev[kH2dBeg], f->s_h2d)) ||
      !ok(hipMemcpyAsync(s.d_in, s.h_in, f->in_bytes, hipMemcpyHostToDevice, f->s_h2d)) ||
      !ok(hipEventRecord(s.ev[kH2dEnd], f->s_h2d)))
    return OSC_ERR_DEVICE;
  auto in = [&](size_t off) { return reinterpret_cast<const double*>(s.d_in + off); };
  auto kb = [&](size_t off) { return reinterpret_cast<double*>(s.d_kin + off); };
  if (f->form == OSC_FEED_JOINT_STATES) {
    // joint states: the kinematics runs on the copy stream right behind its H2D (round 6), so it
    // overlaps the previous tick's solve -- the interior point's straggler tail leaves most SIMDs
    // idle -- instead of heading this tick's solve (osc_batch_solve_qpos = osc_batch_kinematics +
    // osc_batch_solve: bitwise the same).  The slot's d_kin was last read by the solve of tick -
    // depth, which the copy stream has waited for above.
    const Part& p = f->part[0];
    int krc;
    if (f->nparts == 1) {
      krc = osc_batch_kinematics(p.kin, p.nenv, in(p.off_qpos), in(p.off_qvel), kb(p.kin_M),
                                 kb(p.kin_C), kb(p.kin_J), kb(p.kin_b), nullptr, f->s_h2d);
    } else {   // both parts' kinematics in one grid
      const Part& q = f->part[1];
      krc = osc_batch_kinematics_pair(p.kin, p.nenv, in(p.off_qpos), in(p.off_qvel), kb(p.kin_M),
                                      kb(p.kin_C), kb(p.kin_J), kb(p.kin_b), q.kin, q.nenv,
                                      in(q.off_qpos), in(q.off_qvel), kb(q.kin_M), kb(q.kin_C),
                                      kb(q.kin_J), kb(q.kin_b), f->s_h2d);
    }
    if (krc != OSC_OK) return krc;
  }
  if (!ok(hipEventRecord(s.ev[kKinEnd], f->s_h2d))) return OSC_ERR_DEVICE;
  // solve: after this tick's H2D (and kinematics), and after the D2H of tick - depth has read the
  // slot's outputs
  if (!ok(hipStreamWaitEvent(f->s_solve, s.ev[kKinEnd], 0)) ||
      (reuse && !ok(hipStreamWaitEvent(f->s_solve, s.ev[kD2hEnd], 0))) ||
      !ok(hipEventRecord(s.ev[kSolveBeg], f->s_solve)))
    return OSC_ERR_DEVICE;
  int rc;
  if (f->nparts == 1) {
    const Part& p = f->part[0];
    double* tau = reinterpret_cast<double*>(s.d_out + p.off_tau);
    int32_t* status = reinterpret_cast<int32_t*>(s.d_out + p.off_status);
    int32_t* iters = reinterpret_cast<int32_t*>(s.d_out + p.off_iters);
    const bool qp = f->form == OSC_FEED_QP;
    const double* M = qp ? in(p.off_M) : kb(p.kin_M);
    const double* C = qp ? in(p.off_C) : kb(p.kin_C);
    const double* J = qp ? in(p.off_J) : kb(p.kin_J);
    const double* b = qp ? in(p.off_b) : kb(p.kin_b);
    rc = p.warm ? osc_batch_solve_warm(p.model, p.nenv, M, C, J, b, in(p.off_T), in(p.off_mask),
                                       tau, nullptr, status, iters, p.warm, p.warm_bytes, p.ws,
                                       p.ws_bytes, f->s_solve)
                : osc_batch_solve(p.model, p.nenv, M, C, J, b, in(p.off_T), in(p.off_mask), tau,
                                  nullptr, status, iters, p.ws, p.ws_bytes, f->s_solve);
  } else {
    // two parts: one osc_batch_tick_multi over both (QP jobs: a joint-state feed's M, C, J, b are
    // the kinematics' of this slot, above)
    osc_tick_job jobs[kMaxParts] = {};
    for (int i = 0; i < f->nparts; ++i) {
      const Part& p = f->part[i];
      osc_tick_job& j = jobs[i];
      const bool qp = f->form == OSC_FEED_QP;
      j.model = p.model;
      j.nenv = p.nenv;
      j.M = qp ? in(p.off_M) : kb(p.kin_M);
      j.C = qp ? in(p.off_C) : kb(p.kin_C);
      j.J = qp ? in(p.off_J) : kb(p.kin_J);
      j.b = qp ? in(p.off_b) : kb(p.kin_b);
      j.T = in(p.off_T);
      j.contact_mask = in(p.off_mask);
      j.tau = reinterpret_cast<double*>(s.d_out + p.off_tau);
      j.status = reinterpret_cast<int32_t*>(s.d_out + p.off_status);
      j.iters = reinterpret_cast<int32_t*>(s.d_out + p.off_iters);
      j.warm_state = p.warm;
      j.warm_state_bytes = p.warm_bytes;
      j.workspace = p.ws;
      j.workspace_bytes = p.ws_bytes;
    }
    rc = osc_batch_tick_multi(jobs, f->nparts, f->s_solve);
  }
  if (rc != OSC_OK) return rc;
  if (!ok(hipEventRecord(s.ev[kSolveEnd], f->s_solve))) return OSC_ERR_DEVICE;
  // D2H of the outputs
  if (!ok(hipStreamWaitEvent(f->s_d2h, s.ev[kSolveEnd], 0)) ||
      !ok(hipEventRecord(s.ev[kD2hBeg], f->s_d2h)) ||
      !ok(hipMemcpyAsync(s.h_out, s.d_out, f->out_bytes, hipMemcpyDeviceToHost, f->s_d2h)) ||
      !ok(hipEventRecord(s.ev[kD2hEnd], f->s_d2h)))
    return OSC_ERR_DEVICE;
  s.tick = tick;
  ++f->next;
  return OSC_OK;
}
}  // namespace

extern "C" int osc_host_feed_wait_part(osc_host_feed* f, int32_t tick, int32_t part,
                                       osc_feed_outputs* out) {
  if (!f || !out || tick < 0 || tick >= f->next || tick < f->next - f->depth || part < 0 ||
      part >= f->nparts)
    return OSC_ERR_INVALID_ARGUMENT;
  const Part& p = f->part[part];
  Slot& s = f->slot[tick % f->depth];
  if (s.tick != tick) return OSC_ERR_INVALID_ARGUMENT;
  if (!ok(hipEventSynchronize(s.ev[kD2hEnd]))) return OSC_ERR_DEVICE;
  out->tau = reinterpret_cast<const double*>(s.h_out + p.off_tau);
  out->status = reinterpret_cast<const int32_t*>(s.h_out + p.off_status);
  out->iters = reinterpret_cast<const int32_t*>(s.h_out + p.off_iters);
  out->bytes = f->out_bytes;
  return OSC_OK;
}

extern "C" int osc_host_feed_wait(osc_host_feed* f, int32_t tick, osc_feed_outputs* out) {
  if (!f || f->nparts != 1) return OSC_ERR_INVALID_ARGUMENT;   // (two parts: _wait_part)
  return osc_host_feed_wait_part(f, tick, 0, out);
}

extern "C" int osc_host_feed_timing(osc_host_feed* f, int32_t tick, osc_feed_timing* t) {
  if (!f || !t || tick < 0 || tick >= f->next || tick < f->next - f->depth)
    return OSC_ERR_INVALID_ARGUMENT;
  Slot& s = f->slot[tick % f->depth];
  if (s.tick != tick || hipEventQuery(s.ev[kD2hEnd]) != hipSuccess) return OSC_ERR_INVALID_ARGUMENT;
  if (!ok(hipEventElapsedTime(&t->h2d_ms, s.ev[kH2dBeg], s.ev[kH2dEnd])) ||
      !ok(hipEventElapsedTime(&t->solve_ms, s.ev[kSolveBeg], s.ev[kSolveEnd])) ||
      !ok(hipEventElapsedTime(&t->d2h_ms, s.ev[kD2hBeg], s.ev[kD2hEnd])) ||
      !ok(hipEventElapsedTime(&t->kin_ms, s.ev[kH2dEnd], s.ev[kKinEnd])) ||
      !ok(hipEventElapsedTime(&t->h2d_start_to_d2h_end_ms, s.ev[kH2dBeg], s.ev[kD2hEnd])))
    return OSC_ERR_DEVICE;
  return OSC_OK;
}
