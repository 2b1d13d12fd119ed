// osc_ipm.hpp -- kernel 2, the batched interior point + full-space refinement (osc_ipm_kernel,
// osc_ipm_compact_kernel, osc_refine_kernel, osc_ipm_pair_kernel): the reference's OSQP solve
// (unitree_go2/operational_space_controller.h:483-536) on the reduced QP, four environments per
// wavefront, and launch_ipm, the pass sequence of one call.  Device code +
// the launcher template; instantiated once per robot model (osc_ipm_go2.hip, osc_ipm_walter.hip,
// osc_ipm_wheels.hip) so the three compile in parallel.
// This file holds ipm_block, the body of one wavefront; its parts are headers of their own:
// osc_ipm_ldl.hpp (the DPP LDL^T and solves), osc_ipm_lds.hpp (LDS layout per variant),
// osc_ipm_rows.hpp (products with the inequality rows), osc_ipm_wheel.hpp (wheel-row rotations),
// osc_ipm_iter.hpp (the body of one iteration, a fragment included inside ipm_block's loop) and,
// included last, osc_ipm_launch.hpp (the __global__ wrappers and launch_ipm).
#pragma once
#include "osc_internal.hpp"
#include "osc_ipm_ldl.hpp"
#include "osc_ipm_lds.hpp"
#include "osc_ipm_rows.hpp"
#include "osc_ipm_wheel.hpp"

namespace osc {

// The body of one IPM wavefront (envs 4 blk .. 4 blk + 3); `sm` is its ipm_lds_doubles<D, SMALL>
// doubles of LDS.  Wrapped by osc_ipm_kernel (one model) and osc_ipm_pair_kernel (two models).
// WARM = false compiles none of the warm-start / fix-up logic (the cold solve's register budget
// is unchanged by it: the two-wave Go2 variant would otherwise spill more).
// ENV = true (the _env entry points, include/osc_env_params.h): mu, the torque box and the fz
// bounds of each env come from EP's arrays (a NULL one: the model's value) in the row set-up below,
// the only place that reads them; an env whose values are invalid is poisoned there with a NaN
// gradient and ends OSC_SOLVE_NUMERICAL like an env with NaN inputs.  ENV = false compiles none of
// it: the existing kernels' code is unchanged.
// PAIR = true (the two-model kernels, osc_ipm_pair_kernel and osc_multi.hip): Go2's body as it was
// before its start was peeled (kPeel below).
template <class D, bool SMALL, bool WARM, int RF_ = kRfNone, int CP = kCpNone, bool ENV = false,
          bool PAIR = false>
__device__ __forceinline__ void ipm_block(
    const DevParams* __restrict__ P, int blk, int nenv, const double* __restrict__ gmask,
    const double* __restrict__ ws, double* __restrict__ gtau, double* __restrict__ gx,
    int32_t* __restrict__ gstatus, int32_t* __restrict__ giters, double* __restrict__ gwarm,
    int flags, double* __restrict__ sm, ParkArgs PA = ParkArgs{}, EnvPtrs EP = EnvPtrs{}) {
  static_assert(!ENV || (CP == kCpNone && !D::WH), "per-env parameters: no compaction, no wheel rows");
  static_assert(CP == kCpNone || (!WARM && RF_ == kRfFused && !D::WH),
                "compaction: cold solves with the fused refinement only");
  constexpr int NV = D::NV, NU = D::NU, NC = D::NC, NY = D::NY, NY1P = D::NY1P, MI = D::MI,
                NRL = D::NRL;
  // flags: bit 0 = the cold fix-up pass after a warm-started solve, bit 1 = hand the multipliers
  // to the dual kernel (W_SOL q, W_NU)
  const bool fixup = (flags & 1) != 0;
  const bool want_dual = (flags & 2) != 0;
  // the refinement fused: a cold solve is followed by its own fix-up pass too (osc_ipm_kernel)
  constexpr bool kFix = WARM || RF_ == kRfFused;
  constexpr int RF = RF_;
  constexpr bool REFINE = RF == kRfOnly;      // the refinement pass alone (no interior point)
  constexpr bool HRL = ipm_hrl<D, SMALL, RF>();
  using LY = IpmLayout<D, HRL>;
  const int lane = threadIdx.x;
  const int grp = lane / kRow, l = lane % kRow;
  // resume pass: the wave's rows are parked slots (env_raw), their envs from the slot list
  const int cnt = CP == kCpResume ? *PA.count : nenv;
  if (CP == kCpResume && blk * kEnvPerWave >= cnt) return;
  const int env_raw = blk * kEnvPerWave + grp;
  const bool valid = env_raw < cnt;
  const int env = CP == kCpResume ? PA.list[valid ? env_raw : cnt - 1]
                                  : (valid ? env_raw : nenv - 1);   // spare rows replay the last
                                                                     // env, write nothing
  // Fix-up pass after a warm-started solve: only wavefronts holding an env that did not converge
  // run (cold, from the same workspace); only those envs' outputs are rewritten.
  bool write_out = valid;
  if constexpr (kFix) {
    // (an env whose refinement found no KKT point, OSC_SOLVE_UNREFINED, too: the warm start can
    // leave the interior point's early stop with an active set the refinement cannot repair,
    // ~1 env in 4,096 x 10 joint-state ticks; the cold fix-up solve runs to mu <= 1e-12)
    const bool redo = valid && fixup && gstatus[env] != OSC_SOLVE_OK;
    if (fixup && __ballot(redo) == 0) return;
    write_out = valid && (!fixup || redo);
  }

  constexpr bool HRH = ipm_hrh<D, SMALL, RF>();
  constexpr int kEnvLds = LY::IL + refine_lds_extra<D, SMALL, RF>() + hrh_lds_extra<D, SMALL, RF>();
  double* B = sm + grp * kEnvLds;
  double* sHh = B + LY::IL + refine_lds_extra<D, SMALL, RF>();   // HRH: Hr[i][0..15] at i * 16
  // refinement: [X | H_dv | f_dv] of this env; a fused pass with Hr in LDS keeps X in Hr's region
  constexpr bool kXinHr = RF == kRfFused && HRL;
  double* sRX = kXinHr ? B + LY::I_HR : B + LY::IL + RefineLds<D>::X;
  double* sRH = kXinHr ? B + LY::IL : B + LY::IL + RefineLds<D>::HD;
  double* sRG = sRH + (RefineLds<D>::GD - RefineLds<D>::HD);
  // Two-wave variant with the refinement fused: no LDS for [X | H_dv | f_dv] (two waves per SIMD
  // need <= 20 KB per wave), the refinement reads them from the workspace (L2 / Infinity Cache)
  // (the pointers are formed after the interior-point loop: nothing extra lives across it)
  // (so does a model with wheel rows: its LDS block holds the rows A~ instead)
  constexpr bool kRefG = RF == kRfFused && (!SMALL || D::WH);
  constexpr bool WHR = D::WH && RF == kRfFused;   // the wheel rows' rotated Newton systems
  // the one-wave fused refinement with X in Hr's LDS region (Go2): its steps scheduled for a lone
  // wavefront, bitwise the general steps' results.  (WaLTER's one-wave kernels, NV <= 16 and no
  // second dot-product pass to fold, keep the general steps: with these they measured 0.5 %
  // slower and spilled 12 more SGPRs, profiles/r09/refine/)
  constexpr bool kLean = kXinHr && !kRefG;
  using WL = WheelLds<D>;
  WheelRot W = wheel_rot<D>(B + LY::IL);   // (osc_ipm_wheel.hpp; dead without wheel rows)
  // Hr columns are addressed as wave-uniform base (SGPR pair) + 32-bit lane offset + immediate:
  // 64-bit per-lane address registers for 48 loads do not fit, and their spill reloads
  // (scratch loads share vmcnt) used to serialise the whole prefetch.
  // (resume pass: the rows' envs are anywhere in the batch -- the base is the workspace itself
  // and the lane offset the env's whole one; launch_t keeps nenv x WS below 2^32 doubles)
  const double* __restrict__ wsw =
      ws + (CP == kCpResume ? size_t{0} : static_cast<size_t>(blk) * kEnvPerWave * D::WS) +
      D::W_HR;   // L2-resident
  const unsigned lane_off =
      static_cast<unsigned>(CP == kCpResume ? env : env - blk * kEnvPerWave) *
      static_cast<unsigned>(D::WS);
  double* sG = B + LY::I_G;
  double* sVy = B + LY::I_VY;
  double* sVy2 = B + LY::I_VY2;
  double* sVr = B + LY::I_VR;
  double* sDr = B + LY::I_DR;
  double* sMask = B + LY::I_MASK;
  double* sTau = B + LY::I_TAU;
  double* sXb = B + LY::I_XB;

  STAMP_DECL
  STAMP_BEGIN();
  // stage [g (| Hr)] (the workspace prefix has the LDS layout) and the mask: all loads in
  // flight before the first LDS store
  static_assert(LY::STAGE % 2 == 0 && NC <= kRow, "staging layout");
  {
    Batch2<LY::STAGE / 2, kRow> bs;
    bs.load(ws + static_cast<size_t>(env) * D::WS, l);
    const double mk = gmask[static_cast<size_t>(env) * NC + (l < NC ? l : 0)];
    if constexpr (RF == kRfFused && !kRefG && !kXinHr) {
      // the refinement's own LDS block is free all along: its [X | H_dv | f_dv] is staged now,
      // in the same memory latency (with Hr in LDS, [H_dv | f_dv] and X come by DMA later instead)
      static_assert(RefineLds<D>::SIZE % 2 == 0 && D::W_X % 2 == 0, "16-byte staging");
      Batch2<RefineLds<D>::SIZE / 2, kRow> bx;
      bx.load(ws + static_cast<size_t>(env) * D::WS + D::W_X, l);
      bx.store(sRX, l);
    }
    if constexpr (WHR) {   // T, the pin map, q1
      const double* we = ws + static_cast<size_t>(env) * D::WS;
#pragma unroll 8
      for (int p = l; p < NY * NY; p += kRow) W.T[(p / NY) * WL::TST + p % NY] = we[D::W_T + p];
      for (int p = l; p < NY; p += kRow) W.Pin[p] = we[D::W_PIN + p];
      if (l < D::NW) {
        W.Q1[l] = we[D::W_AW + l * NY1P + NY];
        W.Nu[l] = 0.0;
      }
    }
    bs.store(B, l);
    if (l < NC) sMask[l] = mk;
  }
  const double* sHr = B + LY::I_HR;
  if constexpr (HRL && D::HRC) {   // the workspace's compact Hr -> its full LDS layout, once
    const int ca = l, cb = l + kRow < NY ? l + kRow : NY - 1;   // this lane's two columns
    // fused refinement: the compact block is copied whole (16-byte loads) into the refinement's
    // LDS region -- free until the [H_dv | f_dv] DMA of the refinement -- and expanded from there
    // (per-lane addresses into LDS, not into L2); otherwise read from the workspace directly
    const double* src = wsw + lane_off;
    if constexpr (kXinHr) {
      static_assert(D::HR_SIZE % 2 == 0 && D::HR_SIZE <= refine_lds_extra<D, SMALL, RF>() &&
                    D::W_HR % 2 == 0, "compact Hr staged in the refinement region");
      Batch2<D::HR_SIZE / 2, kRow> bh;
      bh.load(ws + static_cast<size_t>(env) * D::WS + D::W_HR, l);
      bh.store(B + LY::IL, l);
      wave_sync();
      src = B + LY::IL;
    }
#pragma unroll
    for (int i0 = 0; i0 < NY; i0 += 8) {
      double hv0[8], hv1[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        hv0[i] = i0 + i < NY ? src[hr_off<D>(i0 + i, ca)] : 0.0;
        hv1[i] = i0 + i < NY ? src[hr_off<D>(i0 + i, cb)] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i0 + i < NY) {
          const_cast<double*>(sHr)[(i0 + i) * NY + ca] = hv0[i];
          if (l + kRow < NY) const_cast<double*>(sHr)[(i0 + i) * NY + cb] = hv1[i];
        }
      }
    }
  }
  if constexpr (HRH) {   // Hr's first column slot, once per solve
    static_assert(NY % 2 == 0 && D::WS % 2 == 0 && D::W_HR % 2 == 0, "16-byte Hr row loads");
#pragma unroll
    for (int i0 = 0; i0 < NY; i0 += 8) {   // (eight loads in flight: few registers live here)
      double hv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        hv[i] = i0 + i < NY ? wsw[lane_off + static_cast<unsigned>(hr_off<D>(i0 + i, l))] : 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i0 + i < NY) sHh[(i0 + i) * kRow + l] = hv[i];
    }
  }
  wave_sync();

  // ---- inequality rows of this lane: r = l + 16 t.  Only (active, h) are kept; the row's
  // kind (torque bound q / sign, or contact k / pyramid side) is recomputed from r. ----
  bool act[NRL];
  double h[NRL];
  // ENV: this env's friction and fz bounds (every lane of the row reads the same address) and
  // their validity; the torque box is checked joint by joint in the loop (each lane holds one side
  // of a joint's box and reads both)
  double env_mu = 0.0, env_zl = 0.0, env_zu = 0.0;
  bool env_bad = false;
  if constexpr (ENV) {
    const size_t e = static_cast<size_t>(env);
    env_mu = EP.mu ? EP.mu[e] : P->mu;
    env_zl = EP.fz_lb ? EP.fz_lb[e] : P->z_lb[2];
    env_zu = EP.fz_ub ? EP.fz_ub[e] : P->z_ub[2];
    env_bad = !isfinite(env_mu) || env_zl != env_zl || env_zu != env_zu;
  }
#pragma unroll
  for (int t = 0; t < NRL; ++t) {
    const int r = l + kRow * t;
    act[t] = false;
    h[t] = 0.0;
    if (r < 2 * NU) {
      const int q = r >> 1;
      const double sg = (r & 1) ? -1.0 : 1.0;
      double bnd;
      if constexpr (ENV) {
        const size_t eq = static_cast<size_t>(env) * NU + q;
        const double lbq = EP.u_lb ? EP.u_lb[eq] : P->u_lb[q];
        const double ubq = EP.u_ub ? EP.u_ub[eq] : P->u_ub[q];
        env_bad = env_bad || !(lbq < ubq);   // (what osc_model_create refuses; a NaN fails it too)
        bnd = (r & 1) ? lbq : ubq;
      } else {
        bnd = (r & 1) ? P->u_lb[q] : P->u_ub[q];
      }
      act[t] = fabs(bnd) < P->inf_thresh;
      h[t] = sg * bnd;                                     // the row is +-y_q
    } else if (r < MI) {
      const int k = (r - 2 * NU) / 6, rt = (r - 2 * NU) % 6;
      const double m = sMask[k];
      if (m != 0.0) {
        if (rt < 4) {
          act[t] = true;                                   // friction pyramid, bineq = 0
        } else if (rt == 4) {
          const double lb = (ENV ? env_zl : P->z_lb[2]) * m;   // -fz <= -lb
          act[t] = fabs(lb) < P->inf_thresh;
          h[t] = -lb;
        } else {
          const double ub = (ENV ? env_zu : P->z_ub[2]) * m;   // fz <= ub
          act[t] = fabs(ub) < P->inf_thresh;
          h[t] = ub;
        }
      }
    }
  }
  const double mu_f = ENV ? env_mu : P->mu;
  if constexpr (ENV) env_bad = row_max(env_bad ? 1.0 : 0.0) != 0.0;   // the env's 16 lanes agree
  // Rows of the initial least-squares fit (Hr + G'G) y0 = -g + G'h: every active row except
  // fz <= big_number, which would drag fz to ~big_number/2 together with fz >= 0 and start
  // the torque rows far outside their box (tools/ipm_model.py "y0_nofz": Go2 lockstep
  // iterations 14.9 -> 12.6, worst case 22 -> 18).
  // (the set-up loop above and this lambda stay in the body, not in osc_ipm_rows.hpp: as
  // functions they cost the two-wave WaLTER kernels scratch)
  auto init_ls = [&](int t) -> bool {
    const int r = l + kRow * t;
    return act[t] && !(r >= 2 * NU && (r - 2 * NU) % 6 == 5);
  };
  STAMP_END(0);

  // variable slots of this lane: j = l + 16 s
  const int j0 = l, j1 = l + kRow;
  const bool v1 = j1 < NY;
  const int jj1 = v1 ? j1 : NY - 1;
  const int jk0 = (j0 >= NU) ? (j0 - NU) / 3 : -1, jc0 = (j0 >= NU) ? (j0 - NU) % 3 : 0;
  const int jk1 = (v1 && j1 >= NU) ? (j1 - NU) / 3 : -1, jc1 = (j1 >= NU) ? (j1 - NU) % 3 : 0;
  const RowLane L{l, j0, j1, jj1, v1, jk0, jc0, jk1, jc1, mu_f};   // (osc_ipm_rows.hpp)

  constexpr int NW = D::NW;
  // rq: the rows' residual at the current y, on the pinned slots (q1 at the start, y = 0)
  double rq0 = 0.0, rq1 = 0.0, rwmax = 0.0;
  if constexpr (WHR) rot_load_pins<D>(W, L);
  rq0 = W.pin0 ? W.q10 : 0.0;
  rq1 = W.pin1 ? W.q11 : 0.0;

  double c0[NY], c1[NY];
  double dinv0, dinv1;
  // One-wave variant whose Hr does not fit the LDS (WaLTER: 32 x 32 x 4 envs): the lane's two Hr
  // columns are loaded once and kept in registers across the iterations (the one-wave kernel has
  // 512 of them, AGPRs included) instead of being re-read from L2 every iteration.
  // (not with wheel rows: their per-iteration products need the registers; Hr comes from L2)
  constexpr bool kHrReg = SMALL && !HRL && !D::WH;
  double hr0[kHrReg ? NY : 1], hr1[kHrReg ? NY : 1];
  if constexpr (kHrReg) {
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      hr0[i] = wsw[lane_off + static_cast<unsigned>(hr_off<D>(i, j0))];
      hr1[i] = wsw[lane_off + static_cast<unsigned>(hr_off<D>(i, jj1))];
    }
  }
  // Hr columns j0, j1 (and their diagonal entries) -> registers; re-issued at the end of every
  // iteration so the loads fly while the step is applied and the next residuals are formed.
  auto load_hr = [&]() {
    // column bases formed here, every time (hidden from loop-invariant hoisting): kept live
    // across the loop they get spilled, and spill reloads wait on vmcnt(0)
    if constexpr (HRL) {
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        c0[i] = sHr[i * NY + j0];
        c1[i] = sHr[i * NY + jj1];
      }
    } else if constexpr (kHrReg) {
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        c0[i] = hr0[i];
        c1[i] = hr1[i];
      }
    } else if constexpr (HRH) {
      unsigned off = lane_off;
      asm volatile("" : "+v"(off));
      // column jj1 = row jj1: this lane's contiguous NY doubles, two per 16-byte load
      const double* p1 = wsw + off + hr_off<D>(jj1, 0);   // (row jj1 of A when compact)
#pragma unroll
      for (int i = 0; i < NY; ++i) c1[i] = p1[i];
#pragma unroll
      for (int i = 0; i < NY; ++i) c0[i] = sHh[i * kRow + l];
    } else {
      unsigned off = lane_off;
      asm volatile("" : "+v"(off));
      const double* p = wsw + off;
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        c0[i] = p[hr_off<D>(i, j0)];
        c1[i] = p[hr_off<D>(i, jj1)];
      }
    }
  };
  const double hdg0 =
      HRL ? sHr[j0 * NY + j0] : wsw[lane_off + static_cast<unsigned>(hr_off<D>(j0, j0))];
  const double hdg1 =
      HRL ? sHr[jj1 * NY + jj1] : wsw[lane_off + static_cast<unsigned>(hr_off<D>(jj1, jj1))];
  load_hr();
  // (ENV: an invalid env's gradient is NaN -- every iterate of it is, its wave-mates' never)
  const double g0 = (ENV && env_bad) ? __builtin_nan("") : sG[j0],
               g1 = (ENV && env_bad) ? __builtin_nan("") : sG[jj1];
  double y0 = 0.0, y1 = 0.0;
  double s[NRL], lam[NRL];
#pragma unroll
  for (int t = 0; t < NRL; ++t) {
    s[t] = 1.0;
    lam[t] = 0.0;
  }
  double nact = 0.0;
#pragma unroll
  for (int t = 0; t < NRL; ++t) nact += act[t] ? 1.0 : 0.0;
  const double m_act = row_sum(nact);
  bool done = !valid;
  int32_t st = OSC_SOLVE_MAX_ITER;
  int it_done = 0;
  bool stalled = false;   // WH: stopped by the late-stall exit, not at mu <= eps_mu

  // One loop body for everything, so factorisation and solve code exist once (I-cache).
  // it == -1 builds the initial point (Mehrotra-style):
  //   (Hr + G'G) y0 = -g + G'h,  s = h - G y0,  lambda = G y0 - h,  both shifted positive.
  // The four environments of the wave iterate in lockstep; a converged one stops moving
  // (step 0) until the slowest has converged.
  // Primal residual rp = G y + s - h.  Every step takes ds = -rp - G dy exactly, so the new
  // residual is (1 - alpha) rp up to rounding, whatever the accuracy of the linear solve: it is
  // carried while mu > 1e-6 and formed from scratch after the initial point and once mu is
  // small, where the ~1e-12 rounding the carried value ignores is as large as the active
  // slacks (tools/ipm_model.py "rpcarry1e-6": same iterations as recomputing every time).
  // rd, which does depend on the solve's accuracy, is recomputed every iteration.
  double rp[NRL];
#pragma unroll
  for (int t = 0; t < NRL; ++t) rp[t] = 0.0;
  // The dual residual rd = Hr y + g + G'lam is carried the same way (round 6): with the Newton
  // system K dy = G'w - rd solved, Hr dy + G'dlam = G'w - rd - G'DG dy + G'(-w + DG dy) = -rd,
  // so the step leaves (1 - alpha) rd -- up to the solve's rounding, which is why it is formed
  // from scratch (Hr y by DPP broadcasts, G'lam from LDS: 8 % of an iteration) whenever rp is:
  // at iteration 0, after a re-centring and once mu <= 1e-6.  Per env (an env's rd never depends
  // on its wave-mates'); a wave forms it only when one of its running envs needs it.  (Not with
  // wheel rows: their rd lives in rotated coordinates.)
  constexpr bool kRdCarry = !D::WH;
  double rdc0 = 0.0, rdc1 = 0.0;
  bool rd_fresh = true, rd_have = false;   // (rd_have: a compaction's resume pass starts mid-solve)
  // Warm start (the reference's OsqpSolver::SetWarmStart, operational_space_controller.h:525):
  // an env whose warm state is valid starts from the previous tick's y and lambda, with the
  // slacks s = max(h - G y, delta) and lambda = max(lambda_prev, delta) (rows active now but not
  // before start at delta).  A wave whose four envs are all warm skips the least-squares initial
  // point; otherwise it runs it and the warm rows override it at iteration 0.  An env without
  // active rows always starts cold (its initial point is then the exact optimum).
  // (nothing warm-related stays live across the loop but one lane mask: the 2-wave variant has
  // no registers to spare)
  // A contact-mode switch (mask differs from the state's) changes the QP's rows: start cold.
  bool warm = false;
  if (WARM && !fixup) {
    const double* w0 = gwarm + static_cast<size_t>(env) * D::WW;
    const double same = (l >= NC || w0[D::WW_M + l] == sMask[l]) ? 1.0 : 0.0;
    warm = row_min(same) == 1.0 && w0[0] == 1.0 && m_act > 0.0;
  }
  bool any_warm = false, all_warm = false;
  if constexpr (WARM) {
    any_warm = __ballot(warm) != 0;
    all_warm = __ballot(!warm) == 0;
  }
  // Compaction (ParkArgs): the park slot's state, exactly as the park pass left it at the top of
  // iteration park_it (the y slots of every lane, v1 or not; s, lambda, rp of every row slot).
  const int pslot = env_raw < cnt ? env_raw : cnt - 1;
  auto park_at = [&](int slot) {
    return PA.park + static_cast<size_t>(slot) * park_doubles<D>();
  };
  auto resume_state = [&]() -> int {
    if constexpr (CP == kCpResume) {
      const double* pk = park_at(pslot);
      y0 = pk[l];
      y1 = pk[kRow + l];
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        s[t] = pk[2 * kRow + l + kRow * t];
        lam[t] = pk[2 * kRow + NRL * kRow + l + kRow * t];
        rp[t] = pk[2 * kRow + 2 * NRL * kRow + l + kRow * t];
      }
      rdc0 = pk[2 * kRow + 3 * NRL * kRow + l];
      rdc1 = pk[3 * kRow + 3 * NRL * kRow + l];
      rd_have = true;
      sVy[j0] = y0;
      if (v1) sVy[j1] = y1;
      wave_sync();
    }
    return PA.park_it;
  };
  bool parked = false;   // park pass: this row's env went to the park area (no outputs here)
  bool refined = false;
  // interior-point stop (the warm fix-up pass is a rescue: its cold solve runs to mu <= 1e-12)
  const double eps_run = (kFix && fixup) ? fmin(P->eps_mu, 1e-12) : P->eps_mu;
  // read once, ahead of the loop: its wave_sync()s are memory barriers to the compiler, so a
  // P->field in the loop body is a scalar load and an s_waitcnt lgkmcnt(0) in every iteration --
  // a cache round trip with nothing to hide it, and a wait for every LDS read in flight as well
  const int max_iter = P->max_iter, restart_iter = P->restart_iter;
  const int warm_restart = WARM ? P->warm_restart : 0;
  // The start, peeled: the one-wave kernels with Hr in LDS (Go2) run iteration -1
  // as a straight-line block ahead of the loop, which then begins at it = 0 as it does for an
  // all-warm wave and a resume pass.  The iteration's body (osc_ipm_iter.hpp) is compiled twice
  // for them, `init` a compile-time constant each time: the loop's copy holds no select or branch
  // on it, and the start's copy the same operations on the same values in the same order for
  // everything live there -- what it loses is dead at the start (the ratio test, dl, dsdl, a_aff,
  // the second pass, mu and the stop test; the warm take-over belongs to iteration 0; the
  // re-centring cannot match: the host refuses restart_iter < 0 and warm_restart < 0).  A lone
  // wave pays an issue slot per instruction whatever it is, and the shared body cost every regular
  // iteration its selects on `init`.  Every other kernel keeps the one loop, `init` a run-time
  // value: its code is what it was.  (Go2's one-wave kernels without the fused refinement too:
  // peeled, the warm one of them spilled 10 more SGPRs; and the two-model kernels, PAIR, which
  // hold a second model's body beside Go2's: 3 and 10 more.)
  constexpr bool kPeel = kLean && !PAIR;
  // The refresh of the rows' residual runs only for envs that go on iterating:
  // kFreshDone leaves out the envs done on entry, which changes no register of any env; the
  // peeled kernels (kFreshStop) also the env that stops in the iteration, whose rp then differs
  // from what it was inside the done env and in no output.  kFlatRecentre: the re-centring's rows
  // branch-free (Gv_all, selects) in the cold one-wave kernels; the warm ones keep the
  // exec-masked arm (branch-free they spilled 2 to 6 more SGPRs).  The two-model kernels (PAIR)
  // keep the parent's body in all three: with the first and the third the mixed workload
  // measured 2.3 % slower.
  constexpr bool kFreshDone = !PAIR;
  constexpr bool kFreshStop = kPeel;
  constexpr bool kFlatRecentre = SMALL && !WARM && !PAIR;
  if constexpr (REFINE) {
    // the interior point's result for this env (osc_ipm_kernel, W_SOL): y, and the active rows
    // as lambda > s with lambda = q > 0
    static_assert(D::W_SOL - D::W_X == RefineLds<D>::SIZE && D::W_X % 2 == 0 &&
                  RefineLds<D>::SIZE % 2 == 0, "refinement LDS block = workspace [X | H_dv | f_dv]");
    {
      Batch2<RefineLds<D>::SIZE / 2, kRow> bx;
      bx.load(ws + static_cast<size_t>(env) * D::WS + D::W_X, l);
      bx.store(sRX, l);
    }
    const double* sol = ws + static_cast<size_t>(env) * D::WS + D::W_SOL;
    y0 = sol[j0];
    y1 = v1 ? sol[j1] : 0.0;
#pragma unroll
    for (int t = 0; t < NRL; ++t) {
      const double q = sol[even(NY) + l + kRow * t];
      lam[t] = q;
      s[t] = q > 0.0 ? 0.0 : 1.0;
    }
    st = static_cast<int32_t>(sol[even(NY) + NRL * kRow]);
    sVy[j0] = y0;
    if (v1) sVy[j1] = y1;
    wave_sync();
  } else if constexpr (kPeel) {
    if (CP != kCpResume && !all_warm) {
      do {   // (the body's `break` sits in its `!init` part: never reached here)
        constexpr bool init = true;
        constexpr int it = -1;
#include "osc_ipm_iter.hpp"
      } while (false);
    }
    for (int it = CP == kCpResume ? resume_state() : 0;; ++it) {
      constexpr bool init = false;
#include "osc_ipm_iter.hpp"
    }
  } else
  for (int it = CP == kCpResume ? resume_state() : (all_warm ? 0 : -1);; ++it) {
    const bool init = it < 0;
#include "osc_ipm_iter.hpp"
  }
#ifdef OSC_STAMPS
  if constexpr (RF != kRfFused) STAMP_STORE();   // the fused pass stores after its refinement
#endif
  if constexpr (RF == kRfNone) {   // hand the result to the refinement kernel
    if (write_out) {
      // (the W_SOL block is written here and read by nothing else in this kernel)
      double* sol = const_cast<double*>(ws) + static_cast<size_t>(env) * D::WS + D::W_SOL;
      sol[j0] = y0;
      if (v1) sol[j1] = y1;
#pragma unroll
      for (int t = 0; t < NRL; ++t)
        sol[even(NY) + l + kRow * t] = (act[t] && lam[t] > s[t]) ? lam[t] : 0.0;
      if (l == 0) sol[even(NY) + NRL * kRow] = static_cast<double>(st);
    }
  }

  // ---------------- full-space refinement (torque coordinates) ---------------
  // Hr is an explicitly formed fp64 product X'H_dv X whose condition number reaches ~1e10, so the
  // interior point's optimum of the reduced QP sits up to ~1e-5 (normwise) off the optimum of
  // the QP the reference defines.  Iterative refinement on the active set of the converged
  // iterate (rows with lambda > s) removes that: the residual is formed in factored form,
  //   r = X_y' (H_dv (X [y;1]) + f_dv) + 2 (w_tau + w_reg) u + 2 w_reg z + G_A' mu,
  // which never goes through Hr, and the correction comes from one LDL^T of
  // K_A = Hr + D G_A'G_A (active rows by penalty D = refine_penalty x max diag Hr; dependent rows
  // of a contact at the pyramid apex are harmless there):
  //   K_A dy = -r - D G_A'(G_A y - h_A),   mu += D (G_A (y + dy) - h_A),   y += dy.
  // Two steps take the worst envs of 32,768-env batches from 7e-6 to ~1e-13 of the exact optimum
  // (tools/ipm_model.py + the refinement study in DESIGN.md).  Envs that did not converge keep
  // their iterate; a refinement that moves y by more than 1e-3 (relative) or is not finite is
  // discarded.
  // (wheel rows: a fixed step count, the same whether or not the duals are asked for, so x and tau
  // do not depend on want_dual -- the rows' multipliers converge more slowly than y, hence 12)
  if constexpr (CP == kCpPark) write_out = write_out && !parked;   // the resume pass writes them
  const int refine_steps = P->refine_steps;
  if constexpr (RF != kRfNone) {
    // WH: an env the interior point left at max_iter is refined too (its rotated Newton systems
    // can stall short of eps_mu with the active set already right): a kept refinement -- no row
    // violated, no multiplier of the wrong sign, its last step converged -- is a KKT point of the
    // strictly convex QP, i.e. its optimum, and the env reports OK
    const bool mine = valid && (st == OSC_SOLVE_OK || (WHR && st == OSC_SOLVE_MAX_ITER));
    if (P->refine_steps > 0 && __ballot(mine) != 0) {
      const double dpen = P->refine_penalty * row_max(fmax(fabs(hdg0), fabs(hdg1)));
      const double ytol = 1e-9 * (1.0 + row_max(fmax(fabs(y0), v1 ? fabs(y1) : 0.0)));
      // the wheel rows keep round 3's fixed steps and move-bound acceptance (their refinement runs
      // refine_steps steps; the generic KKT acceptance measured no different on them)
      constexpr bool kOldWh = WHR;
      double Dr[NRL], mur[NRL];
      // WH: a row whose slack is within 1e-6 of the bound is active too -- next to the rows'
      // Schur solves the interior point's multipliers of a weakly active row can be off by orders
      // of magnitude while y is right (numpy model: 11 of 512 tumbling refinements rejected -> 0)
      const double stol =
          D::WH ? 1e-6 * (1.0 + row_max(fmax(fabs(y0), v1 ? fabs(y1) : 0.0))) : -1.0;
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        const bool a = act[t] && (lam[t] > s[t] || s[t] <= stol);
        Dr[t] = a ? dpen : 0.0;
        mur[t] = a ? lam[t] : 0.0;
      }
      const double wu = 2.0 * (P->w_torque + P->w_reg), wz = 2.0 * P->w_reg;
      double ya0 = y0, ya1 = y1;
      bool viol_env = false;
      const double* wenv = ws + static_cast<size_t>(env) * D::WS;
      const double* rX = kRefG ? wenv + D::W_X : sRX;
      const double* rH = kRefG ? wenv + D::W_HD : sRH;
      const double* rG = kRefG ? wenv + D::W_GD : sRG;
      constexpr int kUr = kRefG ? 2 : 32;   // workspace reads: few in flight (registers)
      double dlast = 0.0;   // the last refinement step's size (its convergence test)
      bool settled = false;                          // this env's final round is done
      const double yscale = row_max(fmax(fabs(y0), v1 ? fabs(y1) : 0.0));
      double yk0 = 0.0, yk1 = 0.0, dk = 0.0, nuk = 0.0;   // its result (WH: step, multiplier)
      // (no wheel rows) steps run until the env's own step has converged -- at least
      // refine_steps, at most kRefineMaxSteps per round -- and then the env is frozen (its later
      // lockstep steps are zero), so its result does not depend on its wave-mates' step counts
      bool conv = false;
      // rounds: a row the refined point violates was active at the optimum with a vanishing
      // multiplier (lambda and s both ~1e-6 when the interior point stops): it joins the active
      // set, a row whose multiplier came out negative leaves it, and the round repeats from the
      // interior point's iterate with the multipliers carried over (numpy model of the kernel on
      // joint-state batches, tools/kkt_study.py: <= 3 rounds, <= 9 steps)
      for (int round = 0; round < (WHR ? 5 : kRefineRounds); ++round) {
        STAMP_BEGIN();
#ifdef OSC_STAMPS
        st_acc[10] += 1ull << 40;   // rounds, in the top bits of the assembly+LDL slot
#endif
        if (round > 0) {   // c0 / c1 hold the last round's factor
          if constexpr (kXinHr && D::HRC && !WARM && !PAIR) {
            // Hr's LDS region holds X now: Hr columns from the (L2-resident) workspace.  The same
            // stored doubles as hr_off<D>(i, j0) and hr_off<D>(i, jj1) name, addressed through the
            // compact layout's structure -- j0 < 16 <= jj1 always: four per-lane offsets plus
            // immediates, and a select between two of them for the packed triangle's 16 entries --
            // instead of 2 NY computed offsets, which the compiler hoists ahead of the rounds, onto
            // the path of every wave, while 3 waves in 1,024 get here.  (Not the warm kernel: it
            // spilled 4 more SGPRs with this; it and the two-model kernels keep the computed
            // offsets below.)
            static_assert(hr_col_offsets_match<D>(), "hr_col_lo / hr_col_hi = hr_off");
            const double* pa = wsw + lane_off;
            unsigned a0 = static_cast<unsigned>(j0), a1 = static_cast<unsigned>(jj1);
            asm volatile("" : "+v"(a0), "+v"(a1));   // (formed here, not ahead of the rounds)
#pragma unroll
            for (int i = 0; i < NY; ++i) {
              c0[i] = pa[hr_col_lo<D>(i, a0)];
              c1[i] = pa[hr_col_hi<D>(i, a1)];
            }
          } else if constexpr (kXinHr) {
            // (the same columns, every offset computed)
#pragma unroll
            for (int i = 0; i < NY; ++i) {
              c0[i] = wsw[lane_off + static_cast<unsigned>(hr_off<D>(i, j0))];
              c1[i] = wsw[lane_off + static_cast<unsigned>(hr_off<D>(i, jj1))];
            }
          } else {
            load_hr();
          }
        }
#pragma unroll
        for (int t = 0; t < NRL; ++t) sDr[l + kRow * t] = Dr[t];
        ya0 = y0;
        ya1 = y1;
        sVy[j0] = y0;
        if (v1) sVy[j1] = y1;
        wave_sync();
        // K_A in c0 / c1 (they hold Hr's columns)
        double dg0 = hdg0, dg1 = hdg1, du = 0.0;
        if constexpr (WHR) {
          wave_sync();
          assemble_rot<D>(W, L, sDr, c0, c1, dg0, dg1);
        } else {
          const double2 dd = *reinterpret_cast<const double2*>(sDr + 2 * (j0 < NU ? j0 : 0));
          du = (j0 < NU) ? dd.x + dd.y : 0.0;
          dg0 += du;
        }
        if constexpr (!WHR) add_contact_blocks<D>(L, sDr, c0, c1, dg0, dg1);
        // HRL: X is copied global -> LDS by DMA (no registers) into Hr's region -- free now, K_A
        // is in registers -- issued before the factorisation, waited for after it, so its latency
        // hides behind the LDL^T.  A DMA wave-instruction writes 16 B per lane to a wave-uniform
        // base + 16 B x lane, so each one fills 1 KB of ONE env's block with all 64 lanes (every
        // lane loads that env's chunk): compile-time bases, no per-env branches.
        if constexpr (kXinHr) {
          constexpr int NCH = D::NV * D::NY1P / 2;               // 16-byte chunks of X
          constexpr int NT = (NCH + kWave - 1) / kWave;
          static_assert(D::NV * D::NY1P <= even(NY * NY) && D::W_X % 2 == 0 &&
                        NT * kWave * 2 <= even(NY * NY), "X (whole DMA rows) in Hr's region");
          if (round == 0) {
            // the loop's last Hr column reads of this region (load_hr) have returned before the DMA
            // overwrites it (K_A's assembly consumed only some of them)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            static_for<0, kEnvPerWave>([&](auto G) {
              constexpr int g = decltype(G)::value;
              const int eg = CP == kCpResume ? __builtin_amdgcn_readlane(env, g * kRow)
                             : (blk * kEnvPerWave + g < nenv ? blk * kEnvPerWave + g : nenv - 1);
              const double2* src =
                  reinterpret_cast<const double2*>(ws + static_cast<size_t>(eg) * D::WS + D::W_X);
              static_for<0, NT>([&](auto T) {
                constexpr int t = decltype(T)::value;
                const int c = lane + kWave * t < NCH ? lane + kWave * t : NCH - 1;
#if defined(__HIP_DEVICE_COMPILE__)   // (a device builtin: the host pass never runs this body)
                __builtin_amdgcn_global_load_lds(src + c, sm + g * kEnvLds + LY::I_HR + 2 * kWave * t,
                                                 16, 0, 0);
#else
                (void)src;
                (void)c;
#endif
              });
              {
                // [H_dv | f_dv] the same way, into the block's refinement region (not staged with
                // the prologue's loads: 11 of the 27 MB every wave requests at once at 4,096 envs)
                constexpr int NCH2 = (RefineLds<D>::SIZE - RefineLds<D>::HD) / 2;
                constexpr int NT2 = (NCH2 + kWave - 1) / kWave;
                static_assert(NT2 * kWave * 2 == refine_lds_extra<D, SMALL, RF>() &&
                              D::W_HD == D::W_X + RefineLds<D>::HD && D::W_HD % 2 == 0,
                              "[H_dv | f_dv] (whole DMA rows) in the refinement region");
                const double2* src2 =
                    reinterpret_cast<const double2*>(ws + static_cast<size_t>(eg) * D::WS + D::W_HD);
                static_for<0, NT2>([&](auto T) {
                  constexpr int t = decltype(T)::value;
                  const int c = lane + kWave * t < NCH2 ? lane + kWave * t : NCH2 - 1;
#if defined(__HIP_DEVICE_COMPILE__)
                  __builtin_amdgcn_global_load_lds(src2 + c, sm + g * kEnvLds + LY::IL + 2 * kWave * t,
                                                   16, 0, 0);
#else
                  (void)src2;
                  (void)c;
#endif
                });
              }
            });
          }
        }
        wave_sync();
        ldl_rows<NY, SMALL>(c0, c1, B + LY::I_DINV, l, dinv0, dinv1, 1e-13 * dg0, 1e-13 * dg1, du);
        if constexpr (kXinHr) {
          if (round == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // X has landed
        }
        wave_sync();
        STAMP_END(8);   // (the loop's slot 8 doubles as the refinement's LDL)
        STAMP_BEGIN();
        conv = false;
        if constexpr (kLean) {
        for (int k = 0; k < kRefineMaxSteps; ++k) {
          // One wave, [X | H_dv | f_dv] in LDS: the same chains per output element as the general
          // step below, scheduled for a lone wavefront, which waits out every LDS hand-off and
          // every branch alone (DESIGN.md §5 "The refinement's steps").  Four hand-offs (y -> dv ->
          // gx -> r, d -> mu) where the general step has seven; the rows' products branch-free
          // (Gv_all); both row-space vectors stored at the top -- they need nothing of this step
          // (sDr is free here: gx goes to dv's slot, whose reads precede its store in program order)
          // -- so both G' products read beside the X'gx operands; and the rows past the 16th as
          // second chains of the lanes' own loops (their row clamped, their store masked), not as
          // an exec-masked pass of their own.
          constexpr int NT = (NV + kRow - 1) / kRow;
          double R3[NRL];
          {
            double g3[NRL];
            Gv_all<D>(L, act, sVy, g3);
#pragma unroll
            for (int t = 0; t < NRL; ++t) {
              R3[t] = (Dr[t] != 0.0) ? g3[t] - h[t] : 0.0;
              sVr[l + kRow * t] = mur[t];
              sDr[l + kRow * t] = Dr[t] * R3[t];
            }
          }
          int rr[NT];
          double acc[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            rr[t] = (l + kRow * t < NV) ? l + kRow * t : 0;   // (a lane past NV: row 0, unused)
            acc[t] = rX[rr[t] * NY1P + NY];
          }
          static_assert(NY % 2 == 0 && LY::I_VY % 2 == 0, "y read as 16-byte pairs");
#pragma unroll
          for (int i = 0; i < NY; i += 2) {
            const double2 yy = *reinterpret_cast<const double2*>(sVy + i);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              acc[t] = fma(rX[rr[t] * NY1P + i], yy.x, acc[t]);
              acc[t] = fma(rX[rr[t] * NY1P + i + 1], yy.y, acc[t]);
            }
          }
#pragma unroll
          for (int t = 0; t < NT; ++t)
            if (l + kRow * t < NV) sXb[l + kRow * t] = acc[t];
          wave_sync();
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = rG[rr[t]];
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const double di = sXb[i];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = fma(rH[rr[t] * NV + i], di, acc[t]);
          }
          wave_sync();
#pragma unroll
          for (int t = 0; t < NT; ++t)
            if (l + kRow * t < NV) sXb[l + kRow * t] = acc[t];
          wave_sync();
          double r0 = (j0 < NU ? wu : wz) * ya0, r1 = (jj1 < NU ? wu : wz) * ya1;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            r0 = fma(rX[i * NY1P + j0], sXb[i], r0);
            r1 = fma(rX[i * NY1P + jj1], sXb[i], r1);
          }
          double gm0, gm1, b0, b1;
          GTw2<D, SMALL>(L, sVr, gm0, gm1);
          GTw2<D, SMALL>(L, sDr, b0, b1);
          r0 += gm0;
          r1 += gm1;
          double d0 = -r0 - b0, d1 = -r1 - b1;
          ldl_solve_rows<NY>(c0, c1, dinv0, dinv1, d0, d1, l);
          const bool frz = conv;   // converged at an earlier step: no further move
          if (frz) {
            d0 = 0.0;
            d1 = 0.0;
          }
          sVy2[j0] = d0;
          if (v1) sVy2[j1] = d1;
          wave_sync();
          {
            double gd[NRL];
            Gv_all<D>(L, act, sVy2, gd);
#pragma unroll
            for (int t = 0; t < NRL; ++t) {
              double inc = Dr[t] * (gd[t] + R3[t]);
              in_vgpr(inc);   // (a product, then a sum: never one fma with mur)
              mur[t] += frz ? 0.0 : inc;
            }
          }
          ya0 += d0;
          ya1 += d1;
          sVy[j0] = ya0;
          if (v1) sVy[j1] = ya1;
          wave_sync();
          // (the general step's convergence test)
          const double dn = row_max(fmax(fabs(d0), v1 ? fabs(d1) : 0.0));
          if (!frz) dlast = dn;
          conv = conv || (k + 1 >= refine_steps && dn <= 1e-10 * (1.0 + yscale));
          if (k + 1 >= refine_steps && __ballot(mine && !conv) == 0) break;
        }
        } else
        for (int k = 0; k < (kOldWh ? refine_steps : kRefineMaxSteps); ++k) {
          // WH: X holds X^ = X'T, so dv = X^ [y^; 1] (y^ = T'y staged in sVy2, free until the step)
          // and the rows' residual at y comes with y^
          const double* yv = sVy;
          if constexpr (WHR) {
            double yh0, yh1;
            rot_in<D>(W, L, ya0, ya1, yh0, yh1);
            rq0 = W.pin0 ? yh0 + W.q10 : 0.0;
            rq1 = W.pin1 ? yh1 + W.q11 : 0.0;
            sVy2[j0] = yh0;
            if (v1) sVy2[j1] = yh1;
            wave_sync();
            yv = sVy2;
          }
          // dv = X [y; 1] (rows l, l + 16) -> sXb
#pragma unroll
          for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) {
            const int rr = l + kRow * t;
            if (rr < NV) {
              const double* xr = rX + rr * NY1P;
              double a = xr[NY];
#pragma unroll kUr
              for (int i = 0; i < NY; ++i) a = fma(xr[i], yv[i], a);
              sXb[rr] = a;
            }
          }
          wave_sync();
          // gx = H_dv dv + f_dv (rows l, l + 16) -> sDr[0 .. NV)
          double gxr[(NV + kRow - 1) / kRow];
#pragma unroll
          for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) {
            const int rr = l + kRow * t;
            gxr[t] = 0.0;
            if (rr < NV) {
              const double* hr = rH + rr * NV;
              double a = rG[rr];
#pragma unroll kUr
              for (int i = 0; i < NV; ++i) a = fma(hr[i], sXb[i], a);
              gxr[t] = a;
            }
          }
          wave_sync();
#pragma unroll
          for (int t = 0; t < (NV + kRow - 1) / kRow; ++t)
            if (l + kRow * t < NV) sDr[l + kRow * t] = gxr[t];
#pragma unroll
          for (int t = 0; t < NRL; ++t) sVr[l + kRow * t] = mur[t];
          wave_sync();
          if constexpr (D::WH && RF == kRfFused) {
            // gx <- (I - V'V) gx: X's columns are orthogonal to V (setup_env), so this changes
            // nothing in exact arithmetic, but it drops gx's large components along the rows'
            // constrained directions before X' multiplies them (numpy model: 5e-9 -> 1.5e-9 worst)
            const double* Vw = wenv + D::W_WV;
            double vg = 0.0;
            if (l < NW) {
#pragma unroll
              for (int j = 0; j < NV; ++j) vg = fma(Vw[l * NV + j], sDr[j], vg);
            }
            double corr[(NV + kRow - 1) / kRow];
#pragma unroll
            for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) corr[t] = 0.0;
            static_for<0, NW>([&](auto W) {
              constexpr int w = decltype(W)::value;
              const double bw = bcast_guarded<w>(vg);
#pragma unroll
              for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) {
                const int rr = l + kRow * t;
                corr[t] = fma(Vw[w * NV + (rr < NV ? rr : 0)], bw, corr[t]);
              }
            });
            wave_sync();
#pragma unroll
            for (int t = 0; t < (NV + kRow - 1) / kRow; ++t)
              if (l + kRow * t < NV) sDr[l + kRow * t] -= corr[t];
            wave_sync();
          }
          // r_j = X[:, j]' gx + diag_j y_j + (G_A' mu)_j for the lane's two variables
          // (WH, in y^: X^'gx + T'(W y + G_A' mu))
          double r0 = (j0 < NU ? wu : wz) * ya0, r1 = (jj1 < NU ? wu : wz) * ya1;
          double gm0, gm1;
          if constexpr (WHR) {
            GTw2<D, SMALL>(L, sVr, gm0, gm1);
            r0 += gm0;
            r1 += gm1;
            rot_in<D>(W, L, r0, r1, r0, r1);
          }
#pragma unroll kUr
          for (int i = 0; i < NV; ++i) {
            r0 = fma(rX[i * NY1P + j0], sDr[i], r0);
            r1 = fma(rX[i * NY1P + jj1], sDr[i], r1);
          }
          if constexpr (!WHR) {   // (this order: the feature-off results stay bitwise)
            GTw2<D, SMALL>(L, sVr, gm0, gm1);
            r0 += gm0;
            r1 += gm1;
          }
          if constexpr (WHR) {
            // the pinned coordinates of r^ are Q (grad f + G_A' mu): their negatives are the rows'
            // multipliers (least squares; the last step's stand)
            const double p0v = W.Pin[j0], p1v = W.Pin[jj1];
            if (p0v >= 0.0) W.Nu[static_cast<int>(p0v)] = -r0;
            if (v1 && p1v >= 0.0) W.Nu[static_cast<int>(p1v)] = -r1;
          }
          wave_sync();
          double R3[NRL];
#pragma unroll
          for (int t = 0; t < NRL; ++t) {
            R3[t] = (Dr[t] != 0.0) ? Gv<D>(L, act, sVy, t) - h[t] : 0.0;
            sVr[l + kRow * t] = Dr[t] * R3[t];
          }
          wave_sync();
          double b0, b1;
          GTw2<D, SMALL>(L, sVr, b0, b1);
          if constexpr (WHR) rot_in<D>(W, L, b0, b1, b0, b1);
          double d0 = -r0 - b0, d1 = -r1 - b1;
          if constexpr (WHR) {
            d0 = W.pin0 ? -rq0 : d0;
            d1 = W.pin1 ? -rq1 : d1;
          }
          ldl_solve_rows<NY>(c0, c1, dinv0, dinv1, d0, d1, l);
          if constexpr (WHR) {
            rot_out<D>(W, L, d0, d1, d0, d1);
            dlast = row_max(fmax(fabs(d0), v1 ? fabs(d1) : 0.0));
          }
          const bool frz = !kOldWh && conv;   // converged at an earlier step: no further move
          if (frz) {
            d0 = 0.0;
            d1 = 0.0;
          }
          sVy2[j0] = d0;
          if (v1) sVy2[j1] = d1;
          wave_sync();
#pragma unroll
          for (int t = 0; t < NRL; ++t)
            mur[t] += frz ? 0.0 : Dr[t] * (Gv<D>(L, act, sVy2, t) + R3[t]);
          ya0 += d0;
          ya1 += d1;
          wave_sync();
          sVy[j0] = ya0;
          if (v1) sVy[j1] = ya1;
          wave_sync();
          if constexpr (!kOldWh) {
            // converged: the step fell below 1e-10 of the env's |y| (a row-wide scale: a lane
            // holding only near-zero variables must not hold the env to 1e-10 absolute)
            const double dn = row_max(fmax(fabs(d0), v1 ? fabs(d1) : 0.0));
            if (!frz) dlast = dn;
            conv = conv || (k + 1 >= refine_steps && dn <= 1e-10 * (1.0 + yscale));
            if (k + 1 >= refine_steps && __ballot(mine && !conv) == 0) break;
          }
        }
        // rows the refined point violates join the active set -- (no wheel rows) only the most
        // violated one, and then no row leaves this round: adding every violated row while dropping
        // every negative multiplier at once cycles on the joint-state envs whose interior point
        // missed one weakly active pyramid row (a period-3 cycle through 8 rounds, ~1e-4 of the
        // envs at joint_range 1.0, tests/golden/go2_unrefined_joint_states.npz; tools/kkt_study.py
        // one_change: every such env settles in <= 4 rounds on its exact optimum)
        double nviol = 0.0, vl = 0.0, gv[NRL];
        if constexpr (kLean) Gv_all<D>(L, act, sVy, gv);
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          gv[t] = (kLean ? gv[t] : Gv<D>(L, act, sVy, t)) - h[t];
          vl = fmax(vl, (act[t] && Dr[t] == 0.0 && gv[t] > ytol) ? gv[t] : 0.0);
        }
        const double vbest = WHR ? 0.0 : row_max(vl);
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          const bool v = act[t] && Dr[t] == 0.0 && gv[t] > ytol && (WHR || gv[t] == vbest);
          Dr[t] = v ? dpen : Dr[t];
          nviol += v ? 1.0 : 0.0;
        }
        {
          // ... and rows whose multiplier came out negative leave it (WH: its slack-based active
          // set can include a row the optimum leaves; otherwise a row the interior point's
          // lambda > s test took with a vanishing multiplier) -- (no wheel rows) in a round that
          // added none, and only the most negative one
          const bool drops = WHR || vbest == 0.0;   // (uniform over the env's row of lanes)
          double mmax = 0.0, mlo = 0.0;
#pragma unroll
          for (int t = 0; t < NRL; ++t) {
            mmax = fmax(mmax, Dr[t] != 0.0 ? fabs(mur[t]) : 0.0);
            mlo = fmin(mlo, Dr[t] != 0.0 ? mur[t] : 0.0);
          }
          const double mtol = 1e-9 * (1.0 + row_max(mmax));
          const double mworst = WHR ? 0.0 : row_min(mlo);
#pragma unroll
          for (int t = 0; t < NRL; ++t) {
            const bool leave = drops && Dr[t] != 0.0 && mur[t] < -mtol && (WHR || mur[t] == mworst);
            Dr[t] = leave ? 0.0 : Dr[t];
            // (its multiplier leaves with it: the residual sums G'mu over every row slot, and a
            // stale negative multiplier there would move the next round's fixed point off the
            // optimum while no test looks at that row any more)
            mur[t] = leave ? 0.0 : mur[t];
            nviol += leave ? 1.0 : 0.0;
          }
        }
        viol_env = mine && row_max(nviol) > 0.0;
        // a round whose steps have not converged asks for another one as well (it restarts
        // from the interior point's iterate with the multipliers carried over)
        const bool more =
            viol_env || (mine && (kOldWh ? dlast > 1e-10 * (1.0 + yscale) : !conv));
        // an env whose round ended without a violation is final: a further round that a wave-mate
        // asks for must not move it (its multipliers carry over between rounds), so each env's
        // result is independent of the envs sharing its wavefront -- and of the compaction's
        // packing (ParkArgs)
        if (mine && !more && !settled) {
          settled = true;
          yk0 = ya0;
          yk1 = ya1;
          if constexpr (WHR) {
            dk = dlast;
            nuk = l < NW ? W.Nu[l] : 0.0;
          }
        }
        STAMP_END(11);
        if (__ballot(more && !settled) == 0) break;
      }
      if (settled) {   // (its own last round had no violation, whatever later rounds found)
        ya0 = yk0;
        ya1 = yk1;
        viol_env = false;
        if constexpr (WHR) dlast = dk;
      }
      // Keep the refined iterate when it is a KKT point of the QP: its last round added no row
      // (primal feasible to ytol), dropped no row (no multiplier of the wrong sign) and its steps
      // converged, and it is finite.  The QP is strictly convex, so that point is its optimum,
      // however far the interior point's iterate was from it: with the internal-force curvature
      // 2 w_reg = 2e-4, the barrier of a nearly active row pushes the iterate at mu = 1e-9 up to
      // ~2e-2 off along such directions (joint-state batches, tools/kkt_study.py) -- the move
      // bound 1e-3 per lane that stood here rejected those envs (OSC_SOLVE_UNREFINED).
      // refine_max_move (default: none) remains as a tuning knob that forces rejections.
      const double mv = fmax(fabs(ya0 - y0), v1 ? fabs(ya1 - y1) : 0.0);
      const double myr = row_max(fmax(fabs(y0), v1 ? fabs(y1) : 0.0));
      // (WH: the rotated Newton systems; kept when converged -- its last step below 1e-10 of the
      // env's |y| scale, a row-wide maximum -- within 0.1 of y)
      const double ok =
          (isfinite(ya0) && isfinite(ya1) &&
           (kOldWh ? (mv <= 0.1 * (1.0 + myr) && dlast <= 1e-10 * (1.0 + myr))
                : (settled && mv <= P->refine_max_move * (1.0 + myr)))) ? 1.0 : 0.0;
      // (WH: and the wheel rows hold at the refined point)
      double wres = 0.0;
      if constexpr (WHR) {
        double yh0, yh1;
        rot_in<D>(W, L, ya0, ya1, yh0, yh1);
        wres = row_max(fmax(W.pin0 ? fabs(yh0 + W.q10) : 0.0, W.pin1 ? fabs(yh1 + W.q11) : 0.0));
      }
      const bool keep = !viol_env && row_min(ok) == 1.0 && wres <= ytol;
      if (mine && keep) {
        y0 = ya0;
        y1 = ya1;
        refined = true;
        st = OSC_SOLVE_OK;
      }
      // a converged env whose refinement is rejected keeps the interior point's iterate, and says
      // so: it is only as accurate as the interior point's stop.  (Wheel rows: the interior point
      // runs to mu <= 1e-12 and its pinned coordinates hold the rows to rounding; where they hold
      // to ytol its iterate stands as the solution -- census, profiles/r04g_census_*: every such
      // env within 4e-12 of the exact optimum, while the refinement, started from it, ended with
      // rows violated after its rounds; the exported duals come from stationarity, not from the
      // refinement, osc_dual_kernel) -- but not an iterate the late-stall exit left at mu > eps_mu:
      // with 4 refinement steps per round one such env stood 3e-4 off (profiles/r04zd/); it is
      // UNREFINED, and the fused entries' active-set fallback solves it)
      if (mine && !keep && st == OSC_SOLVE_OK && !(WHR && rwmax <= ytol && !stalled))
        st = OSC_SOLVE_UNREFINED;
#ifdef OSC_REFINE_DIAG   // diagnostic builds only: why the refinement was rejected
      if (mine && !keep)
        st = OSC_SOLVE_UNREFINED + 16 * (viol_env ? 1 : 0) + 32 * (row_min(ok) == 1.0 ? 0 : 1) +
             64 * (wres <= ytol ? 0 : 1) + 128 * (row_min(dlast <= 1e-10 * (1.0 + myr) ? 1.0 : 0.0) == 1.0 ? 0 : 1) +
             256 * (row_min(mv <= 0.1 * (1.0 + myr) ? 1.0 : 0.0) == 1.0 ? 0 : 1);
#endif
      if constexpr (D::WH)
        put_wheel_duals<D>(ws, env, l, want_dual, write_out,
                           (mine && keep && l < NW) ? (settled ? nuk : W.Nu[l]) : 0.0);
      wave_sync();
      sVy[j0] = y0;
      if (v1) sVy[j1] = y1;
      wave_sync();
    }
  }

#ifdef OSC_STAMPS
  if constexpr (RF == kRfFused) STAMP_STORE();
#endif
  if constexpr (D::WH) {
    if (!refined) put_wheel_duals<D>(ws, env, l, want_dual, write_out, 0.0);
  }
  // ---------------- outputs: tau = y_u;  x = (dv, u, z) with dv = X [y; 1] -----------------
  if (REFINE && !refined) {   // the interior point kernel's outputs stand
    if (write_out && l == 0 && gstatus && st == OSC_SOLVE_UNREFINED) gstatus[env] = st;
    write_out = false;
  }
  if (l < NU) {
    const double tq = sVy[l];
    sTau[l] = tq;
    if (write_out) gtau[static_cast<size_t>(env) * NU + l] = tq;
  }
  if (gx != nullptr) {   // dv = X [y; 1], two rows per lane
    const double* yv = sVy;
    if constexpr (WHR) {   // X^ = X'T: dv = X^ [T'y; 1]
      double yh0, yh1;
      rot_in<D>(W, L, y0, y1, yh0, yh1);
      sVy2[j0] = yh0;
      if (v1) sVy2[j1] = yh1;
      wave_sync();
      yv = sVy2;
    }
#pragma unroll
    for (int t = 0; t < (NV + kRow - 1) / kRow; ++t) {
      const int rr = l + kRow * t;
      if (rr < NV) {
        const double* xr = ws + static_cast<size_t>(env) * D::WS + D::W_X + rr * NY1P;
        double xb = xr[NY];
#pragma unroll
        for (int i = 0; i < NY; ++i) xb = fma(xr[i], yv[i], xb);
        sXb[rr] = xb;
      }
    }
  }
  wave_sync();
  const double fin = (isfinite(y0) && (!v1 || isfinite(y1))) ? 1.0 : 0.0;
  if (row_min(fin) == 0.0) st = OSC_SOLVE_NUMERICAL;
  if (write_out) {
    if (gx != nullptr) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int idx = l + kRow * t;
        if (idx < D::NX) {
          double v;
          if (idx < NV) v = sXb[idx];
          else if (idx < NV + NU) v = sTau[idx - NV];
          else v = sVy[NU + idx - NV - NU];
          gx[static_cast<size_t>(env) * D::NX + idx] = v;
        }
      }
    }
    if (l == 0 && !REFINE) {
      if (gstatus) gstatus[env] = st;
      if (giters) giters[env] = (kFix && fixup) ? P->max_iter + it_done : it_done;   // both passes
    }
    if (WARM && !REFINE) {   // this tick's y and lambda for the next one (NaN: next tick cold)
      double* wo = gwarm + static_cast<size_t>(env) * D::WW;
      wo[D::WW_Y + j0] = y0;
      if (v1) wo[D::WW_Y + j1] = y1;
#pragma unroll
      for (int t = 0; t < NRL; ++t) wo[D::WW_L + l + kRow * t] = lam[t];
      if (l < NC) wo[D::WW_M + l] = sMask[l];
      if (l == 0) wo[0] = (st == OSC_SOLVE_NUMERICAL) ? 0.0 : 1.0;
    }
  }
}

}  // namespace osc

#include "osc_ipm_launch.hpp"
