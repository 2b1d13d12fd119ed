// osc_ipm_iter.hpp -- the body of one interior-point iteration of ipm_block (osc_ipm.hpp): a
// fragment, included inside that function's iteration loop (no include guard), where `it` is the
// iteration and `init` says whether it is the start (it == -1).  The one-wave Go2 kernels include
// it twice more, as the peeled start (init = true) and as the loop that follows it (init = false),
// both compile-time constants; every other kernel once, `init` a run-time value.  Its one `break`
// leaves the iteration loop.
    STAMP_BEGIN();
    double mu = 0.0;
    if (WARM && it == 0 && any_warm) {
      const double* wst = gwarm + static_cast<size_t>(env) * D::WW;
      if (warm) {
        y0 = wst[D::WW_Y + j0];
        y1 = v1 ? wst[D::WW_Y + j1] : 0.0;
        sVy[j0] = y0;
        if (v1) sVy[j1] = y1;
      }
      wave_sync();
      wave_sync();
      if (warm) {
        const double dlt = P->warm_delta;
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          const double gy = Gv<D>(L, act, sVy, t);
          const double wl = wst[D::WW_L + l + kRow * t];
          s[t] = act[t] ? fmax(h[t] - gy, dlt) : 1.0;
          lam[t] = act[t] ? fmax(wl, dlt) : 0.0;
        }
      }
      // centre the warm pairs: no s_i lambda_i below warm_center x their mean (numpy model, 1 %
      // random walk, 0.1: WaLTER mean 9.2 -> 6.5 iterations, lockstep 11.3 -> 7.8; Go2 6.6 ->
      // 5.8; most warm stalls vanish)
      double c0s = 0.0;
#pragma unroll
      for (int t = 0; t < NRL; ++t) c0s += act[t] ? s[t] * lam[t] : 0.0;
      const double mu0 = P->warm_center * row_sum(c0s) / fmax(m_act, 1.0);
      if (warm) {
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          if (act[t]) {
            lam[t] = fmax(lam[t], mu0 * recip(s[t]));
            s[t] = fmax(s[t], mu0 * recip(lam[t]));
          }
        }
      }
      if constexpr (WHR) {
        // the wheel rows' residual at the warm y (this tick's rows: directions and mask are new
        // every tick; the first Newton step's pinned coordinates step onto them exactly)
        double yh0, yh1;
        rot_in<D>(W, L, y0, y1, yh0, yh1);
        rq0 = W.pin0 ? yh0 + W.q10 : 0.0;
        rq1 = W.pin1 ? yh1 + W.q11 : 0.0;
        rwmax = row_max(fmax(fabs(rq0), fabs(rq1)));
      }
    }
    // An env still far from converged (mu > 1e-6) at iteration `restart_iter` (warm-started:
    // `warm_restart`) is re-centred in place -- slacks h - G y + 1, multipliers 1: the cold
    // start's shape, no factorisation.  The rare solves that fall into a two-iteration limit
    // cycle of the step rule (mu oscillating near 1e-4; random-walk inputs, ~3e-6 of env-ticks,
    // round-3 warm-stall study) then finish ~10 iterations later instead of at max_iter.  No env of
    // the fresh-batch sweeps is still that far off at iteration 20 (tools/ipm_model.py
    // "recenter20": identical iteration counts).
    // Unit multipliers are a fresh start only where the iterate's own are of that scale (the
    // stalled envs of the censuses: largest multiplier <= 25).  A model whose bounds cut deep into
    // the tracking objective (torque boxes of a few N m, an fz cap of tens of N) has multipliers
    // of 1e6-1e8; the unit-scale cold start takes ~25 iterations to climb there and the env is a
    // few full steps from its optimum at `restart_iter` -- re-centred, it is thrown back to the
    // start and ends at max_iter (tests/test_gpu_descriptors.py).  Such an env keeps its iterate.
    bool restart = false;
    // (never at the peeled start: both are >= 0, a model is not created otherwise)
    if ((!kPeel || !init) && (it == restart_iter || (WARM && any_warm && it == warm_restart))) {
      double cr = 0.0, lmax = 0.0;
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        cr += act[t] ? s[t] * lam[t] : 0.0;
        lmax = fmax(lmax, lam[t]);   // (inactive rows hold lambda = 0)
      }
      const bool far = row_sum(cr) / fmax(m_act, 1.0) > 1e-6 && row_max(lmax) <= kRecentreLamMax;
      const bool mine = far && !done && it == (warm ? warm_restart : restart_iter);
      restart = __ballot(mine) != 0;
      if (restart) wave_sync();
      if constexpr (kFlatRecentre) {
        if (restart) {   // (wave-uniform; the env's own rows by selects, as the refresh below)
          double gy[NRL];
          Gv_all<D>(L, act, sVy, gy);
#pragma unroll
          for (int t = 0; t < NRL; ++t) {
            double sn = fmax(h[t] - gy[t], 0.0) + 1.0;
            in_vgpr(sn);
            sn = act[t] ? sn : 1.0;
            s[t] = mine ? sn : s[t];
            lam[t] = mine ? (act[t] ? 1.0 : 0.0) : lam[t];
          }
        }
      } else if (mine) {
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          const double slack = h[t] - Gv<D>(L, act, sVy, t);
          s[t] = act[t] ? fmax(slack, 0.0) + 1.0 : 1.0;
          lam[t] = act[t] ? 1.0 : 0.0;
        }
      }
    }
    if (!init) {
      double cs = 0.0;
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        // (inactive rows hold s = 1, lambda = +0 exactly: their product is the select's +0)
        // (the product rounded on its own, as the select's arm was: no fused multiply-add)
        if constexpr (SMALL) {
          double sl = s[t] * lam[t];
          in_vgpr(sl);
          cs += sl;
        } else {
          cs += act[t] ? s[t] * lam[t] : 0.0;
        }
      }
      mu = row_sum(cs) / fmax(m_act, 1.0);
      const bool fresh = it == 0 || mu <= 1e-6 || restart;
      rd_fresh = fresh || !rd_have;
      // this iteration's stop test (`done` is still the env's state on entry), formed ahead of the
      // refresh by the one-wave kernels (the two-wave kernels keep theirs below, where it was:
      // formed here it cost three of WaLTER's 4 to 8 more bytes of scratch per lane)
      bool stop = false;
      if constexpr (SMALL) stop = !done && mu <= eps_run && (!D::WH || rwmax <= P->wheel_tol);
      // Only an env that goes on iterating needs rp (DESIGN.md §5 "The refresh of the rows'
      // residual"): a done env's y and s are frozen, so the refresh would give it the bits it
      // holds (and does, when a wave-mate runs the block); kFreshStop: nor does the env that
      // stops here, whose rp nothing reads any more.
      const bool refresh = fresh && (!kFreshDone || (!done && !(kFreshStop && stop)));
      if (__ballot(refresh) != 0) {   // wave-uniform
#ifdef OSC_STAMPS
        st_acc[1] += 1ull << 40;   // refreshes entered, in the top bits of the iteration head's slot
#endif
        wave_sync();
        // (the per-row-slot Gv, in the one-wave kernels too: on Gv_all this block, which the Go2
        // headline now runs once per solve, cost the whole gain of skipping it -- DESIGN.md §5)
#pragma unroll
        for (int t = 0; t < NRL; ++t) {
          const double r = act[t] ? Gv<D>(L, act, sVy, t) + s[t] - h[t] : 0.0;
          rp[t] = fresh ? r : rp[t];
        }
      }
      if constexpr (SMALL) {   // (selects: a lone wave pays a slot per exec-mask instruction)
        done = done || stop;
        st = stop ? OSC_SOLVE_OK : st;
        it_done = stop ? it : it_done;
      } else if (!done && mu <= eps_run && (!D::WH || rwmax <= P->wheel_tol)) {
        done = true;
        st = OSC_SOLVE_OK;
        it_done = it;
      }
      if constexpr (CP == kCpPark) {
        if (it == PA.park_it && __ballot(!done) != 0) {
          // one slot per unconverged row (lane 0 of the row takes it), its state written by
          // every lane of the row; the row then counts as done in this wave
          int slot = 0;
          if (!done && l == 0) slot = atomicAdd(PA.count, 1);
          slot = __shfl(slot, grp * kRow, kWave);
          if (!done) {
            double* pk = park_at(slot);
            pk[l] = y0;
            pk[kRow + l] = y1;
#pragma unroll
            for (int t = 0; t < NRL; ++t) {
              pk[2 * kRow + l + kRow * t] = s[t];
              pk[2 * kRow + NRL * kRow + l + kRow * t] = lam[t];
              pk[2 * kRow + 2 * NRL * kRow + l + kRow * t] = rp[t];
            }
            pk[2 * kRow + 3 * NRL * kRow + l] = rdc0;
            pk[3 * kRow + 3 * NRL * kRow + l] = rdc1;
            if (l == 0) PA.list[slot] = env;
            parked = true;
            done = true;
          }
        }
      }
      if (__ballot(!done) == 0 || it >= max_iter) {
        if (!done) it_done = it;
        break;
      }
    }
    double inv_s[NRL];                   // 1/s on active rows, 0 elsewhere (s = 1 at init)
#pragma unroll
    for (int t = 0; t < NRL; ++t) {
      const int r = l + kRow * t;
      if constexpr (SMALL) {
        // no select on `init`: the start has s = 1 and lambda = 0 on every row, recip(1) is 1
        // exactly (v_rcp_f64(1) = 1, both Newton corrections 0) and inactive rows hold lambda = +0
        inv_s[t] = act[t] ? recip(s[t]) : 0.0;
        sVr[r] = lam[t];
      } else {
        inv_s[t] = act[t] ? (init ? 1.0 : recip(s[t])) : 0.0;
        sVr[r] = init ? 0.0 : (act[t] ? lam[t] : 0.0);
      }
      sDr[r] = init ? (init_ls(t) ? 1.0 : 0.0) : lam[t] * inv_s[t];
    }
    wave_sync();

    STAMP_END(1);
    STAMP_BEGIN();
    // ---- Newton matrix K = Hr + G' D G (columns j0, j1 in registers) and rd = Hr y + g + G'lam
    double rd0 = rdc0, rd1 = rdc1;
    if (!kRdCarry || init || __ballot(rd_fresh && !done) != 0) {   // (wave-uniform)
      double rn0, rn1;
      GTw2<D, SMALL>(L, sVr, rn0, rn1);
      if constexpr (WHR) rot_in<D>(W, L, rn0, rn1, rn0, rn1);   // T'G'lam
      rn0 += g0;
      rn1 += g1;
      if constexpr (WHR) {   // rd^ += H^ y^
        if (!init) {
          double yh0, yh1;
          rot_in<D>(W, L, y0, y1, yh0, yh1);
          dot_rows<NY>(rn0, rn1, yh0, yh1, c0, c1);
        }
      } else {
        if (!init) dot_rows<NY>(rn0, rn1, y0, y1, c0, c1);    // rd += Hr y (y broadcast by DPP)
      }
      rd0 = (!kRdCarry || rd_fresh) ? rn0 : rd0;
      rd1 = (!kRdCarry || rd_fresh) ? rn1 : rd1;
    }
    rd_have = true;
    double dg0 = hdg0, dg1 = hdg1, du = 0.0;
    STAMP_END(8);
    STAMP_BEGIN();
    // G_u' D G_u is diagonal, d_q = D[2q] + D[2q+1] on (q, q): lane q's column j0 = q
    if constexpr (WHR) {
      assemble_rot<D>(W, L, sDr, c0, c1, dg0, dg1);
    } else {
      static_assert(D::NU <= kRow, "torque variables in the first column slot");
      const double2 dd = *reinterpret_cast<const double2*>(sDr + 2 * (j0 < NU ? j0 : 0));
      du = (j0 < NU) ? dd.x + dd.y : 0.0;   // (added to the pivots by ldl_rows)
      dg0 += du;
    }
    STAMP_END(9);
    STAMP_BEGIN();
    if constexpr (!WHR) add_contact_blocks<D>(L, sDr, c0, c1, dg0, dg1);
    wave_sync();
    STAMP_END(2);
    STAMP_BEGIN();
    ldl_rows<NY, SMALL>(c0, c1, B + LY::I_DINV, l, dinv0, dinv1, 1e-13 * dg0, 1e-13 * dg1, du);
    wave_sync();
    STAMP_END(3);

    // pass 0: affine (predictor) direction, rc = s lambda
    // pass 1: corrector, rc = s lambda + ds_aff dl_aff - sigma mu
    double ds[NRL], dl[NRL], dsdl[NRL];
#pragma unroll
    for (int t = 0; t < NRL; ++t) ds[t] = dl[t] = dsdl[t] = 0.0;
    double dy0 = 0.0, dy1 = 0.0, sig_mu = 0.0, step = 1.0, a_aff = 1.0;
    const int npass = init ? 1 : 2;
    for (int pass = 0; pass < npass; ++pass) {
      STAMP_BEGIN();
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        const double rc = fma(s[t], lam[t], dsdl[t]) - sig_mu;   // dsdl = sig_mu = 0 in pass 0
        sVr[l + kRow * t] = init ? (init_ls(t) ? h[t] : 0.0) : (rc - lam[t] * rp[t]) * inv_s[t];
      }
      wave_sync();
      GTw2<D, SMALL>(L, sVr, dy0, dy1);
      if constexpr (WHR) {   // in y^: T'(G'w) - rd^, the pinned slots step to the rows
        rot_in<D>(W, L, dy0, dy1, dy0, dy1);
        dy0 = W.pin0 ? -rq0 : dy0 - rd0;
        dy1 = W.pin1 ? -rq1 : dy1 - rd1;
      } else {
        dy0 -= rd0;
        dy1 -= rd1;
      }
      STAMP_END(4);
      STAMP_BEGIN();
      ldl_solve_rows<NY>(c0, c1, dinv0, dinv1, dy0, dy1, l);
      if constexpr (WHR) rot_out<D>(W, L, dy0, dy1, dy0, dy1);
      sVy2[j0] = dy0;
      if (v1) sVy2[j1] = dy1;
      wave_sync();
      STAMP_END(5);
      STAMP_BEGIN();
      wave_sync();
      // step to the boundary, division-free: 1 / max(1, max_r(-ds/s), max_r(-dl/lambda))
      double rmax = 1.0;
      double gdy_all[NRL];
      if constexpr (SMALL) Gv_all<D>(L, act, sVy2, gdy_all);
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        const double rc = fma(s[t], lam[t], dsdl[t]) - sig_mu;
        const double gdy = SMALL ? gdy_all[t] : Gv<D>(L, act, sVy2, t);
        ds[t] = act[t] ? -rp[t] - gdy : 0.0;
        dl[t] = -(rc + lam[t] * ds[t]) * inv_s[t];
        const double inv_l = (act[t] && !init) ? recip1(lam[t]) : 0.0;
        rmax = fmax(rmax, fmax(-ds[t] * inv_s[t], -dl[t] * inv_l));
      }
      step = recip(row_max(rmax));
      if (pass == 0 && !init) {
        double ca = 0.0;
#pragma unroll
        for (int t = 0; t < NRL; ++t)
          ca += act[t] ? (s[t] + step * ds[t]) * (lam[t] + step * dl[t]) : 0.0;
        a_aff = step;
        const double mu_aff = row_sum(ca) / fmax(m_act, 1.0);
        const double q = mu_aff / fmax(mu, 1e-300);
        sig_mu = q * q * mu;   // sigma = (mu_aff/mu)^2: the cube jams on rare envs (tools/ipm_hard.py)
#pragma unroll
        for (int t = 0; t < NRL; ++t) dsdl[t] = ds[t] * dl[t];
        if constexpr (WHR) {
          // late stall: once the active rows' barrier terms pass ~1e10 their dense rank-one terms
          // in the rotated Newton matrix swamp its small curvature and the affine step collapses
          // (round-3 wheel traces).  The iterate is as good as it gets there: stop on it
          // (no step) and let the refinement finish the solve.
          if (!done && mu <= 1e-8 && step < 0.1 && rwmax <= P->wheel_tol) {
            done = true;
            st = OSC_SOLVE_OK;
            it_done = it;
            stalled = true;
          }
        }
      }
      wave_sync();
      STAMP_END(6);
    }
    STAMP_BEGIN();
    if (init) {
      // here rp = 0, so ds = -G y0 and  G y0 - h = -ds - h
      y0 = dy0;
      y1 = dy1;
      double zmax = -1e300, nzmax = -1e300;
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        const double zr = -ds[t] - h[t];
        if (act[t]) {
          zmax = fmax(zmax, zr);
          nzmax = fmax(nzmax, -zr);
        }
      }
      const double ap = row_max(zmax);    // = max(-s)
      const double ad = row_max(nzmax);   // = max(-lambda)
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        const double zr = -ds[t] - h[t];
        s[t] = act[t] ? ((ap >= 0.0) ? -zr + 1.0 + ap : -zr) : 1.0;
        lam[t] = act[t] ? ((ad >= 0.0) ? zr + 1.0 + ad : zr) : 0.0;
      }
      if (m_act == 0.0 && !done) {        // unconstrained: y0 = -Hr^-1 g is the optimum
        done = true;
        st = OSC_SOLVE_OK;
        it_done = 0;
      }
    } else {
      // fraction to the boundary: 0.99 early, closer to 1 as mu -> 0 or when the affine step was
      // nearly full, never above 1 - 1e-5 (tools/ipm_model.py + tools/etatest.sh: -15% lockstep
      // iterations vs a fixed 0.99; uncapped, a few envs stall at the boundary).  The fix-up
      // pass (an env the first pass left not OK) keeps 0.99: the envs of round 5's census that
      // stalled at max_iter with the adaptive rule (~1 in 600,000 joint-state envs) converge in
      // 15-20 iterations with it (numpy model of the kernel, tools/ipm_model.py)
      const double eta =
          fixup ? 0.99
                : fmin(1.0 - 1e-5, fmax(0.99, fmax(1.0 - mu, 1.0 - 0.1 * (1.0 - a_aff))));
      const double alpha = done ? 0.0 : fmin(1.0, eta * step);
      y0 = fma(alpha, dy0, y0);
      y1 = fma(alpha, dy1, y1);
#pragma unroll
      for (int t = 0; t < NRL; ++t) {
        s[t] = act[t] ? fma(alpha, ds[t], s[t]) : 1.0;
        lam[t] = act[t] ? fma(alpha, dl[t], lam[t]) : 0.0;
        rp[t] *= 1.0 - alpha;
      }
      if constexpr (kRdCarry) {
        rdc0 = (1.0 - alpha) * rd0;
        rdc1 = (1.0 - alpha) * rd1;
      }
    }
    sVy[j0] = y0;
    if (v1) sVy[j1] = y1;
    // next iteration's Hr columns (the factor in c0/c1 is dead now).  (Round 6: issuing them right
    // after the last pass's solve instead, so the L2 loads of the two-wave kernel fly during the
    // ratio tests, measured no gain -- Go2 8,192 0.2534 vs 0.2531 ms, 65,536 1.593 vs 1.600.)
    load_hr();
    wave_sync();
    if constexpr (WHR) {   // the rows' residual at the new iterate (next step, stop test)
      double yh0, yh1;
      rot_in<D>(W, L, y0, y1, yh0, yh1);
      rq0 = W.pin0 ? yh0 + W.q10 : 0.0;
      rq1 = W.pin1 ? yh1 + W.q11 : 0.0;
      rwmax = row_max(fmax(fabs(rq0), fabs(rq1)));
    }
    STAMP_END(7);
