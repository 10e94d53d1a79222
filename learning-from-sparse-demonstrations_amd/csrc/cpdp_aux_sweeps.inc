// The two auxiliary sweep kernels (COCSys.auxSysSolver, CPDP.py:316-381).  Included by cpdp_aux.h -- inside namespace lfsd -- once per
// interpolation level of the nominal trajectory, with
//   LFSD_AUX_LVL              1 (linear interpolant, CPDP.py:386) or 2 (cubic, CPDP.py:388-390)
//   LFSD_AUX_ARGS             the kernels' argument struct (AuxArgs / AuxArgsCubic)
//   LFSD_AUX_RICCATI_KERNEL, LFSD_AUX_FORWARD_KERNEL   their names
//   LFSD_AUX_WEIGHTED         defined (ABI 16): the forward kernel alone, with a weight per waypoint (a.wp_weight, never NULL)
// One text, two pairs of kernels -- and not one function template that two thin kernels call: the sweeps leave early (a skipped row, a
// wrong launch shape), and a `return` of an inlined function is a branch the optimiser treats differently from a kernel's own.  The
// level-1 kernels must stay instruction for instruction what they were before level 2 existed (DESIGN.md section 11).
#ifndef LFSD_AUX_WEIGHTED
template <class M, typename T, int G>
__global__ void __launch_bounds__(64, (sizeof(T) == 4 ? 2 : 1)) LFSD_AUX_RICCATI_KERNEL(LFSD_AUX_ARGS<T> a) {
  constexpr int LVL = LFSD_AUX_LVL;
  if (blockDim.x != 64) return;                   // one wavefront per workgroup: see the note on barriers above
  using Ctx = AuxCtx<M, T, G, 0, LVL>;
  using Lay = typename Ctx::Lay;
  constexpr int NX = M::NX, NP = M::NP, NZ = NX + NP;
  constexpr int GPB = 64 / G;
  static_assert(64 % G == 0 && G >= NZ && G >= Lay::NNODE, "lane group must hold one column of [P W] per lane");
  // pair staging (LFSD_RIC_PAIR_STAGE, cpdp_aux.h): nine staging lanes; the parking slot holds the NZ columns only, and the lanes
  // beyond them park into the exchange buffer LDS_T and read back whatever ric_rhs left there: their z[] is private and ARBITRARY (not
  // zero), and nothing below may consume it (AuxLayout::ric_pstride)
  constexpr bool PAIR = Lay::PAIR;
  constexpr int PS = Lay::template ric_pstride<G>();
  static_assert(!PAIR || (G >= 2 * Lay::NNODE - 1 && !Lay::template ric_adaptive<G>() && (G - NZ) + (NX - 1) * NZ <= Lay::LDS_TSZ &&
                          GPB * Lay::template lds_elems_ric<G>() * (int)sizeof(T) <= kRicLdsPerWorkgroup),
                "pair staging: nine staging lanes, uniform units only, idle lanes park inside LDS_T, eight workgroups per CU");
  constexpr int LDS_SLICE = Lay::template lds_elems_ric<G>() + (LVL == 2 ? Lay::CURV : 0);
  __shared__ T lds_all[GPB * LDS_SLICE];
  poison_lds(lds_all, GPB * LDS_SLICE);
  const long long slot = (long long)blockIdx.x * GPB + threadIdx.x / G;
  const bool valid = slot < a.batch;
  const long long traj = valid ? slot : (long long)a.batch - 1;
  if (a.skipped(traj)) {                          // a solve the caller does not want differentiated: this lane group is done
    if (valid && a.stats && threadIdx.x % G == 0) { a.stats[traj * 4 + 0] = 0; a.stats[traj * 4 + 1] = 0; }
    if (valid) {                                  // its [P W] is NaN, not whatever the buffer held (include/lfsd_cpdp.h)
      T* Zs = a.Z_grid + traj * (long long)(a.n_grid + 1) * NZ * NX;
      const T nan = T(0) / T(0);
      for (int i = threadIdx.x % G; i < (a.n_grid + 1) * NZ * NX; i += G) Zs[i] = nan;
    }
    return;                                       // (its lanes leave together; the other groups of the wavefront share nothing with it)
  }
  Ctx s;
  aux_setup<M, T, G, 0>(s, a, traj, lds_all, LDS_SLICE);
  const int N = a.n_grid, Sa = a.substeps;
  const int lane = s.lane;
  {
    const int col = lane < NZ ? lane : 0;
    const T* n0 = s.lds + Lay::LDS_L;
#pragma unroll
    for (int i = 0; i < NX; ++i) s.hcol[i] = n0 + (lane < NZ ? M::hcol_off0(col, i) : M::OFF_ZERO);
#pragma unroll
    for (int a2 = 0; a2 < M::NU; ++a2) s.ucol[a2] = n0 + (lane < NZ ? M::ucol_off0(col, a2) : M::OFF_ZERO);
  }
  T* Zt = a.Z_grid + traj * (long long)(N + 1) * NZ * NX;
  T z[NX];
  {
    T xN[NX];
    const T* xs = a.state_grid + (traj * (N + 1) + N) * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) xN[i] = xs[i];
    const T tN = M::TIME_VARYING ? s.dgrid * T(N) : T(0);
    M::final_hess_mul(tN, xN, s.e, s.c, s.ox, s.oe, z);      // [ddhxx ddhxe], CPDP.py:330-331
    if (lane >= NZ) {
#pragma unroll
      for (int i = 0; i < NX; ++i) z[i] = T(0);
    }
    if (valid && lane < NZ) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Zt[((long long)N * NZ + lane) * NX + i] = z[i];
    }
  }
  T* ldsT = s.lds + Lay::LDS_T;
  int units_hint = Sa;
  int n_units = 0, n_unmet = 0;      // (group-uniform) units executed incl. rejected attempts; intervals accepted above tolerance
  const int budget = a.budget(traj);
  for (int k = N - 1; k >= 0; --k) {
    s.load_interval(a, traj, k, N, -1);
    // stiffness-aware sub-stepping: P is largest at the later end of the interval (terminal transient).  The coefficients
    // are staged for the first unit of the expected unit count at once: node 0 sits at the interval end either way, and
    // when the stiffness estimate confirms the count the first unit need not stage again
    const int units_guess = units_hint;
    int ahead = 1;      // units whose nodes the last staging pass has put in place (pair staging: 2 after a nine-node pass)
    if constexpr (PAIR) {
      const T st0 = T(-1) / T(4 * units_guess), s_nx = T(1) - T(1) / T(units_guess);
      if (units_guess >= 2 && Ctx::pair_ok(T(1), st0, s_nx)) ahead = 2;
      s.node_base(0);
      s.stage_nodes(T(1), st0, s_nx, ahead == 2 ? 2 * Lay::NNODE - 1 : Lay::NNODE);
    } else {
      s.stage_nodes(T(1), T(-1) / T(4 * units_guess));
    }
    const int refine_k = (budget > 0 && n_units >= budget) ? 1 : a.max_refine;      // budget spent: no refinement
    int units = s.units_for(s.stiff_rate(z, s.node(0)), Sa, a.rate_max, refine_k);
    // error-driven refinement stops at max_refine x the minimum units -- and as soon as a doubling fails to halve the
    // estimate: next to a conjugate point (finite escape of the Riccati solution) no step size meets a relative tolerance,
    // and one such trajectory must not stall the batch
    const long long units_cap = (long long)Sa * refine_k;
    if (units < units_hint) units = (int)t_min((long long)units_hint, units_cap);
    T ratio_prev = T(-1);
    bool staged = (units == units_guess);
    // Step-size control INSIDE a stiff interval (round 6).  The uniform refinement below sizes every unit of an interval for its
    // stiffest point.  The interval before a heavy final cost is a transient: P starts at h_xx and decays like 1 / (1/P_0 + R tau) --
    // on the robot arm dgrid x rate falls from 2 000 to 1 inside that one interval, which took 500 of the sweep's 565 units (and
    // 2.6 ms of a 15 ms learner step).  From kRicAdapt units up the interval is integrated with steps of its own: every step is a
    // Richardson pair as before, judged on ITS estimate against the same tolerances; a refused step is redone from its parked start
    // value with half the length; after a step whose estimate leaves an 8-fold margin the length doubles when the stiffness at the
    // NEW position allows it (dt x rate <= rate_max, evaluated on the coefficients the step has just staged at its far node).
    // Positions are integers on the interval's finest admissible grid (units_cap ticks), steps powers of two: the last step lands on
    // the grid node exactly.  Quiet intervals (the headline's 1-4 units) keep the uniform path, bit for bit.
    // fp32 only: the fp64 sweep is the parity reference; its uniform intervals over-deliver by orders (steps sized for the stiffest point
    // everywhere), its floors against the tight oracle were set on that, and it stays bit for bit what it was.
    bool adaptive_done = false;
    if constexpr (sizeof(T) == 4 && Lay::template ric_adaptive<G>()) {
    if (a.rtol > T(0) && units >= kRicAdapt && units_cap % units == 0) {
      adaptive_done = true;
      const int R = (int)units_cap;
      int stp = R / units, pos = R;
      bool unmet = false;
      T* zpark = s.lds + Lay::template ric_park<G>();
      T* zstart = s.lds + Lay::template ric_park2<G>();
      while (pos > 0) {
        const T f = T(stp) / T(R), s_hi = T(pos) / T(R);
        if (!(staged && pos == R && stp * units_guess == R)) s.stage_nodes(s_hi, -f * T(0.25));
        staged = false;
        const T hc = s.dgrid * f;
#pragma unroll
        for (int i = 0; i < NX; ++i) { zpark[i * G + lane] = z[i]; zstart[i * G + lane] = z[i]; }
        s.ric_strang(z, 0, 2, 4, hc);
#pragma unroll
        for (int i = 0; i < NX; ++i) { const T z0 = zpark[i * G + lane]; zpark[i * G + lane] = z[i]; z[i] = z0; }
        s.ric_strang2(z, hc);
        T err_l = T(0), scl_l = T(0);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const T zc = zpark[i * G + lane];
          err_l = t_max(err_l, t_abs(z[i] - zc));
          z[i] = (T(4) * z[i] - zc) * (T(1) / T(3));
          scl_l = t_max(scl_l, t_abs(z[i]));
        }
        ++n_units;
        ldsT[lane] = err_l; ldsT[G + lane] = scl_l;
        LFSD_WAVE_SYNC();
        T eP = T(0), sP = T(0), eW = T(0), sW = T(0);
        for (int l = 0; l < NZ; ++l) {
          if (l < NX) { eP = t_max(eP, ldsT[l]); sP = t_max(sP, ldsT[G + l]); }
          else { eW = t_max(eW, ldsT[l]); sW = t_max(sW, ldsT[G + l]); }
        }
        LFSD_WAVE_SYNC();
        const T tolP = T(3) * a.rtol * sP, tolW = T(3) * a.rtol * (sW + T(1e-3) * sP);
        const bool fine_enough = (eP <= tolP && eW <= tolW) || !(t_finite(eP) && t_finite(eW));
        const T ratio = t_max(eP / t_max(tolP, T(1e-30)), eW / t_max(tolW, T(1e-30)));
        const bool no_gain = ratio_prev >= T(0) && ratio > T(0.5) * ratio_prev;      // (the halved step did not halve the estimate: next to a conjugate point)
        if (fine_enough || no_gain || stp == 1 || !valid) {
          if (!fine_enough) unmet = true;
          pos -= stp;
          ratio_prev = T(-1);
          // (the margin of the estimate before a step may grow is the uniform path's before it halves the next interval's units.  Steps
          //  sized for the LOCAL stiffness each contribute what only the stiffest units of a uniform interval did: measured in fp64 -- robot
          //  arm n_grid 30, [P W] against the tight oracle -- 1e-8 uniform, 6.1e-7 with this margin, 7.0e-8 with a 256-fold one; in fp32
          //  the rounding floor of the sweep, 1e-5, hides the difference: [P W] 2.4e-6 / 8.7e-6 either way)
          constexpr int MARGIN = kAuxDown;
          if (pos > 0 && eP * T(MARGIN) <= tolP && eW * T(MARGIN) <= tolW && pos % (2 * stp) == 0 && (long long)2 * stp * Sa <= R) {
            // (the stiffness where the NEXT step starts: node 4 of this step's staging sits exactly there)
            const int need = s.units_for(s.stiff_rate(z, s.node(4)), Sa, a.rate_max, refine_k);
            if ((long long)need * 2 * stp <= R) stp *= 2;
          }
        } else {
          ratio_prev = ratio;
          stp /= 2;
#pragma unroll
          for (int i = 0; i < NX; ++i) z[i] = zstart[i * G + lane];
        }
      }
      if (unmet) ++n_unmet;
      units_hint = (int)t_max((long long)Sa, (long long)(R / stp));      // the next interval starts with the step this one ended on
    }
    }
    if (!adaptive_done)
    // Error-controlled sub-stepping (a.rtol > 0): the Richardson pair gives |fine - coarse| / 3 as an estimate of the
    // second-order error that the extrapolation removes; while it exceeds rtol relative to the column's size the interval
    // is redone from its stored start value Z(t_k+1) with twice the units.  (solve_ivp's rtol of the reference, CPDP.py:335,
    // is 1e-3 on the un-extrapolated estimate of its pair, and so is the default here.)
    for (;;) {
      const T hc = s.dgrid / T(units);
      const T ds = T(1) / T(4 * units);
      T err_l = T(0), scl_l = T(0);
      if (!staged) ahead = 0;      // (a redo, or a unit count other than the guess: staged anew from the first unit on)
      for (int unit = 0; unit < units; ++unit) {
        const T s_hi = T(1) - T(unit) / T(units);
        if constexpr (PAIR) {
          // two units per staging pass while two are left (and their shared node is one fraction); the second of a pair reads slots 4-8
          if (ahead == 0) {
            const T s_nx = T(1) - T(unit + 1) / T(units);
            ahead = (unit + 1 < units && Ctx::pair_ok(s_hi, -ds, s_nx)) ? 2 : 1;
            s.node_base(0);
            s.stage_nodes(s_hi, -ds, s_nx, ahead == 2 ? 2 * Lay::NNODE - 1 : Lay::NNODE);
          } else if (unit > 0) {
            s.node_base(Lay::NNODE - 1);
          }
          --ahead;
        } else {
          if (!(staged && unit == 0)) s.stage_nodes(s_hi, -ds);      // node i sits at fraction s_hi - i/(4 units)
        }
        staged = false;
        // coarse chain in place, then the fine chain in place from the parked start value (the barriers inside the chains
        // keep the compiler from carrying the parked column in registers)
        T* zpark = s.lds + ((PAIR && lane >= NZ) ? Lay::LDS_T + lane - NZ : Lay::template ric_park<G>() + lane);
#pragma unroll
        for (int i = 0; i < NX; ++i) zpark[i * PS] = z[i];
        s.ric_strang(z, 0, 2, 4, hc);
#pragma unroll
        for (int i = 0; i < NX; ++i) { const T z0 = zpark[i * PS]; zpark[i * PS] = z[i]; z[i] = z0; }
        s.ric_strang2(z, hc);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const T zc = zpark[i * PS];
          err_l = t_max(err_l, t_abs(z[i] - zc));
          z[i] = (T(4) * z[i] - zc) * (T(1) / T(3));     // Richardson (Strang is O(h^2), symmetric); constant reciprocal: no division
          scl_l = t_max(scl_l, t_abs(z[i]));
        }
      }
      n_units += units;
      if (!(a.rtol > T(0))) break;
      // per block of columns (P: lanes < NX, W: the rest) the worst estimate against that block's magnitude
      ldsT[lane] = err_l; ldsT[G + lane] = scl_l;
      LFSD_WAVE_SYNC();
      T eP = T(0), sP = T(0), eW = T(0), sW = T(0);
      for (int l = 0; l < NZ; ++l) {
        if (l < NX) { eP = t_max(eP, ldsT[l]); sP = t_max(sP, ldsT[G + l]); }
        else { eW = t_max(eW, ldsT[l]); sW = t_max(sW, ldsT[G + l]); }
      }
      LFSD_WAVE_SYNC();
      const T tolP = T(3) * a.rtol * sP, tolW = T(3) * a.rtol * (sW + T(1e-3) * sP);
      const bool fine_enough = (eP <= tolP && eW <= tolW) || !(t_finite(eP) && t_finite(eW));
      const T ratio = t_max(eP / t_max(tolP, T(1e-30)), eW / t_max(tolW, T(1e-30)));
      const bool no_gain = ratio_prev >= T(0) && ratio > T(0.5) * ratio_prev;
      ratio_prev = ratio;
      if (fine_enough || no_gain || !valid || (long long)units * 2 > units_cap) {
        if (!fine_enough) ++n_unmet;       // refinement gave up (next to a conjugate point, or at the cap): reported, not hidden
        // next interval: start from this interval's units, or half of them when the estimate leaves room for it
        units_hint = (eP * T(kAuxDown) <= tolP && eW * T(kAuxDown) <= tolW && units > Sa) ? units / 2 : units;
        break;
      }
      units *= 2;
      if (lane < NZ) {
#pragma unroll
        for (int i = 0; i < NX; ++i) z[i] = Zt[((long long)(k + 1) * NZ + lane) * NX + i];
      }
    }
    // keep P symmetric (the closed-form stiff update relies on it) and store the grid value
    if (lane < NX) {
#pragma unroll
      for (int i = 0; i < NX; ++i) ldsT[lane * NZ + i] = z[i];
    }
    LFSD_WAVE_SYNC();
    if (lane < NX) {
#pragma unroll
      for (int i = 0; i < NX; ++i) z[i] = T(0.5) * (z[i] + ldsT[i * NZ + lane]);
    }
    LFSD_WAVE_SYNC();
    if (valid && lane < NZ) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Zt[((long long)k * NZ + lane) * NX + i] = z[i];
    }
  }
  if (valid && a.stats && lane == 0) { a.stats[traj * 4 + 0] = n_units; a.stats[traj * 4 + 1] = n_unmet; }
}
#endif  // LFSD_AUX_WEIGHTED

template <class M, typename T, int G>
__global__ void __launch_bounds__(64, 1) LFSD_AUX_FORWARD_KERNEL(LFSD_AUX_ARGS<T> a) {
  constexpr int LVL = LFSD_AUX_LVL;
#ifdef LFSD_AUX_WEIGHTED
  constexpr bool WTD = true;
#else
  constexpr bool WTD = false;
#endif
  if (blockDim.x != 64) return;                   // one wavefront per workgroup: see the note above aux_riccati_kernel
  using Ctx = AuxCtx<M, T, G, 1, LVL>;
  using Lay = AuxLayout<M, 1>;
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NZ = NX + NP;
  constexpr int GPB = 64 / G;
  static_assert(64 % G == 0 && G >= NX && G >= 2 * NP && G >= Lay::NNODE && G >= 3 * sub_lanes<NU <= 4 ? NU : 1>(),
                "forward lane group: one P column per lane, and one X column per lane in each half (fine / coarse chain)");
  constexpr int LDS_SLICE = Lay::lds_elems_fwd() + (LVL == 2 ? Lay::CURV : 0);
  __shared__ T lds_all[GPB * LDS_SLICE];
  poison_lds(lds_all, GPB * LDS_SLICE);
  const long long slot = (long long)blockIdx.x * GPB + threadIdx.x / G;
  const bool valid = slot < a.batch;
  const long long traj = valid ? slot : (long long)a.batch - 1;
  if (a.skipped(traj)) {                          // not differentiated: NaN loss / gradient / sensitivity grids
    const int l = threadIdx.x % G;
    const T nan = T(0) / T(0);
    if (valid) {
      if (l == 0) { a.loss[traj] = nan; if (a.stats) { a.stats[traj * 4 + 2] = 0; a.stats[traj * 4 + 3] = 0; } }
      if (l < NP) a.grad[traj * NP + l] = nan;
      if (a.auxX_grid) { T* o = a.auxX_grid + traj * (long long)(a.n_grid + 1) * NP * NX; for (int i = l; i < (a.n_grid + 1) * NP * NX; i += G) o[i] = nan; }
      if (a.auxU_grid) { T* o = a.auxU_grid + traj * (long long)(a.n_grid + 1) * NP * NU; for (int i = l; i < (a.n_grid + 1) * NP * NU; i += G) o[i] = nan; }
    }
    return;
  }
  Ctx s;
  aux_setup<M, T, G, 1>(s, a, traj, lds_all, LDS_SLICE);
  const int N = a.n_grid, Sa = a.substeps;
  const int lane = s.lane;
  const bool xlane = s.xlane, coarse = s.coarse;
  const bool fine_x = xlane && !coarse;           // the lanes that own the results of a column
  const T* Zt = a.Z_grid + traj * (long long)(N + 1) * NZ * NX;
  T xa[NX], wA[NX], wB[NX];     // X column; W column at both ends of the interval (the P columns live in LDS)
#pragma unroll
  for (int i = 0; i < NX; ++i) { xa[i] = T(0); wA[i] = T(0); wB[i] = T(0); }     // X(0) = 0, CPDP.py:355
  T* ldsPA = s.lds + Lay::FWD_P;
  T* ldsPB = ldsPA + NX * NX;
  T* ldsP0 = ldsPB + NX * NX;                                  // zero row
  for (int i = lane; i < NX; i += G) ldsP0[i] = T(0);
  const T* pA = (lane < NX) ? ldsPA + lane * NX : ldsP0;
  const T* pB = (lane < NX) ? ldsPB + lane * NX : ldsP0;
  T pN[NX], wN[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) { pN[i] = T(0); wN[i] = T(0); }
  T* xprev = s.lds + Lay::FWD_XPREV;                 // X(t_k), parked in LDS: start value of a redone interval, and the loss needs it
  T* xch = s.lds + Lay::FWD_XCH;
  T* ldsR = s.lds + Lay::FWD_RED;
  T loss = T(0), gacc = T(0);
  int units_hint = Sa;
  int n_units = 0, n_unmet = 0;
  const int budget = a.budget(traj);
  T* Xo = a.auxX_grid ? a.auxX_grid + traj * (long long)(N + 1) * NP * NX : nullptr;
  T* Uo = a.auxU_grid ? a.auxU_grid + traj * (long long)(N + 1) * NP * NU : nullptr;
  if (valid && Xo && fine_x) {
#pragma unroll
    for (int i = 0; i < NX; ++i) Xo[(long long)s.xcol * NX + i] = T(0);
  }
  for (int k = 0; k < N; ++k) {
    s.load_interval(a, traj, k, N, +1);
    // [P W] at the two ends of the interval: the later end of interval k is the earlier end of interval k+1, and the new end is
    // fetched into registers one interval ahead (pN: this lane's column of P, wN: its column of W) -- as the grid rows above
    if (k == 0 || !Ctx::PF) {
      if (lane < NX) {           // (load_interval's barriers fence the previous interval's readers; stage_nodes' the writers)
#pragma unroll
        for (int i = 0; i < NX; ++i) { ldsPA[lane * NX + i] = Zt[((long long)k * NZ + lane) * NX + i]; ldsPB[lane * NX + i] = Zt[((long long)(k + 1) * NZ + lane) * NX + i]; }
      }
      if (xlane) {
#pragma unroll
        for (int i = 0; i < NX; ++i) { wA[i] = Zt[((long long)k * NZ + NX + s.xcol) * NX + i]; wB[i] = Zt[((long long)(k + 1) * NZ + NX + s.xcol) * NX + i]; }
      }
    } else {
      { T* t_ = ldsPA; ldsPA = ldsPB; ldsPB = t_; }
      pA = (lane < NX) ? ldsPA + lane * NX : ldsP0;
      pB = (lane < NX) ? ldsPB + lane * NX : ldsP0;
      if (lane < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) ldsPB[lane * NX + i] = pN[i];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) { wA[i] = wB[i]; wB[i] = wN[i]; }
    }
    if (Ctx::PF && k + 2 <= N) {
      if (lane < NX) {
#pragma unroll
        for (int i = 0; i < NX; ++i) pN[i] = Zt[((long long)(k + 2) * NZ + lane) * NX + i];
      }
      if (xlane) {
#pragma unroll
        for (int i = 0; i < NX; ++i) wN[i] = Zt[((long long)(k + 2) * NZ + NX + s.xcol) * NX + i];
      }
      LFSD_ISSUE_FENCE();
    }
    if (fine_x) {
#pragma unroll
      for (int i = 0; i < NX; ++i) xprev[i * NP + s.xcol] = xa[i];
    }
    s.stage_nodes(T(0), T(0.25));          // nodes at 0, 1/4 .. 1 of the interval: the stiffness at both ends -- and exactly
    const T rate = t_max(s.stiff_rate(pA, s.node(0)), s.stiff_rate(pB, s.node(4)));      // the staging of a single unit
    const int refine_k = (budget > 0 && n_units >= budget) ? 1 : a.max_refine;      // budget spent: no refinement
    int units = s.units_for(rate, Sa, a.rate_max, refine_k);
    const long long units_cap = (long long)Sa * refine_k;
    if (units < units_hint) units = (int)t_min((long long)units_hint, units_cap);
    T ratio_prev = T(-1);
    bool staged = (units == 1);
    for (;;) {                         // error-controlled sub-stepping, as in the Riccati sweep; the start value X(t_k) is `xprev`
      const T hc = s.dgrid / T(units);
      const T ds = T(1) / T(4 * units);
      T err_l = T(0), scl_l = T(0);
      for (int unit = 0; unit < units; ++unit) {
        const T s_lo = T(unit) / T(units);
        if (!(staged && unit == 0)) s.stage_nodes(s_lo, ds);
        staged = false;
        if (Uo && unit == 0) {
          T uo[NU];
          s.aux_control(xa, pA, wA, s.node(0), uo);
          if (valid && fine_x) {
#pragma unroll
            for (int b = 0; b < NU; ++b) Uo[((long long)k * NP + s.xcol) * NU + b] = uo[b];
          }
        }
        const T hq = hc * T(0.25);
        s.fwd_prep(pA, pB, s_lo, ds, hq);
        s.fwd_cols(wA, wB, s_lo, ds);
        LFSD_WAVE_SYNC();      // the parked columns b_j of every node are in place
        // the Richardson pair: coarse Strang step on the upper half of the lane group, two fine ones on the lower half,
        // both in place from the same start value
        s.fwd_chain(xa, hc, hq);
        if (xlane) {
#pragma unroll
          for (int i = 0; i < NX; ++i) xch[((coarse ? NX : 0) + i) * NP + s.xcol] = xa[i];
        }
        LFSD_WAVE_SYNC();      // (also: all reads of this unit's staged coefficients are done before the next staging)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const T xo = xlane ? xch[((coarse ? 0 : NX) + i) * NP + s.xcol] : T(0);      // the other chain's result
          const T xf = coarse ? xo : xa[i], xc = coarse ? xa[i] : xo;
          err_l = t_max(err_l, t_abs(xf - xc));
          xa[i] = xlane ? (T(4) * xf - xc) * (T(1) / T(3)) : T(0);      // both halves continue from the extrapolated value
          scl_l = t_max(scl_l, t_abs(xa[i]));
        }
        if (Uo && k == N - 1 && unit == units - 1) {
          T uo[NU];
          s.aux_control(xa, pB, wB, s.node(4), uo);
          if (valid && fine_x) {
#pragma unroll
            for (int b = 0; b < NU; ++b) Uo[((long long)N * NP + s.xcol) * NU + b] = uo[b];
          }
        }
      }
      n_units += units;
      if (!(a.rtol > T(0))) break;
      LFSD_WAVE_SYNC();
      ldsR[lane] = err_l; ldsR[G + lane] = scl_l;
      LFSD_WAVE_SYNC();
      T eX = T(0), sX = T(0);
      for (int l = 0; l < NP; ++l) { eX = t_max(eX, ldsR[l]); sX = t_max(sX, ldsR[G + l]); }
      LFSD_WAVE_SYNC();
      const T tolX = T(3) * a.rtol * (sX + T(1e-2));       // dx/dtheta starts from zero: absolute floor 1e-2 * rtol
      const T ratio = eX / tolX;
      const bool no_gain = ratio_prev >= T(0) && ratio > T(0.5) * ratio_prev;
      ratio_prev = ratio;
      if (eX <= tolX || no_gain || !t_finite(eX) || (long long)units * 2 > units_cap) {
        if (!(eX <= tolX)) ++n_unmet;
        units_hint = (eX * T(kAuxDown) <= tolX && units > Sa) ? units / 2 : units;
        break;
      }
      units *= 2;
#pragma unroll
      for (int i = 0; i < NX; ++i) xa[i] = xlane ? xprev[i * NP + s.xcol] : T(0);
    }
    if (valid && Xo && fine_x) {
#pragma unroll
      for (int i = 0; i < NX; ++i) Xo[((long long)(k + 1) * NP + s.xcol) * NX + i] = xa[i];
    }
    // loss and gradient contributions of the waypoints that fall into this interval
    // (opt_sol(tau) on the interpolant of the level -- linear, CPDP.py:386, or cubic, :388-390; auxsys_sol(tau) is the linear
    //  interpolant of its grid values at either level: CPDP.py:381 calls interpolation() at its default level)
    // (weighted kernels, ABI 16: loss = sum w |r|^2 and gradient sum w r^T dy/dx X through the scaled residual rs = w r, formed once
    //  -- exact for w = 1 and for powers of two, so all-ones weights give the bits of the unweighted kernel; a waypoint of weight 0 does
    //  not exist: its tau and its target are never read)
    for (int w = 0; w < a.n_waypoints; ++w) {
      T wk = T(1);
      if constexpr (WTD) {
        wk = a.wp_weight[traj * a.n_waypoints + w];
        if (wk == T(0)) continue;
      }
      const T tau = a.taus[traj * a.n_waypoints + w];
      int kw = (int)t_floor(tau / s.dgrid);
      kw = kw < 0 ? 0 : (kw > N - 1 ? N - 1 : kw);
      if (kw != k) continue;
      const T sw = (tau - T(k) * s.dgrid) / s.dgrid;
      T rvec[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) rvec[i] = T(0);
      bool compiled_iface = false;
      if constexpr (M::NIF > 0) {
        // the interface function compiled into the model (iface_idx == NULL): y = g(x(tau)) on the interpolated state, residual
        // r = y - waypoint, and r^T dg/dx as the vector the sensitivity is contracted with (lib/QuadAlgorithm.py:625-637: an
        // arbitrary CasADi expression of the state and its jacobian)
        if (a.iface_idx == nullptr) {
          compiled_iface = true;
          T cur[NX], y[M::NIF], r[M::NIF];
#pragma unroll
          for (int i = 0; i < NX; ++i) cur[i] = s.state_at(i, sw);
          M::iface(cur, s.c, y);
          if constexpr (WTD) {
            T rs[M::NIF];
#pragma unroll
            for (int q = 0; q < M::NIF; ++q) {
              r[q] = y[q] - a.waypoints[(traj * a.n_waypoints + w) * M::NIF + q];
              rs[q] = wk * r[q];
              loss += rs[q] * r[q];
            }
            M::iface_vjp(cur, s.c, rs, rvec);
          } else {
#pragma unroll
          for (int q = 0; q < M::NIF; ++q) {
            r[q] = y[q] - a.waypoints[(traj * a.n_waypoints + w) * M::NIF + q];
            loss += r[q] * r[q];
          }
          M::iface_vjp(cur, s.c, r, rvec);
          }
        }
      }
      for (int q = 0; q < (compiled_iface ? 0 : a.n_iface); ++q) {
        const int idx = a.iface_idx[q];
        const T target = a.waypoints[(traj * a.n_waypoints + w) * a.n_iface + q];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          if (i == idx) {
            const T cur = s.state_at(i, sw);
            const T r = cur - target;
            if constexpr (WTD) {
              const T rs = wk * r;
              rvec[i] += rs;
              loss += rs * r;
            } else {
            rvec[i] += r;
            loss += r * r;
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) { const T xp = xprev[i * NP + s.xcol]; gacc += rvec[i] * (xp + sw * (xa[i] - xp)); }
    }
  }
  if (valid) {
    if (lane == 0) a.loss[traj] = loss;
    if (fine_x) a.grad[traj * NP + s.xcol] = gacc;
    if (a.stats && lane == 0) { a.stats[traj * 4 + 2] = n_units; a.stats[traj * 4 + 3] = n_unmet; }
  }
}

