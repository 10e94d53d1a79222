// Auxiliary control system: Riccati and forward-sensitivity sweeps + waypoint loss (COCSys.auxSysSolver, CPDP.py:316-381).
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).
#pragma once
#include "cpdp_common.h"
#include "cpdp_spline.h"

namespace lfsd {

// =====================================================================================
//  Auxiliary control system (differentiated maximum principle)
// =====================================================================================
// (Measured and removed: the Z-dependent product fx^T Z of the Riccati right-hand side on the matrix cores -- +12 % -- and the stiff
//  update's Gram matrix by m lanes + an LDS hand-over -- +1.5 %: profiles/HISTORY.md, profiles/r03_mfma_aux.txt, r04_h_*.)

template <typename T> struct AuxArgs {
  int batch, n_grid, substeps;    // substeps = minimum coarse split-steps per grid interval (fine = 2x, Richardson)
  T rate_max;                     // refine an interval until  dt * |Huu^-1 fu^T P fu|_inf <= rate_max
  int max_refine;                 // cap on that refinement (factor over `substeps`)
  int unit_budget;                // > 0, for rows whose OC solve did NOT end converged / at working precision (oc_status given and not
                                  // 1 or 2): once such a trajectory has spent this many split units in a sweep its remaining intervals
                                  // run at `substeps` units without refinement (and count as accepted above rtol when they are).  Its
                                  // grids are not a KKT point, so its sensitivities are approximate whatever the sweeps do; and a row whose
                                  // parameters have left the well-posed region must not hold its launch at the cap of EVERY interval
  T rtol;                         // > 0: error-controlled sub-stepping -- an interval is redone with twice the units while the
                                  // Richardson estimate |fine - coarse| / 3 of a column exceeds rtol * (its magnitude + floor)
  const T* horizon;               // [B]
  const T* auxvar;                // [B][NP]
  const T* consts; int const_stride;
  const T* state_grid;            // [B][N+1][NX]
  const T* control_grid;          // [B][N+1][NU]
  const T* costate_grid;          // [B][N+1][NX]
  T* Z_grid;                      // [B][N+1][NX+NP][NX]   column-major Z = [P W]
  // forward sweep / loss
  int n_waypoints, n_iface;
  const int* iface_idx;           // [n_iface] state components the interface exposes; nullptr: the interface function compiled into
                                  // the model (Model::NIF outputs; n_iface must equal it)
  const T* taus;                  // [B][n_waypoints]
  const T* waypoints;             // [B][n_waypoints][n_iface]
  T* loss;                        // [B]
  T* grad;                        // [B][NP]
  T* auxX_grid;                   // [B][N+1][NP][NX] or nullptr  (dx/dtheta, column-major)
  T* auxU_grid;                   // [B][N+1][NP][NU] or nullptr
  int* stats;                     // [B][4] or nullptr: split units executed and intervals accepted ABOVE rtol, Riccati | forward sweep
  const int* oc_status;           // [B] or nullptr: status of the OC solve; rows whose status bit is set in skip_mask are not
  int skip_mask;                  // differentiated (no sweep, NaN loss / gradient): include/lfsd_cpdp.h, ABI 8
  LFSD_DEV bool skipped(long long traj) const { return oc_status != nullptr && ((skip_mask >> (oc_status[traj] & 31)) & 1) != 0; }
  LFSD_DEV int budget(long long traj) const {
    if (oc_status == nullptr || unit_budget <= 0) return 0;
    const int st = oc_status[traj];
    return (st == ST_CONVERGED || st == ST_STALLED) ? 0 : unit_budget;
  }
};

// Interpolation level 2 (COCSys.cocSolver(..., interplation_level=2), CPDP.py:388-390): the sweeps integrate along the not-a-knot
// cubic spline of the grid values, given as one curvature grid per solution grid (cpdp_spline.h).  The level-1 kernels keep
// AuxArgs and their kernel arguments as they are.
template <typename T> struct AuxArgsCubic : AuxArgs<T> {
  const T* state_curv;            // [B][N+1][NX]
  const T* control_curv;          // [B][N+1][NU]
  const T* costate_curv;          // [B][N+1][NX]
};

// Waypoint weights (ABI 16): loss = sum_k w_k |y(tau_k) - wp_k|^2.  The weighted forward sweeps are instantiations of their own with
// argument structs of their own: the unweighted kernels keep their arguments and their code as they are, instruction for
// instruction.  wp_weight is never NULL here -- a NULL weight array is served by the unweighted kernel.
template <typename T> struct AuxArgsWeighted : AuxArgs<T> {
  const T* wp_weight;             // [B][n_waypoints], non-negative and finite (the caller's to guarantee); 0: the waypoint does not exist
};
template <typename T> struct AuxArgsCubicWeighted : AuxArgsCubic<T> {
  const T* wp_weight;
};

// LAY: which packing of the staged coefficients the kernel uses (codegen: 0 Riccati sweep, every matrix; 1 forward sweep,
// without Hxx / Hxe) -- the node stride NCOEF and every offset behind it follow
// NSLOT: node slots in LDS -- NNODE (one split unit), or 2 NNODE - 1 where the Riccati sweep stages the nodes of two consecutive
// units in one pass (ric_pair_stage below)
template <class M, int LAY = 0, int NSLOT = 5> struct AuxLayout {
  static constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NZ = NX + NP, NNODE = 5;
  static constexpr bool PAIR = NSLOT > NNODE;
  static_assert(NSLOT == NNODE || (LAY == 0 && NSLOT == 2 * NNODE - 1), "node slots");
  static constexpr int NCOEF = M::NCOEF_L[LAY];
  static constexpr int LDS_L = 0;
  static constexpr int LDS_S = LDS_L + NSLOT * NCOEF;
  static constexpr int LDS_T = LDS_S + NX * NU;
  // LDS_T (transposed exchange of the Riccati right-hand side) and LDS_KN/LDS_PSI (forward sweep) share one region:
  // each kernel uses only its own
  static constexpr int LDS_KN = LDS_T;                        // 3 stiff nodes x (NX x NU) feedback rows K^T
  static constexpr int LDS_PSI = LDS_KN + 3 * NX * NU;        // 3 stiff nodes x {phi1(h/4 K fu), phi1(h/2 K fu)}
  static constexpr int LDS_TSZ0 = (LAY == 0) ? NX * NZ : 3 * NX * NU + 6 * NU * NU;
  static constexpr int LDS_TSZ = LDS_TSZ0 > 128 ? LDS_TSZ0 : 128;      // (>= 2 x 64: the error reduction of the step control)
  static constexpr int LDS_E = LDS_T + LDS_TSZ;
                                                              // cold per-trajectory state: auxvar, consts,
  static constexpr int LDS_C = LDS_E + NP;                    // and the (x,u,lambda) grid values at both interval ends
  static constexpr int LDS_GA = LDS_C + M::NCX;               // [x_k u_k l_k]
  static constexpr int LDS_GB = LDS_GA + 2 * NX + NU;         // [x_k+1 u_k+1 l_k+1]
  static constexpr int LDS_END = LDS_GB + 2 * NX + NU;
  static constexpr int lds_elems() { return ((LDS_END + 3) / 4) * 4; }
  // level-2 kernels only, behind everything else of the kernel's slice: the curvature rows [cx cu cl] of the interval's two nodes
  static constexpr int CURV = ((2 * (2 * NX + NU) + 3) / 4) * 4;
  // forward kernel only, behind LDS_END:
  static constexpr int FWD_XPREV = LDS_END;                   // parking slot for X(t_k) (row i of column j at [i*NP + j])
  // ... per node and column, the X-independent part of the right-hand side (fe - fu Huu^-1 (fu^T W + Hue)) e_j
  static constexpr int FWD_BC = FWD_XPREV + NX * NP;
  // ... the P columns at both ends of the interval ([end][column][row], and one zero row that lanes without a P column
  // point at): they are needed three times per unit only, too cold for 2*NX registers per lane
  static constexpr int FWD_P = FWD_BC + NNODE * NX * NP;
  // ... the hand-over of the two Richardson chains, which run on different lanes ([chain][row][column])
  static constexpr int FWD_XCH = FWD_P + 2 * NX * NX + NX;
  // ... and the reductions of the step control (one word per lane, twice)
  static constexpr int FWD_RED = FWD_XCH + 2 * NX * NP;
  static constexpr int lds_elems_fwd() { return ((FWD_RED + 128 + 3) / 4) * 4; }
  // Riccati kernel only: one parking slot per lane for a column of Z (row i of lane l at [i*G + l]): of the unit's start value and
  // the coarse Richardson result only one has to be in registers at a time
  // (pair staging: rows NZ words apart instead of G.  The lanes beyond the last column carry no column of Z: their words of the slot are
  //  what pays for the four extra node slots.  They park into LDS_T instead -- words [l + i*NZ], l < G - NZ, inside the exchange
  //  buffer -- which ric_rhs overwrites between a parking write and its read: such a lane reads back ARBITRARY words, and from the
  //  first unit on its z[] is private garbage, not zero.  That is harmless only because nothing of an idle lane is ever consumed:
  //  the writes to LDS_S / LDS_T are gated by lane < NX, the error reduction, the symmetrisation and the stores of Z by lane < NZ,
  //  and its hcol / ucol point at the node's zero word.  Code that reads z[] or the reduction words of lanes >= NZ must not rely on
  //  zeros there.)
  template <int G> static constexpr int ric_pstride() { return PAIR ? NZ : G; }
  template <int G> static constexpr int ric_park() { return LDS_END; }
  // ... and a second one: the start value of a STEP of the step-size control inside a stiff interval (aux_riccati_kernel, "adaptive")
  // (compiled into the fp32 instantiations with lane groups of at most 16 lanes -- pendulum, robot arm, cart-pole: the small models,
  //  whose sweeps have registers to spare; the 32-lane sweeps of the quadrotor / rocket run two waves per SIMD at 252 registers, spilled
  //  60 B per lane with it (headline aux_riccati 1.50 -> 1.545 ms) and stay exactly what they were)
  template <int G> static constexpr bool ric_adaptive() { return G <= 16; }
  template <int G> static constexpr int ric_park2() { return ric_park<G>() + NX * ric_pstride<G>(); }
  template <int G> static constexpr int lds_elems_ric() { return ((ric_park2<G>() + (ric_adaptive<G>() ? NX * G : 0) + 3) / 4) * 4; }
};

// Lanes per trajectory of the forward sweep.  Only the NP columns of X = dx/dtheta advance there; the NX columns of P are
// merely interpolated.  The two chains of a Richardson pair run side by side on the two halves of the lane group -- lanes
// j < NP carry column j through the two fine Strang steps, lanes G/2 + j carry the same column through the coarse one --
// and lanes < NX double as the owners of P column `lane` where the feedback gains are formed, so max(NX, 2 NP) lanes are
// needed (quadrotor: 16, four trajectories per wavefront; the Riccati sweep needs 32 for its NX+NP columns).  The m x m
// matrix functions of the three stiff nodes run row per lane on sub-groups of sub_lanes<NU>() lanes.
template <class M> constexpr int fwd_lanes() {
  int need = M::NX > 2 * M::NP ? M::NX : 2 * M::NP;
  if (need < 5) need = 5;                                      // AuxLayout::NNODE staging lanes
  if (need < 3 * sub_lanes<M::NU>()) need = 3 * sub_lanes<M::NU>();
  int g = 8;
  while (g < need) g *= 2;
  return g;
}

// LFSD_RIC_PAIR_STAGE (cpdp_common.h): the fp32 Riccati sweep of the 32-lane models along the linear interpolant stages the nine
// distinct coefficient nodes of two consecutive split units in one pass.  Everything else -- fp64, level 2, the step-controlled sweep
// of the small models, the forward sweep -- stages one unit at a time.
// ... and only where the nine slots fit: the sweep runs two waves per SIMD, eight one-wave workgroups share the 160 KB of a CU, so a
// workgroup (64 / G trajectories) may take 20 480 B.  A model whose slice is larger with nine slots (the rocket: 12 parameters, 204
// coefficients per node -- 20 864 B) keeps five slots and the one-unit staging, bit for bit the LFSD_RIC_PAIR_STAGE=0 kernel.
constexpr int kRicLdsPerWorkgroup = 20480;
template <class M, typename T, int G, int LAY, int LVL> constexpr int aux_node_slots() {
  if constexpr (LFSD_RIC_PAIR_STAGE != 0 && sizeof(T) == 4 && G == 32 && LAY == 0 && LVL == 1)
    return (64 / G) * AuxLayout<M, 0, 9>::template lds_elems_ric<G>() * (int)sizeof(T) <= kRicLdsPerWorkgroup ? 9 : 5;
  else
    return 5;
}
// (the node slot the unit in hand starts at: a member only where units are staged in pairs, so that every other AuxCtx is what it was)
template <bool PAIR> struct AuxNodeSlot { int nslot = 0; };
template <> struct AuxNodeSlot<false> {};

// (the prefetch registers of the curvature rows: an empty base where a kernel has none, so that AuxCtx is what it was at level 1)
template <typename T, int N> struct AuxCurvPf { T cpf[N]; };
template <typename T> struct AuxCurvPf<T, 0> {};

// LVL: interpolation level of the nominal trajectory (1 linear, CPDP.py:386; 2 cubic, CPDP.py:388-390)
template <class M, typename T, int G, int LAY, int LVL = 1> struct AuxCtx
    : AuxCurvPf<T, (sizeof(T) == 4 && LVL == 2 && (LAY == 1 || G <= 16)) ? (2 * M::NX + M::NU + G - 1) / G : 0>,
      AuxNodeSlot<(aux_node_slots<M, T, G, LAY, LVL>() > 5)> {
  static_assert(LVL == 1 || LVL == 2, "interpolation level");
  static constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NC = M::NC, NZ = NX + NP;
  using Lay = AuxLayout<M, LAY, aux_node_slots<M, T, G, LAY, LVL>()>;
  static constexpr int H = G / 2;      // forward sweep: first lane of the coarse Richardson chain
  int lane;
  int xcol;                  // forward sweep: column of X = dx/dtheta (and of W) this lane carries (fine chain: lanes < NP,
  bool xlane, coarse;        // coarse chain: lanes H .. H+NP-1), else 0
  const T *e, *c;            // [NP], [NC] in LDS
  const T *xa_, *ua_, *la_, *xb_, *ub_, *lb_;   // grid values at both ends of the interval, in LDS
  T t_a, dgrid;
  T* lds;
  T ox[NX], oe[NP];    // one-hot selectors of this lane's column
  // Riccati sweep: where this lane's column of [Hxx Hxe] (NX rows) and of [Hux Hue] (NU rows) sits in node 0 (structural
  // zeros point at the node's zero word): `y += H e_lane` is a gather of NX words, not a product with a one-hot vector
  const T* hcol[LAY == 0 ? NX : 1];
  const T* ucol[LAY == 0 ? NU : 1];

  // Grid values (x, u, lambda) of the two nodes of interval k into LDS.  Consecutive intervals share a node, and the sweeps walk
  // the grid in one direction (`dir` = +1 forward sweep, -1 Riccati sweep): only the NEW node is read from memory, and it is
  // fetched into registers ONE INTERVAL AHEAD (`gpf`, one or two words per lane) -- an interval is a few thousand clocks of work
  // on a wavefront that is (nearly) alone on its SIMD, and used to start by waiting a global round trip for 60 words.
  static constexpr int NR = 2 * NX + NU, GPF = (NR + G - 1) / G;
  static constexpr bool PF = sizeof(T) == 4;      // (fp64: the registers are not there -- aux_forward 2.03 -> 2.57 ms, aux_riccati 4.60 -> 4.78 with it)
  T gpf[GPF];
  T *gA_ = nullptr, *gB_ = nullptr;
  // level 2: the curvature rows [cx cu cl] of the same two nodes sit in a region of their own behind the kernel's slice, laid out
  // as LDS_GA / LDS_GB are: the row of a node is CDELTA words behind its grid row, so the rows change ends with the grid rows and
  // need no pointers of their own.  They take the same prefetch where the registers are there: the forward sweep, and the Riccati
  // sweep of the small models (AuxLayout::ric_adaptive).  The 32-lane fp32 Riccati sweep runs two waves per SIMD at 252 of 256
  // registers; with one more word per lane it spilled 20 B, so its new node's curvature row goes from memory straight to LDS at the
  // start of the interval.
  static constexpr int CURV_OFF = LAY == 0 ? Lay::template lds_elems_ric<G>() : Lay::lds_elems_fwd();
  static constexpr int CDELTA = CURV_OFF - Lay::LDS_GA;
  static constexpr bool CPF = PF && LVL == 2 && (LAY == 1 || G <= 16);      // (the size of the AuxCurvPf base says the same)
  template <class A> LFSD_DEV void fetch_node(const A& a, long long traj, int node, int N) {
    const T* xs = a.state_grid + (traj * (N + 1) + node) * NX;
    const T* us = a.control_grid + (traj * (N + 1) + node) * NU;
    const T* ls = a.costate_grid + (traj * (N + 1) + node) * NX;
#pragma unroll
    for (int j = 0; j < GPF; ++j) {
      const int idx = lane + j * G;
      gpf[j] = (idx < NX) ? xs[idx] : ((idx < NX + NU) ? us[idx - NX] : ((idx < NR) ? ls[idx - NX - NU] : T(0)));
    }
    if constexpr (CPF) {
      const T* cx = a.state_curv + (traj * (N + 1) + node) * NX;
      const T* cu = a.control_curv + (traj * (N + 1) + node) * NU;
      const T* cl = a.costate_curv + (traj * (N + 1) + node) * NX;
#pragma unroll
      for (int j = 0; j < GPF; ++j) {
        const int idx = lane + j * G;
        this->cpf[j] = (idx < NX) ? cx[idx] : ((idx < NX + NU) ? cu[idx - NX] : ((idx < NR) ? cl[idx - NX - NU] : T(0)));
      }
    }
  }
  template <class A> LFSD_DEV void load_interval(const A& a, long long traj, int k, int N, int dir) {
    LFSD_WAVE_SYNC();                         // previous interval's readers are done
    if (gA_ == nullptr || !PF) {              // first interval of the sweep: both nodes straight from memory
      gA_ = lds + Lay::LDS_GA; gB_ = lds + Lay::LDS_GB;
      const T* xs = a.state_grid + (traj * (N + 1) + k) * NX;
      const T* us = a.control_grid + (traj * (N + 1) + k) * NU;
      const T* ls = a.costate_grid + (traj * (N + 1) + k) * NX;
      for (int i = lane; i < NX; i += G) { gA_[i] = xs[i]; gB_[i] = xs[NX + i]; gA_[NX + NU + i] = ls[i]; gB_[NX + NU + i] = ls[NX + i]; }
      for (int i = lane; i < NU; i += G) { gA_[NX + i] = us[i]; gB_[NX + i] = us[NU + i]; }
      if constexpr (LVL == 2) {
        T* cA_ = gA_ + CDELTA; T* cB_ = gB_ + CDELTA;
        const T* cx = a.state_curv + (traj * (N + 1) + k) * NX;
        const T* cu = a.control_curv + (traj * (N + 1) + k) * NU;
        const T* cl = a.costate_curv + (traj * (N + 1) + k) * NX;
        for (int i = lane; i < NX; i += G) { cA_[i] = cx[i]; cB_[i] = cx[NX + i]; cA_[NX + NU + i] = cl[i]; cB_[NX + NU + i] = cl[NX + i]; }
        for (int i = lane; i < NU; i += G) { cA_[NX + i] = cu[i]; cB_[NX + i] = cu[NU + i]; }
      }
    } else {                                  // the shared node changes ends, the new node comes out of the registers
      T* t_ = gA_; gA_ = gB_; gB_ = t_;
      T* dst = (dir > 0) ? gB_ : gA_;
#pragma unroll
      for (int j = 0; j < GPF; ++j) { const int idx = lane + j * G; if (idx < NR) dst[idx] = gpf[j]; }
      if constexpr (LVL == 2) {
        T* cdst = dst + CDELTA;
        if constexpr (CPF) {
#pragma unroll
          for (int j = 0; j < GPF; ++j) { const int idx = lane + j * G; if (idx < NR) cdst[idx] = this->cpf[j]; }
        } else {
          const int nd = (dir > 0) ? k + 1 : k;      // the node this interval adds
          const T* cx = a.state_curv + (traj * (N + 1) + nd) * NX;
          const T* cu = a.control_curv + (traj * (N + 1) + nd) * NU;
          const T* cl = a.costate_curv + (traj * (N + 1) + nd) * NX;
          for (int i = lane; i < NX; i += G) { cdst[i] = cx[i]; cdst[NX + NU + i] = cl[i]; }
          for (int i = lane; i < NU; i += G) cdst[NX + i] = cu[i];
        }
      }
    }
    xa_ = gA_; ua_ = gA_ + NX; la_ = gA_ + NX + NU; xb_ = gB_; ub_ = gB_ + NX; lb_ = gB_ + NX + NU;
    t_a = M::TIME_VARYING ? dgrid * T(k) : T(0);
    LFSD_WAVE_SYNC();
    const int nn = (dir > 0) ? k + 2 : k - 1;     // the node the NEXT interval adds
    if (PF && nn >= 0 && nn <= N) fetch_node(a, traj, nn, N);
  }
  // Lane `node` (< 5) evaluates the packed PMP coefficients at its own time node s (fraction of the
  // interval) on the reference's interpolant of (x,u,lambda) (CPDP.py:320-323; linear, or at level 2 cubic) and stages them in LDS.
  // Pair staging (`nn` = 9): lanes 5-8 take nodes 1-4 of the NEXT unit, whose first node sits at s_next; node 4 of this unit is node 0
  // of the next and is stored once -- the caller pairs two units only where both expressions give the same fraction (pair_ok).  Every
  // lane forms its fraction as the one-unit pass of ITS unit does, first node + s_step * index: the staged coefficients are bit-equal.
  LFSD_DEV void stage_nodes(T s_first, T s_step, T s_next = T(0), int nn = Lay::NNODE) {
    if (lane < (Lay::PAIR ? nn : Lay::NNODE)) {
      T sf = s_first;
      int li = lane;
      if constexpr (Lay::PAIR) { if (lane >= Lay::NNODE) { sf = s_next; li = lane - (Lay::NNODE - 1); } }
      const T s = sf + s_step * T(li);
      T x[NX], u[NU], l[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) { x[i] = xa_[i] + s * (xb_[i] - xa_[i]); l[i] = la_[i] + s * (lb_[i] - la_[i]); }
#pragma unroll
      for (int i = 0; i < NU; ++i) u[i] = ua_[i] + s * (ub_[i] - ua_[i]);
      if constexpr (LVL == 2) {             // + ((1-s)^3 - (1-s)) c_k + (s^3 - s) c_k+1  (cpdp_spline.h)
        const T wa = cubic_wa(s), wb = cubic_wb(s);
        const T *cA_ = xa_ + CDELTA, *cB_ = xb_ + CDELTA;
#pragma unroll
        for (int i = 0; i < NX; ++i) { x[i] += wa * cA_[i] + wb * cB_[i]; l[i] += wa * cA_[NX + NU + i] + wb * cB_[NX + NU + i]; }
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] += wa * cA_[NX + i] + wb * cB_[NX + i];
      }
      T* L = lds + Lay::LDS_L + lane * Lay::NCOEF;
      M::template pmp_coeffs<LAY>(t_a + s * dgrid, x, u, l, e, c, L);
      if constexpr (!M::IHUU_CLOSED) {      // (a diagonal Huu is inverted in closed form by pmp_coeffs itself)
        T Huu[NU * NU], iH[NU * NU];
#pragma unroll
        for (int i = 0; i < NU * NU; ++i) Huu[i] = L[M::OFF_HUU_L[LAY] + i];
        mat_inverse<NU>(Huu, iH);       // casadi.pinv(ddHuu) of a nonsingular Huu (CPDP.py:262)
#pragma unroll
        for (int i = 0; i < NU * NU; ++i) L[M::OFF_IHUU_L[LAY] + i] = iH[i];
      }
    }
    LFSD_WAVE_SYNC();
  }
  LFSD_DEV static bool pair_ok(T s_first, T s_step, T s_next) { return s_first + s_step * T(Lay::NNODE - 1) == s_next; }
  // Pair staging: the unit in hand reads its five nodes from slot `nslot` on (0 or 4); node() and the column pointers move with it
  LFSD_DEV void node_base(int slot) {
    if constexpr (Lay::PAIR) {
      const int d = (slot - this->nslot) * Lay::NCOEF;
      this->nslot = slot;
#pragma unroll
      for (int i = 0; i < NX; ++i) hcol[i] += d;
#pragma unroll
      for (int a = 0; a < NU; ++a) ucol[a] += d;
    }
  }
  LFSD_DEV const T* node(int i) const {
    if constexpr (Lay::PAIR) return lds + Lay::LDS_L + (this->nslot + i) * Lay::NCOEF;
    else return lds + Lay::LDS_L + i * Lay::NCOEF;
  }
  // component i of x(t_k + s dgrid) on the interpolant (the waypoint loss: opt_sol(tau), lib/QuadAlgorithm.py:625)
  LFSD_DEV T state_at(int i, T s) const {
    T v = xa_[i] + s * (xb_[i] - xa_[i]);
    if constexpr (LVL == 2) v += cubic_wa(s) * xa_[CDELTA + i] + cubic_wb(s) * xb_[CDELTA + i];
    return v;
  }

  // |Huu^-1 fu^T P fu|_inf : rate of the stiff closed-loop modes at one node (P = first NX lanes' columns)
  LFSD_DEV T stiff_rate(const T* zt, const T* L) {
    T* ldsS = lds + Lay::LDS_S;
    T s[NU], kj[NU];
    M::template fu_mulT<false, LAY>(L, zt, s);
    M::template ihuu_mul<LAY>(L, s, kj);
    if (lane < NX) {
#pragma unroll
      for (int a = 0; a < NU; ++a) ldsS[lane * NU + a] = kj[a];
    }
    LFSD_WAVE_SYNC();
    T Mx[NU * NU];
    M::template fu_gram<false, LAY>(L, ldsS, Mx);
    T nrm = T(0);
#pragma unroll
    for (int a = 0; a < NU; ++a) {
      T r = T(0);
#pragma unroll
      for (int b = 0; b < NU; ++b) r += t_abs(Mx[a * NU + b]);
      nrm = t_max(nrm, r);
    }
    LFSD_WAVE_SYNC();
    return nrm;
  }
  LFSD_DEV int units_for(T rate, int Sa, T rate_max, int max_refine) const {
    T want = rate * dgrid / rate_max;
    if (!t_finite(want)) want = T(Sa);
    int u = Sa;
    const long long cap = (long long)Sa * max_refine;
    while ((T)u < want && (long long)u * 2 <= cap) u *= 2;
    return u;
  }
  // ---- Riccati (backward in time; tau = -t) -------------------------------------------------
  // stiff sub-flow  dZ/dtau = -P R Z,  R = fu Huu^-1 fu^T :   Z <- Z - P fu (Huu/dt + fu^T P fu)^-1 fu^T Z
  LFSD_DEV void ric_stiff(T* z, const T* L, T dt) {
    T* ldsS = lds + Lay::LDS_S;
    T s[NU];
    M::template fu_mulT<false, LAY>(L, z, s);
    if (lane < NX) {
#pragma unroll
      for (int a = 0; a < NU; ++a) ldsS[lane * NU + a] = s[a];
    }
    LFSD_WAVE_SYNC();
    T Gm[NU * NU];
    const T idt = T(1) / dt;
#pragma unroll
    for (int i = 0; i < NU * NU; ++i) Gm[i] = L[M::OFF_HUU_L[LAY] + i] * idt;
    M::template fu_gram<true, LAY>(L, ldsS, Gm);
    lu_factor<NU>(Gm);
    lu_solve<NU>(Gm, s);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      T d = T(0);
#pragma unroll
      for (int a = 0; a < NU; ++a) d += ldsS[i * NU + a] * s[a];
      z[i] -= d;
    }
    LFSD_WAVE_SYNC();
  }
  // non-stiff part  dZ/dtau = [Qt qt] + A^T Z + P [A rt]   (A, Qt, rt, qt of CPDP.py:265-269)
  LFSD_DEV void ric_rhs(const T* z, int nd, T* y) {
    T* ldsT = lds + Lay::LDS_T;
    const T* L = node(nd);
    T s[NU], v[NU], w[NU], nv[NU], r[NP], wq[NU];
    {
      // (this lane's column of Huu^-1 [Hux Hue] is recomputed per right-hand side: with the midpoint rule's six per unit that is
      //  cheaper than parking it per node and lane -- measured 1.37 against 1.47 / 2.30 ms, profiles/HISTORY.md)
      T hu[NU];
#pragma unroll
      for (int a = 0; a < NU; ++a) hu[a] = ucol[a][nd * Lay::NCOEF];      // (Hux | Hue) e_lane
      M::template ihuu_mul<LAY>(L, hu, wq);
    }
    M::template fu_mulT<false, LAY>(L, z, s);
    M::template ihuu_mul<LAY>(L, s, v);
#pragma unroll
    for (int a = 0; a < NU; ++a) { nv[a] = -v[a]; w[a] = -(wq[a] + v[a]); }
    M::template fx_mulT<false, LAY>(L, z, y);
    if (lane < NX) {
      T tv[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) tv[i] = y[i];
      M::template Hxu_mul<true, LAY>(L, nv, tv);
      M::template fe_mulT<false, LAY>(L, z, r);
      M::template Hue_mulT<true, LAY>(L, nv, r);
#pragma unroll
      for (int i = 0; i < NX; ++i) ldsT[lane * NZ + i] = tv[i];
#pragma unroll
      for (int i = 0; i < NP; ++i) ldsT[lane * NZ + NX + i] = r[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) y[i] += hcol[i][nd * Lay::NCOEF];      // [Hxx Hxe] e_lane
    M::template Hxu_mul<true, LAY>(L, w, y);
    LFSD_WAVE_SYNC();
    if (lane < NZ) {
#pragma unroll
      for (int i = 0; i < NX; ++i) y[i] += ldsT[i * NZ + lane];
    }
    LFSD_WAVE_SYNC();
  }
  // non-stiff RK4 step of length h over nodes (n0, n1, n2)
  LFSD_DEV void ric_rk4(T* z, int n0, int n1, int n2, T h) {
    T k[NX], acc[NX], zs[NX];
    if constexpr (aux_rk<T>() == 2) {
      // explicit midpoint rule: the Strang splitting around it is second order anyway, and in fp32 the rounding floor of
      // the sweep hides the two orders the Richardson pair gains with RK4 (cpdp_common.h, kAuxRk32)
      (void)n2; (void)acc;
      ric_rhs(z, n0, k);
#pragma unroll
      for (int i = 0; i < NX; ++i) zs[i] = z[i] + T(0.5) * h * k[i];
      ric_rhs(zs, n1, k);
#pragma unroll
      for (int i = 0; i < NX; ++i) z[i] += h * k[i];
      return;
    }
    ric_rhs(z, n0, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] = k[i]; zs[i] = z[i] + T(0.5) * h * k[i]; }
    ric_rhs(zs, n1, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] += T(2) * k[i]; zs[i] = z[i] + T(0.5) * h * k[i]; }
    ric_rhs(zs, n1, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] += T(2) * k[i]; zs[i] = z[i] + h * k[i]; }
    ric_rhs(zs, n2, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) z[i] += h / T(6) * (acc[i] + k[i]);
  }
  // Strang step: stiff h/2, non-stiff h, stiff h/2
  LFSD_DEV void ric_strang(T* z, int n0, int n1, int n2, T h) {
    ric_stiff(z, node(n0), h * T(0.5));
    ric_rk4(z, n0, n1, n2, h);
    ric_stiff(z, node(n2), h * T(0.5));
  }
  // two Strang steps of length h/2 over nodes (0,1,2) and (2,3,4): the two adjacent stiff quarter-steps at the middle
  // node are the exact flow of the same frozen system, so they compose exactly into one half-step
  LFSD_DEV void ric_strang2(T* z, T h) {
    ric_stiff(z, node(0), h * T(0.25));
    ric_rk4(z, 0, 1, 2, h * T(0.5));
    ric_stiff(z, node(2), h * T(0.5));
    ric_rk4(z, 2, 3, 4, h * T(0.5));
    ric_stiff(z, node(4), h * T(0.25));
  }

  // ---- forward auxiliary state -----------------------------------------------------------------
  // Lane roles.  Lanes < NX own P column `lane` (both interval ends in LDS) wherever feedback gains are formed.  Lanes
  // j < NP carry X / W column j through the FINE chain of a Richardson pair (two Strang steps), lanes H + j carry the same
  // column through the COARSE one (one Strang step): the pair costs the instructions of the fine chain alone, and a lane
  // holds one chain's state, not two.
  // stiff sub-flow  X' = -fu K X,  K = Huu^-1 fu^T P (frozen over the sub-step), solved exactly:
  //   X(dt) = X - dt fu phi1(dt K fu) K X,   phi1(M) = M^-1 (I - e^-M)   (m x m matrix function).
  // (An A-stable rational step is not enough here: with a cheap control cost dt*|K fu| reaches O(10^2).)
  // fwd_prep: for the three stiff nodes (0, 2, 4) of a unit the P lanes gather K(t_node); then the matrix function of
  // each node (quarter and half step) is evaluated once per unit, ROW PER LANE on a sub-group of Q lanes per node
  // (phi1_neg_rows: the m x m products cost m FMAs + m DPP moves per lane instead of m^3 FMAs on one lane of the group).
  LFSD_DEV void fwd_prep(const T* zA, const T* zB, T s0, T ds, T hq) {
    T* ldsK = lds + Lay::LDS_KN;
    T* ldsP = lds + Lay::LDS_PSI;
    // (outer per-node loops rolled: 5 % faster than unrolled, profiles/r01_tune_aux_occupancy.txt, r01_tune_compiler_flags.txt)
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
      const T* L = node(2 * r);
      const T sr = s0 + T(2 * r) * ds;
      T zt[NX], sv[NU], kj[NU];
#pragma unroll
      for (int i = 0; i < NX; ++i) zt[i] = zA[i] + sr * (zB[i] - zA[i]);
      M::template fu_mulT<false, LAY>(L, zt, sv);
      M::template ihuu_mul<LAY>(L, sv, kj);
      if (lane < NX) {
#pragma unroll
        for (int a = 0; a < NU; ++a) ldsK[(r * NX + lane) * NU + a] = kj[a];
      }
    }
    LFSD_WAVE_SYNC();
    if constexpr (NU <= 4) {
      constexpr int Q = sub_lanes<NU>();
      // every lane of the group runs the same instructions (sub_bcast needs its sources active): sub-groups beyond the
      // third repeat node 4 and drop the result
      const int sg = lane / Q, a = lane % Q;
      const int r = sg < 2 ? sg : 2;
      const bool row = a < NU;
      const bool mine = sg < 3 && row;
      const int ar = row ? a : 0;
      T sa[NX], Mrow[NU], Pq[NU], Ph[NU];
#pragma unroll
      for (int i = 0; i < NX; ++i) sa[i] = ldsK[(r * NX + i) * NU + ar];
      M::template fu_mulT<false, LAY>(node(2 * r), sa, Mrow);                  // row a of K fu = fu^T (row a of K)
      T rs = T(0);
#pragma unroll
      for (int j = 0; j < NU; ++j) { Mrow[j] = row ? Mrow[j] * hq : T(0); rs += t_abs(Mrow[j]); }
      // one scaling for the three nodes (|.|_inf over all rows of the group): uniform trip count of the squaring loop
      T* red = lds + Lay::FWD_RED;
      red[lane] = mine ? rs : T(0);
      LFSD_WAVE_SYNC();
      T nrm = T(0);
#pragma unroll
      for (int l = 0; l < 3 * Q; ++l) nrm = t_max(nrm, red[l]);
      LFSD_WAVE_SYNC();
      int sq = 0;
      T sc = T(1);
      while (nrm * sc > T(0.25) && sq < 60) { sc *= T(0.5); ++sq; }
      phi1_neg_rows<NU, Q>(Mrow, a, sq, sc, Pq, Ph);
      if (mine) {
#pragma unroll
        for (int j = 0; j < NU; ++j) { ldsP[(r * 2) * NU * NU + a * NU + j] = Pq[j]; ldsP[(r * 2 + 1) * NU * NU + a * NU + j] = Ph[j]; }
      }
    } else {
      if (lane < 3) {
        T Mx[NU * NU], Pq[NU * NU], Ph[NU * NU];
        M::template fu_gram<false, LAY>(node(2 * lane), ldsK + lane * NX * NU, Mx);       // K fu
#pragma unroll
        for (int i = 0; i < NU * NU; ++i) Mx[i] *= hq;
        phi1_neg<NU>(Mx, Pq, Ph);
#pragma unroll
        for (int i = 0; i < NU * NU; ++i) { ldsP[lane * 2 * NU * NU + i] = Pq[i]; ldsP[(lane * 2 + 1) * NU * NU + i] = Ph[i]; }
      }
    }
    LFSD_WAVE_SYNC();
  }
  // apply the prepared exact stiff step of stiff node r (0..2) over dt = hq (half == 0) or 2 hq (half == 1); r and half
  // may differ between the lanes (the two chains sit at different nodes)
  static constexpr bool FETCH = sizeof(T) == 4;      // (fp64: the registers are not there, cpdp_common.h)
  LFSD_DEV void fwd_stiff(T* xa, int r, int half, T dt) {
    if constexpr (!FETCH) {
      const T* Kn = lds + Lay::LDS_KN + r * NX * NU;
      const T* Psi = lds + Lay::LDS_PSI + (r * 2 + half) * NU * NU;
      T kx[NU], y[NU];
#pragma unroll
      for (int a = 0; a < NU; ++a) kx[a] = T(0);
#pragma unroll
      for (int i = 0; i < NX; ++i) {
#pragma unroll
        for (int a = 0; a < NU; ++a) kx[a] += Kn[i * NU + a] * xa[i];
      }
      matvec<NU>(Psi, kx, y);
#pragma unroll
      for (int a = 0; a < NU; ++a) y[a] *= -dt;
      M::template fu_mul<true, LAY>(node(2 * r), y, xa);
      return;
    }
    // gain rows, matrix function and fu of the node: fetched into registers with back-to-back reads, one wait (lds_fetch)
    T Kn[NX * NU], Psi[NU * NU], Lf[M::FU_N_L[LAY]];
    lds_issue<NX * NU>(lds + Lay::LDS_KN + r * NX * NU, Kn);
    lds_issue<NU * NU>(lds + Lay::LDS_PSI + (r * 2 + half) * NU * NU, Psi);
    lds_issue<M::FU_N_L[LAY]>(node(2 * r), Lf);
    lds_land<NX * NU>(Kn); lds_land<NU * NU>(Psi); lds_land<M::FU_N_L[LAY]>(Lf);
    T kx[NU], y[NU];
#pragma unroll
    for (int a = 0; a < NU; ++a) kx[a] = T(0);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
#pragma unroll
      for (int a = 0; a < NU; ++a) kx[a] += Kn[i * NU + a] * xa[i];
    }
    matvec<NU>(Psi, kx, y);
#pragma unroll
    for (int a = 0; a < NU; ++a) y[a] *= -dt;
    M::template fu_mul<true, LAY>(Lf, y, xa);
  }
  // non-stiff part  X' = fx X + fe - fu Huu^-1 (Hux X + Hue + fu^T W).  Its X-independent part
  //   b_j(t) = (fe - fu Huu^-1 (fu^T W(t) + Hue)) e_j
  // is evaluated once per staged node (fwd_cols) and parked per column; the right-hand sides of a unit then cost
  //   y = fx x - fu Huu^-1 Hux x + b_j.
  // Three rounds for the five nodes: the fine lanes of a column take nodes 0, 1, 2, its coarse lanes nodes 3, 4 (and 4 again).
  LFSD_DEV void fwd_cols(const T* zA, const T* zB, T s0, T ds) {
    T* bc = lds + Lay::FWD_BC;
#pragma unroll 1
    for (int rd = 0; rd < 3; ++rd) {
      const int nd = coarse ? (rd < 2 ? 3 + rd : 4) : rd;
      const T* L = node(nd);
      const T sr = s0 + T(nd) * ds;
      T wt[NX], sv[NU], v[NU], b[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) wt[i] = zA[i] + sr * (zB[i] - zA[i]);
      M::template fu_mulT<false, LAY>(L, wt, sv);
      M::template Hue_mul<true, LAY>(L, oe, sv);
      M::template ihuu_mul<LAY>(L, sv, v);
#pragma unroll
      for (int a = 0; a < NU; ++a) v[a] = -v[a];
      M::template fe_mul<false, LAY>(L, oe, b);
      M::template fu_mul<true, LAY>(L, v, b);
      if (xlane) {
#pragma unroll
        for (int i = 0; i < NX; ++i) bc[(nd * NX + i) * NP + xcol] = b[i];
      }
    }
  }
  LFSD_DEV void fwd_rhs(const T* xa, int nd, T* y) {
    if constexpr (!FETCH) {
      const T* L = node(nd);
      const T* bc = lds + Lay::FWD_BC + nd * NX * NP;     // lanes without an X column read column 0; their result is dropped
      T s[NU], v[NU];
      M::template Hxu_mulT<false, LAY>(L, xa, s);
      M::template ihuu_mul<LAY>(L, s, v);
#pragma unroll
      for (int a = 0; a < NU; ++a) v[a] = -v[a];
      M::template fx_mul<false, LAY>(L, xa, y);
      M::template fu_mul<true, LAY>(L, v, y);
#pragma unroll
      for (int i = 0; i < NX; ++i) y[i] += bc[i * NP + xcol];
      return;
    }
    // the node's fu, fx, Hxu, Huu^-1 (a prefix of the forward packing) and this column's b_j: registers first (lds_fetch)
    T L[M::RHS_N_L[LAY]], b[NX];
    lds_issue<M::RHS_N_L[LAY]>(node(nd), L);
    lds_issue_strided<NX>(lds + Lay::FWD_BC + nd * NX * NP + xcol, NP, b);     // lanes without an X column read column 0; their result is dropped
    lds_land<M::RHS_N_L[LAY]>(L); lds_land<NX>(b);
    T s[NU], v[NU];
    M::template Hxu_mulT<false, LAY>(L, xa, s);
    M::template ihuu_mul<LAY>(L, s, v);
#pragma unroll
    for (int a = 0; a < NU; ++a) v[a] = -v[a];
    M::template fx_mul<false, LAY>(L, xa, y);
    M::template fu_mul<true, LAY>(L, v, y);
#pragma unroll
    for (int i = 0; i < NX; ++i) y[i] += b[i];
  }
  // non-stiff RK4 step of length h over nodes (n0, n1, n2) -- per-lane values
  LFSD_DEV void fwd_rk4(T* xa, int n0, int n1, int n2, T h) {
    T k[NX], acc[NX], xs[NX];
    if constexpr (aux_rk<T>() == 2) {
      (void)n2; (void)acc;
      fwd_rhs(xa, n0, k);
#pragma unroll
      for (int i = 0; i < NX; ++i) xs[i] = xa[i] + T(0.5) * h * k[i];
      fwd_rhs(xs, n1, k);
#pragma unroll
      for (int i = 0; i < NX; ++i) xa[i] += h * k[i];
      return;
    }
    fwd_rhs(xa, n0, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] = k[i]; xs[i] = xa[i] + T(0.5) * h * k[i]; }
    fwd_rhs(xs, n1, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] += T(2) * k[i]; xs[i] = xa[i] + T(0.5) * h * k[i]; }
    fwd_rhs(xs, n1, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) { acc[i] += T(2) * k[i]; xs[i] = xa[i] + h * k[i]; }
    fwd_rhs(xs, n2, k);
#pragma unroll
    for (int i = 0; i < NX; ++i) xa[i] += h / T(6) * (acc[i] + k[i]);
  }
  // One split unit of length hc for this lane's chain:
  //   fine    stiff(node 0, hq)   RK(nodes 0 1 2, hc/2)  stiff(node 2, 2 hq)  RK(nodes 2 3 4, hc/2)  stiff(node 4, hq)
  //   coarse  stiff(node 0, 2 hq) RK(nodes 0 2 4, hc)    stiff(node 4, 2 hq)
  // (hq = hc/4; the two adjacent fine stiff quarter-steps at the middle node compose exactly into one half-step.)  The
  // first three operations are the same instructions with per-lane nodes and step lengths; the coarse lanes sit out the
  // last two.
  LFSD_DEV void fwd_chain(T* x, T hc, T hq) {
    const int c = coarse ? 1 : 0;
    fwd_stiff(x, 0, c, coarse ? T(2) * hq : hq);
    fwd_rk4(x, 0, 1 + c, 2 + 2 * c, coarse ? hc : hc * T(0.5));
    fwd_stiff(x, 1 + c, 1, T(2) * hq);
    if (!coarse) {
      fwd_rk4(x, 2, 3, 4, hc * T(0.5));
      fwd_stiff(x, 2, 0, hq);
    }
  }
  // auxiliary control at a grid point (CPDP.py:295):  U = -Huu^-1((Hux + fu^T P) X + fu^T W + Hue)
  LFSD_DEV void aux_control(const T* xa, const T* pt, const T* wt, const T* L, T* uo) {
    T* ldsS = lds + Lay::LDS_S;
    T s[NU];
    M::template fu_mulT<false, LAY>(L, pt, s);          // P role: row `lane` of (fu^T P)^T
    if (lane < NX) {
#pragma unroll
      for (int a = 0; a < NU; ++a) ldsS[lane * NU + a] = s[a];
    }
    LFSD_WAVE_SYNC();
    M::template fu_mulT<false, LAY>(L, wt, s);          // X role: s = fu^T w_j + Hue e_j + Hux x_j + fu^T P x_j
    M::template Hue_mul<true, LAY>(L, oe, s);
    M::template Hxu_mulT<true, LAY>(L, xa, s);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
#pragma unroll
      for (int a = 0; a < NU; ++a) s[a] += ldsS[i * NU + a] * xa[i];
    }
    M::template ihuu_mul<LAY>(L, s, uo);
#pragma unroll
    for (int a = 0; a < NU; ++a) uo[a] = -uo[a];
    LFSD_WAVE_SYNC();
  }
};

template <class M, typename T, int G, int LAY, int LVL> LFSD_DEV void aux_setup(AuxCtx<M, T, G, LAY, LVL>& s, const AuxArgs<T>& a, long long traj,
                                                            T* lds_all, int lds_stride) {
  constexpr int NX = M::NX, NP = M::NP, NC = M::NC;
  using Lay = typename AuxCtx<M, T, G, LAY, LVL>::Lay;
  const int gib = threadIdx.x / G;
  s.lane = threadIdx.x % G;
  s.coarse = (LAY == 1) && (s.lane >= G / 2);
  const int xl = s.coarse ? s.lane - G / 2 : s.lane;
  s.xlane = (LAY == 1) && (xl < NP);
  s.xcol = s.xlane ? xl : 0;
  s.lds = lds_all + gib * lds_stride;
  {
    T* le = s.lds + Lay::LDS_E;
    T* lc = s.lds + Lay::LDS_C;
    for (int i = s.lane; i < NP; i += G) le[i] = a.auxvar[traj * NP + i];
    for (int i = s.lane; i < NC; i += G) lc[i] = a.consts[traj * a.const_stride + i];
    if constexpr (M::ND > 0) { LFSD_WAVE_SYNC(); if (s.lane == 0) M::derive_consts(lc); }
    s.e = le; s.c = lc;
  }
  LFSD_WAVE_SYNC();
  s.dgrid = a.horizon[traj] / T(a.n_grid);
#pragma unroll
  for (int i = 0; i < NX; ++i) s.ox[i] = (s.lane == i) ? T(1) : T(0);
#pragma unroll
  for (int i = 0; i < NP; ++i) s.oe[i] = (LAY == 1 ? (s.xlane && s.xcol == i) : (s.lane == NX + i)) ? T(1) : T(0);
}

// Synchronisation in the two auxiliary sweeps: the number of split units per interval (`units`) follows each trajectory's
// own stiffness, so the lane groups of one wavefront pass DIFFERENT numbers of synchronisation points.  A workgroup barrier
// (__syncthreads / s_barrier) under such data-dependent control flow is undefined; what the sweeps need is less than a
// barrier anyway: a workgroup is exactly ONE wavefront (launched with 64 threads, checked on entry), every lane group
// works on its own private LDS slice, and the only hand-over is between lanes of the same wavefront.  LFSD_WAVE_SYNC
// (cpdp_common.h) is exactly that: an LDS-scoped release/acquire fence pair (s_waitcnt lgkmcnt(0) -- the DS queue of a
// wavefront is in order) around a wave_barrier (a scheduling fence for the compiler, no instruction).  A port to multi-wave
// workgroups would have to make `units` block-uniform first (as oc_solve_kernel does with its votes).
// Occupancy, measured on MI355X (profiles/r01_tune_aux_occupancy.txt, r01_tune_compiler_flags.txt): compiled without clang's SLP
// vectoriser the fp32 Riccati sweep runs two waves per SIMD -- the 2048 waves of the benchmark batch in one round instead of two,
// 8.2 -> 5.7 ms once the coarse and the fine Richardson chain run in place with the other column parked in LDS (246 VGPRs).  The
// forward sweep and fp64 stay at one wave per SIMD (256 + 256 registers): in place the forward sweep is 20 % slower.
// the sweeps along the linear interpolant ...
#define LFSD_AUX_LVL 1
#define LFSD_AUX_ARGS AuxArgs
#define LFSD_AUX_RICCATI_KERNEL aux_riccati_kernel
#define LFSD_AUX_FORWARD_KERNEL aux_forward_kernel
#include "cpdp_aux_sweeps.inc"
#undef LFSD_AUX_LVL
#undef LFSD_AUX_ARGS
#undef LFSD_AUX_RICCATI_KERNEL
#undef LFSD_AUX_FORWARD_KERNEL
// ... and along the cubic one
#define LFSD_AUX_LVL 2
#define LFSD_AUX_ARGS AuxArgsCubic
#define LFSD_AUX_RICCATI_KERNEL aux_riccati_cubic_kernel
#define LFSD_AUX_FORWARD_KERNEL aux_forward_cubic_kernel
#include "cpdp_aux_sweeps.inc"
#undef LFSD_AUX_LVL
#undef LFSD_AUX_ARGS
#undef LFSD_AUX_RICCATI_KERNEL
#undef LFSD_AUX_FORWARD_KERNEL
// ... and the forward sweeps of both levels with a weight per waypoint (the Riccati sweep knows no waypoints: not included again)
#define LFSD_AUX_WEIGHTED 1
#define LFSD_AUX_LVL 1
#define LFSD_AUX_ARGS AuxArgsWeighted
#define LFSD_AUX_FORWARD_KERNEL aux_forward_weighted_kernel
#include "cpdp_aux_sweeps.inc"
#undef LFSD_AUX_LVL
#undef LFSD_AUX_ARGS
#undef LFSD_AUX_FORWARD_KERNEL
#define LFSD_AUX_LVL 2
#define LFSD_AUX_ARGS AuxArgsCubicWeighted
#define LFSD_AUX_FORWARD_KERNEL aux_forward_cubic_weighted_kernel
#include "cpdp_aux_sweeps.inc"
#undef LFSD_AUX_LVL
#undef LFSD_AUX_ARGS
#undef LFSD_AUX_FORWARD_KERNEL
#undef LFSD_AUX_WEIGHTED

}  // namespace lfsd
