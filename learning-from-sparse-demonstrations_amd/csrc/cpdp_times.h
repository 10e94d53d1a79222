// Learnable waypoint times (ABI 17): the derivative of the fused waypoint loss with respect to the times tau_k, and the projection that
// keeps an updated time vector ordered.  The reference never measures the times it learns from: its human-input path invents them from
// chord length over an average speed (lib/InputWaypoints.py:212-228), its examples write them by hand; the loss they enter is
// lib/QuadAlgorithm.py:616-673.  The state interpolant is already on the device, and d(loss)/d(tau_k) needs only its slope at tau_k.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).  waypoint_time_grad_kernel takes the
// model as a template argument: a compiled-in interface function (M::NIF > 0) is evaluated as the fused loss evaluates it, so the
// kernel lives in the model library.  tau_project_kernel is model-blind.  Instantiated in the third translation unit only
// (lfsd_cubic.inc).  No atomics, no LDS, no cross-lane operation, fixed summation orders, 64-bit indices: a row's outputs are the same
// bits in any batch and at any position in it.
#pragma once
#include "cpdp_common.h"
#include "cpdp_spline.h"
#include "cpdp_sample.h"

namespace lfsd {

template <typename T> struct TimeGradArgs {
  int batch, n_grid, n_waypoints, n_iface;
  const T* state_grid;    // [B][n_grid+1][NX]
  const T* curv;          // [B][n_grid+1][NX] (grid_curvature_kernel) or nullptr: linear interpolant
  const T* horizon;       // [B]
  const T* consts;        // constants of the compiled-in interface: [B][NC] (const_stride = NC) or [NC] (0); never read by the index path
  int const_stride;
  const T* taus;          // [B][K]
  const T* waypoints;     // [B][K][n_iface]
  const int* iface_idx;   // [n_iface] state components, or nullptr: the interface compiled into the model
  const T* wp_weight;     // [B][K] or nullptr (= 1); a waypoint of weight 0 does not exist
  const T* tau_ref;       // [B][K] or nullptr: the times the prior pulls towards
  T tau_prior;
  T* dtau;                // [B][K]   (must not alias an input)
};

// dtau[b][k] = w_k r^T (dy/dx)(x(tau_k)) xdot(tau_k) + tau_prior (tau_k - tau_ref_k),  r = y(x(tau_k)) - wp_k: HALF the derivative of
// the weighted squared distance, the "no factor 2" convention of the fused gradient.  Interval and fraction are sample_interval and
// the fraction of grid_sample_kernel (the expressions of the fused loss, cpdp_aux_sweeps.inc): a tau on a node belongs to the interval
// on its right, tau = horizon is interval N-1 at s = 1.  The slope is the derivative in tau of exactly the expression
// grid_sample_kernel evaluates: (x_b - x_a) / h, plus (cubic_dwa c_a + cubic_dwb c_b) / h along the cubic interpolant.
// One thread per (trajectory, waypoint) sums the components in ascending order.  The weight enters through the scaled residual
// rs = w r, formed once: exact for w = 1 and for powers of two.  A waypoint of weight 0 gets +0 and none of its tau / target / tau_ref
// is read (they may be NaN padding).  An interface index outside [0, NX) is seen by every thread: nothing is written.  A NaN state row
// gives NaN for its own waypoints only.
template <class M, typename T> __global__ void __launch_bounds__(256) waypoint_time_grad_kernel(TimeGradArgs<T> a) {
  constexpr int NX = M::NX;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.n_grid, K = a.n_waypoints, C = a.n_iface;
  if (e >= (long long)a.batch * K) return;
  if (a.iface_idx) {
    bool in_range = true;
    for (int c = 0; c < C; ++c) in_range = in_range && a.iface_idx[c] >= 0 && a.iface_idx[c] < NX;
    if (!in_range) return;
  }
  T wk = T(1);
  if (a.wp_weight) {
    wk = a.wp_weight[e];
    if (wk == T(0)) { a.dtau[e] = T(0); return; }
  }
  const long long traj = e / K;
  const T tau = a.taus[e];
  const T h = a.horizon[traj] / T(N);
  const int k = sample_interval(tau, h, N);
  const T s = (tau - T(k) * h) / h;
  const T* xa = a.state_grid + (traj * (long long)(N + 1) + k) * NX;
  const T* xb = xa + NX;
  const T* ca = a.curv ? a.curv + (traj * (long long)(N + 1) + k) * NX : nullptr;
  const T wa = cubic_wa(s), wb = cubic_wb(s), dwa = cubic_dwa(s), dwb = cubic_dwb(s);
  auto value = [&](int i) {
    T v = xa[i] + s * (xb[i] - xa[i]);
    if (ca) v += wa * ca[i] + wb * ca[NX + i];
    return v;
  };
  auto slope = [&](int i) {
    T d = (xb[i] - xa[i]) / h;
    if (ca) d += (dwa * ca[i] + dwb * ca[NX + i]) / h;
    return d;
  };
  T acc = T(0);
  bool compiled_iface = false;
  if constexpr (M::NIF > 0) {
    if (a.iface_idx == nullptr) {
      compiled_iface = true;
      // (the trajectory's constants and the ones derived from them, staged as aux_setup stages them for the fused loss)
      constexpr int NCA = M::NCX > 0 ? M::NCX : 1;
      T cst[NCA];
      for (int i = 0; i < M::NC; ++i) cst[i] = a.consts[traj * a.const_stride + i];
      if constexpr (M::ND > 0) M::derive_consts(cst);
      T cur[NX], y[M::NIF], rs[M::NIF], rvec[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) { cur[i] = value(i); rvec[i] = T(0); }
      M::iface(cur, cst, y);
#pragma unroll
      for (int q = 0; q < M::NIF; ++q) rs[q] = wk * (y[q] - a.waypoints[e * M::NIF + q]);
      M::iface_vjp(cur, cst, rs, rvec);
#pragma unroll
      for (int i = 0; i < NX; ++i) acc += rvec[i] * slope(i);
    }
  }
  if (!compiled_iface) {
    for (int q = 0; q < C; ++q) {
      const int i = a.iface_idx[q];
      const T rs = wk * (value(i) - a.waypoints[e * C + q]);
      acc += rs * slope(i);
    }
  }
  if (a.tau_ref && a.tau_prior != T(0)) acc += a.tau_prior * (tau - a.tau_ref[e]);
  a.dtau[e] = acc;
}

template <typename T> struct TauProjectArgs {
  int batch, n_waypoints;
  const T* tau_ref;        // [B][K] the ordered times the step started from
  T* tau_io;               // [B][K] in: the proposal, out: the projected times   (must not alias tau_ref)
  const T* horizon;        // [B]
  const T* wp_weight;      // [B][K] or nullptr
  const T* tau_lo;         // [B][K] or nullptr
  const T* tau_hi;         // [B][K] or nullptr
  T max_shift;             // c, 0 < c < 0.5 (the host's check)
  const int* row_active;   // [B] or nullptr: rows with 0 keep every word
};

// tau_io[k] <- clamp(tau_io[k], ref_k - c (ref_k - ref_prev), ref_k + c (ref_next - ref_k)) for every existing waypoint (weight != 0),
// prev / next the nearest existing waypoints in tau_ref, 0 before the first and the horizon after the last.  With c < 0.5 two
// neighbours keep at least (1 - 2c) of their gap: the order cannot invert whatever was proposed.  tau_lo / tau_hi are applied FIRST
// and the window last, so where the two do not intersect the order wins.  A non-finite proposal keeps ref_k.  One thread per row walks
// k ascending; every clamp reads tau_ref only, so the result does not depend on the order of the writes.  Rows with row_active == 0
// and waypoints of weight 0 keep their words (of a waypoint that does not exist nothing is read either).
template <typename T> __global__ void __launch_bounds__(256) tau_project_kernel(TauProjectArgs<T> a) {
  // (no fused multiply-add in the window's two bounds: every product and difference is rounded on its own, so the result is the one
  //  plain IEEE arithmetic gives anywhere -- the host restatement of the tests, the emulator build -- bit for bit)
  // (g++, the emulator build: it honours no contraction pragma; it contracts only when the target has FMA instructions, and the
  //  emulator is built for baseline x86-64 (tests/conftest.py: no -march, no -mfma).  A build with such flags must add
  //  -ffp-contract=off, or the bit-for-bit comparison with numpy in tests/tau_cases.py fails and says so)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = a.n_waypoints;
  if (b >= a.batch) return;
  if (a.row_active && !a.row_active[b]) return;
  const T* ref = a.tau_ref + b * K;
  const T* w = a.wp_weight ? a.wp_weight + b * K : nullptr;
  T* io = a.tau_io + b * K;
  const T c = a.max_shift;
  T prev = T(0);
  for (int k = 0; k < K; ++k) {
    if (w && w[k] == T(0)) continue;
    const T rk = ref[k];
    T next = a.horizon[b];
    for (int j = k + 1; j < K; ++j) {
      if (!w || w[j] != T(0)) { next = ref[j]; break; }
    }
    const T lo = rk - c * (rk - prev), hi = rk + c * (next - rk);
    T v = io[k];
    if (!t_finite(v)) {
      v = rk;
    } else {
      if (a.tau_lo) v = t_max(v, a.tau_lo[b * K + k]);
      if (a.tau_hi) v = t_min(v, a.tau_hi[b * K + k]);
      v = v < lo ? lo : (v > hi ? hi : v);
    }
    io[k] = v;
    prev = rk;
  }
}

}  // namespace lfsd
