// Calling the interpolants on the device (ABI 12): the batched opt_sol(t) / auxsys_sol(t) of the reference's loss functions
// (Examples/pendulum_timewarping.py:72-86, Examples/rocket_groundtruth.py:45-84, lib/QuadAlgorithm.py:306-317, 616-673) and the chain
// rule of a user-written loss through auxsys_sol(tau).  Part of the kernel sources collected by cpdp_kernels.h (include that header,
// not this one).  Nothing of the model enters: any model library serves any grid.
//
// Interval and fraction follow the waypoint rule of the fused loss (cpdp_aux_sweeps.inc, cpdp_aux.h: dgrid = horizon / n_grid):
//   h = horizon / N,   k = clamp(floor(t / h), 0, N - 1),   s = (t - k h) / h,
// so t = horizon is interval N-1 at s = 1 and a t outside [0, horizon] extrapolates its end interval (the range check is the
// host's).  A NaN time selects interval 0 with s = NaN: its row is NaN.
#pragma once
#include "cpdp_common.h"
#include "cpdp_spline.h"

namespace lfsd {

// (the comparisons are false for a NaN quotient: interval 0; no conversion of an out-of-range float to int)
template <typename T> LFSD_DEV int sample_interval(T t, T h, int N) {
  const T q = t_floor(t / h);
  return q >= T(1) ? (q < T(N - 1) ? (int)q : N - 1) : 0;
}

template <typename T> struct SampleArgs {
  int batch, n_grid, n_comp, n_times, times_per_traj;
  const T* grid;      // [B][n_grid+1][n_comp]
  const T* curv;      // [B][n_grid+1][n_comp] (grid_curvature_kernel) or NULL: linear interpolant
  const T* horizon;   // [B]
  const T* times;     // [B][n_times] (times_per_traj) or [n_times]
  T* out;             // [B][n_times][n_comp]   (must not alias an input)
};

// interp1d(time_grid, grid)(t) -- CPDP.py:386 -- or, with `curv`, interp1d(..., kind='cubic')(t) -- CPDP.py:388-390 -- for every
// trajectory, time and component.  One thread per (trajectory, time, component), lanes along the component index: the lanes of a
// wavefront read consecutive words of the two node rows (of at most a few sampling times) and write consecutive words of `out`.
// No LDS, no atomics; 64-bit indices throughout.
template <typename T> __global__ void __launch_bounds__(256) grid_sample_kernel(SampleArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.n_grid, C = a.n_comp, K = a.n_times;
  if (e >= (long long)a.batch * K * C) return;
  const long long row = e / C;                 // trajectory * K + time
  const int comp = (int)(e - row * C);
  const long long traj = row / K;
  const T t = a.times[a.times_per_traj ? row : row - traj * K];
  const T h = a.horizon[traj] / T(N);
  const int k = sample_interval(t, h, N);
  const T s = (t - T(k) * h) / h;
  const long long at = (traj * (long long)(N + 1) + k) * C + comp;
  const T ya = a.grid[at], yb = a.grid[at + C];
  T y = ya + s * (yb - ya);
  if (a.curv) y += cubic_wa(s) * a.curv[at] + cubic_wb(s) * a.curv[at + C];
  a.out[e] = y;
}

template <typename T> struct WaypointVjpArgs {
  int batch, n_grid, n_state, n_control, n_param, n_waypoints;
  const T* horizon;     // [B]
  const T* taus;        // [B][K]
  const T* rx;          // [B][K][n]    dLoss/dx(tau_k)
  const T* ru;          // [B][K][m]    dLoss/du(tau_k), or NULL (then auxU_grid is NULL too)
  const T* auxX_grid;   // [B][n_grid+1][p][n]
  const T* auxU_grid;   // [B][n_grid+1][p][m] or NULL
  T* grad;              // [B][p]
};

// grad[b][q] = sum_k ( sum_i rx[b][k][i] X(tau_k)[q][i] + sum_j ru[b][k][j] U(tau_k)[q][j] ) with X, U the LINEAR interpolants of the
// sensitivity grids (auxsys_sol is linear at either interpolation level, CPDP.py:381): the `diff_loss += r @ dxdp` of every example's
// getloss_corrections without materialising auxsys_sol(tau).  One thread per (trajectory, parameter) sums in a fixed order -- waypoints
// ascending, states then controls, components ascending -- so a row's result does not depend on the batch it is part of.  No atomics,
// no LDS.  (A few KB per trajectory: the launch is latency, not bandwidth.)
template <typename T> __global__ void __launch_bounds__(256) waypoint_vjp_kernel(WaypointVjpArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.n_grid, n = a.n_state, m = a.n_control, p = a.n_param, K = a.n_waypoints;
  if (e >= (long long)a.batch * p) return;
  const long long traj = e / p;
  const int q = (int)(e - traj * p);
  const T h = a.horizon[traj] / T(N);
  const T* Xq = a.auxX_grid + (traj * (long long)(N + 1) * p + q) * n;
  const T* Uq = a.auxU_grid ? a.auxU_grid + (traj * (long long)(N + 1) * p + q) * m : nullptr;
  T acc = T(0);
  for (int w = 0; w < K; ++w) {
    const long long tw = traj * K + w;
    const T tau = a.taus[tw];
    const int k = sample_interval(tau, h, N);
    const T s = (tau - T(k) * h) / h;
    const T* xa = Xq + (long long)k * p * n;
    const T* xb = xa + (long long)p * n;
    const T* r = a.rx + tw * n;
    for (int i = 0; i < n; ++i) acc += r[i] * (xa[i] + s * (xb[i] - xa[i]));
    if (Uq) {
      const T* ua = Uq + (long long)k * p * m;
      const T* ub = ua + (long long)p * m;
      const T* g = a.ru + tw * m;
      for (int j = 0; j < m; ++j) acc += g[j] * (ua[j] + s * (ub[j] - ua[j]));
    }
  }
  a.grad[e] = acc;
}

}  // namespace lfsd
