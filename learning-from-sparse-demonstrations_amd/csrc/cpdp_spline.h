// Curvature grids of the cubic interpolant (COCSys.interpolation(x, y, 2), CPDP.py:388-390: scipy's interp1d(kind='cubic'),
// the not-a-knot cubic spline).  Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).
//
// On the uniform time grid the spline is kept in second-derivative form with c_k = h^2 M_k / 6: on interval k at fraction s,
//   y(s) = y_k + s (y_k+1 - y_k) + ((1-s)^3 - (1-s)) c_k + (s^3 - s) c_k+1,
// the linear interpolant plus a correction that holds neither h nor the horizon (cubic_corr below; the level-2 instantiations of the
// auxiliary sweeps in cpdp_aux.h evaluate it).  With d_k = y_k-1 - 2 y_k + y_k+1 the curvatures solve
//   c_k-1 + 4 c_k + c_k+1 = d_k   (k = 1 .. N-1),     c_0 = 2 c_1 - c_2,   c_N = 2 c_N-1 - c_N-2   (not-a-knot),
// and eliminating the two end rows leaves c_1 = d_1 / 6, c_N-1 = d_N-1 / 6 and the (1,4,1) tridiagonal system for c_2 .. c_N-2
// with those two as known neighbours.  Its pivots p_2 = 4, p_k = 4 - 1 / p_k-1 depend on nothing but k and reach their limit
// 2 + sqrt(3) to the last bit of a double within 16 steps (the map contracts by 1 / p^2 = 0.072): a table of 24 reciprocals
// serves every grid length.
#pragma once
#include "cpdp_common.h"

namespace lfsd {

// weights of c_k and c_k+1 at fraction s of an interval
template <typename T> LFSD_DEV T cubic_wa(T s) { const T r = T(1) - s; return r * r * r - r; }
template <typename T> LFSD_DEV T cubic_wb(T s) { return s * s * s - s; }
// their derivatives in s (the slope of the interpolant, cpdp_times.h: divided by h they are derivatives in time)
template <typename T> LFSD_DEV T cubic_dwa(T s) { const T r = T(1) - s; return T(1) - T(3) * r * r; }
template <typename T> LFSD_DEV T cubic_dwb(T s) { return T(3) * s * s - T(1); }

struct SplinePivots {
  static constexpr int N = 24;
  double q[N];      // q[j] = 1 / p_(j+2)
  constexpr SplinePivots() : q{} {
    double p = 4.0;
    for (int j = 0; j < N; ++j) { q[j] = 1.0 / p; p = 4.0 - q[j]; }
  }
};

template <typename T> LFSD_DEV T spline_q(int k) {      // 1 / p_k, k >= 2 (the same k on every lane: a uniform table read)
  constexpr SplinePivots tab{};
  const int j = k - 2;
  return (T)tab.q[j < SplinePivots::N - 1 ? j : SplinePivots::N - 1];
}

template <typename T> struct SplineArgs {
  int batch, n_grid, n_comp;
  const T* grid;      // [B][n_grid+1][n_comp]
  T* curv;            // [B][n_grid+1][n_comp]   (must not alias grid)
};

// One thread per (trajectory, component), lanes along the component index: the lanes of a wavefront read and write consecutive
// words of one node's row (and run on into the next trajectory's).  Every node is read once on the way up -- a window of three
// values -- plus the last three up front for c_N-1.  Forward elimination leaves the normalised right-hand sides in `curv`;
// back-substitution overwrites them in place.  n_grid >= 3 (checked by the caller); no atomics, no LDS.
template <typename T> __global__ void __launch_bounds__(256) grid_curvature_kernel(SplineArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)a.batch * a.n_comp) return;
  const int N = a.n_grid, C = a.n_comp;
  const long long traj = e / C;
  const int comp = (int)(e - traj * C);
  const T* y = a.grid + traj * (long long)(N + 1) * C + comp;
  T* c = a.curv + traj * (long long)(N + 1) * C + comp;
  const T sixth = T(1) / T(6);
  const T c_last = (y[(long long)(N - 2) * C] - T(2) * y[(long long)(N - 1) * C] + y[(long long)N * C]) * sixth;      // c_N-1
  T ym = y[0], y0 = y[C], yp = y[2 * (long long)C];
  const T c_1 = (ym - T(2) * y0 + yp) * sixth;
  c[C] = c_1;
  c[(long long)(N - 1) * C] = c_last;      // (N == 3: the same value as c_1's neighbour, no interior unknowns)
  T r = c_1;                               // the normalised right-hand side of the row below (row 1: the known c_1)
  for (int k = 2; k <= N - 2; ++k) {
    ym = y0; y0 = yp; yp = y[(long long)(k + 1) * C];
    T d = ym - T(2) * y0 + yp - r;
    if (k == N - 2) d -= c_last;
    r = d * spline_q<T>(k);
    c[(long long)k * C] = r;
  }
  T cn = r;                                // c_N-2 (N == 3: r is still c_1 = c_N-2)
  c[(long long)N * C] = T(2) * c_last - cn;
  for (int k = N - 3; k >= 2; --k) {
    cn = c[(long long)k * C] - spline_q<T>(k) * cn;
    c[(long long)k * C] = cn;
  }
  // c_2 for the first end: N == 3 -> c_2 = c_N-1; N == 4 -> c_2 = c_N-2 = r; else the last value of the loop above
  const T c_2 = (N == 3) ? c_last : cn;
  c[0] = T(2) * c_1 - c_2;
}

}  // namespace lfsd
