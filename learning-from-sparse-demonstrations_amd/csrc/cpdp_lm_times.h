// Levenberg-Marquardt over parameters and waypoint times jointly (ABI 18).  The residual block of waypoint k of a row is
// r_k = y(tau_k) - wp_k; its Jacobian in theta is J_k (normal_matrix_kernel, cpdp_lm.h), in tau_k the interface rows t_k of the slope
// xdot(tau_k) (waypoint_time_grad_kernel, cpdp_times.h), and in no other time.  The Gauss-Newton matrix of (theta, tau) is therefore an
// arrow: H = sum w J^T J in the corner, the couplings c_k = w_k J_k^T t_k along the border, a DIAGONAL time block d_k = w_k t_k^T t_k.
// time_blocks_kernel forms the border and the diagonal; lm_step_times_kernel is the accept / reject state machine of lm_step_kernel
// with the times eliminated one waypoint at a time -- a rank-one correction of the p x p matrix each, so the factorisation stays p x p
// whatever K and the group size are.  The reference has first-order rules and fixed times only (lib/QuadAlgorithm.py:454-578,
// lib/InputWaypoints.py:212-228): new surface, nothing of it is consulted by the other update paths.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).  Nothing of the model enters: any model
// library serves them.  Instantiated in the third translation unit only (lfsd_cubic.inc).  No atomics, fixed summation orders, 64-bit
// indices: a row's (a group's) outputs are the same bits in any batch and at any position in it.
#pragma once
#include "cpdp_common.h"
#include "cpdp_spline.h"
#include "cpdp_sample.h"
#include "cpdp_lm.h"

namespace lfsd {

template <typename T> struct TimeBlocksArgs {
  int batch, n_grid, n_state, n_param, n_waypoints, n_iface;
  const int* iface_idx;   // [n_iface] state components of the interface
  const T* horizon;       // [B]
  const T* taus;          // [B][K]
  const T* wp_weight;     // [B][K] or nullptr (= 1); a waypoint of weight 0 does not exist
  const T* state_grid;    // [B][n_grid+1][n]
  const T* curv;          // [B][n_grid+1][n] (grid_curvature_kernel of the state grid) or nullptr: linear interpolant
  const T* auxX_grid;     // [B][n_grid+1][p][n]
  T* C;                   // [B][K][p]   (must not alias an input)
  T* d;                   // [B][K]      (must not alias an input)
};

// C[b][k][q] = sum_c (w_k t_c) X(tau_k)[q][idx_c],  d[b][k] = sum_c (w_k t_c) t_c,  t_c = xdot(tau_k)[idx_c].  X is the linear
// interpolant of auxX_grid, expression for expression that of normal_matrix_kernel; t the slope of waypoint_time_grad_kernel on its
// index path (the linear interpolant's, plus the derivative of the cubic correction with a curvature grid).  One thread per
// (trajectory, waypoint, parameter) sums the interface components in ascending order; the thread of parameter 0 also writes d.  The
// weight enters once, through (w t_c): all-ones weights give the bits of nullptr, powers of two scale exactly.  A waypoint of weight 0
// gets +0 and none of its tau is read (NaN padding is legal).  An interface index outside [0, n_state) is seen by every thread of the
// launch: nothing is written (the documented choice of lfsd_normal_matrix).  A NaN row gives NaN for its own waypoints only.
template <typename T> __global__ void __launch_bounds__(256) time_blocks_kernel(TimeBlocksArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.n_grid, n = a.n_state, p = a.n_param, K = a.n_waypoints, C = a.n_iface;
  if (e >= (long long)a.batch * K * p) return;
  bool in_range = true;
  for (int c = 0; c < C; ++c) in_range = in_range && a.iface_idx[c] >= 0 && a.iface_idx[c] < n;
  if (!in_range) return;
  const long long wpt = e / p;                 // (trajectory, waypoint)
  const int q = (int)(e - wpt * p);
  const long long traj = wpt / K;
  T wk = T(1);
  const bool weighted = a.wp_weight != nullptr;
  if (weighted) {
    wk = a.wp_weight[wpt];
    if (wk == T(0)) {
      a.C[e] = T(0);
      if (q == 0) a.d[wpt] = T(0);
      return;
    }
  }
  const T tau = a.taus[wpt];
  const T h = a.horizon[traj] / T(N);
  const int k = sample_interval(tau, h, N);
  const T s = (tau - T(k) * h) / h;
  const T* xa = a.state_grid + (traj * (long long)(N + 1) + k) * n;
  const T* xb = xa + n;
  const T* ca = a.curv ? a.curv + (traj * (long long)(N + 1) + k) * n : nullptr;
  const T dwa = cubic_dwa(s), dwb = cubic_dwb(s);
  const long long node = (long long)p * n;
  const T* a1 = a.auxX_grid + (traj * (long long)(N + 1) * p + q) * n + (long long)k * node;
  T acc = T(0), dacc = T(0);
  for (int c = 0; c < C; ++c) {
    const int i = a.iface_idx[c];
    T t = (xb[i] - xa[i]) / h;
    if (ca) t += (dwa * ca[i] + dwb * ca[n + i]) / h;
    const T x1 = a1[i] + s * (a1[node + i] - a1[i]);
    if (weighted) {
      const T wt = wk * t;
      acc += wt * x1;
      dacc += wt * t;
    } else {
      acc += t * x1;
      dacc += t * t;
    }
  }
  a.C[e] = acc;
  if (q == 0) a.d[wpt] = dacc;
}

template <typename T> struct LmStepTimesArgs {
  int n_groups, group_size, n_param, n_waypoints;
  T lambda_down, lambda_up, lambda_min, lambda_max;
  // per group (in/out): the state of lfsd_lm_step
  T* theta;                // [G][p]     last accepted point
  T* loss_acc;             // [G]        loss there (+inf: nothing accepted yet)
  T* grad_acc;             // [G][p]
  T* H_acc;                // [G][p][p]
  T* lambda;               // [G]
  T* theta_trial;          // [G][p]     in: the point just evaluated; out: the next point to evaluate
  // per row (in/out), B = G * group_size rows, row g * group_size + r belongs to group g
  T* tau;                  // [B][K]     accepted times
  T* tau_trial;            // [B][K]     in: the times just evaluated; out: the next (unprojected) times
  T* gtau_acc;             // [B][K]     dLoss/dtau (no factor 2, no prior) at the accepted point
  T* C_acc;                // [B][K][p]
  T* d_acc;                // [B][K]
  int* ok_acc;             // [B]        rows that counted at the accepted point
  // the evaluation at (theta_trial, tau_trial)
  const T* loss_t;         // [G]
  const T* grad_t;         // [G][p]
  const T* H_t;            // [G][p][p]
  const T* gtau_t;         // [B][K]
  const T* C_t;            // [B][K][p]
  const T* d_t;            // [B][K]
  const int* row_ok;       // [B] or nullptr: rows with 0 did not count in this evaluation (their values are never read)
  const T* wp_weight;      // [B][K] or nullptr; weight 0: the waypoint does not exist
  const T* proj_lo;        // [p] or nullptr
  const int* group_active; // [G] or nullptr: groups with 0 keep every word of their state and of their rows' state
  int* accepted;           // [G] or nullptr
};

// One group per lane, built like lm_step_kernel: the matrix S that is factored lives in the lane's column of an LDS array laid out
// [element][lane], the lanes never read each other's column, so there is no barrier; every loop makes the same number of trips in
// every lane (group_size, n_waypoints and n_param are launch constants, the retry loop always makes LM_RETRIES + 1 trips), a bad pivot
// is remembered, not branched out of.  Per attempt the lower triangle of
//   S = H_acc + lambda (diag H_acc + floor I) - sum_k c_k c_k^T / D_k,    D_k = d_k + lambda (d_k + ftau),
// and b = -grad_acc + sum_k c_k gtau_k / D_k are formed in LDS -- rows ascending, waypoints ascending, over the rows with ok_acc != 0
// and the waypoints that exist and whose D_k is positive -- and factored IN PLACE by the arithmetic of lm_step_kernel, expression for
// expression: with every c_k and d_k zero no correction is executed (D_k = 0 is not positive) and theta, theta_trial, lambda and
// accepted are the bits lm_step_kernel gives.  The rows' records are read straight from global memory, uncoalesced, as lm_step_kernel
// reads H_acc; the launch is latency.
template <typename T> __global__ void __launch_bounds__(LM_BLOCK) lm_step_times_kernel(LmStepTimesArgs<T> a) {
  __shared__ T Ls[LM_MAX_PARAM * (LM_MAX_PARAM + 1) / 2 * LM_BLOCK];
  __shared__ T ys[LM_MAX_PARAM * LM_BLOCK];
  const int lane = threadIdx.x;
  const long long g = (long long)blockIdx.x * blockDim.x + lane;
  const int p = a.n_param, K = a.n_waypoints, D = a.group_size;
  if (g >= a.n_groups) return;
  if (a.group_active && !a.group_active[g]) {
    if (a.accepted) a.accepted[g] = 0;
    return;
  }
  T* th = a.theta + g * p;
  T* tt = a.theta_trial + g * p;
  T* ga = a.grad_acc + g * p;
  T* Ha = a.H_acc + g * p * p;
  const T* gt = a.grad_t + g * p;
  const T* Ht = a.H_t + g * p * p;
  const long long row0 = g * D;
  T* L = Ls + lane;
  T* y = ys + lane;
  const T inf = T(__builtin_huge_val());
  // 1. accept or reject the trial point (theta_trial, tau_trial)
  const T lt = a.loss_t[g];
  bool finite = t_finite(lt);
  for (int j = 0; j < p; ++j) finite = finite && t_finite(gt[j]);
  for (int j = 0; j < p * p; ++j) finite = finite && t_finite(Ht[j]);
  for (int r = 0; r < D; ++r) {
    const long long row = row0 + r;
    const bool counted = !a.row_ok || a.row_ok[row] != 0;
    for (int k = 0; k < K; ++k) {
      const long long w = row * K + k;
      const bool exists = !a.wp_weight || a.wp_weight[w] != T(0);
      if (counted && exists) {
        finite = finite && t_finite(a.gtau_t[w]) && t_finite(a.d_t[w]);
        for (int j = 0; j < p; ++j) finite = finite && t_finite(a.C_t[w * p + j]);
      }
    }
  }
  const bool accept = finite && lt < a.loss_acc[g];
  T lam = a.lambda[g];
  if (accept) {
    for (int j = 0; j < p; ++j) { th[j] = tt[j]; ga[j] = gt[j]; }
    for (int j = 0; j < p * p; ++j) Ha[j] = Ht[j];
    a.loss_acc[g] = lt;
    lam = t_max(lam * a.lambda_down, a.lambda_min);
  } else {
    lam = t_min(lam * a.lambda_up, a.lambda_max);
  }
  for (int r = 0; r < D; ++r) {
    const long long row = row0 + r;
    const bool counted = !a.row_ok || a.row_ok[row] != 0;
    if (accept) {
      for (int k = 0; k < K; ++k) {
        const long long w = row * K + k;
        a.tau[w] = a.tau_trial[w];
        if (counted) {
          a.gtau_acc[w] = a.gtau_t[w];
          a.d_acc[w] = a.d_t[w];
          for (int j = 0; j < p; ++j) a.C_acc[w * p + j] = a.C_t[w * p + j];
        }
      }
      a.ok_acc[row] = counted ? 1 : 0;
    }
  }
  if (a.accepted) a.accepted[g] = accept ? 1 : 0;
  // 2. a group without an accepted point, or without any sensitivity, cannot move
  T hmax = Ha[0];
  for (int j = 1; j < p; ++j) hmax = t_max(hmax, Ha[(long long)j * p + j]);
  const bool can_move = a.loss_acc[g] != inf && hmax > T(0);
  const T floor_ = T(1e-8) * hmax;
  // 3. the floor of the time block: the largest d among the waypoints that enter
  T dmax = T(0);
  for (int r = 0; r < D; ++r) {
    const long long row = row0 + r;
    const bool counted = a.ok_acc[row] != 0;
    for (int k = 0; k < K; ++k) {
      const long long w = row * K + k;
      const bool exists = !a.wp_weight || a.wp_weight[w] != T(0);
      if (counted && exists) dmax = t_max(dmax, a.d_acc[w]);
    }
  }
  const T ftau = T(1e-8) * dmax;
  // 3.-4. the times eliminated, Cholesky without pivoting in place, more damping while a pivot is not positive
  bool need = can_move, solved = false;
  for (int attempt = 0; attempt <= LM_RETRIES; ++attempt) {
    if (need) {
      for (int j = 0; j < p; ++j) {
        const int rj = j * (j + 1) / 2;
        const T hjj = Ha[(long long)j * p + j];
        L[(rj + j) * LM_BLOCK] = hjj + lam * (hjj + floor_);
        for (int k = 0; k < j; ++k) L[(rj + k) * LM_BLOCK] = Ha[(long long)j * p + k];
        y[j * LM_BLOCK] = -ga[j];
      }
      for (int r = 0; r < D; ++r) {
        const long long row = row0 + r;
        const bool counted = a.ok_acc[row] != 0;
        for (int k = 0; k < K; ++k) {
          const long long w = row * K + k;
          const bool exists = !a.wp_weight || a.wp_weight[w] != T(0);
          if (counted && exists) {
            const T dk = a.d_acc[w];
            const T Dk = dk + lam * (dk + ftau);
            if (Dk > T(0)) {
              const T* c = a.C_acc + w * p;
              const T gk = a.gtau_acc[w];
              for (int i = 0; i < p; ++i) {
                const int ri = i * (i + 1) / 2;
                const T ui = c[i] / Dk;
                y[i * LM_BLOCK] += ui * gk;
                for (int j = 0; j <= i; ++j) L[(ri + j) * LM_BLOCK] -= ui * c[j];
              }
            }
          }
        }
      }
      bool bad = false;
      for (int j = 0; j < p; ++j) {
        const int rj = j * (j + 1) / 2;
        T d = L[(rj + j) * LM_BLOCK];
        for (int k = 0; k < j; ++k) d -= L[(rj + k) * LM_BLOCK] * L[(rj + k) * LM_BLOCK];
        bad = bad || !(d > T(0)) || !t_finite(d);
        const T ljj = t_sqrt(d);
        L[(rj + j) * LM_BLOCK] = ljj;
        for (int i = j + 1; i < p; ++i) {
          const int ri = i * (i + 1) / 2;
          T s = L[(ri + j) * LM_BLOCK];
          for (int k = 0; k < j; ++k) s -= L[(ri + k) * LM_BLOCK] * L[(rj + k) * LM_BLOCK];
          L[(ri + j) * LM_BLOCK] = s / ljj;
        }
      }
      if (bad) {
        if (attempt < LM_RETRIES) lam = t_min(lam * a.lambda_up, a.lambda_max);
      } else {
        need = false;
        solved = true;
      }
    }
  }
  // 4.-5. S dtheta = b by the two substitutions, the step and the projection, then the times by back-substitution -- or the group
  // stays where it is
  if (solved) {
    for (int i = 0; i < p; ++i) {
      const int ri = i * (i + 1) / 2;
      T s = y[i * LM_BLOCK];
      for (int k = 0; k < i; ++k) s -= L[(ri + k) * LM_BLOCK] * y[k * LM_BLOCK];
      y[i * LM_BLOCK] = s / L[(ri + i) * LM_BLOCK];
    }
    for (int i = p - 1; i >= 0; --i) {
      T s = y[i * LM_BLOCK];
      for (int k = i + 1; k < p; ++k) s -= L[(k * (k + 1) / 2 + i) * LM_BLOCK] * y[k * LM_BLOCK];
      y[i * LM_BLOCK] = s / L[(i * (i + 1) / 2 + i) * LM_BLOCK];
    }
    for (int j = 0; j < p; ++j) {
      T v = th[j] + y[j * LM_BLOCK];
      if (a.proj_lo) v = t_max(v, a.proj_lo[j]);
      tt[j] = v;
    }
  } else {
    for (int j = 0; j < p; ++j) tt[j] = th[j];
  }
  for (int r = 0; r < D; ++r) {
    const long long row = row0 + r;
    const bool counted = a.ok_acc[row] != 0;
    for (int k = 0; k < K; ++k) {
      const long long w = row * K + k;
      const bool exists = !a.wp_weight || a.wp_weight[w] != T(0);
      T v = a.tau[w];
      if (solved && counted && exists) {
        const T dk = a.d_acc[w];
        const T Dk = dk + lam * (dk + ftau);
        if (Dk > T(0)) {
          const T* c = a.C_acc + w * p;
          T s = a.gtau_acc[w];
          for (int i = 0; i < p; ++i) s += c[i] * y[i * LM_BLOCK];
          v = v - s / Dk;
        }
      }
      a.tau_trial[w] = v;
    }
  }
  a.lambda[g] = lam;
}

}  // namespace lfsd
