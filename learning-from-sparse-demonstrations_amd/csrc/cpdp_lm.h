// Levenberg-Marquardt outer update from per-seed Gauss-Newton matrices (ABI 14).  The default loss is a sum of squares,
// loss = sum_k |y(tau_k) - wp_k|^2, and the forward sweep already returns dx/dtheta on the grid: its linear interpolant at the waypoint
// times, restricted to the interface components, is the Jacobian J of the residuals.  normal_matrix_kernel forms H = J^T J per
// trajectory; lm_step_kernel is the accept / reject state machine and the damped solve of every row in one launch.  The reference has
// first-order rules only (lib/QuadAlgorithm.py:454-578): this is new surface, nothing of it is consulted by the five rules.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).  Nothing of the model enters: any model
// library serves them.  Instantiated in the third translation unit only (lfsd_cubic.inc).  No atomics, fixed summation orders, 64-bit
// indices: a row's outputs are the same bits in any batch and at any position in it.
#pragma once
#include "cpdp_common.h"
#include "cpdp_sample.h"

namespace lfsd {

template <typename T> struct NormalMatrixArgs {
  int batch, n_grid, n_state, n_param, n_waypoints, n_iface;
  const int* iface_idx;   // [n_iface] state components of the interface
  const T* horizon;       // [B]
  const T* taus;          // [B][K]
  const T* auxX_grid;     // [B][n_grid+1][p][n]
  T* H;                   // [B][p][p]   (must not alias an input)
  const T* wp_weight;     // [B][K] or nullptr (ABI 16): H = sum_k w_k J_k^T J_k; a waypoint of weight 0 does not exist (its tau is not read)
};

// H[b][q1][q2] = sum_k sum_c X(tau_k)[q1][idx_c] X(tau_k)[q2][idx_c], X the linear interpolant of auxX_grid (interval rule of
// sample_interval and the fraction of grid_sample_kernel / waypoint_vjp_kernel, expression for expression).  One thread per (trajectory, q1, q2); the thread of the
// lower triangle (q2 <= q1) sums -- waypoints ascending, then interface components ascending -- and stores the element and its mirror
// image: both triangles hold the same bits.  The threads above the diagonal leave at once.  An interface index outside [0, n_state)
// is seen by every thread of the launch (the list is shared by the batch): nothing is written.  A few hundred bytes per trajectory:
// the launch is latency, not bandwidth.  Symmetry with weights: w x1 x2 is formed as (w x1) x2 by the one thread that stores both
// images, so which factor carries the weight cannot show.
template <typename T> __global__ void __launch_bounds__(256) normal_matrix_kernel(NormalMatrixArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = a.n_grid, n = a.n_state, p = a.n_param, K = a.n_waypoints, C = a.n_iface;
  const long long pp = (long long)p * p;
  if (e >= (long long)a.batch * pp) return;
  const long long traj = e / pp;
  const int r = (int)(e - traj * pp);
  const int q1 = r / p, q2 = r - q1 * p;
  if (q2 > q1) return;
  bool in_range = true;
  for (int c = 0; c < C; ++c) in_range = in_range && a.iface_idx[c] >= 0 && a.iface_idx[c] < n;
  if (!in_range) return;
  const T h = a.horizon[traj] / T(N);
  const T* X1 = a.auxX_grid + (traj * (long long)(N + 1) * p + q1) * n;
  const T* X2 = a.auxX_grid + (traj * (long long)(N + 1) * p + q2) * n;
  const long long node = (long long)p * n;
  T acc = T(0);
  // (weights: on ONE factor of each product, scaled once -- exact for w = 1 and for powers of two, so all-ones weights give the bits of
  //  the unweighted call; the thread of the lower triangle still stores both mirror images)
  const bool weighted = a.wp_weight != nullptr;
  for (int w = 0; w < K; ++w) {
    T wk = T(1);
    if (weighted) {
      wk = a.wp_weight[traj * K + w];
      if (wk == T(0)) continue;
    }
    const T tau = a.taus[traj * K + w];
    const int k = sample_interval(tau, h, N);
    const T s = (tau - T(k) * h) / h;
    const T* a1 = X1 + (long long)k * node;
    const T* a2 = X2 + (long long)k * node;
    for (int c = 0; c < C; ++c) {
      const int i = a.iface_idx[c];
      const T x1 = a1[i] + s * (a1[node + i] - a1[i]);
      const T x2 = a2[i] + s * (a2[node + i] - a2[i]);
      if (weighted) acc += (wk * x1) * x2;
      else acc += x1 * x2;
    }
  }
  a.H[traj * pp + (long long)q1 * p + q2] = acc;
  a.H[traj * pp + (long long)q2 * p + q1] = acc;
}

static constexpr int LM_MAX_PARAM = 16;      // p x p factorisation per lane: the triangle of 16 x 17 / 2 words in LDS
static constexpr int LM_RETRIES = 8;         // damping increases inside one launch
static constexpr int LM_BLOCK = 64;          // one wavefront: a row per lane

template <typename T> struct LmStepArgs {
  int batch, n_param;
  T lambda_down, lambda_up, lambda_min, lambda_max;
  T* theta;                // [B][p]     last accepted point
  T* loss_acc;             // [B]        loss there (+inf: nothing accepted yet)
  T* grad_acc;             // [B][p]
  T* H_acc;                // [B][p][p]
  T* lambda;               // [B]
  T* theta_trial;          // [B][p]     in: the point just evaluated; out: the next point to evaluate
  const T* loss_t;         // [B]        the evaluation at theta_trial
  const T* grad_t;         // [B][p]
  const T* H_t;            // [B][p][p]
  const T* proj_lo;        // [p] or nullptr
  const int* row_active;   // [B] or nullptr: rows with 0 keep every word of their state
  int* accepted;           // [B] or nullptr: 1 = the row accepted its trial point in this launch (0 for a row that is not active)
};

// One row per lane.  The Cholesky factor of A = H_acc + lambda (diag(H_acc) + 1e-8 max_j H_acc[j][j] I) lives in the lane's column of
// an LDS array laid out [element][lane] (consecutive lanes on consecutive banks, for 4- and 8-byte words alike); the lanes never read
// each other's column, so there is no barrier.  A row's own [p][p] records are read and written by its lane straight from global
// memory: lanes are p * p words apart, so these accesses are NOT coalesced (and H_acc is read again on every retry); they are not
// staged through LDS.  At most 2 KB per row and a handful of launches' worth of microseconds were expected, nothing was measured.  Control flow: the retry loop always makes LM_RETRIES + 1 trips, a row that
// is done skips the body; a bad pivot is remembered, not branched out of -- every loop's trip count is the same in every lane.
template <typename T> __global__ void __launch_bounds__(LM_BLOCK) lm_step_kernel(LmStepArgs<T> a) {
  __shared__ T Ls[LM_MAX_PARAM * (LM_MAX_PARAM + 1) / 2 * LM_BLOCK];
  __shared__ T ys[LM_MAX_PARAM * LM_BLOCK];
  const int lane = threadIdx.x;
  const long long b = (long long)blockIdx.x * blockDim.x + lane;
  const int p = a.n_param;
  if (b >= a.batch) return;
  if (a.row_active && !a.row_active[b]) {
    if (a.accepted) a.accepted[b] = 0;
    return;
  }
  T* th = a.theta + b * p;
  T* tt = a.theta_trial + b * p;
  T* ga = a.grad_acc + b * p;
  T* Ha = a.H_acc + b * p * p;
  const T* gt = a.grad_t + b * p;
  const T* Ht = a.H_t + b * p * p;
  T* L = Ls + lane;
  T* y = ys + lane;
  const T inf = T(__builtin_huge_val());
  // 1. accept or reject the trial point
  const T lt = a.loss_t[b];
  bool finite = t_finite(lt);
  for (int j = 0; j < p; ++j) finite = finite && t_finite(gt[j]);
  for (int j = 0; j < p * p; ++j) finite = finite && t_finite(Ht[j]);
  const bool accept = finite && lt < a.loss_acc[b];
  T lam = a.lambda[b];
  if (accept) {
    for (int j = 0; j < p; ++j) { th[j] = tt[j]; ga[j] = gt[j]; }
    for (int j = 0; j < p * p; ++j) Ha[j] = Ht[j];
    a.loss_acc[b] = lt;
    lam = t_max(lam * a.lambda_down, a.lambda_min);
  } else {
    lam = t_min(lam * a.lambda_up, a.lambda_max);
  }
  if (a.accepted) a.accepted[b] = accept ? 1 : 0;
  // 2. a row without an accepted point, or without any sensitivity, cannot move
  T hmax = Ha[0];
  for (int j = 1; j < p; ++j) hmax = t_max(hmax, Ha[(long long)j * p + j]);
  const bool can_move = a.loss_acc[b] != inf && hmax > T(0);
  const T floor_ = T(1e-8) * hmax;
  // 3.-5. damped normal equations, Cholesky without pivoting, more damping while a pivot is not positive
  bool need = can_move, solved = false;
  for (int attempt = 0; attempt <= LM_RETRIES; ++attempt) {
    if (need) {
      bool bad = false;
      for (int j = 0; j < p; ++j) {
        const int rj = j * (j + 1) / 2;
        const T hjj = Ha[(long long)j * p + j];
        T d = hjj + lam * (hjj + floor_);
        for (int k = 0; k < j; ++k) d -= L[(rj + k) * LM_BLOCK] * L[(rj + k) * LM_BLOCK];
        bad = bad || !(d > T(0)) || !t_finite(d);
        const T ljj = t_sqrt(d);
        L[(rj + j) * LM_BLOCK] = ljj;
        for (int i = j + 1; i < p; ++i) {
          const int ri = i * (i + 1) / 2;
          T s = Ha[(long long)i * p + j];
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
  // 6. A delta = -grad_acc by the two substitutions, the step and the projection -- or the row stays where it is
  if (solved) {
    for (int i = 0; i < p; ++i) {
      const int ri = i * (i + 1) / 2;
      T s = -ga[i];
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
  a.lambda[b] = lam;
}

}  // namespace lfsd
