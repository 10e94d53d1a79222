// Parameter update rules (lib/QuadAlgorithm.py:454-578).
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).
#pragma once
#include "cpdp_common.h"

namespace lfsd {

// =====================================================================================
//  Parameter update rules (lib/QuadAlgorithm.py:454-578), one thread per (trajectory, parameter)
// =====================================================================================
template <typename T> struct OptArgs {
  int batch, n_param, method, iter_idx;      // iter_idx starts from 0 (QuadAlgorithm.py:507)
  T lr, mu, beta1, beta2, eps;
  T* theta;            // [B][p]  in/out
  const T* grad;       // [B][p]
  T* m;                // [B][p]  Nesterov velocity / first moment
  T* v;                // [B][p]  second moment
  T* vhat;             // [B][p]  AMSGrad running max
  const T* proj_lo;    // [p] lower bound applied after the step (-inf = none); examples clamp theta[0] >= 1e-8
  const int* row_active;   // [B] or nullptr: rows with 0 keep theta AND their optimizer state (a frozen trajectory)
};

template <typename T> __global__ void optimizer_kernel(OptArgs<T> a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.batch * a.n_param) return;
  if (a.row_active && !a.row_active[i / a.n_param]) return;
  const int j = (int)(i % a.n_param);
  const T g = a.grad[i];
  T th = a.theta[i];
  const T idx = T(a.iter_idx + 1);
  if (a.method == OPT_VANILLA) {
    th -= a.lr * g;
  } else if (a.method == OPT_NESTEROV) {
    // grad was evaluated at the look-ahead point theta + mu*v (QuadAlgorithm.py:478-486)
    const T vel = a.mu * a.m[i] - a.lr * g;
    a.m[i] = vel;
    th += vel;
  } else {
    const T mm = a.beta1 * a.m[i] + (T(1) - a.beta1) * g;
    const T vv = a.beta2 * a.v[i] + (T(1) - a.beta2) * g * g;
    a.m[i] = mm; a.v[i] = vv;
    if (a.method == OPT_AMSGRAD) {
      const T vh = t_max(a.vhat[i], vv);
      a.vhat[i] = vh;
      th -= a.lr * mm / (t_sqrt(vh) + a.eps);
    } else {
      const T c1 = T(1) - t_pow(a.beta1, idx), c2 = T(1) - t_pow(a.beta2, idx);
      const T mh = mm / c1, vh = vv / c2;
      if (a.method == OPT_ADAM) th -= a.lr * mh / (t_sqrt(vh) + a.eps);
      else th -= a.lr * (a.beta1 * mh + (T(1) - a.beta1) / c1 * g) / (t_sqrt(vh) + a.eps);
    }
  }
  if (a.proj_lo) th = t_max(th, a.proj_lo[j]);
  a.theta[i] = th;
}

// look-ahead point of Nesterov: out = theta + mu * v   (QuadAlgorithm.py:478)
template <typename T> __global__ void lookahead_kernel(long long n, T mu, const T* theta, const T* v, T* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = theta[i] + mu * v[i];
}

// =====================================================================================
//  Hyper-parameter sweeps in one batch (ABI 13): every row its own update rule and hyper-parameters -- the comparison scripts of the
//  reference (test/opt_methods_comparison.py, test/*_learning_rate_comparison.py) as ONE batch -- and loss / gradient-norm /
//  parameter traces kept on the device (lib/QuadAlgorithm.py:244-252 reads them back every iteration).
//  Instantiated in the third translation unit only (lfsd_cubic.inc): the device code of the other two is untouched.
// =====================================================================================
static constexpr int OPT_HYPER = 5;      // lr, mu, beta1, beta2, eps

template <typename T> struct OptRowsArgs {
  int batch, n_param, iter_idx;
  const int* method;       // [B] OptMethod per row; a code outside 0..4 leaves the row untouched
  const T* hyper;          // [B][OPT_HYPER]
  T* theta;                // [B][p]  in/out
  const T* grad;           // [B][p]
  T* m;                    // [B][p]
  T* v;                    // [B][p]
  T* vhat;                 // [B][p]
  const T* proj_lo;        // [p] or nullptr
  const int* row_active;   // [B] or nullptr
};

// optimizer_kernel with the rule and the five hyper-parameters read per row.  The expressions are optimizer_kernel's, restated one
// for one (its text stays as it is so that its assembly does): a row's new theta / m / v / vhat are the bits the scalar launch
// gives with that row's values.
template <typename T> __global__ void optimizer_rows_kernel(OptRowsArgs<T> a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.batch * a.n_param) return;
  const long long b = i / a.n_param;
  if (a.row_active && !a.row_active[b]) return;
  const int method = a.method[b];
  if (method < OPT_VANILLA || method > OPT_AMSGRAD) return;
  const T* h = a.hyper + b * OPT_HYPER;
  const T lr = h[0], mu = h[1], beta1 = h[2], beta2 = h[3], eps = h[4];
  const int j = (int)(i % a.n_param);
  const T g = a.grad[i];
  T th = a.theta[i];
  const T idx = T(a.iter_idx + 1);
  if (method == OPT_VANILLA) {
    th -= lr * g;
  } else if (method == OPT_NESTEROV) {
    const T vel = mu * a.m[i] - lr * g;
    a.m[i] = vel;
    th += vel;
  } else {
    const T mm = beta1 * a.m[i] + (T(1) - beta1) * g;
    const T vv = beta2 * a.v[i] + (T(1) - beta2) * g * g;
    a.m[i] = mm; a.v[i] = vv;
    if (method == OPT_AMSGRAD) {
      const T vh = t_max(a.vhat[i], vv);
      a.vhat[i] = vh;
      th -= lr * mm / (t_sqrt(vh) + eps);
    } else {
      const T c1 = T(1) - t_pow(beta1, idx), c2 = T(1) - t_pow(beta2, idx);
      const T mh = mm / c1, vh = vv / c2;
      if (method == OPT_ADAM) th -= lr * mh / (t_sqrt(vh) + eps);
      else th -= lr * (beta1 * mh + (T(1) - beta1) / c1 * g) / (t_sqrt(vh) + eps);
    }
  }
  if (a.proj_lo) th = t_max(th, a.proj_lo[j]);
  a.theta[i] = th;
}

template <typename T> struct LookaheadRowsArgs {
  int batch, n_param;
  const int* method;       // [B]
  const T* hyper;          // [B][OPT_HYPER]
  const T* theta;          // [B][p]
  const T* m;              // [B][p]
  T* out;                  // [B][p]
};

// evaluation point of a mixed batch: theta + mu_b * m for a Nesterov row, theta itself -- its bits -- for every other row.  A select,
// not a product with zero: m of an Adam row is its first moment and may be Inf / NaN.
template <typename T> __global__ void lookahead_rows_kernel(LookaheadRowsArgs<T> a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.batch * a.n_param) return;
  const long long b = i / a.n_param;
  const T th = a.theta[i];
  T o = th;
  if (a.method[b] == OPT_NESTEROV) o = th + a.hyper[b * OPT_HYPER + 1] * a.m[i];
  a.out[i] = o;
}

template <typename T> struct TraceArgs {
  int batch, n_param, iter_idx, capacity;
  const T* loss;           // [B]
  const T* grad;           // [B][p]
  const T* theta;          // [B][p]  after the update and the projection
  const int* row_active;   // [B] or nullptr
  T* loss_trace;           // [B][capacity]       or nullptr
  T* gnorm_trace;          // [B][capacity]       or nullptr
  T* theta_trace;          // [B][capacity+1][p]  or nullptr (slot 0 is theta_0, the caller's)
};

// One thread per (row, parameter): theta_trace[b][iter_idx+1][j] = theta[b][j]; the thread of j = 0 also files the row's loss and
// ||grad||_2 (summed by that one thread, components ascending, in T: the same bits in any batch).  Nothing else is written.
template <typename T> __global__ void trace_append_kernel(TraceArgs<T> a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)a.batch * a.n_param) return;
  const long long b = i / a.n_param;
  if (a.row_active && !a.row_active[b]) return;
  const int j = (int)(i % a.n_param);
  if (a.theta_trace) a.theta_trace[(b * ((long long)a.capacity + 1) + a.iter_idx + 1) * a.n_param + j] = a.theta[i];
  if (j == 0) {
    if (a.loss_trace) a.loss_trace[b * a.capacity + a.iter_idx] = a.loss[b];
    if (a.gnorm_trace) {
      const T* g = a.grad + b * a.n_param;
      T s = T(0);
      for (int k = 0; k < a.n_param; ++k) s += g[k] * g[k];
      a.gnorm_trace[b * a.capacity + a.iter_idx] = t_sqrt(s);
    }
  }
}

}  // namespace lfsd
