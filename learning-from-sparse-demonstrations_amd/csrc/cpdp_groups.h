// Several demonstrations per seed (ABI 15): the deterministic per-group reduction of loss, gradient and Gauss-Newton matrix.  A batch of
// B = n_groups * group_size rows holds the demonstrations of a group next to each other (row g * D + d is demonstration d of group g);
// group_reduce_kernel sums them per group, so that the update kernels (cpdp_opt.h, cpdp_lm.h) run on n_groups rows unchanged.  J^T J of
// the stacked residuals of a group is the sum of the per-demonstration matrices of normal_matrix_kernel.  The reference learns from one
// demonstration per run (lib/QuadAlgorithm.py:239-257): this is new surface.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).  Nothing of the model enters: any model
// library serves it.  Instantiated in the third translation unit only (lfsd_cubic.inc).  No atomics, no LDS, no cross-lane operation,
// a fixed summation order, 64-bit indices: a group's outputs are the same bits in any batch and at any position in it (the property
// cpdp_lm.h states for its kernels).
#pragma once
#include "cpdp_common.h"

namespace lfsd {

template <typename T> struct GroupReduceArgs {
  int n_groups, group_size, n_param;
  const T* loss;        // [B]
  const T* grad;        // [B][p]
  const T* H;           // [B][p][p] or nullptr
  const int* row_ok;    // [B] or nullptr: rows with 0 are left out (their values are never read)
  T* loss_g;            // [G]
  T* grad_g;            // [G][p]
  T* H_g;               // [G][p][p] or nullptr (with H)
  int* n_ok;            // [G] rows counted
};

// One thread per (group, element); a group's elements -- its loss, the p components of its gradient, the p * p entries of H when H is
// given -- are on consecutive threads, so the reads of a row's gradient and of its H coalesce.  Every thread starts from T(0) and adds
// the values of the rows with row_ok != 0 one at a time, demonstrations ascending, in T: sums only, in one order, so H_g is as
// bit-symmetric as its inputs.  The loop always makes group_size trips; a masked row is skipped inside it (its value, possibly NaN, is
// not loaded).  The thread of the loss also files the number of rows counted.  A few hundred bytes per group: the launch is latency,
// not bandwidth (DESIGN.md section 15 has the figures).
template <typename T> __global__ void __launch_bounds__(256) group_reduce_kernel(GroupReduceArgs<T> a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = a.n_param, D = a.group_size;
  const long long pp = (long long)p * p;
  const long long per = 1 + p + (a.H ? pp : 0);
  if (e >= (long long)a.n_groups * per) return;
  const long long g = e / per, r = e - g * per;
  const long long row0 = g * D;
  const T* src;
  T* dst;
  long long stride;
  if (r == 0) {
    src = a.loss + row0; stride = 1; dst = a.loss_g + g;
  } else if (r <= p) {
    src = a.grad + row0 * p + (r - 1); stride = p; dst = a.grad_g + g * p + (r - 1);
  } else {
    src = a.H + row0 * pp + (r - 1 - p); stride = pp; dst = a.H_g + g * pp + (r - 1 - p);
  }
  T acc = T(0);
  int count = 0;
  for (int d = 0; d < D; ++d) {
    const bool ok = !a.row_ok || a.row_ok[row0 + d] != 0;
    if (ok) {
      acc += src[(long long)d * stride];
      ++count;
    }
  }
  *dst = acc;
  if (r == 0) a.n_ok[g] = count;
}

}  // namespace lfsd
