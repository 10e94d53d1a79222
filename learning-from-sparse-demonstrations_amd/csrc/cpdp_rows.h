// Per-seed stop rule of the learning loop (lib/QuadAlgorithm.py:239-257) and the row plumbing of a shrinking batch:
// the stop test + stable compaction of the active set as ONE kernel, and type-blind row gather / scatter.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).
//
// The reference learns every seed on its own and leaves its loop when `loss > 0.9 and ||dloss|| > 0.05` fails
// (QuadAlgorithm.py:242; Examples/robotarm_random.py:60-73 solve the seeds independently).  A batched learner that wants the same
// per seed keeps a list of the seeds still learning; the solver kernels then run on a DENSE batch of those (they have no row mask
// that frees a slot of a lock-step wavefront), which is what the gather / scatter kernels feed and drain.
#pragma once
#include "cpdp_common.h"

namespace lfsd {

// wave_rank(keep, total): number of lanes BELOW this one in its wavefront whose `keep` is set; `total` = number of all such
// lanes of the wavefront.  Must be reached by every lane of the workgroup.  One v_cmp into a 64-bit mask + two s_bcnt1 / v_mbcnt:
// no LDS, no barrier.  The emulator has LDS and __syncthreads() only.
#if defined(LFSD_EMU)
inline int wave_rank(bool keep, int& total) {
  static int sk[EMU_MAXT];
  const int t = threadIdx.x, w0 = t & ~63, lane = t & 63;
  sk[t] = keep ? 1 : 0;
  __syncthreads();
  int below = 0, all = 0;
  for (int l = 0; l < 64; ++l) {
    all += sk[w0 + l];
    if (l < lane) below += sk[w0 + l];
  }
  __syncthreads();
  total = all;
  return below;
}
#else
LFSD_DEV int wave_rank(bool keep, int& total) {
  const unsigned long long mask = __ballot(keep ? 1 : 0);
  const int lane = (int)(threadIdx.x & 63u);
  total = __popcll(mask);
  return __popcll(mask & ((1ull << lane) - 1ull));
}
#endif

// =====================================================================================
//  Stop test + compaction of the active set, one workgroup (a whole number of wavefronts, at most 16)
// =====================================================================================
template <typename T> struct StopArgs {
  int n_rows, n_param, iter_idx;
  T loss_tol, grad_tol;
  const T* loss;          // [n_rows]
  const T* grad;          // [n_rows][n_param]
  const int* rows_in;     // [n_rows] original row ids, ascending; nullptr = identity
  const int* eligible;    // [n_rows] or nullptr: 0 = kept whatever its loss / gradient (a row frozen for this step)
  int* rows_out;          // [<= n_rows] original ids of the survivors, in the order of rows_in (must not alias rows_in)
  int* pos_out;           // [<= n_rows] their positions in the input list
  int* n_out;             // [1]
  int* active;            // [full batch] set to 0 for a row that stops now
  int* stop_iter;         // [full batch] set to iter_idx + 1 for a row that stops now
};

// Row i continues while loss > loss_tol AND ||grad||_2 > grad_tol (QuadAlgorithm.py:242) -- both comparisons are false for a NaN,
// so a seed whose loss or gradient is not a number stops, as the reference's `if` does.  Survivors are written in ascending order
// of their position: rank inside the wavefront from the vote mask, the wavefronts' totals through LDS, a running base from chunk to
// chunk of blockDim.x rows.  Every step is a prefix sum in a fixed order: no atomics, the same output on every run.
template <typename T> __global__ void __launch_bounds__(1024) stop_compact_kernel(StopArgs<T> a) {
  __shared__ int wave_total[16];
  const int t = (int)threadIdx.x, nt = (int)blockDim.x, lane = t & 63, w = t >> 6, nw = nt >> 6;
  int base = 0;
  for (int c0 = 0; c0 < a.n_rows; c0 += nt) {      // (uniform trip count: every thread reaches the barriers of every chunk)
    const int i = c0 + t;
    const bool in = i < a.n_rows;
    bool keep = false;
    int orig = 0;
    if (in) {
      orig = a.rows_in ? a.rows_in[i] : i;
      if (a.eligible && a.eligible[i] == 0) {
        keep = true;
      } else {
        const T* g = a.grad + (long long)i * a.n_param;
        T s = T(0);
        for (int j = 0; j < a.n_param; ++j) s += g[j] * g[j];
        keep = (a.loss[i] > a.loss_tol) && (t_sqrt(s) > a.grad_tol);
      }
    }
    int total;
    const int rank = wave_rank(keep, total);
    if (lane == 0) wave_total[w] = total;
    __syncthreads();
    int off = base, all = 0;
    for (int k = 0; k < nw; ++k) {
      const int v = wave_total[k];
      if (k < w) off += v;
      all += v;
    }
    if (in) {
      if (keep) {
        a.rows_out[off + rank] = orig;
        a.pos_out[off + rank] = i;
      } else {
        a.active[orig] = 0;
        a.stop_iter[orig] = a.iter_idx + 1;
      }
    }
    base += all;
    __syncthreads();      // (wave_total is rewritten by the next chunk)
  }
  if (t == 0) *a.n_out = base;
}

// =====================================================================================
//  Row gather / scatter: dst[i][:] = src[index[i]][:]  /  dst[index[i]][:] = src[i][:], rows of row_words words of type W
// =====================================================================================
struct alignas(16) RowWord16 { unsigned x, y, z, w; };      // one global_load / global_store_dwordx4

struct RowCopyArgs {
  int n_rows;
  long long row_words;      // words of the instantiation's W per row
  const int* index;         // [n_rows]
  const void* src;
  void* dst;
};

// Grid-stride over the n_rows x row_words words of the DENSE side, consecutive lanes on consecutive words of a row (and on into the
// next row: the rows gathered here are short -- a parameter vector, a control grid).  (row, column) advance by the stride's own
// quotient and remainder: one division per thread, none in the loop.  Copies bits: no arithmetic type is involved.
template <typename W, bool SCATTER> LFSD_DEV void copy_rows(const RowCopyArgs& a) {
  const long long total = (long long)a.n_rows * a.row_words;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e0 >= total) return;
  const long long dr = stride / a.row_words, dc = stride % a.row_words;
  long long r = e0 / a.row_words, c = e0 % a.row_words;
  const W* src = (const W*)a.src;
  W* dst = (W*)a.dst;
  for (long long e = e0; e < total; e += stride) {
    const long long far = (long long)a.index[r] * a.row_words + c, near = r * a.row_words + c;
    if (SCATTER) dst[far] = src[near];
    else dst[near] = src[far];
    r += dr; c += dc;
    if (c >= a.row_words) { c -= a.row_words; r += 1; }
  }
}

template <typename W> __global__ void gather_rows_kernel(RowCopyArgs a) { copy_rows<W, false>(a); }
template <typename W> __global__ void scatter_rows_kernel(RowCopyArgs a) { copy_rows<W, true>(a); }

}  // namespace lfsd
