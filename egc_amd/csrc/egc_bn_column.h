// The training-mode BatchNorm's per-column step and the last-block arrival protocol it rides on: ONE definition for the
// layer tail (egc_tail.hip) and the graph head (egc_head.hip).
//
// What is NOT here, on purpose: the column TOTALS of the partial moments.  Each kernel keeps its own summation order --
//   moment_totals (egc_tail.hip)                      64 lanes take the partials p, p + 64, .., then runs of eight lanes
//   the in-kernel FIN totals (column_moments_kernel)  eight runs of eight partials, then the eight run totals
//   hd_col_totals (egc_head.hip)                      8 lanes x 32 columns: lane j takes j, j + 8, .., then the eight lane sums
// -- documented in its file and in include/egc_hip.h, and part of that kernel's bit-level contract (the determinism and the
// graph-replay tests hold it).  They are not to be merged.
#pragma once
#include "egc_common.h"

namespace egc {

// A partial another block's arrive_last() will read: an agent-scope store (write-through: no cache write-back fence)
__device__ inline void store_partial(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The arrival counter: true in the block that arrives last (all other blocks' agent-scope stores are then visible to its
// loads), which also re-zeroes the counter.  *sync is zero on entry of the launch and zero again on its exit; every thread of
// every block calls it, once.  Why this is enough, with relaxed atomics only:
//   - a block's partials left through store_partial; vmcnt(0) holds each thread until the memory system has acknowledged its
//     stores at agent scope, and the barrier holds thread 0 until every thread of the block is past that wait -- so the
//     block's fetch_add is issued after all of its partials are visible device-wide (the wait and the barrier are the release);
//   - the counter is one agent-scope location: exactly one block reads n_blocks - 1, and by then every other block's
//     fetch_add, hence every other block's partials, have happened;
//   - the acquire fence drops what this CU (and its XCD's L2) may still hold of the partials' lines, so the last block's
//     plain loads after it fetch what the writers wrote;
//   - nobody else touches the counter after the last arrival, so the re-zeroing cannot race; the next launch on the
//     stream finds zero.
// No block waits for another: no grid barrier, no spin, no cooperative launch.
__device__ inline bool arrive_last(int* sync, int n_blocks) {
  __shared__ int last_block;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this block's partials have left
  __syncthreads();
  if (threadIdx.x == 0)
    last_block = __hip_atomic_fetch_add(sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n_blocks - 1;
  __syncthreads();
  if (!last_block) return false;
  if (threadIdx.x == 0) __hip_atomic_store(sync, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}

// Forward, one column, from its totals s1 = sum h, s2 = sum h^2 over n_rows rows: batch mean / biased variance (clamped at 0) /
// 1/std in float64 -> stats [3][cols]; the affine pair the elementwise pass applies -> affine [2][cols]; and the module's
// running statistics (nn.BatchNorm1d: unbiased variance; momentum, or -- momentum < 0 -- the cumulative average 1 / n_tracked,
// the count already incremented).
__device__ inline void bn_forward_column(double s1, double s2, int col, int cols, double n_rows, const float* gamma, const float* beta,
                                         double eps, double* stats, float* affine, float* running_mean, float* running_var,
                                         double momentum, double n_tracked) {
  const double mean = s1 / n_rows;
  double var = s2 / n_rows - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const double rstd = 1.0 / sqrt(var + eps);
  const double g = gamma != nullptr ? (double)gamma[col] : 1.0, b = beta != nullptr ? (double)beta[col] : 0.0;
  stats[col] = mean;
  stats[cols + col] = var;
  stats[2 * cols + col] = rstd;
  affine[col] = (float)(g * rstd);
  affine[cols + col] = (float)(b - mean * g * rstd);
  if (running_mean != nullptr) {
    const double m = momentum >= 0.0 ? momentum : 1.0 / n_tracked;
    running_mean[col] = (float)((1.0 - m) * (double)running_mean[col] + m * mean);
    running_var[col] = (float)((1.0 - m) * (double)running_var[col] + m * var * (n_rows > 1.0 ? n_rows / (n_rows - 1.0) : 1.0));
  }
}

// Backward, one column, from s1 = sum g, sgh = sum g h: outv [5][cols] = d gamma, d beta, c_g, c_h, c_1 of dh = c_g g + c_h h + c_1
__device__ inline void bn_backward_column(double s1, double sgh, int col, int cols, double n_rows, const double* stats,
                                          const float* gamma, float* outv, float* dh_sums) {
  const double mean = stats[col], rstd = stats[2 * cols + col];
  const double s2 = (sgh - mean * s1) * rstd;                 // sum g * h_hat
  const double a = (gamma != nullptr ? (double)gamma[col] : 1.0) * rstd;
  const float cg = (float)a, ch = (float)(-(a / n_rows) * rstd * s2), c1 = (float)(-(a / n_rows) * (s1 - mean * rstd * s2));
  outv[col] = (float)s2;                                      // d gamma
  outv[cols + col] = (float)s1;                               // d beta
  outv[2 * cols + col] = cg;                                  // dh = a g - (a / n) (s1 + (h - mean) rstd s2)
  outv[3 * cols + col] = ch;
  outv[4 * cols + col] = c1;
  // The column sum of the dh the elementwise pass will write (the gradient of a bias in front of the BatchNorm: zero but for
  // rounding -- autograd's value is the float sum of its own dh): sum_rows (cg g + ch h + c1) with the three coefficients AS
  // ROUNDED above, from the sums this step already holds (sum g = s1, sum h = n mean) -- no pass over dh.
  if (dh_sums != nullptr) dh_sums[col] = (float)((double)cg * s1 + (double)ch * (n_rows * mean) + n_rows * (double)c1);
}

}  // namespace egc
