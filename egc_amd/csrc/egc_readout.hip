// Graph-level readouts: sum / mean / max of the rows of x [n_rows, width] over consecutive row segments (the graphs of a
// PyG batch), forward and backward.  gfx950 only.  The reference ends every graph-level net with
// `x = self.pool(x, batch.batch)`, pool = global_mean_pool | global_add_pool | global_max_pool by `readout`
// (zinc/models.py:45-52,73; mol/pna_style_models.py:52-59,79; cifar/models.py:47-52,75; code/models.py:86-91).
//
// Order rule.  For every (segment, column) the float32 sum is ((0 + x[r0]) + x[r0+1]) + ..., rows ascending, one IEEE add
// each (-ffp-contract=off): the result is a pure function of the input -- no atomics, no tree, no dependence on how rows
// are spread over lanes (the rule of the tile kernels, tests/test_determinism_gpu.py).  Mean divides that sum by
// float(max(count, 1)).  Max takes the first row whatever it holds and then every row with x > current (strict), rows
// ascending: the FIRST row in input order wins a tie (oracle/egc_oracle.py:130); `arg` is that row's absolute index, -1
// for an empty segment.  NaN / Inf follow the strict compare and nothing else: a NaN in the segment's first row stays (no
// later value is greater than it), a NaN in a later row is never taken.  An empty segment gives 0 for every op.
//
// Mapping.  No lane ever needs another lane's data: a lane owns four adjacent columns of one segment and walks the
// segment's rows.  ceil(width / 4) lanes form the group of a segment; groups are laid over the threads of the grid back to
// back (two groups per wavefront at width 128; at 168 a group is 42 lanes and groups straddle wavefronts), so every lane of a block has
// work whatever the width.  Speed comes from many (segment, column) chains in flight and from requesting RD_AHEAD rows
// before the first add that consumes them -- not from reordering the sum.  x is read once: non-temporal 16-byte loads when
// width % 4 == 0 and the pointers are 16-byte aligned, scalar loads of the same four columns otherwise.
// One very long segment (a whole ogbn-arxiv graph as one "graph") is walked by ONE group: correct and slow.  Accepted;
// splitting it would need a second pass in a fixed order.
//
// Backward: same mapping over n_segments + 2 row ranges -- the segments, then the rows in front of the first and behind
// the last one, which receive 0 -- so every element of d_x is written exactly once by seg_ptr alone: no batch vector,
// no zero-fill launch, no atomics.  Row ranges are clamped to [0, n_rows] in both kernels: a seg_ptr that is not a
// partition of the rows gives garbage, never an access outside the arrays.
#include "egc_common.h"

namespace egc {

constexpr int RD_AHEAD = 8;   // rows requested before the first add that consumes them (8 x 16 bytes per lane in flight)

// one row into the running state of a lane's four columns, in input order (`live` false: the state stays as it is)
template <int OP>
__device__ inline void take_row(f4& acc, i4& win, f4 v, int64_t r, bool live = true) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (OP == EGC_READOUT_MAX) {
      const bool take = live && (win[j] < 0 || v[j] > acc[j]);
      acc[j] = take ? v[j] : acc[j];
      win[j] = take ? (int)r : win[j];
    } else {
      acc[j] = live ? acc[j] + v[j] : acc[j];
    }
  }
}

template <int OP, bool VEC>
__global__ void __launch_bounds__(256) segment_reduce_kernel(const float* __restrict__ x, const int64_t* __restrict__ seg_ptr,
                                                             int64_t n_segments, int64_t n_rows, int width, int lanes,
                                                             float* __restrict__ out, int32_t* __restrict__ arg) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t g = t / lanes;
  if (g >= n_segments) return;
  const int c = (int)(t - g * lanes) * 4;
  const int64_t r0 = min(max(seg_ptr[g], (int64_t)0), n_rows), r1 = min(max(seg_ptr[g + 1], r0), n_rows);
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  i4 win = i4{-1, -1, -1, -1};   // max: -1 = "nothing yet", the first row is then taken whatever it holds
  int64_t r = r0;
#pragma unroll 1
  for (; r + RD_AHEAD <= r1; r += RD_AHEAD) {   // (not unrolled further: typical segments are a few batches long)
    f4 v[RD_AHEAD];
#pragma unroll
    for (int k = 0; k < RD_AHEAD; ++k) v[k] = tm_load<VEC, true>(x + (r + k) * width + c, c, width);
#pragma unroll
    for (int k = 0; k < RD_AHEAD; ++k) take_row<OP>(acc, win, v[k], r + k);
  }
  if (r < r1) {   // the last, partial batch: every load issued (past the end: the last row again, not taken), no branch
    f4 v[RD_AHEAD - 1];
#pragma unroll
    for (int k = 0; k < RD_AHEAD - 1; ++k) v[k] = tm_load<VEC, true>(x + min(r + k, r1 - 1) * width + c, c, width);
#pragma unroll
    for (int k = 0; k < RD_AHEAD - 1; ++k) take_row<OP>(acc, win, v[k], r + k, r + k < r1);
  }
  if (OP == EGC_READOUT_MEAN) acc /= (float)(r1 > r0 ? r1 - r0 : 1);   // scatter-mean divides the sum by the count
  tm_store<VEC>(out + g * width + c, c, width, acc);
  if (OP == EGC_READOUT_MAX && arg != nullptr) tm_store_i<VEC>(arg + g * width + c, c, width, win);
}

template <int OP, bool VEC>
__global__ void __launch_bounds__(256) segment_reduce_backward_kernel(const float* __restrict__ d_out,
                                                                      const int64_t* __restrict__ seg_ptr,
                                                                      const int32_t* __restrict__ arg, int64_t n_segments,
                                                                      int64_t n_rows, int width, int lanes,
                                                                      float* __restrict__ d_x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t g = t / lanes;
  if (g >= n_segments + 2) return;
  const int c = (int)(t - g * lanes) * 4;
  int64_t r0, r1;
  f4 d = f4{0.f, 0.f, 0.f, 0.f};
  i4 win = i4{-1, -1, -1, -1};
  if (g < n_segments) {
    r0 = min(max(seg_ptr[g], (int64_t)0), n_rows), r1 = min(max(seg_ptr[g + 1], r0), n_rows);
    if (r0 < r1) {
      d = tm_load<VEC>(d_out + g * width + c, c, width);
      if (OP == EGC_READOUT_MAX) win = tm_load_i<VEC>(arg + g * width + c, c, width);
      if (OP == EGC_READOUT_MEAN) d /= (float)(r1 - r0);
    }
  } else if (g == n_segments) {   // rows in front of the first segment
    r0 = 0, r1 = min(max(seg_ptr[0], (int64_t)0), n_rows);
  } else {                        // rows behind the last segment
    r0 = min(max(seg_ptr[n_segments], (int64_t)0), n_rows), r1 = n_rows;
  }
#pragma unroll 4
  for (int64_t r = r0; r < r1; ++r) {
    f4 v = d;
    if (OP == EGC_READOUT_MAX) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = win[j] == (int)r ? d[j] : 0.f;
    }
    tm_store<VEC>(d_x + r * width + c, c, width, v);
  }
}

// threads of the grid: one group of ceil(width / 4) lanes per row range
static inline int64_t readout_blocks(int64_t n_ranges, int lanes) { return ceil_div(n_ranges * lanes, 256); }

int launch_segment_reduce(const float* x, const int64_t* seg_ptr, int64_t n_segments, int64_t n_rows, int32_t width,
                          int32_t op, float* out, int32_t* arg, hipStream_t stream) {
  const int lanes = (width + 3) / 4;
  const int64_t blocks = readout_blocks(n_segments, lanes);
  if (blocks >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  const bool vec = (width & 3) == 0 && aligned16(x) && aligned16(out) && aligned16(arg);
#define EGC_READOUT_FWD(OP)                                                                                               \
  do {                                                                                                                    \
    if (vec)                                                                                                              \
      segment_reduce_kernel<OP, true><<<(unsigned)blocks, 256, 0, stream>>>(x, seg_ptr, n_segments, n_rows, width, lanes, \
                                                                            out, arg);                                    \
    else                                                                                                                  \
      segment_reduce_kernel<OP, false><<<(unsigned)blocks, 256, 0, stream>>>(x, seg_ptr, n_segments, n_rows, width,      \
                                                                             lanes, out, arg);                            \
  } while (0)
  if (op == EGC_READOUT_SUM) EGC_READOUT_FWD(EGC_READOUT_SUM);
  else if (op == EGC_READOUT_MEAN) EGC_READOUT_FWD(EGC_READOUT_MEAN);
  else EGC_READOUT_FWD(EGC_READOUT_MAX);
#undef EGC_READOUT_FWD
  EGC_LAUNCH_CHECK("segment_reduce_kernel");
  return EGC_OK;
}

}  // namespace egc

using namespace egc;

static inline bool readout_op_ok(int32_t op) { return op == EGC_READOUT_SUM || op == EGC_READOUT_MEAN || op == EGC_READOUT_MAX; }

int egc_segment_reduce_f32(const float* x, const int64_t* seg_ptr, int64_t n_segments, int64_t n_rows, int32_t width,
                           int32_t op, float* out, int32_t* arg, egc_stream_t stream_) {
  if (!readout_op_ok(op) || n_segments < 0 || n_rows < 0 || width <= 0) return EGC_ERR_INVALID;
  if (op == EGC_READOUT_MAX && n_rows >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;   // arg is int32
  if (n_segments == 0) return EGC_OK;
  // x may be NULL when there are no rows (a zero-row tensor has no storage); the kernel then reads nothing
  if (seg_ptr == nullptr || out == nullptr || (x == nullptr && n_rows > 0)) return EGC_ERR_INVALID;
  return launch_segment_reduce(x, seg_ptr, n_segments, n_rows, width, op, out, op == EGC_READOUT_MAX ? arg : nullptr,
                               (hipStream_t)stream_);
}

int egc_segment_reduce_backward_f32(const float* d_out, const int64_t* seg_ptr, const int32_t* arg, int64_t n_segments,
                                    int64_t n_rows, int32_t width, int32_t op, float* d_x, egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!readout_op_ok(op) || n_segments < 0 || n_rows < 0 || width <= 0) return EGC_ERR_INVALID;
  if (op == EGC_READOUT_MAX && arg == nullptr) return EGC_ERR_INVALID;
  if (op == EGC_READOUT_MAX && n_rows >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  if (n_rows == 0) return EGC_OK;
  if (d_x == nullptr) return EGC_ERR_INVALID;
  if (n_segments == 0) {   // no segment owns a row (and seg_ptr may be NULL): every row is outside
    EGC_HIP_TRY(hipMemsetAsync(d_x, 0, (size_t)n_rows * width * sizeof(float), stream));
    return EGC_OK;
  }
  if (seg_ptr == nullptr || d_out == nullptr) return EGC_ERR_INVALID;
  const int lanes = (width + 3) / 4;
  const int64_t blocks = readout_blocks(n_segments + 2, lanes);
  if (blocks >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  const bool vec = (width & 3) == 0 && aligned16(d_out) && aligned16(d_x) && aligned16(arg);
#define EGC_READOUT_BWD(OP)                                                                                      \
  do {                                                                                                           \
    if (vec)                                                                                                     \
      segment_reduce_backward_kernel<OP, true><<<(unsigned)blocks, 256, 0, stream>>>(d_out, seg_ptr, arg, n_segments, \
                                                                                     n_rows, width, lanes, d_x); \
    else                                                                                                         \
      segment_reduce_backward_kernel<OP, false><<<(unsigned)blocks, 256, 0, stream>>>(d_out, seg_ptr, arg, n_segments, \
                                                                                      n_rows, width, lanes, d_x); \
  } while (0)
  if (op == EGC_READOUT_SUM) EGC_READOUT_BWD(EGC_READOUT_SUM);
  else if (op == EGC_READOUT_MEAN) EGC_READOUT_BWD(EGC_READOUT_MEAN);
  else EGC_READOUT_BWD(EGC_READOUT_MAX);
#undef EGC_READOUT_BWD
  EGC_LAUNCH_CHECK("segment_reduce_backward_kernel");
  return EGC_OK;
}
