// The chunked row walk of the gather kernels (egc_typed_mean.hip, egc_mpnn.hip, egc_gatv2.hip, egc_gat.hip, egc_pna.hip): its index
// arithmetic, written once.  What is loaded per entry and how it is folded is each kernel's own, except the float32 gather-sum
// of the first two and egc_nbr_sum.hip, which is egc_gather_sum.h's.
//
// Order rule.  A row's entries are cut into consecutive chunks of ROW_CHUNK entries, counted from the row's first entry.  A chunk
// is reduced from a fresh accumulator in entry order; the row's value is chunk 0's with the values of chunks 1, 2, ... merged in
// ascending order.  So the bits are a function of the CSR and the inputs alone, never of the launch geometry.  Two launches: the
// CHUNK kernel reduces chunks 1.. of the rows longer than one chunk into the workspace (one group of lanes per chunk: a hub row
// of 10^5 entries is spread over 400 groups), then the ROW kernel reduces every row's chunk 0, merges the row's partials in
// order, finishes and stores.  The chunk list is derived on the device: the group of workspace slot b looks at CSR position
// b * ROW_CHUNK, finds its row by bisection of rowptr, and owns the one chunk k >= 1 of that row that starts inside
// [b * ROW_CHUNK, (b + 1) * ROW_CHUNK) if there is one (chunks of a row are ROW_CHUNK apart, so there is at most one, and every
// chunk k >= 1 starts in exactly one such window of its own row).  Nothing is read back: the slot of a chunk is
// floor(start / ROW_CHUNK), and a CSR of more than ROW_CHUNK entries has ceil(n_edges / ROW_CHUNK) slots.  A chunk kernel
// stores to slot g with nothing but g < slots in front of it: chunk_slots, slot_chunk and row_partials are the workspace bound
// (tests/row_chunks runs them on the host).
//
// Mapping.  A lane owns four adjacent columns (16-byte accesses; 4-byte ones of the same columns when a width, stride or
// pointer is not a multiple of 16 bytes), `lanes` lanes form a group, one group per row (ROW kernel) or slot (CHUNK kernel),
// groups laid back to back over a grid of 256-thread blocks.  A batch of entries' column indices, then their rows, are
// requested before the first operation that consumes them; the last, partial batch issues all its loads too (position clamped
// to the last entry, surplus not taken: DESIGN.md section 3.9).  Column indices are clamped to the input's rows and row offsets
// to the entry count: malformed input gives garbage, never an access outside.
#pragma once
#include "egc_common.h"

namespace egc {

constexpr int ROW_CHUNK = EGC_TYPED_MEAN_CHUNK;

// min(max(v, lo), hi)
__host__ __device__ inline int64_t clamp_to(int64_t v, int64_t lo, int64_t hi) {
  const int64_t t = v > lo ? v : lo;
  return t < hi ? t : hi;
}

// the entry range [p0, p1) of a row, inside [0, n_edges] and never reversed whatever rowptr holds
__host__ __device__ inline void row_range(const int32_t* __restrict__ rowptr, int64_t n_edges, int64_t row, int64_t& p0,
                                          int64_t& p1) {
  p0 = clamp_to(rowptr[row], 0, n_edges);
  p1 = clamp_to(rowptr[row + 1], p0, n_edges);
}

// workspace slots of a CSR of n_edges entries
__host__ __device__ inline int64_t chunk_slots(int64_t n_edges) {
  return n_edges > ROW_CHUNK ? (n_edges + ROW_CHUNK - 1) / ROW_CHUNK : 0;
}

// the chunk k >= 1 of some row that starts in [slot * ROW_CHUNK, (slot + 1) * ROW_CHUNK): its row and range [s0, s1) (false:
// there is none, the outputs mean nothing).  The start is one selected value and not three early returns: with those,
// pna_chunks_kernel<VEC, SUM, no MOM2, EXT> takes 83 VGPRs for 75 and loses a wave per SIMD.
__host__ __device__ inline bool slot_chunk(const int32_t* __restrict__ rowptr, int64_t n_rows, int64_t n_edges, int64_t slot,
                                           int64_t& row, int64_t& s0, int64_t& s1) {
  const int64_t at = slot * ROW_CHUNK;
  int64_t lo = 0, hi = n_rows;   // the last row that starts at or before `at`
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr[mid] <= at) lo = mid;
    else hi = mid;
  }
  int64_t p0, p1;
  row_range(rowptr, n_edges, lo, p0, p1);
  int64_t s = -1;   // a short row; or chunk 0, which the row kernel takes
  if (p1 - p0 > ROW_CHUNK && at > p0) {
    s = p0 + (at - p0 + ROW_CHUNK - 1) / ROW_CHUNK * ROW_CHUNK;
    if (s >= p1) s = -1;
  }
  s0 = s;
  s1 = s + ROW_CHUNK < p1 ? s + ROW_CHUNK : p1;
  row = lo;
  return s >= 0;
}

// the slots that hold the partials of row [p0, p1): `first` and the n_part - 1 after it (chunks 1, 2, ... in this order)
__host__ __device__ inline void row_partials(int64_t p0, int64_t p1, int64_t& first, int64_t& n_part) {
  first = (p0 + ROW_CHUNK) / ROW_CHUNK;
  n_part = p1 - p0 > ROW_CHUNK ? (p1 - p0 - 1) / ROW_CHUNK : 0;
}

// this thread's group and the first of its four columns, for groups of `lanes` lanes
__device__ inline void group_lane(int lanes, int64_t& g, int& c) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  g = t / lanes;
  c = (int)(t - g * lanes) * 4;
}

// entry k of the batch that starts at p (FULL: it exists; else the entries from p1 on read entry p1 - 1 again)
template <bool FULL>
__device__ inline int64_t batch_entry(int64_t p, int k, int64_t p1) {
  return FULL ? p + k : min(p + k, p1 - 1);
}

__device__ inline int clamp_index(int j, int last) { return min(max(j, 0), last); }

// the rows of the input (0 .. last_in) that a batch of N entries from p on names
template <int N, bool FULL>
__device__ inline void batch_rows(int (&j)[N], const int32_t* __restrict__ col, int64_t p, int64_t p1, int last_in) {
#pragma unroll
  for (int k = 0; k < N; ++k) j[k] = clamp_index(col[batch_entry<FULL>(p, k, p1)], last_in);
}

// ------------------------------------------------------------------------------------------------------------------- host

// every count is below 2^31: rows, entries and source rows index int32 arrays, a block count is a 32-bit grid dimension
template <class... T>
static inline bool counts_fit_int32(T... n) {
  return ((n < ((int64_t)1 << 31)) && ...);
}

// blocks of a grid that holds `items` at `per_block` to a 256-thread block (lanes at 256, or groups at 256 / G)
static inline int grid_blocks(int64_t items, int64_t per_block, unsigned& blocks) {
  const int64_t n = ceil_div(items, per_block);
  if (!counts_fit_int32(n)) return EGC_ERR_UNSUPPORTED;
  blocks = (unsigned)n;
  return EGC_OK;
}

static inline bool workspace_ok(const void* workspace, size_t workspace_bytes, size_t needed) {
  return workspace != nullptr && aligned16(workspace) && workspace_bytes >= needed;
}

// the 16-byte access form: every width and stride a multiple of four floats, every pointer 16-byte aligned (NULL counts)
template <class... T>
static inline bool all_mult4(T... n) {
  return (((n & 3) == 0) && ...);
}
template <class... T>
static inline bool all_aligned16(T... p) {
  return (aligned16(p) && ...);
}

}  // namespace egc
