// The float32 gather-sum of egc_mpnn.hip, egc_nbr_sum.hip and egc_typed_mean.hip, written once: what a batch of a row's
// entries contributes (stage 1: the terms), how it is folded into the running sum (stage 2), the reduction of an entry range,
// the chunk kernel, the merge of a row's partials, the host side of the two launches.  The Mpnn max takes stage 1 and folds
// with its own running max; the typed mean makes its own terms and takes everything else.  Its term stays in its file: the relation, and with it the term, is chosen at run time inside one launch, an
// identity relation has no col, and its factor is 1.0f / float(deg) times the row (two roundings; GS_DIV_DEG divides once).
//
// Order rule and mapping: egc_row_chunks.h.  A batch is GS_AHEAD entries.  Its column indices, then the factor and id lookups
// at those (clamped) indices, then its rows, then (GS_MATCH) the arg rows are requested before the first operation that
// consumes one; the term's division, product or select is one IEEE operation (-ffp-contract=off); the fold is
// ((acc + t0) + t1) + ... in entry order, an entry past p1 or (SKIP) one that names its own row keeping its place and
// contributing nothing.
#pragma once
#include <type_traits>
#include "egc_row_chunks.h"

namespace egc {

constexpr int GS_AHEAD = 8;
// the entries a batch holds in registers: a partial batch has at most GS_AHEAD - 1
template <bool FULL>
constexpr int GS_BATCH = FULL ? GS_AHEAD : GS_AHEAD - 1;

// what an entry contributes: the row it names; that row over the named row's degree; that row times the entry's / the named
// row's scale; that row where arg names the entry's edge and 0 elsewhere
enum { GS_PLAIN = 0, GS_DIV_DEG = 1, GS_EDGE_SCALE = 2, GS_SRC_SCALE = 3, GS_MATCH = 4 };

// (a table that the term kind does not read costs kernarg bytes only)
struct GsWalk {
  const int32_t* rowptr;       // the CSR walked: n_rows + 1 offsets
  const int32_t* col;          // n_edges entries: rows of `in`
  const float* in;             // n_in_rows rows of ld_in floats
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_in, width, lanes;
  const int32_t* deg_rowptr;   // GS_DIV_DEG: n_in_rows + 1 offsets, the degree of a named row
  const float* src_scale;      // GS_SRC_SCALE: n_in_rows factors
  const float* edge_scale;     // GS_EDGE_SCALE: n_edges factors
  const int32_t* eid;          // GS_MATCH: forward CSR position of each entry (NULL: the entry's own position)
  const int32_t* f_eid;        // GS_MATCH: edge id of each forward CSR position (NULL: the position)
  const int32_t* arg;          // GS_MATCH: [n_in_rows, width] edge ids, dense
};

// the terms of a batch and the rows of the input they come from
template <bool FULL>
struct GsTerms {
  f4 v[GS_BATCH<FULL>];
  int j[GS_BATCH<FULL>];
};

// Stage 1.  The terms of the GS_BATCH<FULL> entries from p on (FULL: all of them exist; else those before p1, the others load
// entry p1 - 1 again and are not to be taken).  Worked out in local arrays and copied into the result at the end: filled in
// place the four GS_MATCH kernels take 8 - 16 VGPRs less and wait between their row loads (mpnn arxiv max backward 525 ->
// 552 us), and mpnn_message_rows_kernel<VEC, MAX> takes 68 VGPRs for 64 (8 -> 7 waves per SIMD).
template <bool VEC, int TERM, bool FULL>
__device__ inline GsTerms<FULL> gs_batch_terms(const GsWalk& W, int64_t p, int64_t p1, int c) {
  constexpr int N = GS_BATCH<FULL>;
  const int last_in = (int)W.n_in_rows - 1, last_e = (int)W.n_edges - 1;   // (both < 2^31: the entries are int32)
  f4 v[N];
  int j[N];
  batch_rows<N, FULL>(j, W.col, p, p1, last_in);
  float f[N];
  int e[N];
  if (TERM == GS_DIV_DEG || TERM == GS_EDGE_SCALE || TERM == GS_SRC_SCALE) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      f[k] = TERM == GS_DIV_DEG      ? (float)max(W.deg_rowptr[j[k] + 1] - W.deg_rowptr[j[k]], 1)
             : TERM == GS_EDGE_SCALE ? W.edge_scale[batch_entry<FULL>(p, k, p1)]
                                     : W.src_scale[j[k]];
  }
  if (TERM == GS_MATCH) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int64_t q = batch_entry<FULL>(p, k, p1);
      e[k] = W.eid != nullptr ? clamp_index(W.eid[q], last_e) : (int)q;
    }
  }
  if (TERM == GS_MATCH && W.f_eid != nullptr) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = W.f_eid[e[k]];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = tm_load<VEC>(W.in + (int64_t)j[k] * W.ld_in + c, c, W.width);
  if (TERM == GS_MATCH) {
    i4 a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = tm_load_i<VEC>(W.arg + (int64_t)j[k] * W.width + c, c, W.width);
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = a[k][i] == e[k] ? v[k][i] : 0.f;
  }
  if (TERM == GS_DIV_DEG || TERM == GS_EDGE_SCALE || TERM == GS_SRC_SCALE) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = TERM == GS_DIV_DEG ? v[k] / f[k] : f[k] * v[k];
  }
  GsTerms<FULL> t;
#pragma unroll
  for (int k = 0; k < N; ++k) t.v[k] = v[k], t.j[k] = j[k];
  return t;
}

// Stage 2.  The batch's terms added to acc in entry order.
template <bool SKIP, bool FULL>
__device__ inline void gs_fold_sum(f4& acc, const GsTerms<FULL>& t, int row, int64_t p, int64_t p1) {
#pragma unroll
  for (int k = 0; k < GS_BATCH<FULL>; ++k) {
    const bool live = (FULL || p + k < p1) && !(SKIP && t.j[k] == row);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = live ? acc[i] + t.v[k][i] : acc[i];
  }
}

// the entries [p0, p1) in order: take(p, FULL) for every full batch, then for the partial one
template <class Take>
__device__ inline void gs_for_batches(int64_t p0, int64_t p1, Take&& take) {
  int64_t p = p0;
#pragma unroll 1
  for (; p + GS_AHEAD <= p1; p += GS_AHEAD) take(p, std::true_type{});
  if (p < p1) take(p, std::false_type{});
}

// the entries [p0, p1) of row `row` in order: ((0 + t[p0]) + t[p0 + 1]) + ...
template <bool VEC, int TERM, bool SKIP>
__device__ inline f4 gs_sum_entries(const GsWalk& W, int row, int64_t p0, int64_t p1, int c) {
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  gs_for_batches(p0, p1, [&](int64_t p, auto full) {
    constexpr bool FULL = decltype(full)::value;
    gs_fold_sum<SKIP, FULL>(acc, gs_batch_terms<VEC, TERM, FULL>(W, p, p1, c), row, p, p1);
  });
  return acc;
}

// workspace: [slots][lanes] f4 chunk sums
template <bool VEC, int TERM, bool SKIP>
__global__ void __launch_bounds__(256) gather_sum_chunks_kernel(const GsWalk W, int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  *reinterpret_cast<f4*>(ws + (g * W.lanes) * 4 + c) = gs_sum_entries<VEC, TERM, SKIP>(W, (int)row, s0, s1, c);
}

// the sums of chunks 1, 2, ... of row [p0, p1) added to acc in ascending order (slot0: the first slot of the row's CSR in ws)
__device__ inline void gs_add_partials(f4& acc, const float* __restrict__ ws, int64_t slot0, int64_t p0, int64_t p1, int lanes,
                                       int c) {
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 4
  for (int64_t k = 0; k < n_part; ++k) acc += *reinterpret_cast<const f4*>(ws + ((slot0 + first + k) * lanes) * 4 + c);
}

// the sum of row `row` = [p0, p1), p0 < p1: chunk 0 here, then the partials
template <bool VEC, int TERM, bool SKIP>
__device__ inline f4 gs_sum_row(const GsWalk& W, int row, int64_t p0, int64_t p1, int c, const float* __restrict__ ws) {
  f4 acc = gs_sum_entries<VEC, TERM, SKIP>(W, row, p0, min(p0 + ROW_CHUNK, p1), c);
  gs_add_partials(acc, ws, 0, p0, p1, W.lanes, c);
  return acc;
}

// ------------------------------------------------------------------------------------------------------------------- host

// bytes of `slots` workspace slots of `fields` f4 (or i4) per lane
static inline size_t gs_workspace_bytes(int64_t slots, int32_t width, int fields = 1) {
  if (slots <= 0 || width <= 0) return 0;
  return (size_t)slots * (size_t)((width + 3) / 4) * 16 * fields;
}

// the kernel's name and its VEC and non-VEC instances (the template arguments after VEC follow the name)
#define EGC_VEC_PAIR(kernel, ...) #kernel, kernel<true, ##__VA_ARGS__>, kernel<false, ##__VA_ARGS__>

// one of the two instances over `items` lanes at 256 to a block
template <class... P, class... A>
static int launch_lanes(bool vec, int64_t items, hipStream_t stream, const char* name, void (*k_vec)(P...), void (*k_any)(P...),
                        A... args) {
  unsigned blocks;
  if (grid_blocks(items, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  void (*const kernel)(P...) = vec ? k_vec : k_any;
  kernel<<<blocks, 256, 0, stream>>>(args...);
  EGC_LAUNCH_CHECK(name);
  return EGC_OK;
}

// the chunk sums of a CSR of `slots` slots (none: no launch)
template <int TERM, bool SKIP>
static int gs_launch_chunks(const GsWalk& W, bool vec, int64_t slots, float* ws, hipStream_t stream) {
  if (slots == 0) return EGC_OK;
  return launch_lanes(vec, slots * W.lanes, stream, EGC_VEC_PAIR(gather_sum_chunks_kernel, TERM, SKIP), W, slots, ws);
}

}  // namespace egc
