// The neighbour sum of GCNConv, SAGEConv and GINConv (PyG 2.x; the baselines of the reference's experiments/code/models.py): a
// row-scaled sum of source-scaled neighbour rows plus a multiple of the row's own features.  With agg_i the sum over row i's
// entries p of the per-entry term t_p:
//
//   EGC_NBR_SUM      t_p = x[col[p]]                                      out_i = agg_i + s * x_self_i
//   EGC_NBR_MEAN     t_p = x[col[p]]                                      out_i = agg_i / float(deg_i) + s * x_self_i
//   EGC_NBR_MEAN_T   t_p = x[col[p]] / float(max(deg_of(col[p]), 1))      out_i = agg_i + s * x_self_i
//   EGC_NBR_SYM      t_p = e_p * x[col[p]]                                out_i = row_scale[i] * (agg_i + row_scale[i] * x_self_i)
//
// (without x_self: agg, agg / float(deg_i), agg, row_scale[i] * agg).  s is self_scale, or 1.f + *eps read on the device;
// e_p is edge_scale[p] when that table is given and src_scale[col[p]] otherwise; deg_of comes from a second rowptr; an empty
// row has agg = 0 and is not divided.  With skip_self_entries an entry with col[p] == i is not taken: it keeps its place in
// the chunk layout and contributes nothing (the LOOPED edge set of include/egc_hip.h, the self term standing for the one
// self loop).  The transpose of each form is one of the forms on the transposed CSR (SUM -> SUM, MEAN -> MEAN_T, SYM -> SYM
// with the same tables), so the backward is this file again.  gfx950 only.
//
// Order rule and mapping: egc_row_chunks.h.  A chunk's sum is ((0 + t0) + t1) + ... in entry order, the row's sum is chunk 0's
// with the sums of chunks 1, 2, ... added in ascending order; the term's product or division, then the finish's division,
// products and additions are one IEEE operation each (-ffp-contract=off).  Every element named is written exactly once: no
// zero fill, no atomics, nothing read back.  A batch is NS_AHEAD entries; the scale and degree lookups of a batch are
// requested with its rows, at clamped indices.
#include "egc_row_chunks.h"

namespace egc {

constexpr int NS_AHEAD = 8;

// what an entry contributes: the row it names; that row over the named row's degree; that row times the entry's / the named row's scale
enum { NS_PLAIN = 0, NS_DIV_DEG = 1, NS_EDGE_SCALE = 2, NS_SRC_SCALE = 3 };
// how a row ends: agg (+ s * x_self); agg / deg (+ s * x_self); r * agg or r * (agg + r * x_self)
enum { NS_FIN_SUM = 0, NS_FIN_MEAN = 1, NS_FIN_SYM = 2 };

struct NsWalk {
  const int32_t* rowptr;       // the CSR walked: n_rows + 1 offsets
  const int32_t* col;          // n_edges entries: rows of `in`
  const int32_t* deg_rowptr;   // NS_DIV_DEG: n_in_rows + 1 offsets
  const float* src_scale;      // NS_SRC_SCALE: n_in_rows factors
  const float* edge_scale;     // NS_EDGE_SCALE: n_edges factors
  const float* in;             // n_in_rows rows of ld_in floats
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_in, width, lanes;
};

struct NsFinish {
  const float* x_self;      // n_rows rows of ld_self floats (SELF forms)
  const float* eps;         // device scalar: s = 1.f + *eps (NULL: s = self_scale)
  const float* row_scale;   // NS_FIN_SYM: n_rows factors
  float* out;               // n_rows rows of ld_out floats
  float self_scale;
  int32_t ld_self, ld_out;
};

// NS_AHEAD consecutive entries of row `row` from p on (FULL: all of them exist; else those before p1, the others load entry
// p1 - 1 again and are not taken) folded into acc in entry order
template <bool VEC, int TERM, bool SKIP, bool FULL>
__device__ inline void ns_take_batch(f4& acc, const NsWalk& W, int row, int64_t p, int64_t p1, int c) {
  constexpr int N = FULL ? NS_AHEAD : NS_AHEAD - 1;
  const int last_in = (int)W.n_in_rows - 1;   // (< 2^31: the entries are int32)
  int j[N];
  batch_rows<N, FULL>(j, W.col, p, p1, last_in);
  float e[N];
  if (TERM == NS_DIV_DEG) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = (float)max(W.deg_rowptr[j[k] + 1] - W.deg_rowptr[j[k]], 1);
  }
  if (TERM == NS_EDGE_SCALE) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = W.edge_scale[batch_entry<FULL>(p, k, p1)];
  }
  if (TERM == NS_SRC_SCALE) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = W.src_scale[j[k]];
  }
  f4 v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = tm_load<VEC>(W.in + (int64_t)j[k] * W.ld_in + c, c, W.width);
  if (TERM == NS_DIV_DEG) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] /= e[k];
  }
  if (TERM == NS_EDGE_SCALE || TERM == NS_SRC_SCALE) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = e[k] * v[k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const bool live = (FULL || p + k < p1) && !(SKIP && j[k] == row);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = live ? acc[i] + v[k][i] : acc[i];
  }
}

// the entries [p0, p1), p0 < p1, of row `row` in order: ((0 + t[p0]) + t[p0 + 1]) + ...
template <bool VEC, int TERM, bool SKIP>
__device__ inline f4 ns_reduce_entries(const NsWalk& W, int row, int64_t p0, int64_t p1, int c) {
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  int64_t p = p0;
#pragma unroll 1
  for (; p + NS_AHEAD <= p1; p += NS_AHEAD) ns_take_batch<VEC, TERM, SKIP, true>(acc, W, row, p, p1, c);
  if (p < p1) ns_take_batch<VEC, TERM, SKIP, false>(acc, W, row, p, p1, c);
  return acc;
}

// workspace: [slots][lanes] f4 chunk sums
template <bool VEC, int TERM, bool SKIP>
__global__ void __launch_bounds__(256) nbr_sum_chunks_kernel(const NsWalk W, int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  *reinterpret_cast<f4*>(ws + (g * W.lanes) * 4 + c) = ns_reduce_entries<VEC, TERM, SKIP>(W, (int)row, s0, s1, c);
}

// one group per row: chunk 0 here, chunks 1, 2, ... from the workspace in ascending order, the finish, the store
template <bool VEC, int TERM, bool SKIP, int FIN, bool SELF>
__global__ void __launch_bounds__(256) nbr_sum_rows_kernel(const NsWalk W, const NsFinish F, const float* __restrict__ ws) {
  int64_t row, p0, p1;
  int c;
  group_lane(W.lanes, row, c);
  if (row >= W.n_rows) return;
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 agg = f4{0.f, 0.f, 0.f, 0.f};
  if (p1 > p0) {
    agg = ns_reduce_entries<VEC, TERM, SKIP>(W, (int)row, p0, min(p0 + ROW_CHUNK, p1), c);
    int64_t first, n_part;
    row_partials(p0, p1, first, n_part);
#pragma unroll 4
    for (int64_t k = 0; k < n_part; ++k) agg += *reinterpret_cast<const f4*>(ws + ((first + k) * W.lanes) * 4 + c);
    if (FIN == NS_FIN_MEAN) agg = agg / (float)(p1 - p0);
  }
  if (FIN == NS_FIN_SYM) {
    const float r = F.row_scale[row];
    if (SELF) agg = agg + r * tm_load<VEC>(F.x_self + row * F.ld_self + c, c, W.width);
    agg = r * agg;
  } else if (SELF) {
    const float s = F.eps != nullptr ? 1.f + *F.eps : F.self_scale;
    agg = agg + s * tm_load<VEC>(F.x_self + row * F.ld_self + c, c, W.width);
  }
  tm_store<VEC>(F.out + row * F.ld_out + c, c, W.width, agg);
}

static inline size_t ns_workspace_bytes(int64_t n_edges, int32_t width) {
  if (n_edges <= 0 || width <= 0) return 0;
  return (size_t)chunk_slots(n_edges) * (size_t)((width + 3) / 4) * 16;
}

template <int TERM, bool SKIP, int FIN, bool SELF>
static int ns_launch(const NsWalk& W, const NsFinish& F, bool vec, int64_t slots, float* ws, hipStream_t stream) {
  unsigned blocks;
  if (slots > 0) {
    if (grid_blocks(slots * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
    if (vec) nbr_sum_chunks_kernel<true, TERM, SKIP><<<blocks, 256, 0, stream>>>(W, slots, ws);
    else nbr_sum_chunks_kernel<false, TERM, SKIP><<<blocks, 256, 0, stream>>>(W, slots, ws);
    EGC_LAUNCH_CHECK("nbr_sum_chunks_kernel");
  }
  if (grid_blocks(W.n_rows * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  if (vec) nbr_sum_rows_kernel<true, TERM, SKIP, FIN, SELF><<<blocks, 256, 0, stream>>>(W, F, ws);
  else nbr_sum_rows_kernel<false, TERM, SKIP, FIN, SELF><<<blocks, 256, 0, stream>>>(W, F, ws);
  EGC_LAUNCH_CHECK("nbr_sum_rows_kernel");
  return EGC_OK;
}

// The forms compiled: what GCNConv, SAGEConv and GINConv launch, forward and backward.
//   SUM      plain (GCN without either flag, SAGE sum, both directions); skip + self (GCN normalize=False, both directions);
//            self (GIN, both directions; the backward of SAGE sum's [agg | x] operand)
//   MEAN     plain (SAGE mean forward)
//   MEAN_T   plain (SAGE mean backward, root_weight=False); self (SAGE mean backward of the [agg | x] operand)
//   SYM      skip + self, plain (GCN with / without add_self_loops), each with the per-entry table or the gather
static bool ns_compiled(int form, bool skip, bool self) {
  switch (form) {
    case EGC_NBR_SUM: return !skip || self;
    case EGC_NBR_MEAN: return !skip && !self;
    case EGC_NBR_MEAN_T: return !skip;
    case EGC_NBR_SYM: return skip == self;
  }
  return false;
}

}  // namespace egc

using namespace egc;

size_t egc_nbr_sum_workspace_bytes(int64_t n_edges, int32_t width) { return ns_workspace_bytes(n_edges, width); }

int egc_nbr_sum_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows, const float* x,
                    int32_t ld_x, const float* x_self, int32_t ld_self, int32_t width, int32_t form, int32_t skip_self_entries,
                    float self_scale, const float* eps, const int32_t* deg_rowptr, const float* row_scale, const float* src_scale,
                    const float* edge_scale, float* out, int32_t ld_out, void* workspace, size_t workspace_bytes,
                    egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (width <= 0 || n_rows < 0 || n_edges < 0 || n_src_rows < 0) return EGC_ERR_INVALID;
  if (form != EGC_NBR_SUM && form != EGC_NBR_MEAN && form != EGC_NBR_MEAN_T && form != EGC_NBR_SYM) return EGC_ERR_INVALID;
  if (ld_x < width || ld_out < width || (x_self != nullptr && ld_self < width)) return EGC_ERR_INVALID;
  if (form == EGC_NBR_SYM && (row_scale == nullptr || (edge_scale == nullptr && src_scale == nullptr))) return EGC_ERR_INVALID;
  if (form == EGC_NBR_MEAN_T && deg_rowptr == nullptr) return EGC_ERR_INVALID;
  const bool skip = skip_self_entries != 0, self = x_self != nullptr;
  if (!ns_compiled(form, skip, self)) return EGC_ERR_UNSUPPORTED;
  if (n_rows == 0) return EGC_OK;
  if (rowptr == nullptr || out == nullptr) return EGC_ERR_INVALID;
  if (n_edges > 0 && (col == nullptr || x == nullptr || n_src_rows == 0)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  NsWalk W = {};
  W.rowptr = rowptr, W.col = col, W.deg_rowptr = deg_rowptr, W.src_scale = src_scale, W.edge_scale = edge_scale, W.in = x;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows;
  W.ld_in = ld_x, W.width = width, W.lanes = (width + 3) / 4;
  NsFinish F = {};
  F.x_self = x_self, F.eps = eps, F.row_scale = row_scale, F.out = out;
  F.self_scale = self_scale, F.ld_self = ld_self, F.ld_out = ld_out;
  const bool vec = all_mult4(width, ld_x, ld_out, self ? ld_self : 0) && all_aligned16(x, x_self, out);
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0 && !workspace_ok(ws, workspace_bytes, ns_workspace_bytes(n_edges, width))) return EGC_ERR_WORKSPACE;
#define EGC_NBR(T, S, FI, X) return ns_launch<T, S, FI, X>(W, F, vec, slots, ws, stream)
  switch (form) {
    case EGC_NBR_SUM:
      if (skip) EGC_NBR(NS_PLAIN, true, NS_FIN_SUM, true);
      if (self) EGC_NBR(NS_PLAIN, false, NS_FIN_SUM, true);
      EGC_NBR(NS_PLAIN, false, NS_FIN_SUM, false);
    case EGC_NBR_MEAN:
      EGC_NBR(NS_PLAIN, false, NS_FIN_MEAN, false);
    case EGC_NBR_MEAN_T:
      if (self) EGC_NBR(NS_DIV_DEG, false, NS_FIN_SUM, true);
      EGC_NBR(NS_DIV_DEG, false, NS_FIN_SUM, false);
    default:   // EGC_NBR_SYM
      if (edge_scale != nullptr) {
        if (skip) EGC_NBR(NS_EDGE_SCALE, true, NS_FIN_SYM, true);
        EGC_NBR(NS_EDGE_SCALE, false, NS_FIN_SYM, false);
      }
      if (skip) EGC_NBR(NS_SRC_SCALE, true, NS_FIN_SYM, true);
      EGC_NBR(NS_SRC_SCALE, false, NS_FIN_SYM, false);
  }
#undef EGC_NBR
}
