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
// zero fill, no atomics, nothing read back.  The terms (GS_PLAIN, GS_DIV_DEG, GS_EDGE_SCALE, GS_SRC_SCALE), their fold, the
// chunk kernel and the merge of the partials are egc_gather_sum.h's; this file holds the finish and the forms compiled.
#include "egc_gather_sum.h"

namespace egc {

// how a row ends: agg (+ s * x_self); agg / deg (+ s * x_self); r * agg or r * (agg + r * x_self)
enum { NS_FIN_SUM = 0, NS_FIN_MEAN = 1, NS_FIN_SYM = 2 };

struct NsFinish {
  const float* x_self;      // n_rows rows of ld_self floats (SELF forms)
  const float* eps;         // device scalar: s = 1.f + *eps (NULL: s = self_scale)
  const float* row_scale;   // NS_FIN_SYM: n_rows factors
  float* out;               // n_rows rows of ld_out floats
  float self_scale;
  int32_t ld_self, ld_out;
};

// one group per row: chunk 0 here, chunks 1, 2, ... from the workspace in ascending order, the finish, the store
template <bool VEC, int TERM, bool SKIP, int FIN, bool SELF>
__global__ void __launch_bounds__(256) nbr_sum_rows_kernel(const GsWalk W, const NsFinish F, const float* __restrict__ ws) {
  int64_t row, p0, p1;
  int c;
  group_lane(W.lanes, row, c);
  if (row >= W.n_rows) return;
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 agg = f4{0.f, 0.f, 0.f, 0.f};
  if (p1 > p0) {
    agg = gs_sum_row<VEC, TERM, SKIP>(W, (int)row, p0, p1, c, ws);
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

template <int TERM, bool SKIP, int FIN, bool SELF>
static int ns_launch(const GsWalk& W, const NsFinish& F, bool vec, int64_t slots, float* ws, hipStream_t stream) {
  const int st = gs_launch_chunks<TERM, SKIP>(W, vec, slots, ws, stream);
  if (st != EGC_OK) return st;
  return launch_lanes(vec, W.n_rows * W.lanes, stream, EGC_VEC_PAIR(nbr_sum_rows_kernel, TERM, SKIP, FIN, SELF), W, F, ws);
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

size_t egc_nbr_sum_workspace_bytes(int64_t n_edges, int32_t width) { return gs_workspace_bytes(chunk_slots(n_edges), width); }

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
  GsWalk W = {};
  W.rowptr = rowptr, W.col = col, W.deg_rowptr = deg_rowptr, W.src_scale = src_scale, W.edge_scale = edge_scale, W.in = x;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows;
  W.ld_in = ld_x, W.width = width, W.lanes = (width + 3) / 4;
  NsFinish F = {};
  F.x_self = x_self, F.eps = eps, F.row_scale = row_scale, F.out = out;
  F.self_scale = self_scale, F.ld_self = ld_self, F.ld_out = ld_out;
  const bool vec = all_mult4(width, ld_x, ld_out, self ? ld_self : 0) && all_aligned16(x, x_self, out);
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0 && !workspace_ok(ws, workspace_bytes, gs_workspace_bytes(slots, width))) return EGC_ERR_WORKSPACE;
#define EGC_NBR(T, S, FI, X) return ns_launch<T, S, FI, X>(W, F, vec, slots, ws, stream)
  switch (form) {
    case EGC_NBR_SUM:
      if (skip) EGC_NBR(GS_PLAIN, true, NS_FIN_SUM, true);
      if (self) EGC_NBR(GS_PLAIN, false, NS_FIN_SUM, true);
      EGC_NBR(GS_PLAIN, false, NS_FIN_SUM, false);
    case EGC_NBR_MEAN:
      EGC_NBR(GS_PLAIN, false, NS_FIN_MEAN, false);
    case EGC_NBR_MEAN_T:
      if (self) EGC_NBR(GS_DIV_DEG, false, NS_FIN_SUM, true);
      EGC_NBR(GS_DIV_DEG, false, NS_FIN_SUM, false);
    default:   // EGC_NBR_SYM
      if (edge_scale != nullptr) {
        if (skip) EGC_NBR(GS_EDGE_SCALE, true, NS_FIN_SYM, true);
        EGC_NBR(GS_EDGE_SCALE, false, NS_FIN_SYM, false);
      }
      if (skip) EGC_NBR(GS_SRC_SCALE, true, NS_FIN_SYM, true);
      EGC_NBR(GS_SRC_SCALE, false, NS_FIN_SYM, false);
  }
#undef EGC_NBR
}
