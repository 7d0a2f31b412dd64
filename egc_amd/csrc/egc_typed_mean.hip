// Typed mean aggregation of the relational baseline: the sparse part of the reference's RGCNConv,
// `adj_t.matmul(x_dict[src], reduce="mean")` per relation (rmag/models.py:66-70), and what autograd derives from it, as ONE
// kernel form run over a list of relations in one launch.  gfx950 only.
//
//   out[row, block(r)] (+)= post(row, r) * sum over p in rowptr_r[row] .. rowptr_r[row+1] of pre_r(col_r[p]) * in_r[col_r[p], :]
//
// Forward, one launch per TARGET type: in_r = x of the relation's source type, pre = 1, post = 1 / deg (the float32 sum divided
// by float(deg), 0 for a row without entries); every relation writes its own column block of one operand A_t.  Backward, one
// launch per SOURCE type over the transposed CSRs of the relations that leave it: in_r = the relation's column block of d A of
// its target type, pre(d) = 1 / float(deg(d)) from the forward graph's rowptr, post = 1, and the relations ADD into one d x in
// the order of the descriptor table.  A descriptor without a rowptr is the identity relation (row i has the one entry i): the
// forward copies x_t into block 0 of A_t with it, the backward starts d x_s from d A_s' block 0.  Every element of `out` is
// written exactly once: no zero fill, no atomics.
//
// Order rule and mapping: egc_row_chunks.h.  A chunk's sum is ((0 + v0) + v1) + ... in entry order, one IEEE add each
// (-ffp-contract=off), v = pre * in (one multiply) where there is a pre; the row's sum is the sum of chunk 0 with the sums of
// chunks 1, 2, ... added in ascending order; then post.  Every relation whose n_edges exceed one chunk has its own run of
// workspace slots (TypedTable::slot0).  The fold, the walk of an entry range, the merge of the partials and the launches are
// egc_gather_sum.h's, which says why the term is not.
#include "egc_gather_sum.h"

namespace egc {

struct TypedTable {
  egc_typed_rel rel[EGC_TYPED_MAX_RELATIONS];
  int64_t slot0[EGC_TYPED_MAX_RELATIONS + 1];   // first workspace slot of each relation; [n_rels] = all of them
  int32_t n_rels;
};

// the terms v = pre * in of the GS_BATCH<FULL> entries from p on and the rows j they name (stage 1 of egc_gather_sum.h)
template <bool VEC, bool FULL>
__device__ inline GsTerms<FULL> batch_terms(const egc_typed_rel& R, int64_t p, int64_t p1, int c, int width) {
  constexpr int N = GS_BATCH<FULL>;
  const int last_in = (int)R.n_in_rows - 1;   // (n_in_rows < 2^31: the entries are int32)
  f4 v[N];
  int j[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int64_t q = batch_entry<FULL>(p, k, p1);
    j[k] = clamp_index(R.col != nullptr ? R.col[q] : (int)q, last_in);
  }
  float s[N];
  if (R.pre_rowptr != nullptr) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 1.0f / (float)max(R.pre_rowptr[j[k] + 1] - R.pre_rowptr[j[k]], 1);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = tm_load<VEC>(R.in + (int64_t)j[k] * R.ld_in + c, c, width);
  if (R.pre_rowptr != nullptr) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] *= s[k];
  }
  GsTerms<FULL> t;
#pragma unroll
  for (int k = 0; k < N; ++k) t.v[k] = v[k], t.j[k] = j[k];
  return t;
}

// ((0 + v[p0]) + v[p0 + 1]) + ... over the entries [p0, p1)
template <bool VEC>
__device__ inline f4 sum_entries(const egc_typed_rel& R, int64_t p0, int64_t p1, int c, int width) {
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  gs_for_batches(p0, p1, [&](int64_t p, auto full) {
    constexpr bool FULL = decltype(full)::value;
    gs_fold_sum<false, FULL>(acc, batch_terms<VEC, FULL>(R, p, p1, c, width), 0, p, p1);
  });
  return acc;
}

// the entry range of a row: [row, row + 1) of the identity relation, the clamped rowptr pair otherwise
__device__ inline void row_range(const egc_typed_rel& R, int64_t row, int64_t& p0, int64_t& p1) {
  if (R.rowptr == nullptr) {
    p0 = row;
    p1 = row < R.n_in_rows ? row + 1 : row;
    return;
  }
  row_range(R.rowptr, R.n_edges, row, p0, p1);
}

template <bool VEC>
__global__ void __launch_bounds__(256) typed_mean_chunks_kernel(const TypedTable T, int64_t n_rows, int width, int lanes,
                                                                float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(lanes, g, c);
  if (g >= T.slot0[T.n_rels]) return;
  int r = 0;
  while (r + 1 < T.n_rels && g >= T.slot0[r + 1]) ++r;
  const egc_typed_rel& R = T.rel[r];
  int64_t row, s0, s1;
  if (!slot_chunk(R.rowptr, n_rows, R.n_edges, g - T.slot0[r], row, s0, s1)) return;
  const f4 acc = sum_entries<VEC>(R, s0, s1, c, width);
  *reinterpret_cast<f4*>(ws + (g * lanes) * 4 + c) = acc;
}

template <bool VEC, bool ACCUM>
__global__ void __launch_bounds__(256) typed_mean_rows_kernel(const TypedTable T, int64_t n_rows, int width, int lanes,
                                                              float* __restrict__ out, int ld_out,
                                                              const float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(lanes, g, c);
  if (g >= (ACCUM ? n_rows : n_rows * T.n_rels)) return;
  const int64_t row = ACCUM ? g : g / T.n_rels;
  const int r_begin = ACCUM ? 0 : (int)(g - row * T.n_rels), r_end = ACCUM ? T.n_rels : r_begin + 1;
  f4 total = f4{0.f, 0.f, 0.f, 0.f};
  int out_col = 0;
#pragma unroll 1
  for (int r = r_begin; r < r_end; ++r) {
    const egc_typed_rel& R = T.rel[r];
    int64_t p0, p1;
    row_range(R, row, p0, p1);
    f4 acc = sum_entries<VEC>(R, p0, min(p0 + ROW_CHUNK, p1), c, width);
    gs_add_partials(acc, ws, T.slot0[r], p0, p1, lanes, c);   // chunks 1, 2, ...: their sums wait in the workspace
    if (R.post_mean) {
      const float deg = (float)(p1 - p0);
      acc = p1 > p0 ? acc / deg : f4{0.f, 0.f, 0.f, 0.f};
    }
    if (ACCUM) total += acc;
    else total = acc, out_col = R.out_col;
  }
  tm_store<VEC>(out + row * ld_out + out_col + c, c, width, total);
}

static inline int64_t tm_slots(const egc_typed_rel& R) {
  return R.rowptr != nullptr ? chunk_slots(R.n_edges) : 0;
}

}  // namespace egc

using namespace egc;

int32_t egc_typed_mean_chunk(void) { return ROW_CHUNK; }

size_t egc_typed_mean_workspace_bytes(const egc_typed_rel* rels, int32_t n_rels, int32_t width) {
  if (rels == nullptr || n_rels <= 0 || n_rels > EGC_TYPED_MAX_RELATIONS || width <= 0) return 0;
  int64_t slots = 0;
  for (int r = 0; r < n_rels; ++r) slots += tm_slots(rels[r]);
  return gs_workspace_bytes(slots, width);
}

int egc_typed_mean_f32(const egc_typed_rel* rels, int32_t n_rels, int64_t n_rows, int32_t width, int32_t accumulate,
                       float* out, int32_t ld_out, void* workspace, size_t workspace_bytes, egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rels < 0 || n_rows < 0 || width <= 0 || (n_rels > 0 && rels == nullptr)) return EGC_ERR_INVALID;
  if (n_rels > EGC_TYPED_MAX_RELATIONS) return EGC_ERR_UNSUPPORTED;
  if (n_rows == 0 || (n_rels == 0 && !accumulate)) return EGC_OK;
  if (out == nullptr) return EGC_ERR_INVALID;
  const int lanes = (width + 3) / 4;
  TypedTable T;
  T.n_rels = n_rels;
  T.slot0[0] = 0;
  int64_t cols_end = accumulate ? width : 0;
  bool vec = all_mult4(width, ld_out) && all_aligned16(out);
  for (int r = 0; r < n_rels; ++r) {
    const egc_typed_rel& R = rels[r];
    if (R.n_edges < 0 || R.n_in_rows < 0 || R.ld_in < width || R.out_col < 0) return EGC_ERR_INVALID;
    if (R.rowptr != nullptr && R.n_edges > 0 && (R.col == nullptr || R.n_in_rows == 0)) return EGC_ERR_INVALID;
    if (R.in == nullptr && R.n_in_rows > 0) return EGC_ERR_INVALID;
    if (!counts_fit_int32(R.n_edges, R.n_in_rows)) return EGC_ERR_UNSUPPORTED;   // int32 rowptr / col
    T.rel[r] = R;
    if (R.rowptr == nullptr) T.rel[r].col = nullptr, T.rel[r].n_edges = 0;
    T.slot0[r + 1] = T.slot0[r] + tm_slots(R);
    if (!accumulate) cols_end = R.out_col + width > cols_end ? R.out_col + width : cols_end;
    vec = vec && (R.ld_in & 3) == 0 && aligned16(R.in) && (accumulate || (R.out_col & 3) == 0);
  }
  if (ld_out < cols_end) return EGC_ERR_INVALID;
  const int64_t slots = T.slot0[n_rels];
  float* ws = static_cast<float*>(workspace);
  if (slots > 0) {
    if (!workspace_ok(ws, workspace_bytes, gs_workspace_bytes(slots, width))) return EGC_ERR_WORKSPACE;
    const int st = launch_lanes(vec, slots * lanes, stream, EGC_VEC_PAIR(typed_mean_chunks_kernel), T, n_rows, width, lanes, ws);
    if (st != EGC_OK) return st;
  }
#define EGC_TYPED_ROWS(A, groups) \
  launch_lanes(vec, (groups) * lanes, stream, EGC_VEC_PAIR(typed_mean_rows_kernel, A), T, n_rows, width, lanes, out, ld_out, ws)
  return accumulate ? EGC_TYPED_ROWS(true, n_rows) : EGC_TYPED_ROWS(false, n_rows * n_rels);
#undef EGC_TYPED_ROWS
}
