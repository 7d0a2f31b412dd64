// Message aggregation of the baseline MPNN layer (reference experiments/layers.py:231-267) without its [E, 2 d] and [E, d] edge
// arrays.  A tower's message Linear acts on [x_i | x_j], so it splits into a target half and a source half: with
// P = x BD(Ws)^T and Q = x BD(Wd)^T + b (two dense [N, d] arrays, one product on the host side) the aggregated message of row i is
//
//   add   m_i = (sum over the row's entries of P[col]) + float(deg_i) * Q_i
//   mean  m_i = (that sum) / float(deg_i) + Q_i
//   max   m_i = (max over the row's entries of P[col]) + Q_i          per column; arg = the FIRST entry attaining the max
//
// and 0 (arg -1) for a row without entries.  gfx950 only.  Forward: one gather pass over P, the self term fused in, m stored
// into a column block of the caller's [m | x] operand.  Backward: d Q_i = s_i d m_i (s_i = deg_i / 1 / 1, 0 for an empty row) and
// d P_j = sum over j's entries of the TRANSPOSED CSR of d m_i (add), d m_i / float(deg_i) (mean), or d m_i[c] where arg[i, c]
// names that edge and 0 elsewhere (max: the transposed entry q is forward CSR position t_edge_id[q], edge edge_id[that]).
// Every output element is written exactly once: no zero fill, no atomics, nothing read back.
//
// Order rule and mapping: egc_row_chunks.h.  A chunk's sum is ((0 + v0) + v1) + ... in entry order, the row's sum is chunk 0's
// with the sums of chunks 1, 2, ... added in ascending order; then the division (mean), then the self term -- each one IEEE
// operation (-ffp-contract=off).  The max is exact in any order; its argument follows the same walk with a strict `>`, so the
// first entry wins a tie inside a chunk and the first chunk wins between chunks (a NaN is never selected).  The terms
// (GS_PLAIN forward; GS_PLAIN, GS_DIV_DEG, GS_MATCH backward), the sum's fold, chunk kernel and merge of the partials are
// egc_gather_sum.h's; this file holds the running max over the same terms, the finishes and the arg store.
#include "egc_gather_sum.h"

namespace egc {

// the batch's terms (stage 1 of egc_gather_sum.h) folded into the running max acc and its entry pos, in entry order
template <bool VEC, bool FULL>
__device__ inline void mp_max_batch(f4& acc, i4& pos, const GsWalk& W, int64_t p, int64_t p1, int c) {
  const GsTerms<FULL> t = gs_batch_terms<VEC, GS_PLAIN, FULL>(W, p, p1, c);
#pragma unroll
  for (int k = 0; k < GS_BATCH<FULL>; ++k) {
    const bool live = FULL || p + k < p1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool better = live && t.v[k][i] > acc[i];
      acc[i] = better ? t.v[k][i] : acc[i];
      pos[i] = better ? (int)(p + k) : pos[i];
    }
  }
}

// the running max of the entries [p0, p1), p0 < p1, from (-inf, p0) on; pos = the entry that holds it.  The walk is written
// out and not gs_for_batches: through that, mpnn_message_rows_kernel<VEC, MAX> takes 68 VGPRs for 64 (8 -> 7 waves per SIMD).
template <bool VEC>
__device__ inline void mp_max_entries(f4& acc, i4& pos, const GsWalk& W, int64_t p0, int64_t p1, int c) {
  const float start = -__builtin_inff();
  acc = f4{start, start, start, start};
  pos = i4{(int)p0, (int)p0, (int)p0, (int)p0};
  int64_t p = p0;
#pragma unroll 1
  for (; p + GS_AHEAD <= p1; p += GS_AHEAD) mp_max_batch<VEC, true>(acc, pos, W, p, p1, c);
  if (p < p1) mp_max_batch<VEC, false>(acc, pos, W, p, p1, c);
}

// workspace: [slots][lanes] f4 partial maxima, then [slots][lanes] i4 CSR positions of them
template <bool VEC>
__global__ void __launch_bounds__(256) mpnn_max_chunks_kernel(const GsWalk W, int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  f4 acc;
  i4 pos;
  mp_max_entries<VEC>(acc, pos, W, s0, s1, c);
  *reinterpret_cast<f4*>(ws + (g * W.lanes) * 4 + c) = acc;
  *reinterpret_cast<i4*>(ws + ((slots + g) * W.lanes) * 4 + c) = pos;
}

// a row's max: chunk 0 here, chunks 1, 2, ... from the workspace in ascending order
template <bool VEC>
__device__ inline void mp_max_row(f4& acc, i4& pos, const GsWalk& W, int64_t p0, int64_t p1, int c, int64_t slots,
                                  const float* __restrict__ ws) {
  mp_max_entries<VEC>(acc, pos, W, p0, min(p0 + ROW_CHUNK, p1), c);
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 4
  for (int64_t k = 0; k < n_part; ++k) {
    const f4 v = *reinterpret_cast<const f4*>(ws + ((first + k) * W.lanes) * 4 + c);
    const i4 q = *reinterpret_cast<const i4*>(ws + ((slots + first + k) * W.lanes) * 4 + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool better = v[i] > acc[i];
      acc[i] = better ? v[i] : acc[i];
      pos[i] = better ? q[i] : pos[i];
    }
  }
}

template <bool VEC, int OP>
__global__ void __launch_bounds__(256) mpnn_message_rows_kernel(const GsWalk W, const int32_t* __restrict__ edge_id,
                                                                const float* __restrict__ Q, int ld_q, float* __restrict__ out,
                                                                int ld_out, int32_t* __restrict__ arg, int64_t slots,
                                                                const float* __restrict__ ws) {
  constexpr bool MAX = OP == EGC_MPNN_MAX;
  int64_t row, p0, p1;
  int c;
  group_lane(W.lanes, row, c);
  if (row >= W.n_rows) return;
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 m = f4{0.f, 0.f, 0.f, 0.f};
  i4 e = i4{-1, -1, -1, -1};
  if (p1 > p0) {
    const f4 q = tm_load<VEC>(Q + row * ld_q + c, c, W.width);
    f4 acc;
    i4 pos;
    if (MAX) mp_max_row<VEC>(acc, pos, W, p0, p1, c, slots, ws);
    else acc = gs_sum_row<VEC, GS_PLAIN, false>(W, (int)row, p0, p1, c, ws);
    const float deg = (float)(p1 - p0);
    if (OP == EGC_MPNN_ADD) m = acc + deg * q;
    else if (OP == EGC_MPNN_MEAN) m = acc / deg + q;
    else m = acc + q;
    if (MAX && arg != nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = edge_id != nullptr ? edge_id[pos[i]] : pos[i];
    }
  }
  tm_store<VEC>(out + row * ld_out + c, c, W.width, m);
  if (MAX && arg != nullptr) tm_store_i<VEC>(arg + row * W.width + c, c, W.width, e);
}

// group g: d P of transposed row g (g < W.n_rows) and d Q of forward row g (g < W.n_in_rows; W.deg_rowptr is the forward rowptr)
template <bool VEC, int TERM>
__global__ void __launch_bounds__(256) mpnn_backward_rows_kernel(const GsWalk W, int op, float* __restrict__ dP, int ld_dp,
                                                                 float* __restrict__ dQ, int ld_dq,
                                                                 const float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(W.lanes, g, c);
  if (dP != nullptr && g < W.n_rows) {
    int64_t p0, p1;
    row_range(W.rowptr, W.n_edges, g, p0, p1);
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    if (p1 > p0) acc = gs_sum_row<VEC, TERM, false>(W, (int)g, p0, p1, c, ws);
    tm_store<VEC>(dP + g * ld_dp + c, c, W.width, acc);
  }
  if (dQ != nullptr && g < W.n_in_rows) {
    const int deg = max(W.deg_rowptr[g + 1] - W.deg_rowptr[g], 0);
    f4 d = f4{0.f, 0.f, 0.f, 0.f};
    if (deg > 0) {
      d = tm_load<VEC>(W.in + g * W.ld_in + c, c, W.width);
      if (op == EGC_MPNN_ADD) d = (float)deg * d;
    }
    tm_store<VEC>(dQ + g * ld_dq + c, c, W.width, d);
  }
}

// the two launches of the forward (slots == 0: the row launch alone)
template <int OP>
static int mp_forward(const GsWalk& W, bool vec, int64_t slots, float* ws, hipStream_t stream, const int32_t* edge_id,
                      const float* Q, int ld_q, float* out, int ld_out, int32_t* arg) {
  const int st = OP != EGC_MPNN_MAX ? gs_launch_chunks<GS_PLAIN, false>(W, vec, slots, ws, stream) : slots == 0 ? EGC_OK
                 : launch_lanes(vec, slots * W.lanes, stream, EGC_VEC_PAIR(mpnn_max_chunks_kernel), W, slots, ws);
  if (st != EGC_OK) return st;
  return launch_lanes(vec, W.n_rows * W.lanes, stream, EGC_VEC_PAIR(mpnn_message_rows_kernel, OP), W, edge_id, Q, ld_q, out,
                      ld_out, arg, slots, ws);
}

// the two launches of the backward over `groups` rows
template <int TERM>
static int mp_backward(const GsWalk& W, bool vec, int64_t groups, int64_t slots, float* ws, hipStream_t stream, int op, float* dP,
                       int ld_dp, float* dQ, int ld_dq) {
  const int st = gs_launch_chunks<TERM, false>(W, vec, slots, ws, stream);
  if (st != EGC_OK) return st;
  return launch_lanes(vec, groups * W.lanes, stream, EGC_VEC_PAIR(mpnn_backward_rows_kernel, TERM), W, op, dP, ld_dp, dQ, ld_dq,
                      ws);
}

}  // namespace egc

using namespace egc;

size_t egc_mpnn_message_workspace_bytes(int64_t n_edges, int32_t width, int32_t op) {
  return gs_workspace_bytes(chunk_slots(n_edges), width, op == EGC_MPNN_MAX ? 2 : 1);
}

size_t egc_mpnn_message_backward_workspace_bytes(int64_t n_edges, int32_t width) {
  return gs_workspace_bytes(chunk_slots(n_edges), width);
}

int egc_mpnn_message_f32(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, int64_t n_rows, int64_t n_edges,
                         int64_t n_src_rows, const float* P, int32_t ld_p, const float* Q, int32_t ld_q, int32_t width,
                         int32_t op, float* out, int32_t ld_out, int32_t* arg, void* workspace, size_t workspace_bytes,
                         egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (width <= 0 || n_rows < 0 || n_edges < 0 || n_src_rows < 0) return EGC_ERR_INVALID;
  if (op != EGC_MPNN_ADD && op != EGC_MPNN_MEAN && op != EGC_MPNN_MAX) return EGC_ERR_INVALID;
  if (ld_p < width || ld_q < width || ld_out < width) return EGC_ERR_INVALID;
  if (n_rows == 0) return EGC_OK;
  if (rowptr == nullptr || Q == nullptr || out == nullptr) return EGC_ERR_INVALID;
  if (n_edges > 0 && (col == nullptr || P == nullptr || n_src_rows == 0)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  GsWalk W = {};
  W.rowptr = rowptr, W.col = col, W.in = P;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows;
  W.ld_in = ld_p, W.width = width, W.lanes = (width + 3) / 4;
  const bool vec = all_mult4(width, ld_p, ld_q, ld_out) && all_aligned16(P, Q, out, arg);
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0 && !workspace_ok(ws, workspace_bytes, gs_workspace_bytes(slots, width, op == EGC_MPNN_MAX ? 2 : 1)))
    return EGC_ERR_WORKSPACE;
#define EGC_MPNN_FWD(O) mp_forward<O>(W, vec, slots, ws, stream, edge_id, Q, ld_q, out, ld_out, arg)
  return op == EGC_MPNN_ADD ? EGC_MPNN_FWD(EGC_MPNN_ADD) : op == EGC_MPNN_MEAN ? EGC_MPNN_FWD(EGC_MPNN_MEAN) : EGC_MPNN_FWD(EGC_MPNN_MAX);
#undef EGC_MPNN_FWD
}

int egc_mpnn_message_backward_f32(const int32_t* rowptr, const int32_t* edge_id, int64_t n_rows, const int32_t* t_rowptr,
                                  const int32_t* t_col, const int32_t* t_edge_id, int64_t n_src_rows, int64_t n_edges,
                                  const float* dm, int32_t ld_dm, const int32_t* arg, int32_t width, int32_t op, float* dP,
                                  int32_t ld_dp, float* dQ, int32_t ld_dq, void* workspace, size_t workspace_bytes,
                                  egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (width <= 0 || n_rows < 0 || n_edges < 0 || n_src_rows < 0) return EGC_ERR_INVALID;
  if (op != EGC_MPNN_ADD && op != EGC_MPNN_MEAN && op != EGC_MPNN_MAX) return EGC_ERR_INVALID;
  if (ld_dm < width || (dP != nullptr && ld_dp < width) || (dQ != nullptr && ld_dq < width)) return EGC_ERR_INVALID;
  const int64_t p_rows = dP != nullptr ? n_src_rows : 0, q_rows = dQ != nullptr ? n_rows : 0;
  const int64_t groups = p_rows > q_rows ? p_rows : q_rows;
  if (groups == 0) return EGC_OK;
  if (rowptr == nullptr || (n_rows > 0 && dm == nullptr)) return EGC_ERR_INVALID;
  if (dP != nullptr && (t_rowptr == nullptr || (n_edges > 0 && (t_col == nullptr || n_rows == 0)))) return EGC_ERR_INVALID;
  if (dP != nullptr && op == EGC_MPNN_MAX && n_edges > 0 && arg == nullptr) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  GsWalk W = {};
  W.rowptr = t_rowptr, W.col = t_col, W.eid = t_edge_id, W.deg_rowptr = rowptr, W.f_eid = edge_id, W.arg = arg, W.in = dm;
  W.n_rows = n_src_rows, W.n_edges = n_edges, W.n_in_rows = n_rows;
  W.ld_in = ld_dm, W.width = width, W.lanes = (width + 3) / 4;
  const bool vec = all_mult4(width, ld_dm, ld_dp, ld_dq) && all_aligned16(dm, dP, dQ, arg);
  const int64_t slots = dP != nullptr ? chunk_slots(n_edges) : 0;
  float* ws = static_cast<float*>(workspace);
  if (slots > 0 && !workspace_ok(ws, workspace_bytes, gs_workspace_bytes(slots, width))) return EGC_ERR_WORKSPACE;
#define EGC_MPNN_BWD(T) mp_backward<T>(W, vec, groups, slots, ws, stream, op, dP, ld_dp, dQ, ld_dq)
  return op == EGC_MPNN_ADD ? EGC_MPNN_BWD(GS_PLAIN) : op == EGC_MPNN_MEAN ? EGC_MPNN_BWD(GS_DIV_DEG) : EGC_MPNN_BWD(GS_MATCH);
#undef EGC_MPNN_BWD
}
