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
// first entry wins a tie inside a chunk and the first chunk wins between chunks (a NaN is never selected).  A batch is MP_AHEAD
// entries; edge positions are clamped to the entry count like row offsets.
#include "egc_row_chunks.h"

namespace egc {

constexpr int MP_AHEAD = 8;

// what an entry contributes: the row it names; that row over the named row's forward degree; that row where arg names the edge
enum { MP_PLAIN = 0, MP_DIV_DEG = 1, MP_MATCH = 2 };

struct MpWalk {
  const int32_t* rowptr;     // the CSR walked: n_rows + 1 offsets
  const int32_t* col;        // n_edges entries: rows of `in`
  const int32_t* eid;        // MP_MATCH: forward CSR position of each entry (NULL: the entry's own position)
  const int32_t* f_rowptr;   // MP_DIV_DEG: forward rowptr, n_in_rows + 1 offsets
  const int32_t* f_eid;      // MP_MATCH: edge id of each forward CSR position (NULL: the position)
  const int32_t* arg;        // MP_MATCH: [n_in_rows, width] edge ids, dense
  const float* in;           // n_in_rows rows of ld_in floats
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_in, width, lanes;
};

// MP_AHEAD consecutive entries from p on (FULL: all of them exist; else those before p1, the others load entry p1 - 1 again
// and are not taken) folded into acc (and pos: the entry of the running max) in entry order
template <bool VEC, bool MAX, int KIND, bool FULL>
__device__ inline void mp_take_batch(f4& acc, i4& pos, const MpWalk& W, int64_t p, int64_t p1, int c) {
  constexpr int N = FULL ? MP_AHEAD : MP_AHEAD - 1;
  const int last_in = (int)W.n_in_rows - 1, last_e = (int)W.n_edges - 1;   // (both < 2^31: the entries are int32)
  int j[N], e[N];
  batch_rows<N, FULL>(j, W.col, p, p1, last_in);
  if (KIND == MP_MATCH) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int64_t q = batch_entry<FULL>(p, k, p1);
      e[k] = W.eid != nullptr ? clamp_index(W.eid[q], last_e) : (int)q;
    }
  }
  if (KIND == MP_MATCH && W.f_eid != nullptr) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = W.f_eid[e[k]];
  }
  float deg[N];
  if (KIND == MP_DIV_DEG) {
#pragma unroll
    for (int k = 0; k < N; ++k) deg[k] = (float)max(W.f_rowptr[j[k] + 1] - W.f_rowptr[j[k]], 1);
  }
  f4 v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = tm_load<VEC>(W.in + (int64_t)j[k] * W.ld_in + c, c, W.width);
  if (KIND == MP_MATCH) {
    i4 a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = tm_load_i<VEC>(W.arg + (int64_t)j[k] * W.width + c, c, W.width);
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = a[k][i] == e[k] ? v[k][i] : 0.f;
  }
  if (KIND == MP_DIV_DEG) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] /= deg[k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const bool live = FULL || p + k < p1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (MAX) {
        const bool better = live && v[k][i] > acc[i];
        acc[i] = better ? v[k][i] : acc[i];
        pos[i] = better ? (int)(p + k) : pos[i];
      } else {
        acc[i] = live ? acc[i] + v[k][i] : acc[i];
      }
    }
  }
}

// the entries [p0, p1), p0 < p1, in order: ((0 + v[p0]) + v[p0 + 1]) + ..., or the running max from (-inf, p0) on
template <bool VEC, bool MAX, int KIND>
__device__ inline void mp_reduce_entries(f4& acc, i4& pos, const MpWalk& W, int64_t p0, int64_t p1, int c) {
  const float start = MAX ? -__builtin_inff() : 0.f;
  acc = f4{start, start, start, start};
  pos = i4{(int)p0, (int)p0, (int)p0, (int)p0};
  int64_t p = p0;
#pragma unroll 1
  for (; p + MP_AHEAD <= p1; p += MP_AHEAD) mp_take_batch<VEC, MAX, KIND, true>(acc, pos, W, p, p1, c);
  if (p < p1) mp_take_batch<VEC, MAX, KIND, false>(acc, pos, W, p, p1, c);
}

// workspace: [slots][lanes] f4 partial values, then (MAX) [slots][lanes] i4 CSR positions of the partial maxima
template <bool VEC, bool MAX, int KIND>
__global__ void __launch_bounds__(256) mpnn_chunks_kernel(const MpWalk W, int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  f4 acc;
  i4 pos;
  mp_reduce_entries<VEC, MAX, KIND>(acc, pos, W, s0, s1, c);
  *reinterpret_cast<f4*>(ws + (g * W.lanes) * 4 + c) = acc;
  if (MAX) *reinterpret_cast<i4*>(ws + ((slots + g) * W.lanes) * 4 + c) = pos;
}

// a row's reduction: chunk 0 here, chunks 1, 2, ... from the workspace in ascending order
template <bool VEC, bool MAX, int KIND>
__device__ inline void mp_reduce_row(f4& acc, i4& pos, const MpWalk& W, int64_t p0, int64_t p1, int c, int64_t slots,
                                  const float* __restrict__ ws) {
  mp_reduce_entries<VEC, MAX, KIND>(acc, pos, W, p0, min(p0 + ROW_CHUNK, p1), c);
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 4
  for (int64_t k = 0; k < n_part; ++k) {
    const f4 v = *reinterpret_cast<const f4*>(ws + ((first + k) * W.lanes) * 4 + c);
    if (MAX) {
      const i4 q = *reinterpret_cast<const i4*>(ws + ((slots + first + k) * W.lanes) * 4 + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool better = v[i] > acc[i];
        acc[i] = better ? v[i] : acc[i];
        pos[i] = better ? q[i] : pos[i];
      }
    } else {
      acc += v;
    }
  }
}

template <bool VEC, int OP>
__global__ void __launch_bounds__(256) mpnn_message_rows_kernel(const MpWalk W, const int32_t* __restrict__ edge_id,
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
    mp_reduce_row<VEC, MAX, MP_PLAIN>(acc, pos, W, p0, p1, c, slots, ws);
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

// group g: d P of transposed row g (g < W.n_rows) and d Q of forward row g (g < W.n_in_rows)
template <bool VEC, int KIND>
__global__ void __launch_bounds__(256) mpnn_backward_rows_kernel(const MpWalk W, const int32_t* __restrict__ f_rowptr, int op,
                                                                 float* __restrict__ dP, int ld_dp, float* __restrict__ dQ,
                                                                 int ld_dq, int64_t slots, const float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(W.lanes, g, c);
  if (dP != nullptr && g < W.n_rows) {
    int64_t p0, p1;
    row_range(W.rowptr, W.n_edges, g, p0, p1);
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    i4 pos;
    if (p1 > p0) mp_reduce_row<VEC, false, KIND>(acc, pos, W, p0, p1, c, slots, ws);
    tm_store<VEC>(dP + g * ld_dp + c, c, W.width, acc);
  }
  if (dQ != nullptr && g < W.n_in_rows) {
    const int deg = max(f_rowptr[g + 1] - f_rowptr[g], 0);
    f4 d = f4{0.f, 0.f, 0.f, 0.f};
    if (deg > 0) {
      d = tm_load<VEC>(W.in + g * W.ld_in + c, c, W.width);
      if (op == EGC_MPNN_ADD) d = (float)deg * d;
    }
    tm_store<VEC>(dQ + g * ld_dq + c, c, W.width, d);
  }
}

static inline size_t mp_workspace_bytes(int64_t n_edges, int32_t width, bool with_pos) {
  if (n_edges <= 0 || width <= 0) return 0;
  return (size_t)chunk_slots(n_edges) * (size_t)((width + 3) / 4) * 16 * (with_pos ? 2 : 1);
}

template <bool MAX, int KIND>
static int launch_chunks(const MpWalk& W, bool vec, int64_t slots, float* ws, hipStream_t stream) {
  unsigned blocks;
  if (grid_blocks(slots * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  if (vec) mpnn_chunks_kernel<true, MAX, KIND><<<blocks, 256, 0, stream>>>(W, slots, ws);
  else mpnn_chunks_kernel<false, MAX, KIND><<<blocks, 256, 0, stream>>>(W, slots, ws);
  EGC_LAUNCH_CHECK("mpnn_chunks_kernel");
  return EGC_OK;
}

}  // namespace egc

using namespace egc;

size_t egc_mpnn_message_workspace_bytes(int64_t n_edges, int32_t width, int32_t op) {
  return mp_workspace_bytes(n_edges, width, op == EGC_MPNN_MAX);
}

size_t egc_mpnn_message_backward_workspace_bytes(int64_t n_edges, int32_t width) {
  return mp_workspace_bytes(n_edges, width, false);
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
  MpWalk W = {};
  W.rowptr = rowptr, W.col = col, W.in = P;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows;
  W.ld_in = ld_p, W.width = width, W.lanes = (width + 3) / 4;
  const bool vec = all_mult4(width, ld_p, ld_q, ld_out) && all_aligned16(P, Q, out, arg);
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0) {
    if (!workspace_ok(ws, workspace_bytes, mp_workspace_bytes(n_edges, width, op == EGC_MPNN_MAX))) return EGC_ERR_WORKSPACE;
    const int st = op == EGC_MPNN_MAX ? launch_chunks<true, MP_PLAIN>(W, vec, slots, ws, stream)
                                      : launch_chunks<false, MP_PLAIN>(W, vec, slots, ws, stream);
    if (st != EGC_OK) return st;
  }
  unsigned blocks;
  if (grid_blocks(n_rows * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
#define EGC_MPNN_ROWS(V, O) \
  mpnn_message_rows_kernel<V, O><<<blocks, 256, 0, stream>>>(W, edge_id, Q, ld_q, out, ld_out, arg, slots, ws)
  if (op == EGC_MPNN_ADD) { if (vec) EGC_MPNN_ROWS(true, EGC_MPNN_ADD); else EGC_MPNN_ROWS(false, EGC_MPNN_ADD); }
  else if (op == EGC_MPNN_MEAN) { if (vec) EGC_MPNN_ROWS(true, EGC_MPNN_MEAN); else EGC_MPNN_ROWS(false, EGC_MPNN_MEAN); }
  else { if (vec) EGC_MPNN_ROWS(true, EGC_MPNN_MAX); else EGC_MPNN_ROWS(false, EGC_MPNN_MAX); }
#undef EGC_MPNN_ROWS
  EGC_LAUNCH_CHECK("mpnn_message_rows_kernel");
  return EGC_OK;
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
  MpWalk W = {};
  W.rowptr = t_rowptr, W.col = t_col, W.eid = t_edge_id, W.f_rowptr = rowptr, W.f_eid = edge_id, W.arg = arg, W.in = dm;
  W.n_rows = n_src_rows, W.n_edges = n_edges, W.n_in_rows = n_rows;
  W.ld_in = ld_dm, W.width = width, W.lanes = (width + 3) / 4;
  const bool vec = all_mult4(width, ld_dm, ld_dp, ld_dq) && all_aligned16(dm, dP, dQ, arg);
  const int64_t slots = dP != nullptr ? chunk_slots(n_edges) : 0;
  float* ws = static_cast<float*>(workspace);
  if (slots > 0) {
    if (!workspace_ok(ws, workspace_bytes, mp_workspace_bytes(n_edges, width, false))) return EGC_ERR_WORKSPACE;
    const int st = op == EGC_MPNN_ADD    ? launch_chunks<false, MP_PLAIN>(W, vec, slots, ws, stream)
                   : op == EGC_MPNN_MEAN ? launch_chunks<false, MP_DIV_DEG>(W, vec, slots, ws, stream)
                                         : launch_chunks<false, MP_MATCH>(W, vec, slots, ws, stream);
    if (st != EGC_OK) return st;
  }
  unsigned blocks;
  if (grid_blocks(groups * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
#define EGC_MPNN_BWD(V, K) \
  mpnn_backward_rows_kernel<V, K><<<blocks, 256, 0, stream>>>(W, rowptr, op, dP, ld_dp, dQ, ld_dq, slots, ws)
  if (op == EGC_MPNN_ADD) { if (vec) EGC_MPNN_BWD(true, MP_PLAIN); else EGC_MPNN_BWD(false, MP_PLAIN); }
  else if (op == EGC_MPNN_MEAN) { if (vec) EGC_MPNN_BWD(true, MP_DIV_DEG); else EGC_MPNN_BWD(false, MP_DIV_DEG); }
  else { if (vec) EGC_MPNN_BWD(true, MP_MATCH); else EGC_MPNN_BWD(false, MP_MATCH); }
#undef EGC_MPNN_BWD
  EGC_LAUNCH_CHECK("mpnn_backward_rows_kernel");
  return EGC_OK;
}
