// GAT (v1) attention aggregate (PyG GATConv's propagate) without any [E, .] array.  xl [N, H C], a_src [N, H] and a_dst [N, H]
// are column blocks of one dense product (a_src[j, h] = sum_c xl[j, h, c] att_src[h, c], a_dst likewise); for an entry j -> i
// and head h
//
//   z = a_src[j, h] + a_dst[i, h]      s_ij^h = leaky_relu(z)      alpha_ij^h = softmax over i's entries of s_ij^h
//   out_i^h = sum_j alpha_ij^h xl_j^h      lse_i^h = log sum_j exp(s_ij^h)   (0 and -inf for a row without entries)
//
// The score separates into two per-node scalars per head, so NO per-entry operation crosses lanes: a lane reads a_dst of its
// columns' heads once per row and, per entry, a_src of those heads and its quad of xl_j.  With the self-loop flag the row's
// entries whose col equals the row are skipped and ONE self entry (j = i) is taken LAST.  gfx950 only.  Forward: one gather pass
// over xl with egc_gat_dev.h's online softmax (the maximum is subtracted before every exp).  Backward, nothing per-edge kept:
// with g = d out, D_i^h = g_i^h . out_i^h, alpha = exp(s - lse_i), w_ij = alpha_ij leaky_relu'(z_ij), the per-entry
// d s_ij = w_ij (g_i . xl_j - D_i):
//   destination pass (forward CSR)     FACTORED, one head sum per row: v_i = sum_j w_ij xl_j (per column), t_i = sum_j w_ij
//                                      (per head), d a_dst[i, h] = g_i^h . v_i^h - D_i^h t_i^h,   D into the workspace
//   source pass (transposed CSR)       d xl_j = sum_i alpha_ij g_i (the direct term only; the rest flows through a_src, a_dst),
//                                      d a_src[j, h] = sum_i w_ij (g_i^h . xl_j^h - D_i^h): d s PER ENTRY, one gat_head_sums of
//                                      g_i xl_j per entry (skipped when d a_src is not wanted)
// The source pass is not factored (xl_j . sum_i w_ij g_i - sum_i w_ij D_i): where a source feeds the same few destinations many
// times, out_i is close to xl_j, every g_i . xl_j - D_i nearly cancels and the two factored sums cancel only at the row's end --
// in float32 that was 10 to 25 times the per-entry form's error on the sweep graph's out-hub.  The destination
// pass shows no such loss.  Every output element is written exactly once: no zero fill, no atomics.
//
// Mapping: egc_gat_dev.h's (a lane owns four adjacent columns, a row's group is the power of two >= ceil(H C / 4) lanes, at most
// 64, two quads per lane above 256 columns; 16-byte accesses of xl, g, out and d xl when the width, strides and pointers allow,
// 4-byte ones otherwise; the per-head arrays are always read and written 4 bytes at a time).
//
// Order rule.  A per-head sum over the head's C columns (D, g . v, g . xl) is egc_gat_dev.h's gat_head_sums: it depends on H
// and C only.  A row is cut into egc_row_chunks.h's chunks (skipped entries keep their place).  Forward: inside a chunk,
// batches of 8 entries from the chunk's start, folded as egc_gat_dev.h's gat_state_take; the row is chunk 0's state with the
// states of chunks 1, 2, ... merged in ascending order, then the self entry as a batch of one, then out = acc / l and
// lse = m + log l.  Backward sums (v, t, d xl, d a_src): ((0 + x0) + x1) + ... in entry order per chunk, chunk 0's sum with
// those of chunks 1, 2, ... added in ascending order, the self entry last; then, in the destination pass, the row's head sum
// and one subtraction.  So the order of every sum is fixed by H, C and the row's entries alone, never by where in the grid the
// row lands.  -ffp-contract=off.
//
// Attention dropout (the *_drop_kernel instances; every (S, VEC, SMALL) form exists with and without): egc_gat_dev.h's mask m'
// (scale or 0 per entry and head, the self entry included).  out_i = sum_j m'_ij alpha_ij xl_j with alpha and lse those of the
// unmasked row; D_i = g_i . out_i as before;  d s_ij = w_ij (m'_ij g_i . xl_j - D_i).
//   destination pass   v_i = sum_j w_ij m'_ij xl_j,  t_i = sum_j w_ij (unmasked),  d a_dst = g_i . v_i - D_i t_i
//   source pass        d xl_j = sum_i m'_ij alpha_ij g_i,  d a_src[j] = sum_i w_ij (m'_ij g_i . xl_j - D_i); the forward position
//                      of a transposed entry (the mask's counter) is t_edge_id's, one more 4-byte read per entry of this pass
// Order rule: every sum above keeps its order.  Forward: egc_gat_dev.h's (dropped terms left out of acc, scale once at the row's
// end).  Backward: the term of an entry is (w m') xl_j, (alpha m') g_i and w (m' (g_i . xl_j) - D_i), m' applied where written;
// at scale = 1 and nothing dropped these are the bits of the plain kernels.  A batch's Philox calls follow its gathers in
// program order (integer work under the loads' latency).
#include "egc_gat_host.h"

namespace egc {

constexpr int GAT1_AHEAD_DST = 8;
constexpr int GAT1_AHEAD_SRC = 4;

struct Gat1Walk : GatWalk {
  const float* a_src;   // forward / destination pass: gathered; source pass: the row's own
  const float* a_dst;   // forward / destination pass: the row's own; source pass: gathered
  int32_t ld_as, ld_ad;
};

// a[row, head] of every column of the lane, rows of stride ld.  C >= 4: a quad lies in at most two heads, two loads.
template <int S, bool SMALL>
__device__ inline void gat1_heads(f4 (&v)[S], const float* __restrict__ a, int64_t row, int ld, const GatLane<S>& L) {
  const float* __restrict__ r = a + row * ld;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (SMALL) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[s][j] = r[L.hd[s][j]];
    } else {
      const float first = r[L.hd[s][0]], next = r[L.hd[s][3]];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[s][j] = j < L.na[s] ? first : next;
    }
  }
}

// x[row, head] = v of the head's first column
template <int S>
__device__ inline void gat1_store_heads(float* __restrict__ x, int64_t row, int ld, const GatLane<S>& L, const f4 (&v)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (L.head_first[s][i]) x[row * ld + L.hd[s][i]] = v[s][i];
}

// the rows a batch of N entries from p on names, and which of them count
template <int N, bool FULL>
__device__ inline void gat1_batch_rows(int (&j)[N], bool (&live)[N], const Gat1Walk& W, int64_t p, int64_t p1, int64_t row, bool self) {
  const int last_in = (int)W.n_in_rows - 1;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int raw = self ? (int)row : W.col[batch_entry<FULL>(p, k, p1)];
    j[k] = clamp_index(raw, last_in);
    live[k] = self || ((FULL || p + k < p1) && !(W.self_loops && raw == (int)row));
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward

template <int S, bool VEC, bool SMALL, int N, bool FULL, class... Mask>
__device__ inline void gat1_fwd_batch(GatState<S>& st, const Gat1Walk& W, const GatLane<S>& L, const f4 (&ad)[S], int64_t p,
                                      int64_t p1, int64_t row, bool self, const Mask&... mask) {
  int j[N];
  bool live[N];
  gat1_batch_rows<N, FULL>(j, live, W, p, p1, row, self);
  f4 v[N][S], e[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    gat_load_row<S, VEC>(v[k], W.xl, j[k], W.ld_xl, L, W.width);
    gat1_heads<S, SMALL>(e[k], W.a_src, j[k], W.ld_as, L);
  }
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int s = 0; s < S; ++s) e[k][s] = gat_lrelu(e[k][s] + ad[s], W.slope);
  if constexpr (sizeof...(Mask) == 1) {
    uint32_t keep[N];
    gat_batch_keep<S, N, FULL>(keep, gat_only(mask...), L, p, p1, row, self);
    gat_state_take<S, N>(st, e, v, live, keep);
  } else {
    gat_state_take<S, N>(st, e, v, live);
  }
}

template <int S, bool VEC, bool SMALL, class... Mask>
__device__ inline void gat1_fwd_entries(GatState<S>& st, const Gat1Walk& W, const GatLane<S>& L, const f4 (&ad)[S], int64_t p0,
                                        int64_t p1, int64_t row, const Mask&... mask) {
  gat_state_init<S>(st);
  int64_t p = p0;
#pragma unroll 1
  for (; p + GAT_AHEAD <= p1; p += GAT_AHEAD) gat1_fwd_batch<S, VEC, SMALL, GAT_AHEAD, true, Mask...>(st, W, L, ad, p, p1, row, false, mask...);
  if (p < p1) gat1_fwd_batch<S, VEC, SMALL, GAT_AHEAD - 1, false, Mask...>(st, W, L, ad, p, p1, row, false, mask...);
}

// --------------------------------------------------------------------------------------------------------------- backward

// destination pass: N entries of row `row` -> v += w xl_j, t += w
template <int S, bool VEC, bool SMALL, int N, bool FULL, class... Mask>
__device__ inline void gat1_dst_batch(f4 (&va)[S], f4 (&ta)[S], const Gat1Walk& W, const GatLane<S>& L, const f4 (&ad)[S],
                                      const f4 (&lse)[S], int64_t p, int64_t p1, int64_t row, bool self, const Mask&... mask) {
  int j[N];
  bool live[N];
  gat1_batch_rows<N, FULL>(j, live, W, p, p1, row, self);
  f4 v[N][S], as[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    gat_load_row<S, VEC>(v[k], W.xl, j[k], W.ld_xl, L, W.width);
    gat1_heads<S, SMALL>(as[k], W.a_src, j[k], W.ld_as, L);
  }
  uint32_t keep[N] = {};
  if constexpr (sizeof...(Mask) == 1) gat_batch_keep<S, N, FULL>(keep, gat_only(mask...), L, p, p1, row, self);
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f4 z = as[k][s] + ad[s];
      f4 w = gat_exp(gat_lrelu(z, W.slope) - lse[s]) * gat_dlrelu(z, W.slope);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = live[k] ? w[i] : 0.f;
      if constexpr (sizeof...(Mask) == 1) va[s] = va[s] + (w * gat_keep_f4(keep[k], s, gat_only(mask...).scale)) * v[k][s];
      else va[s] = va[s] + w * v[k][s];
      ta[s] = ta[s] + w;
    }
  }
}

// source pass: N entries (destinations i) of transposed row `row` (= source j) -> d xl += alpha g_i, d a_src += w (g_i . xl_j - D_i)
template <int S, bool VEC, bool SMALL, int N, bool FULL, class... Mask>
__device__ inline void gat1_src_batch(f4 (&dx)[S], f4 (&sa)[S], const Gat1Walk& W, const GatLane<S>& L, const f4 (&as)[S],
                                      const f4 (&xl)[S], bool want_das, int64_t p, int64_t p1, int64_t row, bool self, const Mask&... mask) {
  int i_[N];
  bool live[N];
  gat1_batch_rows<N, FULL>(i_, live, W, p, p1, row, self);
  uint32_t pos[N];   // DROP: the entry's forward position (the self entry: its row)
  if constexpr (sizeof...(Mask) == 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) pos[k] = self ? (uint32_t)row : (uint32_t)gat_only(mask...).edge_id[batch_entry<FULL>(p, k, p1)];
  }
  f4 gr[N][S], ad[N][S], lse[N][S], D[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    gat_load_row<S, VEC>(gr[k], W.g, i_[k], W.ld_g, L, W.width);
    gat1_heads<S, SMALL>(ad[k], W.a_dst, i_[k], W.ld_ad, L);
    gat1_heads<S, SMALL>(lse[k], W.lse, i_[k], W.H, L);
    gat1_heads<S, SMALL>(D[k], W.D, i_[k], W.H, L);
  }
  uint32_t keep[N] = {};
  if constexpr (sizeof...(Mask) == 1) gat_batch_keep_at<S, N>(keep, gat_only(mask...), L, pos, self);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    f4 u[S], da[S];
    if (want_das) {   // uniform over the launch
#pragma unroll
      for (int s = 0; s < S; ++s) u[s] = gr[k][s] * xl[s];
      gat_head_sums<S, SMALL>(W, L, u, da);
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s) da[s] = f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f4 z = as[s] + ad[k][s];
      f4 alpha = gat_exp(gat_lrelu(z, W.slope) - lse[k][s]);
#pragma unroll
      for (int i = 0; i < 4; ++i) alpha[i] = live[k] ? alpha[i] : 0.f;
      const f4 w = alpha * gat_dlrelu(z, W.slope);
      if constexpr (sizeof...(Mask) == 1) {
        const f4 mk = gat_keep_f4(keep[k], s, gat_only(mask...).scale);
        dx[s] = dx[s] + (alpha * mk) * gr[k][s];
        sa[s] = sa[s] + w * (mk * da[s] - D[k][s]);
      } else {
        dx[s] = dx[s] + alpha * gr[k][s];
        sa[s] = sa[s] + w * (da[s] - D[k][s]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- kernels

// plain: NAME_kernel, no mask argument anywhere
#define GAT_KERNEL(name) name##_kernel
#define GAT_DROP_PARAM
#define GAT_DROP_SETUP
#define GAT_MASK
#define GAT_SCALED(x) x
#include "egc_gat_kernels.inc"
#undef GAT_KERNEL
#undef GAT_DROP_PARAM
#undef GAT_DROP_SETUP
#undef GAT_MASK
#undef GAT_SCALED

// DROP: NAME_drop_kernel(walk, ..., GatDrop R, ...), the mask X handed on as the device functions' last argument
#define GAT_KERNEL(name) name##_drop_kernel
#define GAT_DROP_PARAM const GatDrop R,
#define GAT_DROP_SETUP const GatMask X = gat_mask(R)
#define GAT_MASK , X
#define GAT_SCALED(x) (x) * X.scale
#include "egc_gat_kernels.inc"
#undef GAT_KERNEL
#undef GAT_DROP_PARAM
#undef GAT_DROP_SETUP
#undef GAT_MASK
#undef GAT_SCALED

// ------------------------------------------------------------------------------------------------------------------- host

// backward workspace, in floats
struct Gat1BwdWs {
  size_t D, part_dst, part_src, total;
  int64_t slots;
};

static inline Gat1BwdWs gat1_bwd_ws(int64_t n_rows, int64_t n_edges, int32_t H, int32_t C) {
  const GatGeom q = gat_geom(H * C);
  Gat1BwdWs w;
  w.slots = chunk_slots(n_edges);
  size_t at = 0;
  w.D = at, at += gat_align((size_t)n_rows * H);
  w.part_dst = at, at += (size_t)w.slots * q.V * 2 * 4;
  w.part_src = at, at += (size_t)w.slots * q.V * 2 * 4;
  w.total = at;
  return w;
}

}  // namespace egc

using namespace egc;

size_t egc_gat_forward_workspace_bytes(int64_t n_edges, int32_t heads, int32_t channels) {
  return gat_fwd_ws_bytes(n_edges, heads, channels);
}

size_t egc_gat_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t heads, int32_t channels) {
  if (n_rows <= 0 || n_edges < 0 || !gat_shape_ok(heads, channels)) return 0;
  return gat1_bwd_ws(n_rows, n_edges, heads, channels).total * sizeof(float);
}

// drop == NULL: the plain instances; else the DROP ones with *drop
static int gat1_forward(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                        const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst, int32_t ld_a_dst,
                        int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out,
                        float* lse, void* workspace, size_t workspace_bytes, egc_stream_t stream_, const GatDrop* drop) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = gat_forward_args(rowptr, col, n_rows, n_edges, n_src_rows, heads, channels, self_loops, xl, ld_xl, out, ld_out, lse,
                                  workspace, workspace_bytes, ld_a_src >= heads && ld_a_dst >= heads,
                                  a_dst != nullptr && (!(n_edges > 0 || self_loops) || a_src != nullptr));
  if (rc != GAT_RUN) return rc;
  Gat1Walk W = {};
  W.rowptr = rowptr, W.col = col, W.xl = xl, W.a_src = a_src, W.a_dst = a_dst;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows, W.ld_xl = ld_xl, W.ld_as = ld_a_src, W.ld_ad = ld_a_dst;
  gat_fill_walk(W, heads, channels, negative_slope, self_loops ? 1 : 0);
  const GatForm form = gat_form(heads, channels, {ld_xl, ld_out}, {xl, out});
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0) {
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat1_fwd_chunks_kernel<f.S, f.VEC, f.SMALL><<<gat_grid(slots, W.G), 256, 0, stream>>>(W, slots, ws);
      else gat1_fwd_chunks_drop_kernel<f.S, f.VEC, f.SMALL><<<gat_grid(slots, W.G), 256, 0, stream>>>(W, *drop, slots, ws);
    });
    EGC_LAUNCH_CHECK("gat1_fwd_chunks_kernel");
  }
  gat_dispatch(form, [&](auto f) {
    if (drop == nullptr) gat1_fwd_rows_kernel<f.S, f.VEC, f.SMALL><<<gat_grid(n_rows, W.G), 256, 0, stream>>>(W, out, ld_out, lse, ws);
    else gat1_fwd_rows_drop_kernel<f.S, f.VEC, f.SMALL><<<gat_grid(n_rows, W.G), 256, 0, stream>>>(W, *drop, out, ld_out, lse, ws);
  });
  EGC_LAUNCH_CHECK("gat1_fwd_rows_kernel");
  return EGC_OK;
}

int egc_gat_forward_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                        const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst, int32_t ld_a_dst,
                        int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out,
                        float* lse, void* workspace, size_t workspace_bytes, egc_stream_t stream) {
  return gat1_forward(rowptr, col, n_rows, n_edges, n_src_rows, xl, ld_xl, a_src, ld_a_src, a_dst, ld_a_dst, heads, channels,
                      negative_slope, self_loops, out, ld_out, lse, workspace, workspace_bytes, stream, nullptr);
}

int egc_gat_forward_dropout_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                                const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst,
                                int32_t ld_a_dst, int32_t heads, int32_t channels, float negative_slope, int32_t self_loops,
                                float* out, int32_t ld_out, float* lse, void* workspace, size_t workspace_bytes, double p,
                                const int64_t* seed, egc_stream_t stream) {
  GatDrop R = {};
  if (!gat_fill_drop(R, p, seed, nullptr, nullptr)) return EGC_ERR_INVALID;
  return gat1_forward(rowptr, col, n_rows, n_edges, n_src_rows, xl, ld_xl, a_src, ld_a_src, a_dst, ld_a_dst, heads, channels,
                      negative_slope, self_loops, out, ld_out, lse, workspace, workspace_bytes, stream, &R);
}

static int gat1_backward(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                         int64_t n_edges, const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst,
                         int32_t ld_a_dst, int32_t heads, int32_t channels, float negative_slope, int32_t self_loops,
                         const float* out, int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl,
                         int32_t ld_dxl, float* d_a_src, int32_t ld_d_a_src, float* d_a_dst, int32_t ld_d_a_dst, void* workspace,
                         size_t workspace_bytes, egc_stream_t stream_, const GatDrop* drop) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool src_pass = dxl != nullptr || d_a_src != nullptr;
  const int rc = gat_backward_args(
      rowptr, col, t_rowptr, t_col, n_rows, n_edges, heads, channels, xl, ld_xl, out, ld_out, lse, g, ld_g, dxl, ld_dxl, workspace,
      workspace_bytes, egc_gat_backward_workspace_bytes,
      ld_a_src >= heads && ld_a_dst >= heads && (d_a_src == nullptr || ld_d_a_src >= heads) && (d_a_dst == nullptr || ld_d_a_dst >= heads),
      src_pass || d_a_dst != nullptr, EGC_OK, a_src != nullptr && a_dst != nullptr, src_pass);
  if (rc != GAT_RUN) return rc;
  const Gat1BwdWs L = gat1_bwd_ws(n_rows, n_edges, heads, channels);
  float* ws = static_cast<float*>(workspace);
  Gat1Walk W = {};
  W.rowptr = rowptr, W.col = col, W.xl = xl, W.a_src = a_src, W.a_dst = a_dst, W.g = g, W.out = out, W.lse = lse, W.D = ws + L.D;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_rows;
  W.ld_xl = ld_xl, W.ld_as = ld_a_src, W.ld_ad = ld_a_dst, W.ld_g = ld_g, W.ld_out = ld_out;
  gat_fill_walk(W, heads, channels, negative_slope, self_loops ? 1 : 0);
  const GatForm form = gat_form(heads, channels, {ld_xl, ld_out, ld_g, ld_dxl}, {xl, out, g, dxl});
  const unsigned chunk_grid = gat_grid(L.slots, W.G), row_grid = gat_grid(n_rows, W.G);
  // destination pass: chunks (only when d a_dst is wanted), then rows (d a_dst, and D, which the source pass reads for d a_src)
  if (d_a_dst != nullptr || d_a_src != nullptr) {
    float* part = ws + L.part_dst;
    if (L.slots > 0 && d_a_dst != nullptr) {
      gat_dispatch(form, [&](auto f) {
        if (drop == nullptr) gat1_bwd_dst_kernel<f.S, f.VEC, f.SMALL, true><<<chunk_grid, 256, 0, stream>>>(W, nullptr, 0, nullptr, L.slots, part);
        else gat1_bwd_dst_drop_kernel<f.S, f.VEC, f.SMALL, true><<<chunk_grid, 256, 0, stream>>>(W, *drop, nullptr, 0, nullptr, L.slots, part);
      });
      EGC_LAUNCH_CHECK("gat1_bwd_dst_kernel(chunks)");
    }
    const Gat1Walk Wr = d_a_dst != nullptr ? W : gat_walk_only_D(W);
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat1_bwd_dst_kernel<f.S, f.VEC, f.SMALL, false><<<row_grid, 256, 0, stream>>>(Wr, d_a_dst, ld_d_a_dst, ws + L.D, L.slots, part);
      else gat1_bwd_dst_drop_kernel<f.S, f.VEC, f.SMALL, false><<<row_grid, 256, 0, stream>>>(Wr, *drop, d_a_dst, ld_d_a_dst, ws + L.D, L.slots, part);
    });
    EGC_LAUNCH_CHECK("gat1_bwd_dst_kernel(rows)");
  }
  if (src_pass) {
    Gat1Walk T = W;
    T.rowptr = t_rowptr, T.col = t_col;
    const int want_das = d_a_src != nullptr ? 1 : 0;
    float* part = ws + L.part_src;
    if (L.slots > 0) {
      gat_dispatch(form, [&](auto f) {
        if (drop == nullptr) gat1_bwd_src_kernel<f.S, f.VEC, f.SMALL, true><<<chunk_grid, 256, 0, stream>>>(T, nullptr, 0, nullptr, 0, want_das, L.slots, part);
        else gat1_bwd_src_drop_kernel<f.S, f.VEC, f.SMALL, true><<<chunk_grid, 256, 0, stream>>>(T, *drop, nullptr, 0, nullptr, 0, want_das, L.slots, part);
      });
      EGC_LAUNCH_CHECK("gat1_bwd_src_kernel(chunks)");
    }
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat1_bwd_src_kernel<f.S, f.VEC, f.SMALL, false><<<row_grid, 256, 0, stream>>>(
          T, dxl, ld_dxl, d_a_src, ld_d_a_src, want_das, L.slots, part);
      else gat1_bwd_src_drop_kernel<f.S, f.VEC, f.SMALL, false><<<row_grid, 256, 0, stream>>>(
          T, *drop, dxl, ld_dxl, d_a_src, ld_d_a_src, want_das, L.slots, part);
    });
    EGC_LAUNCH_CHECK("gat1_bwd_src_kernel(rows)");
  }
  return EGC_OK;
}

int egc_gat_backward_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                         int64_t n_edges, const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst,
                         int32_t ld_a_dst, int32_t heads, int32_t channels, float negative_slope, int32_t self_loops,
                         const float* out, int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl,
                         int32_t ld_dxl, float* d_a_src, int32_t ld_d_a_src, float* d_a_dst, int32_t ld_d_a_dst, void* workspace,
                         size_t workspace_bytes, egc_stream_t stream) {
  return gat1_backward(rowptr, col, t_rowptr, t_col, n_rows, n_edges, xl, ld_xl, a_src, ld_a_src, a_dst, ld_a_dst, heads, channels,
                       negative_slope, self_loops, out, ld_out, lse, g, ld_g, dxl, ld_dxl, d_a_src, ld_d_a_src, d_a_dst, ld_d_a_dst,
                       workspace, workspace_bytes, stream, nullptr);
}

int egc_gat_backward_dropout_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                 const int32_t* t_edge_id, int64_t n_rows, int64_t n_edges, const float* xl, int32_t ld_xl,
                                 const float* a_src, int32_t ld_a_src, const float* a_dst, int32_t ld_a_dst, int32_t heads,
                                 int32_t channels, float negative_slope, int32_t self_loops, const float* out, int32_t ld_out,
                                 const float* lse, const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* d_a_src,
                                 int32_t ld_d_a_src, float* d_a_dst, int32_t ld_d_a_dst, void* workspace, size_t workspace_bytes,
                                 double p, const int64_t* seed, egc_stream_t stream) {
  GatDrop R = {};
  if (!gat_fill_drop(R, p, seed, t_rowptr, t_edge_id)) return EGC_ERR_INVALID;
  return gat1_backward(rowptr, col, t_rowptr, t_col, n_rows, n_edges, xl, ld_xl, a_src, ld_a_src, a_dst, ld_a_dst, heads, channels,
                       negative_slope, self_loops, out, ld_out, lse, g, ld_g, dxl, ld_dxl, d_a_src, ld_d_a_src, d_a_dst, ld_d_a_dst,
                       workspace, workspace_bytes, stream, &R);
}
