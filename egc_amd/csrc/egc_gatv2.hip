// GATv2 attention aggregate (PyG 2.x GATv2Conv's propagate) without any [E, .] array.  xl and xr are the two [N, H C] halves of
// one dense product; for an entry j -> i and head h
//
//   z = xl_j^h + xr_i^h      s_ij^h = sum_c att^h_c leaky_relu(z_c)      alpha_ij^h = softmax over i's entries of s_ij^h
//   out_i^h = sum_j alpha_ij^h xl_j^h      lse_i^h = log sum_j exp(s_ij^h)   (0 and -inf for a row without entries)
//
// With the self-loop flag the row's entries whose col equals the row are skipped and ONE self entry (j = i) is taken LAST, as
// PyG's remove_self_loops + add_self_loops leaves it.  gfx950 only.  Forward: one gather pass over xl with an online softmax
// (running maximum m, running sum l and accumulator rescaled by exp(m_old - m_new); the maximum is subtracted before every exp).
// Backward, nothing per-edge kept: with g = d out, D_i^h = g_i^h . out_i^h, alpha = exp(s - lse), d alpha = g_i^h . xl_j^h,
// d s = alpha (d alpha - D_i), d z = d s att leaky_relu'(z):
//   destination pass (forward CSR)       d xr_i = sum_j d z_ij,   d att = sum_ij d s_ij leaky_relu(z_ij),   D into the workspace
//   source pass (transposed CSR)         d xl_j = sum_i (alpha_ij g_i + d z_ij)
// Every output element is written exactly once: no zero fill, no atomics.
//
// Mapping, and the order rule of a per-head sum over the head's C columns (the score, d alpha, D): egc_gat_dev.h's (a lane owns
// four adjacent columns, a row's group lies inside one wavefront; gat_head_sums depends on H and C only, never on where in the
// grid the row lands).
// Order rule of a row: egc_row_chunks.h's chunks (skipped entries keep their place).  Inside a chunk, batches of AHEAD entries
// (8 forward, 4 backward) from the chunk's start.
// Forward, per batch: bm = max(m, the live scores in entry order); l = l * r + sum in entry order of exp(s_k - bm), acc likewise
// with exp(s_k - bm) * xl_k, r = exp(m - bm) (1 when m == bm); m = bm.  The row is chunk 0's state with the states of chunks
// 1, 2, ... merged in ascending order (M = max(m1, m2); l = l1 exp(m1 - M) + l2 exp(m2 - M)), then the self entry as a batch of
// one, then out = acc / l and lse = m + log l.  Backward sums: ((0 + v0) + v1) + ... in entry order per chunk, chunk 0's sum
// with those of chunks 1, 2, ... added in ascending order, the self entry last.  d att: a lane's sum over its row (entry order,
// chunk by chunk), the workgroup's groups added in ascending order, the workgroups' partials (row workgroups, then chunk
// workgroups) added in ascending order in blocks of 64, and those block sums again, until one is left.  -ffp-contract=off.
//
// Attention dropout (the *_drop_kernel instances; every (S, VEC, SMALL) form exists with and without): egc_gat_dev.h's mask m'
// (scale or 0 per entry and head, the self entry included).  out_i = sum_j m'_ij alpha_ij xl_j with alpha and lse those of the
// unmasked row; D_i = g_i . out_i as before; d s = alpha (m' g_i . xl_j - D_i) in d xr, d att and d xl's chain part, and
// (alpha m') g_i for d xl's direct term.  The source pass reads the forward position of a transposed entry (the mask's counter)
// from t_edge_id: one more 4-byte read per entry of that pass.  Order rule: every sum above keeps its order; forward:
// egc_gat_dev.h's (dropped terms left out of acc, scale once at the row's end); backward: m' is a factor of the entry's term
// where written, so at scale = 1 and nothing dropped the bits are those of the plain kernels.  A batch's Philox calls follow its
// gathers in program order.
#include "egc_gat_host.h"

namespace egc {

// The score's per-column term: s = per-head sum of att * act(z), z = xl_j + xr_i.  (GAT v1's additive score separates into two
// per-node scalars per head and needs no per-entry head sum: it has a kernel of its own, egc_gat.hip, on egc_gat_dev.h's mapping.)
struct GatV2Score {
  float slope;
  __device__ inline f4 act(f4 z) const { return gat_lrelu(z, slope); }
  __device__ inline f4 dact(f4 z) const { return gat_dlrelu(z, slope); }
};

// ---------------------------------------------------------------------------------------------------------------- forward

template <int S, bool VEC, bool SMALL, class Score, bool FULL, class... Mask>
__device__ inline void gat_fwd_batch(GatState<S>& st, const GatWalk& W, const GatLane<S>& L, const Score& sc, const f4 (&xr)[S],
                                     const f4 (&att)[S], int64_t p, int64_t p1, int64_t row, const Mask&... mask) {
  constexpr int N = FULL ? GAT_AHEAD : GAT_AHEAD - 1;
  const int last_in = (int)W.n_in_rows - 1;
  int j[N];
  bool live[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int raw = W.col[batch_entry<FULL>(p, k, p1)];
    j[k] = clamp_index(raw, last_in);
    live[k] = (FULL || p + k < p1) && !(W.self_loops && raw == (int)row);
  }
  f4 v[N][S], e[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) gat_load_row<S, VEC>(v[k], W.xl, j[k], W.ld_xl, L, W.width);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    f4 t[S];
#pragma unroll
    for (int s = 0; s < S; ++s) t[s] = att[s] * sc.act(v[k][s] + xr[s]);
    gat_head_sums<S, SMALL>(W, L, t, e[k]);
  }
  if constexpr (sizeof...(Mask) == 1) {
    uint32_t keep[N];
    gat_batch_keep<S, N, FULL>(keep, gat_only(mask...), L, p, p1, row, false);
    gat_state_take<S, N>(st, e, v, live, keep);
  } else {
    gat_state_take<S, N>(st, e, v, live);
  }
}

template <int S, bool VEC, bool SMALL, class Score, class... Mask>
__device__ inline void gat_fwd_entries(GatState<S>& st, const GatWalk& W, const GatLane<S>& L, const Score& sc, const f4 (&xr)[S],
                                       const f4 (&att)[S], int64_t p0, int64_t p1, int64_t row, const Mask&... mask) {
  gat_state_init<S>(st);
  int64_t p = p0;
#pragma unroll 1
  for (; p + GAT_AHEAD <= p1; p += GAT_AHEAD) gat_fwd_batch<S, VEC, SMALL, Score, true, Mask...>(st, W, L, sc, xr, att, p, p1, row, mask...);
  if (p < p1) gat_fwd_batch<S, VEC, SMALL, Score, false, Mask...>(st, W, L, sc, xr, att, p, p1, row, mask...);
}

// --------------------------------------------------------------------------------------------------------------- backward

// destination pass: N entries of row `row` -> d xr and d att partial sums
template <int S, bool VEC, bool SMALL, class Score, int N, bool FULL, class... Mask>
__device__ inline void gat_dst_batch(f4 (&dxr)[S], f4 (&datt)[S], const GatWalk& W, const GatLane<S>& L, const Score& sc,
                                     const f4 (&xr)[S], const f4 (&att)[S], const f4 (&g)[S], const f4 (&lse)[S], const f4 (&D)[S],
                                     int64_t p, int64_t p1, int64_t row, bool self, const Mask&... mask) {
  const int last_in = (int)W.n_in_rows - 1;
  int j[N];
  bool live[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int raw = self ? (int)row : W.col[batch_entry<FULL>(p, k, p1)];
    j[k] = clamp_index(raw, last_in);
    live[k] = self || ((FULL || p + k < p1) && !(W.self_loops && raw == (int)row));
  }
  f4 v[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) gat_load_row<S, VEC>(v[k], W.xl, j[k], W.ld_xl, L, W.width);
  uint32_t keep[N] = {};
  if constexpr (sizeof...(Mask) == 1) gat_batch_keep<S, N, FULL>(keep, gat_only(mask...), L, p, p1, row, self);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    f4 z[S], lz[S], t[S], u[S], e[S], da[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z[s] = v[k][s] + xr[s], lz[s] = sc.act(z[s]), t[s] = att[s] * lz[s], u[s] = g[s] * v[k][s];
    gat_head_sums<S, SMALL>(W, L, t, e);
    gat_head_sums<S, SMALL>(W, L, u, da);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      f4 alpha = gat_exp(e[s] - lse[s]);
#pragma unroll
      for (int i = 0; i < 4; ++i) alpha[i] = live[k] ? alpha[i] : 0.f;
      if constexpr (sizeof...(Mask) == 1) da[s] = gat_keep_f4(keep[k], s, gat_only(mask...).scale) * da[s];
      const f4 ds = alpha * (da[s] - D[s]);
      dxr[s] = dxr[s] + ds * att[s] * sc.dact(z[s]);
      datt[s] = datt[s] + ds * lz[s];
    }
  }
}

// the workgroup's d att partial: its groups' lane sums added in ascending group order into part[blockIdx.x]
template <int S>
__device__ inline void gat_block_datt(const f4 (&datt)[S], const GatWalk& W, const GatLane<S>& L, float* __restrict__ part) {
  __shared__ float red[1024 * S];
  const int gi = (int)threadIdx.x / W.G;
#pragma unroll
  for (int s = 0; s < S; ++s) *reinterpret_cast<f4*>(red + (gi * W.V + L.v[s]) * 4) = datt[s];
  __syncthreads();
  const int groups = 256 / W.G;
  for (int c = (int)threadIdx.x; c < W.width; c += 256) {
    float sum = 0.f;
    for (int k = 0; k < groups; ++k) sum += red[k * W.V * 4 + c];
    part[(int64_t)blockIdx.x * W.width + c] = sum;
  }
}

// source pass: N entries (destinations i) of transposed row `row` (= source j) -> d xl partial sum
template <int S, bool VEC, bool SMALL, class Score, int N, bool FULL, class... Mask>
__device__ inline void gat_src_batch(f4 (&acc)[S], const GatWalk& W, const GatLane<S>& L, const Score& sc, const f4 (&xl)[S],
                                     const f4 (&att)[S], int64_t p, int64_t p1, int64_t row, bool self, const Mask&... mask) {
  const int last_in = (int)W.n_in_rows - 1;
  int i_[N];
  bool live[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int raw = self ? (int)row : W.col[batch_entry<FULL>(p, k, p1)];
    i_[k] = clamp_index(raw, last_in);
    live[k] = self || ((FULL || p + k < p1) && !(W.self_loops && raw == (int)row));
  }
  uint32_t pos[N];   // DROP: the entry's forward position (the self entry: its row)
  if constexpr (sizeof...(Mask) == 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) pos[k] = self ? (uint32_t)row : (uint32_t)gat_only(mask...).edge_id[batch_entry<FULL>(p, k, p1)];
  }
  f4 xr[N][S], gr[N][S], lse[N][S], D[N][S];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    gat_load_row<S, VEC>(xr[k], W.xr, i_[k], W.ld_xr, L, W.width);
    gat_load_row<S, VEC>(gr[k], W.g, i_[k], W.ld_g, L, W.width);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    gat_load_heads<S>(lse[k], W.lse, i_[k], W, L);
    gat_load_heads<S>(D[k], W.D, i_[k], W, L);
  }
  uint32_t keep[N] = {};
  if constexpr (sizeof...(Mask) == 1) gat_batch_keep_at<S, N>(keep, gat_only(mask...), L, pos, self);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    f4 z[S], t[S], u[S], e[S], da[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z[s] = xl[s] + xr[k][s], t[s] = att[s] * sc.act(z[s]), u[s] = gr[k][s] * xl[s];
    gat_head_sums<S, SMALL>(W, L, t, e);
    gat_head_sums<S, SMALL>(W, L, u, da);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      f4 alpha = gat_exp(e[s] - lse[k][s]);
#pragma unroll
      for (int i = 0; i < 4; ++i) alpha[i] = live[k] ? alpha[i] : 0.f;
      if constexpr (sizeof...(Mask) == 1) {
        const f4 mk = gat_keep_f4(keep[k], s, gat_only(mask...).scale);
        const f4 ds = alpha * (mk * da[s] - D[k][s]);
        acc[s] = acc[s] + ((alpha * mk) * gr[k][s] + ds * att[s] * sc.dact(z[s]));
      } else {
        const f4 ds = alpha * (da[s] - D[k][s]);
        acc[s] = acc[s] + (alpha * gr[k][s] + ds * att[s] * sc.dact(z[s]));
      }
    }
  }
}

// out[b, c] = in[b * 64, c] + in[b * 64 + 1, c] + ... (ascending, from 0)
__global__ void __launch_bounds__(256) gat_sum_rows_kernel(const float* __restrict__ in, int64_t n_in, int width, float* __restrict__ out) {
  const int c = (int)threadIdx.x + 256 * (int)blockIdx.y;
  if (c >= width) return;
  const int64_t r0 = (int64_t)blockIdx.x * GAT_SUM_BLOCK, r1 = min(r0 + GAT_SUM_BLOCK, n_in);
  float sum = 0.f;
#pragma unroll 8
  for (int64_t r = r0; r < r1; ++r) sum += in[r * width + c];
  out[(int64_t)blockIdx.x * width + c] = sum;
}

// ---------------------------------------------------------------------------------------------------------------- kernels

// plain: NAME_kernel, no mask argument anywhere
#define GAT_KERNEL(name) name##_kernel
#define GAT_DROP_PARAM
#define GAT_DROP_SETUP
#define GAT_MASK
#define GAT_SCALED(x) x
#define GAT_SELF_KEEP_SETUP
#define GAT_SELF_KEEP
#include "egc_gatv2_kernels.inc"
#undef GAT_KERNEL
#undef GAT_DROP_PARAM
#undef GAT_DROP_SETUP
#undef GAT_MASK
#undef GAT_SCALED
#undef GAT_SELF_KEEP_SETUP
#undef GAT_SELF_KEEP

// DROP: NAME_drop_kernel(walk, ..., GatDrop R, ...), the mask X handed on as the device functions' last argument
#define GAT_KERNEL(name) name##_drop_kernel
#define GAT_DROP_PARAM const GatDrop R,
#define GAT_DROP_SETUP const GatMask X = gat_mask(R)
#define GAT_MASK , X
#define GAT_SCALED(x) (x) * X.scale
#define GAT_SELF_KEEP_SETUP const uint32_t keep[1] = {gat_keep_bits<S>(X, L, (uint32_t)row, 1u)}
#define GAT_SELF_KEEP , keep
#include "egc_gatv2_kernels.inc"
#undef GAT_KERNEL
#undef GAT_DROP_PARAM
#undef GAT_DROP_SETUP
#undef GAT_MASK
#undef GAT_SCALED
#undef GAT_SELF_KEEP_SETUP
#undef GAT_SELF_KEEP

// ------------------------------------------------------------------------------------------------------------------- host

// backward workspace, in floats
struct GatBwdWs {
  size_t D, part_xr, part_xl, part_att, tmp0, tmp1, total;
  int64_t slots, row_blocks, chunk_blocks;
};

static inline GatBwdWs gat_bwd_ws(int64_t n_rows, int64_t n_edges, int32_t H, int32_t C) {
  const int32_t width = H * C;
  const GatGeom q = gat_geom(width);
  GatBwdWs w;
  w.slots = chunk_slots(n_edges);
  w.row_blocks = gat_blocks(n_rows, q.G), w.chunk_blocks = gat_blocks(w.slots, q.G);
  const int64_t parts = w.row_blocks + w.chunk_blocks;
  size_t at = 0;
  w.D = at, at += gat_align((size_t)n_rows * H);
  w.part_xr = at, at += (size_t)w.slots * q.V * 4;
  w.part_xl = at, at += (size_t)w.slots * q.V * 4;
  w.part_att = at, at += gat_align((size_t)parts * width);
  w.tmp0 = at, at += gat_align((size_t)ceil_div(parts, GAT_SUM_BLOCK) * width);
  w.tmp1 = at, at += gat_align((size_t)ceil_div(ceil_div(parts, GAT_SUM_BLOCK), GAT_SUM_BLOCK) * width);
  w.total = at;
  return w;
}

}  // namespace egc

using namespace egc;

size_t egc_gatv2_forward_workspace_bytes(int64_t n_edges, int32_t heads, int32_t channels) {
  return gat_fwd_ws_bytes(n_edges, heads, channels);
}

size_t egc_gatv2_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t heads, int32_t channels) {
  if (n_rows <= 0 || n_edges < 0 || !gat_shape_ok(heads, channels)) return 0;
  return gat_bwd_ws(n_rows, n_edges, heads, channels).total * sizeof(float);
}

// drop == NULL: the plain instances; else the DROP ones with *drop
static int gat2_forward(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                        const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att, int32_t heads,
                        int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out, float* lse,
                        void* workspace, size_t workspace_bytes, egc_stream_t stream_, const GatDrop* drop) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = gat_forward_args(rowptr, col, n_rows, n_edges, n_src_rows, heads, channels, self_loops, xl, ld_xl, out, ld_out, lse,
                                  workspace, workspace_bytes, ld_xr >= (int64_t)heads * channels, xr != nullptr && att != nullptr);
  if (rc != GAT_RUN) return rc;
  GatWalk W = {};
  W.rowptr = rowptr, W.col = col, W.xl = xl, W.xr = xr, W.att = att;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows, W.ld_xl = ld_xl, W.ld_xr = ld_xr;
  gat_fill_walk(W, heads, channels, negative_slope, self_loops ? 1 : 0);
  const GatV2Score sc = {negative_slope};
  const GatForm form = gat_form(heads, channels, {ld_xl, ld_xr, ld_out}, {xl, xr, out});
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0) {
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat_fwd_chunks_kernel<f.S, f.VEC, f.SMALL, GatV2Score><<<gat_grid(slots, W.G), 256, 0, stream>>>(W, sc, slots, ws);
      else gat_fwd_chunks_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score><<<gat_grid(slots, W.G), 256, 0, stream>>>(W, sc, *drop, slots, ws);
    });
    EGC_LAUNCH_CHECK("gat_fwd_chunks_kernel");
  }
  gat_dispatch(form, [&](auto f) {
    if (drop == nullptr) gat_fwd_rows_kernel<f.S, f.VEC, f.SMALL, GatV2Score><<<gat_grid(n_rows, W.G), 256, 0, stream>>>(W, sc, out, ld_out, lse, slots, ws);
    else gat_fwd_rows_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score><<<gat_grid(n_rows, W.G), 256, 0, stream>>>(W, sc, *drop, out, ld_out, lse, slots, ws);
  });
  EGC_LAUNCH_CHECK("gat_fwd_rows_kernel");
  return EGC_OK;
}

int egc_gatv2_forward_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                          const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att, int32_t heads,
                          int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out, float* lse,
                          void* workspace, size_t workspace_bytes, egc_stream_t stream) {
  return gat2_forward(rowptr, col, n_rows, n_edges, n_src_rows, xl, ld_xl, xr, ld_xr, att, heads, channels, negative_slope,
                      self_loops, out, ld_out, lse, workspace, workspace_bytes, stream, nullptr);
}

int egc_gatv2_forward_dropout_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                                  const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att, int32_t heads,
                                  int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out,
                                  float* lse, void* workspace, size_t workspace_bytes, double p, const int64_t* seed,
                                  egc_stream_t stream) {
  GatDrop R = {};
  if (!gat_fill_drop(R, p, seed, nullptr, nullptr)) return EGC_ERR_INVALID;
  return gat2_forward(rowptr, col, n_rows, n_edges, n_src_rows, xl, ld_xl, xr, ld_xr, att, heads, channels, negative_slope,
                      self_loops, out, ld_out, lse, workspace, workspace_bytes, stream, &R);
}

static int gat2_backward(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                         int64_t n_edges, const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att,
                         int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, const float* out,
                         int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* dxr,
                         int32_t ld_dxr, float* datt, void* workspace, size_t workspace_bytes, egc_stream_t stream_,
                         const GatDrop* drop) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t width = (int64_t)heads * channels;
  const int rc = gat_backward_args(rowptr, col, t_rowptr, t_col, n_rows, n_edges, heads, channels, xl, ld_xl, out, ld_out, lse, g, ld_g,
                                   dxl, ld_dxl, workspace, workspace_bytes, egc_gatv2_backward_workspace_bytes,
                                   ld_xr >= width && (dxr == nullptr || ld_dxr >= width), dxl != nullptr || dxr != nullptr || datt != nullptr,
                                   datt == nullptr ? EGC_OK : EGC_ERR_INVALID,   // (d att of nothing is the caller's zero)
                                   xr != nullptr && att != nullptr, dxl != nullptr);
  if (rc != GAT_RUN) return rc;
  const GatBwdWs L = gat_bwd_ws(n_rows, n_edges, heads, channels);
  float* ws = static_cast<float*>(workspace);
  GatWalk W = {};
  W.rowptr = rowptr, W.col = col, W.xl = xl, W.xr = xr, W.att = att, W.g = g, W.out = out, W.lse = lse, W.D = ws + L.D;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_rows;
  W.ld_xl = ld_xl, W.ld_xr = ld_xr, W.ld_g = ld_g, W.ld_out = ld_out;
  gat_fill_walk(W, heads, channels, negative_slope, self_loops ? 1 : 0);
  const GatV2Score sc = {negative_slope};
  const GatForm form = gat_form(heads, channels, {ld_xl, ld_xr, ld_out, ld_g, ld_dxl, ld_dxr}, {xl, xr, out, g, dxl, dxr});
  const unsigned chunk_grid = gat_grid(L.slots, W.G), row_grid = gat_grid(n_rows, W.G);
  float* part = datt != nullptr ? ws + L.part_att : nullptr;
  // destination pass: chunks (only when something they produce is wanted), then rows (always: the source pass reads D)
  const bool dst_sums = dxr != nullptr || datt != nullptr;
  if (L.slots > 0 && dst_sums) {
    float* cpart = part != nullptr ? part + (size_t)L.row_blocks * width : nullptr;
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat_bwd_dst_kernel<f.S, f.VEC, f.SMALL, GatV2Score, true><<<chunk_grid, 256, 0, stream>>>(
          W, sc, nullptr, 0, nullptr, L.slots, ws + L.part_xr, cpart);
      else gat_bwd_dst_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score, true><<<chunk_grid, 256, 0, stream>>>(
          W, sc, *drop, nullptr, 0, nullptr, L.slots, ws + L.part_xr, cpart);
    });
    EGC_LAUNCH_CHECK("gat_bwd_dst_kernel(chunks)");
  }
  {
    const GatWalk Wr = dst_sums ? W : gat_walk_only_D(W);   // (only D: the self entry's sums are unused too)
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat_bwd_dst_kernel<f.S, f.VEC, f.SMALL, GatV2Score, false><<<row_grid, 256, 0, stream>>>(
          Wr, sc, dxr, ld_dxr, ws + L.D, L.slots, ws + L.part_xr, part);
      else gat_bwd_dst_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score, false><<<row_grid, 256, 0, stream>>>(
          Wr, sc, *drop, dxr, ld_dxr, ws + L.D, L.slots, ws + L.part_xr, part);
    });
    EGC_LAUNCH_CHECK("gat_bwd_dst_kernel(rows)");
  }
  if (datt != nullptr) {
    const bool chunks_ran = L.slots > 0;
    int64_t n = L.row_blocks + (chunks_ran ? L.chunk_blocks : 0);
    const float* in = part;
    float* tmp[2] = {ws + L.tmp0, ws + L.tmp1};
    int flip = 0;
    for (;;) {
      const int64_t n_out = ceil_div(n, GAT_SUM_BLOCK);
      float* o = n_out == 1 ? datt : tmp[flip];
      gat_sum_rows_kernel<<<dim3((unsigned)n_out, (unsigned)ceil_div(width, 256)), 256, 0, stream>>>(in, n, width, o);
      EGC_LAUNCH_CHECK("gat_sum_rows_kernel");
      if (n_out == 1) break;
      in = o, n = n_out, flip ^= 1;
    }
  }
  if (dxl != nullptr) {
    GatWalk T = W;
    T.rowptr = t_rowptr, T.col = t_col;
    if (L.slots > 0) {
      gat_dispatch(form, [&](auto f) {
        if (drop == nullptr) gat_bwd_src_kernel<f.S, f.VEC, f.SMALL, GatV2Score, true><<<chunk_grid, 256, 0, stream>>>(T, sc, nullptr, 0, L.slots, ws + L.part_xl);
        else gat_bwd_src_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score, true><<<chunk_grid, 256, 0, stream>>>(T, sc, *drop, nullptr, 0, L.slots, ws + L.part_xl);
      });
      EGC_LAUNCH_CHECK("gat_bwd_src_kernel(chunks)");
    }
    gat_dispatch(form, [&](auto f) {
      if (drop == nullptr) gat_bwd_src_kernel<f.S, f.VEC, f.SMALL, GatV2Score, false><<<row_grid, 256, 0, stream>>>(T, sc, dxl, ld_dxl, L.slots, ws + L.part_xl);
      else gat_bwd_src_drop_kernel<f.S, f.VEC, f.SMALL, GatV2Score, false><<<row_grid, 256, 0, stream>>>(T, sc, *drop, dxl, ld_dxl, L.slots, ws + L.part_xl);
    });
    EGC_LAUNCH_CHECK("gat_bwd_src_kernel(rows)");
  }
  return EGC_OK;
}

int egc_gatv2_backward_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                           int64_t n_edges, const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att,
                           int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, const float* out,
                           int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* dxr,
                           int32_t ld_dxr, float* datt, void* workspace, size_t workspace_bytes, egc_stream_t stream) {
  return gat2_backward(rowptr, col, t_rowptr, t_col, n_rows, n_edges, xl, ld_xl, xr, ld_xr, att, heads, channels, negative_slope,
                       self_loops, out, ld_out, lse, g, ld_g, dxl, ld_dxl, dxr, ld_dxr, datt, workspace, workspace_bytes, stream,
                       nullptr);
}

int egc_gatv2_backward_dropout_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                   const int32_t* t_edge_id, int64_t n_rows, int64_t n_edges, const float* xl, int32_t ld_xl,
                                   const float* xr, int32_t ld_xr, const float* att, int32_t heads, int32_t channels,
                                   float negative_slope, int32_t self_loops, const float* out, int32_t ld_out, const float* lse,
                                   const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* dxr, int32_t ld_dxr, float* datt,
                                   void* workspace, size_t workspace_bytes, double p, const int64_t* seed, egc_stream_t stream) {
  GatDrop R = {};
  if (!gat_fill_drop(R, p, seed, t_rowptr, t_edge_id)) return EGC_ERR_INVALID;
  return gat2_backward(rowptr, col, t_rowptr, t_col, n_rows, n_edges, xl, ld_xl, xr, ld_xr, att, heads, channels, negative_slope,
                       self_loops, out, ld_out, lse, g, ld_g, dxl, ld_dxl, dxr, ld_dxr, datt, workspace, workspace_bytes, stream, &R);
}
