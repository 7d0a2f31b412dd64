// The four kernels of egc_gatv2.hip, included twice under the macros egc_gatv2.hip defines around the include: once as
// NAME_kernel, the plain instances -- every macro but the name expands to nothing, so their text is what it always was and their
// code is too --, once as NAME_drop_kernel, which takes egc_gat_dev.h's GatDrop after the walk and the score and hands the
// mask on as the device functions' last argument.  The walk stays a by-value kernel argument of both: its pointers are
// then known to be global ones (behind a reference into an inlined body they become flat accesses).

// workspace: per slot and virtual lane three f4: m, l, acc
template <int S, bool VEC, bool SMALL, class Score>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat_fwd_chunks)(const GatWalk W, const Score sc, GAT_DROP_PARAM int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.G, g, c);
  if (g >= slots) return;
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  if (!slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  f4 xr[S], att[S];
  gat_load_row<S, VEC>(xr, W.xr, row, W.ld_xr, L, W.width);
  gat_load_row<S, false>(att, W.att, 0, 0, L, W.width);
  GatState<S> st;
  GAT_DROP_SETUP;
  gat_fwd_entries<S, VEC, SMALL, Score>(st, W, L, sc, xr, att, s0, s1, row GAT_MASK);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f4* o = reinterpret_cast<f4*>(ws) + (g * W.V + L.v[s]) * 3;
    o[0] = st.m[s], o[1] = st.l[s], o[2] = st.acc[s];
  }
}

template <int S, bool VEC, bool SMALL, class Score>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat_fwd_rows)(const GatWalk W, const Score sc, GAT_DROP_PARAM float* __restrict__ out, int ld_out,
                                                           float* __restrict__ lse, int64_t slots, const float* __restrict__ ws) {
  int64_t row, p0, p1;
  int c;
  group_lane(W.G, row, c);
  if (row >= W.n_rows) return;
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 xr[S], att[S];
  gat_load_row<S, VEC>(xr, W.xr, row, W.ld_xr, L, W.width);
  gat_load_row<S, false>(att, W.att, 0, 0, L, W.width);
  GatState<S> st;
  GAT_DROP_SETUP;
  gat_fwd_entries<S, VEC, SMALL, Score>(st, W, L, sc, xr, att, p0, min(p0 + ROW_CHUNK, p1), row GAT_MASK);
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 1
  for (int64_t k = 0; k < n_part; ++k) {
    f4 m2[S], l2[S], a2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f4* o = reinterpret_cast<const f4*>(ws) + ((first + k) * W.V + L.v[s]) * 3;
      m2[s] = o[0], l2[s] = o[1], a2[s] = o[2];
    }
    gat_state_merge<S>(st, m2, l2, a2);
  }
  if (W.self_loops) {
    f4 v[1][S], e[1][S], tt[S];
    const bool live[1] = {true};
    gat_load_row<S, VEC>(v[0], W.xl, min(row, W.n_in_rows - 1), W.ld_xl, L, W.width);
#pragma unroll
    for (int s = 0; s < S; ++s) tt[s] = att[s] * sc.act(v[0][s] + xr[s]);
    gat_head_sums<S, SMALL>(W, L, tt, e[0]);
    GAT_SELF_KEEP_SETUP;
    gat_state_take<S, 1>(st, e, v, live GAT_SELF_KEEP);
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool any = st.l[s][i] > 0.f;
      o[i] = GAT_SCALED(any ? st.acc[s][i] / st.l[s][i] : 0.f);
      if (L.head_first[s][i]) lse[row * W.H + L.hd[s][i]] = any ? st.m[s][i] + logf(st.l[s][i]) : -__builtin_inff();
    }
    gat_store<VEC>(out + row * ld_out + L.c[s], L.c[s], W.width, o);
  }
}

// CHUNKS: group = slot, the chunk's d xr sum into ws_xr; else group = row: chunk 0, the partials, the self entry; d xr and D
// stored.  Both: the workgroup's d att partial (part == NULL: not wanted).  No thread leaves before the barrier.
template <int S, bool VEC, bool SMALL, class Score, bool CHUNKS>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat_bwd_dst)(const GatWalk W, const Score sc, GAT_DROP_PARAM float* __restrict__ dxr_out, int ld_dxr,
                                                          float* __restrict__ D_out, int64_t slots, float* __restrict__ ws_xr,
                                                          float* __restrict__ part) {
  int64_t g;
  int c;
  group_lane(W.G, g, c);
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  int64_t row = g, p0 = 0, p1 = 0;
  bool active;
  if (CHUNKS) {
    active = g < slots && slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, p0, p1);
  } else {
    active = g < W.n_rows;
    if (active) {
      row_range(W.rowptr, W.n_edges, row, p0, p1);
    }
  }
  f4 dxr[S], datt[S];
#pragma unroll
  for (int s = 0; s < S; ++s) dxr[s] = f4{0.f, 0.f, 0.f, 0.f}, datt[s] = dxr[s];
  if (active) {
    f4 xr[S], att[S], gr[S], o[S], lse[S], D[S], u[S];
    gat_load_row<S, VEC>(xr, W.xr, row, W.ld_xr, L, W.width);
    gat_load_row<S, false>(att, W.att, 0, 0, L, W.width);
    gat_load_row<S, VEC>(gr, W.g, row, W.ld_g, L, W.width);
    gat_load_row<S, VEC>(o, W.out, row, W.ld_out, L, W.width);
    gat_load_heads<S>(lse, W.lse, row, W, L);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = gr[s] * o[s];
    gat_head_sums<S, SMALL>(W, L, u, D);
    const int64_t e1 = CHUNKS ? p1 : min(p0 + ROW_CHUNK, p1);
    int64_t p = p0;
    GAT_DROP_SETUP;
#pragma unroll 1
    for (; p + GAT_AHEAD_BWD <= e1; p += GAT_AHEAD_BWD)
      gat_dst_batch<S, VEC, SMALL, Score, GAT_AHEAD_BWD, true>(dxr, datt, W, L, sc, xr, att, gr, lse, D, p, e1, row, false GAT_MASK);
    if (p < e1)
      gat_dst_batch<S, VEC, SMALL, Score, GAT_AHEAD_BWD - 1, false>(dxr, datt, W, L, sc, xr, att, gr, lse, D, p, e1, row, false GAT_MASK);
    if (CHUNKS) {
#pragma unroll
      for (int s = 0; s < S; ++s) *reinterpret_cast<f4*>(ws_xr + (g * W.V + L.v[s]) * 4) = dxr[s];
    } else {
      int64_t first, n_part;
      row_partials(p0, p1, first, n_part);
#pragma unroll 1
      for (int64_t k = 0; k < n_part; ++k)
#pragma unroll
        for (int s = 0; s < S; ++s) dxr[s] = dxr[s] + *reinterpret_cast<const f4*>(ws_xr + ((first + k) * W.V + L.v[s]) * 4);
      if (W.self_loops) gat_dst_batch<S, VEC, SMALL, Score, 1, true>(dxr, datt, W, L, sc, xr, att, gr, lse, D, 0, 0, row, true GAT_MASK);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (dxr_out != nullptr) gat_store<VEC>(dxr_out + row * ld_dxr + L.c[s], L.c[s], W.width, dxr[s]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (L.head_first[s][i]) D_out[row * W.H + L.hd[s][i]] = D[s][i];
      }
    }
  }
  if (part != nullptr) gat_block_datt<S>(datt, W, L, part);
}

template <int S, bool VEC, bool SMALL, class Score, bool CHUNKS>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat_bwd_src)(const GatWalk W, const Score sc, GAT_DROP_PARAM float* __restrict__ dxl, int ld_dxl,
                                                          int64_t slots, float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(W.G, g, c);
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  int64_t row = g, p0 = 0, p1 = 0;
  if (CHUNKS) {
    if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, p0, p1)) return;
  } else {
    if (g >= W.n_rows) return;
    row_range(W.rowptr, W.n_edges, row, p0, p1);
  }
  f4 xl[S], att[S], acc[S];
  gat_load_row<S, VEC>(xl, W.xl, row, W.ld_xl, L, W.width);
  gat_load_row<S, false>(att, W.att, 0, 0, L, W.width);
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = f4{0.f, 0.f, 0.f, 0.f};
  const int64_t e1 = CHUNKS ? p1 : min(p0 + ROW_CHUNK, p1);
  int64_t p = p0;
  GAT_DROP_SETUP;
#pragma unroll 1
  for (; p + GAT_AHEAD_BWD <= e1; p += GAT_AHEAD_BWD)
    gat_src_batch<S, VEC, SMALL, Score, GAT_AHEAD_BWD, true>(acc, W, L, sc, xl, att, p, e1, row, false GAT_MASK);
  if (p < e1) gat_src_batch<S, VEC, SMALL, Score, GAT_AHEAD_BWD - 1, false>(acc, W, L, sc, xl, att, p, e1, row, false GAT_MASK);
  if (CHUNKS) {
#pragma unroll
    for (int s = 0; s < S; ++s) *reinterpret_cast<f4*>(ws + (g * W.V + L.v[s]) * 4) = acc[s];
    return;
  }
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 1
  for (int64_t k = 0; k < n_part; ++k)
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = acc[s] + *reinterpret_cast<const f4*>(ws + ((first + k) * W.V + L.v[s]) * 4);
  if (W.self_loops) gat_src_batch<S, VEC, SMALL, Score, 1, true>(acc, W, L, sc, xl, att, 0, 0, row, true GAT_MASK);
#pragma unroll
  for (int s = 0; s < S; ++s) gat_store<VEC>(dxl + row * ld_dxl + L.c[s], L.c[s], W.width, acc[s]);
}
