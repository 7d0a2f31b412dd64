// The four kernels of egc_gat.hip, included twice under the macros egc_gat.hip defines around the include: once as NAME_kernel,
// the plain instances -- every macro but the name expands to nothing, so their text is what it always was and their code is
// too --, once as NAME_drop_kernel, which takes egc_gat_dev.h's GatDrop after the walk and hands the mask on as the device
// functions' last argument.  The walk stays a by-value kernel argument of both: its pointers are then known to be
// global ones (behind a reference into an inlined body they become flat accesses).

// workspace: per slot and virtual lane three f4: m, l, acc
template <int S, bool VEC, bool SMALL>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat1_fwd_chunks)(const Gat1Walk W, GAT_DROP_PARAM int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.G, g, c);
  if (g >= slots) return;
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  if (!slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  f4 ad[S];
  gat1_heads<S, SMALL>(ad, W.a_dst, row, W.ld_ad, L);
  GatState<S> st;
  GAT_DROP_SETUP;
  gat1_fwd_entries<S, VEC, SMALL>(st, W, L, ad, s0, s1, row GAT_MASK);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f4* o = reinterpret_cast<f4*>(ws) + (g * W.V + L.v[s]) * 3;
    o[0] = st.m[s], o[1] = st.l[s], o[2] = st.acc[s];
  }
}

template <int S, bool VEC, bool SMALL>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat1_fwd_rows)(const Gat1Walk W, GAT_DROP_PARAM float* __restrict__ out, int ld_out,
                                                            float* __restrict__ lse, const float* __restrict__ ws) {
  int64_t row, p0, p1;
  int c;
  group_lane(W.G, row, c);
  if (row >= W.n_rows) return;
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 ad[S];
  gat1_heads<S, SMALL>(ad, W.a_dst, row, W.ld_ad, L);
  GatState<S> st;
  GAT_DROP_SETUP;
  gat1_fwd_entries<S, VEC, SMALL>(st, W, L, ad, p0, min(p0 + ROW_CHUNK, p1), row GAT_MASK);
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
  if (W.self_loops) gat1_fwd_batch<S, VEC, SMALL, 1, true>(st, W, L, ad, 0, 0, row, true GAT_MASK);
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

// CHUNKS: group = slot, the chunk's (v, t) into ws; else group = row: chunk 0, the partials, the self entry; then D into D_out
// and, when wanted, d a_dst.  Workspace: per slot and virtual lane two f4: v, t.
template <int S, bool VEC, bool SMALL, bool CHUNKS>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat1_bwd_dst)(const Gat1Walk W, GAT_DROP_PARAM float* __restrict__ d_ad, int ld_d_ad,
                                                           float* __restrict__ D_out, int64_t slots, float* __restrict__ ws) {
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
  f4 ad[S], lse[S], va[S], ta[S];
  gat1_heads<S, SMALL>(ad, W.a_dst, row, W.ld_ad, L);
  gat1_heads<S, SMALL>(lse, W.lse, row, W.H, L);
#pragma unroll
  for (int s = 0; s < S; ++s) va[s] = f4{0.f, 0.f, 0.f, 0.f}, ta[s] = va[s];
  const int64_t e1 = CHUNKS ? p1 : min(p0 + ROW_CHUNK, p1);
  int64_t p = p0;
  GAT_DROP_SETUP;
#pragma unroll 1
  for (; p + GAT1_AHEAD_DST <= e1; p += GAT1_AHEAD_DST)
    gat1_dst_batch<S, VEC, SMALL, GAT1_AHEAD_DST, true>(va, ta, W, L, ad, lse, p, e1, row, false GAT_MASK);
  if (p < e1) gat1_dst_batch<S, VEC, SMALL, GAT1_AHEAD_DST - 1, false>(va, ta, W, L, ad, lse, p, e1, row, false GAT_MASK);
  if (CHUNKS) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      f4* o = reinterpret_cast<f4*>(ws) + (g * W.V + L.v[s]) * 2;
      o[0] = va[s], o[1] = ta[s];
    }
    return;
  }
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 1
  for (int64_t k = 0; k < n_part; ++k)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f4* o = reinterpret_cast<const f4*>(ws) + ((first + k) * W.V + L.v[s]) * 2;
      va[s] = va[s] + o[0], ta[s] = ta[s] + o[1];
    }
  if (W.self_loops) gat1_dst_batch<S, VEC, SMALL, 1, true>(va, ta, W, L, ad, lse, 0, 0, row, true GAT_MASK);
  f4 gr[S], o[S], u[S], D[S], P[S];
  gat_load_row<S, VEC>(gr, W.g, row, W.ld_g, L, W.width);
  gat_load_row<S, VEC>(o, W.out, row, W.ld_out, L, W.width);
#pragma unroll
  for (int s = 0; s < S; ++s) u[s] = gr[s] * o[s];
  gat_head_sums<S, SMALL>(W, L, u, D);
  gat1_store_heads<S>(D_out, row, W.H, L, D);
  if (d_ad == nullptr) return;
#pragma unroll
  for (int s = 0; s < S; ++s) u[s] = gr[s] * va[s];
  gat_head_sums<S, SMALL>(W, L, u, P);
#pragma unroll
  for (int s = 0; s < S; ++s) P[s] = P[s] - D[s] * ta[s];
  gat1_store_heads<S>(d_ad, row, ld_d_ad, L, P);
}

// workspace: per slot and virtual lane two f4: d xl, d a_src (the head's value in every column of the head)
template <int S, bool VEC, bool SMALL, bool CHUNKS>
__global__ void __launch_bounds__(256) GAT_KERNEL(gat1_bwd_src)(const Gat1Walk W, GAT_DROP_PARAM float* __restrict__ dxl, int ld_dxl,
                                                           float* __restrict__ d_as, int ld_d_as, int want_das_, int64_t slots,
                                                           float* __restrict__ ws) {
  int64_t g;
  int c;
  group_lane(W.G, g, c);
  const GatLane<S> L = gat_lane<S>(W, c / 4);
  const bool want_das = want_das_ != 0;
  int64_t row = g, p0 = 0, p1 = 0;
  if (CHUNKS) {
    if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, p0, p1)) return;
  } else {
    if (g >= W.n_rows) return;
    row_range(W.rowptr, W.n_edges, row, p0, p1);
  }
  f4 as[S], xl[S], dx[S], sa[S];
  gat1_heads<S, SMALL>(as, W.a_src, row, W.ld_as, L);
  gat_load_row<S, VEC>(xl, W.xl, row, W.ld_xl, L, W.width);
#pragma unroll
  for (int s = 0; s < S; ++s) dx[s] = f4{0.f, 0.f, 0.f, 0.f}, sa[s] = dx[s];
  const int64_t e1 = CHUNKS ? p1 : min(p0 + ROW_CHUNK, p1);
  int64_t p = p0;
  GAT_DROP_SETUP;
#pragma unroll 1
  for (; p + GAT1_AHEAD_SRC <= e1; p += GAT1_AHEAD_SRC)
    gat1_src_batch<S, VEC, SMALL, GAT1_AHEAD_SRC, true>(dx, sa, W, L, as, xl, want_das, p, e1, row, false GAT_MASK);
  if (p < e1) gat1_src_batch<S, VEC, SMALL, GAT1_AHEAD_SRC - 1, false>(dx, sa, W, L, as, xl, want_das, p, e1, row, false GAT_MASK);
  if (CHUNKS) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      f4* o = reinterpret_cast<f4*>(ws) + (g * W.V + L.v[s]) * 2;
      o[0] = dx[s], o[1] = sa[s];
    }
    return;
  }
  int64_t first, n_part;
  row_partials(p0, p1, first, n_part);
#pragma unroll 1
  for (int64_t k = 0; k < n_part; ++k)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f4* o = reinterpret_cast<const f4*>(ws) + ((first + k) * W.V + L.v[s]) * 2;
      dx[s] = dx[s] + o[0], sa[s] = sa[s] + o[1];
    }
  if (W.self_loops) gat1_src_batch<S, VEC, SMALL, 1, true>(dx, sa, W, L, as, xl, want_das, 0, 0, row, true GAT_MASK);
  if (dxl != nullptr) {
#pragma unroll
    for (int s = 0; s < S; ++s) gat_store<VEC>(dxl + row * ld_dxl + L.c[s], L.c[s], W.width, dx[s]);
  }
  if (d_as != nullptr) gat1_store_heads<S>(d_as, row, ld_d_as, L, sa);
}
