// Batches of small graphs (BASELINE configs 1 / 3 / 4), the WHOLE layer in one launch: for a tile of whole graphs
//
//     x rows -> fp16x2 planes -> [bases | weightings] on the matrix cores -> LDS -> CSR of the tile's edges in LDS ->
//     multi-aggregator reduction from LDS -> per-head combine -> (+ bias, BatchNorm(eval) / ReLU / residual) -> out
//
// A tile of whole graphs is closed under "in-neighbour of": neither `bases` nor `weightings` ever exist in memory, the
// launch reads x and the edge list once and writes `out` once (SURVEY.md section 8 f2 + f3).  Reference call sites replaced:
// torch.matmul(x, bases_weight) and comb_weight(x) (layers.py:97-101,110; optimized_layers.py:180-182), gcn_norm /
// add_remaining_self_loops (optimized_layers.py:127-175), MessagePassing.propagate + the per-aggregator scatters
// (optimized_layers.py:186-249; layers.py:165-219), the bmm / broadcast combine and bias (optimized_layers.py:195-208;
// layers.py:127-138) and the callers' BatchNorm(eval) / ReLU / residual tail (zinc/models.py:66-73, cifar/models.py:64-71).
//
// Workgroup = 16 wavefronts, ONE per CU (the LDS image of a tile is what limits it), persistent over its share of the
// batch:
//   plan   inside the launch: workgroup b owns the graphs whose first node lies in [b N / nWG, (b + 1) N / nWG) (two
//          64-ary searches in the graph offsets, once); its tiles are greedy runs of those graphs of at most `tcap` nodes,
//          found one tile ahead by wavefront 15 (edge range: the caller's edge offsets, else two searches in the
//          destination row) -- no plan launch, no tile list in memory.
//   GEMM   wavefronts 0-11 each keep ONE 16-column tile of the packed weight planes (k = 128, two fp16 planes: 32 VGPRs)
//          for the whole launch; wavefronts 12-15 fetch x in 16-row chunks (FT_DEPTH chunks in flight, registers), split
//          every row into the two fp16 planes (row scale = power of two, egc_gemm_f16x2.hip's scheme) and stage them in a
//          two-deep LDS ring whose 16-byte pieces are XOR-swizzled by the row (conflict-free A-operand reads without
//          padding); v_mfma_f32_16x16x32_f16, three products per k-step (xh wh, xl wh, xh wl), fp32 accumulate; the D tile
//          is scaled, biased, passed through the weight nonlinearity and written to the LDS image of the tile:
//          bases [T][ldb] and weightings [T][H B 4].
//   CSR    as egc_aggregate_tile.hip: in-degrees by LDS atomics, wavefront scan, scatter; both deg^-1/2 tables.
//   rows   one lane group per row, neighbours gathered from LDS, register epilogue of the fast kernel family
//          (finish_group, weightings read from the LDS image).
// Tiles beyond the LDS image (a single graph with more than `tcap` nodes, more than `emax` edges) and edges that leave
// their tile raise *status and the sticky host flag; the host routes batches whose declared largest graph exceeds the
// capacity to the two-launch path.
#include "egc_pack_map.h"
#include "egc_aggregate_host.h"
#include "egc_fused_tile_dev.h"

namespace egc {

// The packed operands (FtPacked, egc_fused_tile_host.h).  Column scales and the two planes as pack_f16x2_kernel (egc_gemm_f16x2.hip).
// (the operand's source: wcat [K][F_g + W] + bcat [W], or -- FtParamSrc -- the layer's parameters through the pack's index map)
struct FtWcatSrc {
  const float* wcat;
  const float* bcat;
  int ncol;
  __device__ inline float w(int k, int c) const { return wcat[(int64_t)k * ncol + c]; }
  __device__ inline float b(int j) const { return bcat != nullptr ? bcat[j] : 0.f; }
};
struct FtParamSrc {
  PackPtrs bases;
  const float* comb_w;
  const float* comb_b;      // the combination Linear's bias (its rows permuted as the weight's), or nullptr
  const float* bcat;        // or a bias already in the operand's order, or nullptr
  PackDims d;
  __device__ inline float w(int k, int c) const {
    const float* p = pack_param_ptr(bases, const_cast<float*>(comb_w), d, k, c);
    return p != nullptr ? *p : 0.f;
  }
  __device__ inline float b(int j) const { return comb_b != nullptr ? comb_b[pack_comb_row(d, j)] : (bcat != nullptr ? bcat[j] : 0.f); }
};
// One virtual column v of a forward operand, by one wavefront: [bases 0 .. F_g) | zero columns up to wcol0 | weightings wcol0 ..
// wcol0 + W) | zero columns.  TW = 16: the narrow form (wcol0 = ldb); TW = 32: the WIDE form (wcol0 = ldbp).
template <int TW, class S>
__device__ inline void ft_pack_column(int v, const S& src_of, const FtPacked lay, int K, int F_g, int W, int wcol0,
                                      u16* __restrict__ packed) {
  const int lane = threadIdx.x;
  const int src = (v < F_g) ? v : ((v < wcol0 || v >= wcol0 + W) ? -1 : v - wcol0 + F_g);
  unsigned amax = 0;
  if (src >= 0)
    for (int k = lane; k < K; k += 64) amax = max(amax, __float_as_uint(src_of.w(k, src)) & 0x7fffffffu);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, d));
  const F16x2ColScale col = f16x2_col_scale(amax);
  for (int k = lane; k < lay.k_rows(); k += 64) {
    const F16x2Bits b = f16x2_pack_split((src >= 0 && k < K) ? src_of.w(k, src) * col.scale : 0.f);
    const int64_t base = ft_frag_index<TW>(v, k, lay.ksteps);
    packed[base] = b.h;
    packed[base + FT_FRAG] = b.l;
  }
  if (lane == 0) {
    float* tail = reinterpret_cast<float*>(packed + lay.tail_at());
    tail[v] = col.inv;
    const int wcol = v - wcol0;
    tail[lay.bias_at + v] = (wcol >= 0 && wcol < W) ? src_of.b(wcol) : 0.f;
  }
}
__global__ void __launch_bounds__(64) ft_pack_kernel(const float* __restrict__ wcat, const float* __restrict__ bcat, int K,
                                                      int F_g, int W, int ldb, u16* __restrict__ packed) {
  ft_pack_column<16>(blockIdx.x, FtWcatSrc{wcat, bcat, F_g + W}, ft_packed_narrow(), K, F_g, W, ldb, packed);
}
__global__ void __launch_bounds__(64) ft_pack_wide_kernel(const float* __restrict__ wcat, const float* __restrict__ bcat, int K,
                                                           int F_g, int W, int ldbp, FtPacked lay, u16* __restrict__ packed) {
  ft_pack_column<32>(blockIdx.x, FtWcatSrc{wcat, bcat, F_g + W}, lay, K, F_g, W, ldbp, packed);
}

// ---------------------------------------------------------------------------------------------
// host side: the plan (egc_fused_tile_host.h) of a layer, and what follows it
// ---------------------------------------------------------------------------------------------
FtPlan fused_tile_plan(const AggArgs& a, int f_in, bool with_post, bool bwd) {
  FtLayer l = {a.H, a.B, a.A, a.L, a.Ls, a.ldb, a.slots, a.W, a.act, {}, f_in, with_post};
  for (int t = 0; t < EGC_MAX_AGGRS; ++t) l.aggr[t] = a.aggr[t];
  return bwd ? ftb_plan(l) : ft_plan(l);
}

int fused_tile_pack(const FtPlan& p, const AggArgs& a, const float* wcat, const float* bcat, int f_in, void* packed, hipStream_t stream) {
  if (p.form == FT_FORM_NONE) return EGC_ERR_UNSUPPORTED;
  const int f_g = a.B * a.Ls;
  if (p.form == FT_FORM_NARROW) {
    ft_pack_kernel<<<p.packed.columns(), 64, 0, stream>>>(wcat, bcat, f_in, f_g, a.W, a.ldb, (u16*)packed);
    EGC_LAUNCH_CHECK("ft_pack_kernel");
    return EGC_OK;
  }
  ft_pack_wide_kernel<<<p.packed.columns(), 64, 0, stream>>>(wcat, bcat, f_in, f_g, a.W, p.ldbp, p.packed, (u16*)packed);
  EGC_LAUNCH_CHECK("ft_pack_wide_kernel");
  return EGC_OK;
}

// What both directions of the one-launch kernel hand it: AggArgs' share (the lane geometry of a row, the bias strip; the
// weight strip of a lane group IS the row of the LDS image it is handed -- finish_group<W_READY> -- so there is none per
// wavefront) ...
static int ft_row_args(AggArgs& a, const FtPlan& p, bool with_post) {
  agg_lane_geometry(a);
  const int need = agg_need(a);
  agg_lds_strips(a, 0, with_post);
  a.w_lds_stride = 0;
  a.lds_floats_per_wave = 0;
  a.w_aw = p.w_aw;
  return need;
}

// ... and FusedTileArgs': the batch, the plan's fields, the LDS image.
static void ft_tile_args(FusedTileArgs& t, const FtPlan& p, const FtLds& L, const int64_t* ptr, const int64_t* edge_ptr, int64_t n_graphs,
                         const int64_t* src, const int64_t* dst, int64_t n_edges, const int* max_index, const float* x, int f_in,
                         const void* packed, int tcap, int emax, int32_t* status, int32_t* host_flag) {
  t = FusedTileArgs{};
  t.ptr = ptr; t.edge_ptr = edge_ptr; t.n_graphs = n_graphs; t.src = src; t.dst = dst; t.n_edges = n_edges;
  t.max_index = max_index; t.status = status; t.host_flag = host_flag; t.x = x; t.packed = (const u16*)packed;
  t.F_in = f_in;
  t.n_ct = p.n_ct;
  t.tcap = tcap; t.emax = emax;
  t.w_aw = p.w_aw;
  t.wl_floats = p.wl_floats;
  t.nsets = p.nsets;
  t.off_rec = L.off_rec; t.off_planes = L.off_planes; t.off_rowinv = L.off_rowinv; t.off_bases = L.off_bases; t.off_wt = L.off_wt;
  t.off_col = L.off_col; t.off_rowptr = L.off_rowptr; t.off_cnt = L.off_cnt; t.off_dis = L.off_dis; t.csr_stride = L.csr_stride;
  t.off_db = L.off_db; t.off_rowinv2 = L.off_rowinv2;     // (backward form; 0 in the forward's image)
  if (p.bwd) return;
  // WIDE form: the k-slabs of x and the streamed weight fragments; rows of more than 64 slots: the first pass's share of a basis
  t.n_slabs = p.n_slabs; t.k16 = p.k16; t.ldbp = p.ldbp;
  t.p0 = p.p0; t.magic0 = p.magic0; t.magic1 = p.magic1;
}

template <int LPR_LOG2, int HPB, int NEED, class C>
static int launch_ft_one(const AggArgs& a, const FusedTileArgs& t, unsigned grid, size_t lds, hipStream_t stream) {
  const auto kern = &fused_tile_kernel<LPR_LOG2, HPB, NEED, C>;
  EGC_ALLOW_DYNAMIC_LDS(kern, 160 * 1024, "fused_tile_kernel");
  kern<<<grid, FT_THREADS, lds, stream>>>(a, t);
  EGC_LAUNCH_CHECK("fused_tile_kernel");
  return EGC_OK;
}

int launch_fused_tile(AggArgs a, const int64_t* ptr, const int64_t* edge_ptr, int64_t n_graphs, const int64_t* src,
                      const int64_t* dst, int64_t n_edges, const int* max_index, const float* x, int f_in, const void* packed,
                      int tcap, int emax, int32_t* status, int32_t* host_flag, hipStream_t stream) {
  const bool with_post = a.post_scale != nullptr;
  const FtPlan p = fused_tile_plan(a, f_in, with_post, false);
  FtLds L;
  const int ok = ft_tile_ok(p, tcap, emax, &L);
  if (ok != EGC_OK) return ok;
  const FtSwitches sw = ft_switches();
  const int need = ft_row_args(a, p, with_post);
  FusedTileArgs t;
  ft_tile_args(t, p, L, ptr, edge_ptr, n_graphs, src, dst, n_edges, max_index, x, f_in, packed, tcap, emax, status, host_flag);
  const unsigned grid = ft_grid(sw, n_graphs, a.n_nodes);
  if (p.form == FT_FORM_WIDE) {
    switch (p.n_slabs) {
      case 1: return launch_fused_tile_wide1(a, t, need, sw, grid, L.total, stream);
      case 2: return launch_fused_tile_wide2(a, t, need, sw, grid, L.total, stream);
      default: return launch_fused_tile_wide3(a, t, need, sw, grid, L.total, stream);
    }
  }
  // the d = 128 layers with their constants compiled in (contiguous bases): 16-lane groups, two heads per lane
  if (sw.static_cfg && a.Ls == a.L) {
    if (cfg_matches<cfg::EGConvM128>(a)) return launch_ft_one<4, 2, 0, cfg::EGConvM128>(a, t, grid, L.total, stream);
    if (cfg_matches<cfg::EgcM128>(a)) return launch_ft_one<4, 2, 0, cfg::EgcM128>(a, t, grid, L.total, stream);
  }
  return agg_dispatch<NeedCoarse>(a, need, [&](auto lpr, auto hpb, auto nd) {
    return launch_ft_one<decltype(lpr)::value, decltype(hpb)::value, decltype(nd)::value, RtCfg>(a, t, grid, L.total, stream);
  });
}


// ---------------------------------------------------------------------------------------------
// The BACKWARD of the layer on batches of whole graphs, tile-local (fused_tile_kernel<..., MODE = 1>).  What autograd derives
// through layers.py:89-140 / optimized_layers.py:177-210 for a PyG batch -- in the reference: the backward of two Linears, of
// propagate's gathers and of the per-aggregator scatters -- as ONE launch per layer plus the weight gradient x^T d:
//   x rows -> [bases | w'] on the matrix cores -> LDS (as the forward) -> CSR of the tile -> per destination row the
//   aggregates again (with the entry attaining each maximum), d w' = <g, agg>, d agg = w' g, scattered to the sources' rows
//   of a d bases image kept as 64-bit fixed point (integer LDS atomics: order-independent sums) -> d x = [d bases | d w'] [bases_weight | comb_weight^T]^T on the matrix cores.
// x, grad_out and the edge list in; d x and d_cat = the gradient of [bases | pre-activation weightings] out.  No CSR, no
// transposed CSR, no `bases` / `weightings` / statistics in memory.  Envelope: the d = 128 / 64 layers (B = 4 bases of 16
// channels, H = 4 or 8, F_in <= 128), aggregators of sum / mean / max / symnorm, no weight nonlinearity.
// ---------------------------------------------------------------------------------------------
// The transposed operand (ft_packed_t): the B operand of d x = d W^T -- output feature f's fragments hold W[f][k], where k runs over
// the LDS images' columns: [d bases 0 .. ldb) | d w' as [h][b][4] (a = 0 .. A - 1 real, the rest zero), zero from k2 on.  Scale per
// output feature f; tail: float col_inv[128].
template <class S>
__device__ inline void ft_pack_t_feature(int f, const S& src_of, int K, int F_g, int W, int A, int ldb, int k2,
                                         u16* __restrict__ packed) {
  constexpr FtPacked lay = ft_packed_t();
  const int lane = threadIdx.x;       // f: output feature (row of wcat), 0 .. 127
  auto src_col = [&](int k) -> int {  // image column k -> column of wcat, or -1
    if (k < ldb) return k < F_g ? k : -1;
    const int j = k - ldb, hb = j >> 2, aa = j & 3;
    return (aa < A && hb * A + aa < W) ? F_g + hb * A + aa : -1;
  };
  unsigned amax = 0;
  if (f < K)
    for (int k = lane; k < k2; k += 64) {
      const int c = src_col(k);
      if (c >= 0) amax = max(amax, __float_as_uint(src_of.w(f, c)) & 0x7fffffffu);
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, d));
  const F16x2ColScale col = f16x2_col_scale(amax);
  for (int k = lane; k < lay.k_rows(); k += 64) {
    const int c = k < k2 ? src_col(k) : -1;
    const F16x2Bits b = f16x2_pack_split((f < K && c >= 0) ? src_of.w(f, c) * col.scale : 0.f);
    const int64_t base = ft_frag_index<16>(f, k, lay.ksteps);
    packed[base] = b.h;
    packed[base + FT_FRAG] = b.l;
  }
  if (lane == 0) reinterpret_cast<float*>(packed + lay.tail_at())[f] = col.inv;
}
__global__ void __launch_bounds__(64) ft_pack_t_kernel(const float* __restrict__ wcat, int K, int F_g, int W, int A, int ldb,
                                                        int k2, u16* __restrict__ packed) {
  ft_pack_t_feature(blockIdx.x, FtWcatSrc{wcat, nullptr, F_g + W}, K, F_g, W, A, ldb, k2, packed);
}
// both operands of a training step in one launch: the first blocks the forward's columns, the rest the backward's features
template <class S>
__device__ inline void ft_pack_both(const S& src, int K, int F_g, int W, int A, int ldb, int k2, u16* __restrict__ packed,
                                    u16* __restrict__ packed_t) {
  constexpr int NV = ft_packed_narrow().columns();
  if (blockIdx.x < NV) ft_pack_column<16>(blockIdx.x, src, ft_packed_narrow(), K, F_g, W, ldb, packed);
  else ft_pack_t_feature(blockIdx.x - NV, src, K, F_g, W, A, ldb, k2, packed_t);
}
__global__ void __launch_bounds__(64) ft_pack_both_kernel(const float* __restrict__ wcat, const float* __restrict__ bcat, int K,
                                                           int F_g, int W, int A, int ldb, int k2, u16* __restrict__ packed,
                                                           u16* __restrict__ packed_t) {
  ft_pack_both(FtWcatSrc{wcat, bcat, F_g + W}, K, F_g, W, A, ldb, k2, packed, packed_t);
}
// ... straight from the layer's parameters (no wcat / bcat arrays, no egc_weights_pack_f32 launch in front)
__global__ void __launch_bounds__(64) ft_pack_both_params_kernel(FtParamSrc src, int K, int F_g, int W, int A, int ldb, int k2,
                                                                  u16* __restrict__ packed, u16* __restrict__ packed_t) {
  ft_pack_both(src, K, F_g, W, A, ldb, k2, packed, packed_t);
}

// (pb: the layer's backward plan -- a training step's forward operand is the narrow one)
int fused_tile_bwd_pack(const FtPlan& pb, const AggArgs& a, const float* wcat, int f_in, void* packed_t, hipStream_t stream) {
  if (pb.form == FT_FORM_NONE) return EGC_ERR_UNSUPPORTED;
  ft_pack_t_kernel<<<pb.packed_t.columns(), 64, 0, stream>>>(wcat, f_in, a.B * a.Ls, a.W, a.A, a.ldb, pb.k2, (u16*)packed_t);
  EGC_LAUNCH_CHECK("ft_pack_t_kernel");
  return EGC_OK;
}

int fused_tile_train_pack(const FtPlan& pb, const AggArgs& a, const float* wcat, const float* bcat, int f_in, void* packed, void* packed_t,
                          hipStream_t stream) {
  if (pb.form == FT_FORM_NONE) return EGC_ERR_UNSUPPORTED;
  ft_pack_both_kernel<<<pb.packed.columns() + pb.packed_t.columns(), 64, 0, stream>>>(wcat, bcat, f_in, a.B * a.Ls, a.W, a.A, a.ldb, pb.k2,
                                                                                      (u16*)packed, (u16*)packed_t);
  EGC_LAUNCH_CHECK("ft_pack_both_kernel");
  return EGC_OK;
}

int fused_tile_train_pack_params(const FtPlan& pb, const AggArgs& a, const PackPtrs& bases, const float* comb_w, const float* comb_b,
                                 const float* bcat, const PackDims& d, void* packed, void* packed_t, hipStream_t stream) {
  if (pb.form == FT_FORM_NONE) return EGC_ERR_UNSUPPORTED;
  FtParamSrc src{bases, comb_w, comb_b, bcat, d};
  ft_pack_both_params_kernel<<<pb.packed.columns() + pb.packed_t.columns(), 64, 0, stream>>>(src, d.F_in, a.B * a.Ls, a.W, a.A, a.ldb, pb.k2,
                                                                                             (u16*)packed, (u16*)packed_t);
  EGC_LAUNCH_CHECK("ft_pack_both_params_kernel");
  return EGC_OK;
}

template <class C>
static int launch_ftb_one(const AggArgs& a, const FusedTileArgs& t, unsigned grid, size_t lds, hipStream_t stream) {
  const auto kern = &fused_tile_kernel<4, 1, 0, C, 0, 1>;
  EGC_ALLOW_DYNAMIC_LDS(kern, 160 * 1024, "fused_tile_kernel, backward");
  kern<<<grid, FT_THREADS, lds, stream>>>(a, t);
  EGC_LAUNCH_CHECK("fused_tile_kernel (backward)");
  return EGC_OK;
}

int launch_fused_tile_bwd(AggArgs a, const int64_t* ptr, const int64_t* edge_ptr, int64_t n_graphs, const int64_t* src,
                          const int64_t* dst, int64_t n_edges, const int* max_index, const float* x, int f_in, const void* packed,
                          const void* packed_t, const float* grad_out, float* d_x, const float* d_x_add, float* d_cat, int ld_dcat, int tcap, int emax,
                          int32_t* status, int32_t* host_flag, hipStream_t stream) {
  const FtPlan p = fused_tile_plan(a, f_in, false, true);
  FtLds L;
  const int ok = ft_tile_ok(p, tcap, emax, &L);
  if (ok != EGC_OK) return ok;
  const FtSwitches sw = ft_switches();
  // (the envelope -- Ls == 16, no var / std / min -- makes the shared derivations give lpb_log2 == 2, need_var == 0 and an
  // empty need mask: the one instance family the backward has)
  ft_row_args(a, p, false);
  FusedTileArgs t;
  ft_tile_args(t, p, L, ptr, edge_ptr, n_graphs, src, dst, n_edges, max_index, x, f_in, packed, tcap, emax, status, host_flag);
  t.grad_out = grad_out; t.d_x = d_x; t.d_x_add = d_x_add; t.d_cat = d_cat; t.ld_dcat = ld_dcat; t.packed_t = (const u16*)packed_t;
  const unsigned grid = ft_grid(sw, n_graphs, a.n_nodes);
  if (sw.static_cfg && a.Ls == a.L) {
    // the row pass is bound by its vector instructions: with the layer's constants compiled in the aggregator switches, the
    // head count and the edge-set tests fold away (the run-time form is 2,000 instructions per turn, a quarter of them moves)
    if (cfg_matches<cfg::EGConvM128>(a)) return launch_ftb_one<cfg::EGConvM128>(a, t, grid, L.total, stream);
    if (cfg_matches<cfg::EgcM128>(a)) return launch_ftb_one<cfg::EgcM128>(a, t, grid, L.total, stream);
  }
  return launch_ftb_one<RtCfg>(a, t, grid, L.total, stream);
}

}  // namespace egc
