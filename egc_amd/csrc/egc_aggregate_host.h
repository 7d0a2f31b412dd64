// Host side of the register-resident aggregate kernel families: what every launcher (egc_aggregate_fast.hip,
// egc_aggregate_tile.hip, egc_fused_tile.hip, egc_fused_tile_wide.inc) and every capacity query (egc_aggregate.hip) derives from
// an egc_layer before it can launch -- the layer-static fields of AggArgs, the lane geometry of a row, the need mask, the
// per-wavefront LDS strips, the template-instance ladder and the matching of a layer against a compiled-in configuration.  One
// definition each: a capacity query and its launch cannot disagree about LDS, and a change to the row schedule lands once.
// (What only the one-launch batch kernel needs -- its forms, tile range, LDS image, packed operands, grid and switches -- is
// egc_fused_tile_host.h's; agg_magic and the bias strip's size, which that HIP-free header shares with this one, are egc_plain.h's.)
#pragma once
#include <type_traits>

#include "egc_aggregate_fast_dev.h"

namespace egc {

// The fields of AggArgs that are a function of the layer alone (ldw: a plain weightings array; callers with a strided one
// overwrite it).  magic_L and lpr_log2 belong to the generic kernels of egc_aggregate.hip and stay with that path.
inline void agg_layer_fields(const egc_layer* layer, AggArgs& a) {
  a.ldb = egc_bases_ld(layer);
  a.slots = a.ldb / 4;
  a.F_out = layer->out_channels;
  a.H = layer->num_heads;
  a.B = layer->num_bases;
  a.A = layer->num_aggrs;
  a.L = layer->out_channels / layer->num_heads;
  a.Ls = layer_basis_stride(layer);
  a.W = a.H * a.B * a.A;
  a.ldw = a.W;
  for (int t = 0; t < EGC_MAX_AGGRS; ++t) a.aggr[t] = t < a.A ? layer->aggrs[t] : 0;
  a.x_looped = layer->agg_set == EGC_SET_LOOPED;
  a.y_looped = layer->sym_set == EGC_SET_LOOPED;
  a.loops_all = layer->loops_all_nodes != 0;
  if (layer->weight_layout == EGC_LAYOUT_HAB) { a.sa = a.B; a.sb = 1; } else { a.sa = 1; a.sb = a.A; }
  a.act = layer->weight_act;
}

// the caller-side epilogue fused into the store (egc_post; nullptr = none)
inline void agg_set_post(AggArgs& a, const egc_post* post) {
  a.post_scale = post != nullptr ? post->scale : nullptr;
  a.post_shift = post != nullptr ? post->shift : nullptr;
  a.residual = post != nullptr ? post->residual : nullptr;
  a.post_relu = post != nullptr && post->relu != 0;
}

// Lanes per basis: shifts and an xor butterfly when their number is a power of two (lpb_log2 >= 0), else a division by
// multiplication (magic_P) and a rotation butterfly.  `lanes_pb` is Ls / 4 but for the two-slots-per-lane kernel's sets.
inline void agg_lane_geometry(AggArgs& a, int lanes_pb) {
  a.lanes_pb = lanes_pb;
  a.magic_P = agg_magic(lanes_pb);
  a.lpb_log2 = -1;
  if ((lanes_pb & (lanes_pb - 1)) == 0) {
    int lg = 0;
    while ((1 << lg) < lanes_pb) ++lg;
    a.lpb_log2 = lg;
  }
}
inline void agg_lane_geometry(AggArgs& a) { agg_lane_geometry(a, a.Ls / 4); }

// Which optional running aggregates the layer needs: sets need_mean / need_var, returns the NEED_* mask of the kernel template.
inline int agg_need(AggArgs& a) {
  a.need_mean = a.need_var = 0;
  int need = 0;
  for (int t = 0; t < a.A; ++t) {
    if (a.aggr[t] == EGC_AGGR_MEAN || a.aggr[t] == EGC_AGGR_VAR || a.aggr[t] == EGC_AGGR_STD) a.need_mean = 1;
    if (a.aggr[t] == EGC_AGGR_VAR || a.aggr[t] == EGC_AGGR_STD) { a.need_var = 1; need |= NEED_SQ; }
    if (a.aggr[t] == EGC_AGGR_MIN) need |= NEED_MN;
  }
  return need;
}

// Per-wavefront LDS of the epilogue: the bias strip in the (padded) head layout [h][Ls] (>= F_out floats), a second strip with
// the scale when a post-op is fused, and one weightings strip per lane group of the wavefront.
inline int agg_bias_floats(const AggArgs& a) { return bias_strip_floats(a.H, a.Ls); }
inline int agg_w_strip_floats(const AggArgs& a) { return (a.W + 3) & ~3; }
inline int agg_strip_floats(const AggArgs& a, int groups_per_wave, bool with_post) {
  return (with_post ? 2 : 1) * agg_bias_floats(a) + groups_per_wave * agg_w_strip_floats(a);
}
inline void agg_lds_strips(AggArgs& a, int groups_per_wave, bool with_post) {
  a.w_lds_stride = agg_w_strip_floats(a);
  a.bias_lds_floats = agg_bias_floats(a);
  a.lds_floats_per_wave = agg_strip_floats(a, groups_per_wave, with_post);
}

// aggregator codes, 3 bits each, first aggregator in the low bits: the run-time value of StCfg's AGG (agg_pack)
inline unsigned agg_packed_code(const AggArgs& a) { return pack_aggr_codes(a.aggr, a.A); }

// lanes of the group a row occupies: the power of two >= slots, at least 16 (rows of more than 64 slots: two passes of 64)
constexpr int agg_lpr(int slots) { return slots <= 16 ? 16 : slots <= 32 ? 32 : 64; }
constexpr int agg_lpr_log2(int slots) { return slots <= 16 ? 4 : slots <= 32 ? 5 : 6; }
// heads a lane finishes: ceil(H / B)
inline int agg_hpb(const AggArgs& a) { return (a.H + a.B - 1) / a.B; }

// ---------------------------------------------------------------------------------------------
// The run-time (RtCfg) instance ladder: f(int_c<HPB>, int_c<NEED>) with HPB in {1, 2, 4}, and, per kernel family, the need
// masks it is compiled for -- nothing else is ever instantiated:
//   NeedCoarse  {0, NEED_SQ | NEED_MN}: the wide-rows, tile and one-launch kernels
//   NeedFine    {0, NEED_SQ, NEED_MN, NEED_SQ | NEED_MN}, and {NEED_ARG, NEED_SQ | NEED_MN | NEED_ARG} for the training forward
//               of a layer with max / min: the fast kernel (squares without min and min without squares are kernels of their own:
//               either accumulator alone leaves room for a fifth wavefront per SIMD -- DESIGN.md 3.1)
// agg_dispatch adds the lane-group size in front: f(int_c<LPR_LOG2>, int_c<HPB>, int_c<NEED>).
// ---------------------------------------------------------------------------------------------
template <int V>
using int_c = std::integral_constant<int, V>;
enum NeedSet { NeedCoarse, NeedFine };

template <NeedSet SET, class F>
int agg_dispatch_rows(const AggArgs& a, int need, F&& f) {
  auto by_need = [&](auto hpb) {
    if constexpr (SET == NeedFine) {
      if (a.arg_max != nullptr || a.arg_min != nullptr) {
        if (need == 0) return f(hpb, int_c<NEED_ARG>{});
        return f(hpb, int_c<NEED_SQ | NEED_MN | NEED_ARG>{});
      }
      if (need == NEED_SQ) return f(hpb, int_c<NEED_SQ>{});
      if (need == NEED_MN) return f(hpb, int_c<NEED_MN>{});
    }
    if (need == 0) return f(hpb, int_c<0>{});
    return f(hpb, int_c<NEED_SQ | NEED_MN>{});
  };
  const int hpb = agg_hpb(a);
  if (hpb <= 1) return by_need(int_c<1>{});
  if (hpb <= 2) return by_need(int_c<2>{});
  return by_need(int_c<4>{});
}

template <NeedSet SET, class F>
int agg_dispatch(const AggArgs& a, int need, F&& f) {
  switch (agg_lpr(a.slots)) {
    case 16: return agg_dispatch_rows<SET>(a, need, [&](auto hpb, auto nd) { return f(int_c<4>{}, hpb, nd); });
    case 32: return agg_dispatch_rows<SET>(a, need, [&](auto hpb, auto nd) { return f(int_c<5>{}, hpb, nd); });
    default: return agg_dispatch_rows<SET>(a, need, [&](auto hpb, auto nd) { return f(int_c<6>{}, hpb, nd); });
  }
}

// ---------------------------------------------------------------------------------------------
// Compiled-in configurations: a layer runs the StCfg instance whose constants it equals.  cfg_layer_matches compares what shapes
// the kernel (heads, bases, basis length and stride, aggregator list, nonlinearity, the aggregators' edge set); cfg_matches also
// the symnorm edge set and loops_all.  A table adds its own conditions (lane-group size, Ls == L, ...) next to its entries.
// ---------------------------------------------------------------------------------------------
template <class C>
bool cfg_layer_matches(const AggArgs& a) {
  return a.H == C::kH && a.B == C::kB && a.L == C::kL && a.Ls == C::kLs && a.A == C::kA && a.act == C::kAct &&
         (a.x_looped != 0) == C::kXl && agg_packed_code(a) == C::kAgg;
}
template <class C>
bool cfg_matches(const AggArgs& a) {
  return cfg_layer_matches<C>(a) && (a.y_looped != 0) == C::kYl && (a.loops_all != 0) == C::kLoopsAll;
}

// the d = 128 / H8 / B4 layers that the tile kernel and both directions of the one-launch kernel compile in
namespace cfg {
constexpr int S = EGC_AGGR_SUM, M = EGC_AGGR_MEAN, X = EGC_AGGR_MAX, Y = EGC_AGGR_SYMNORM;
// EGConv EGC-M north star (configs 3 / 4 of BASELINE.json): sum+mean+max+symnorm, gcn_norm self-loops on every node
using EGConvM128 = StCfg<8, 4, 16, 4, agg_pack(S, M, X, Y), EGC_ACT_NONE, true, true, true>;
// EfficientGraphConv EGC-M / EGC-S at d = 128 (symadd looped, the others raw): layers.py:166-193
using EgcM128 = StCfg<8, 4, 16, 3, agg_pack(Y, X, M), EGC_ACT_NONE, false, true, true>;
using EgcS128 = StCfg<8, 4, 16, 1, agg_pack(Y), EGC_ACT_NONE, false, true, true>;
}  // namespace cfg

}  // namespace egc
