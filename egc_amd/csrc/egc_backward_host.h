// Host side of the layer backward (egc_backward.hip), one definition each.  The lists name every compiled instance of
// bwd_dst_fast_kernel and bwd_src_kernel: the launches AND the plan's "is this configuration compiled?" expand from them, so a new
// compiled configuration is one row.  bwd_plan: what one call of egc_aggregate_combine_backward_f32 launches for a layer on a graph
// -- refusals, tables and records of the workspace, instance / LDS / grid of the destination, record and source launches; the
// launcher follows it and decides nothing.  arg_plan: the same for the arg pass of the training forward.  bwd_workspace: what
// egc_backward_workspace_bytes(_for) answer.  Plain C++: tests/backward_plan runs it all.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#include "egc_plain.h"

namespace egc {

constexpr int BWD_HMAX = 16;             // heads supported by the register form of the destination kernel
constexpr int REC_FIT_COLUMNS = 10;      // records are built where an entry receives at most this many columns on average (ldb N / E)
constexpr size_t BWD_LDS_MAX = 64 * 1024;
// bwd_dst_fast_kernel<.., AGG>: the aggregator codes packed 3 bits each (first in the low bits) with bit 31 set, or 0 = run time
constexpr unsigned BWD_STATIC = 0x80000000u;
constexpr unsigned bwd_agg_pack(int a0, int a1 = 0, int a2 = 0, int a3 = 0) {
  return BWD_STATIC | (unsigned)a0 | ((unsigned)a1 << 3) | ((unsigned)a2 << 6) | ((unsigned)a3 << 9);
}
template <class... T> constexpr int bwd_agg_count(T...) { return (int)sizeof...(T); }
// bwd_src_kernel<NS, FL>: which tables exist and which edge sets are LOOPED, compiled in (bit 0 set) or read from the arguments (0)
constexpr unsigned SRC_STATIC = 1u, SRC_S = 2u, SRC_V = 4u, SRC_X = 8u, SRC_N = 16u, SRC_XL = 32u, SRC_YL = 64u, SRC_T = 128u,
                   SRC_REC = 256u;   // max / min gradients arrive as per-entry records (REC_*) instead of arg bytes + X sectors

// ROW(LPR_LOG2, HT, AT, aggregators...): bwd_dst_fast_kernel with the aggregator list compiled in (weight nonlinearity: none).  The
// reference's own batched nets train on these; the run-time form's per-aggregator switches are most of
// its instructions.
#define EGC_BWD_DST_LISTS(ROW)                                                                                                    \
  ROW(6, 4, 3, EGC_AGGR_SUM, EGC_AGGR_MEAN, EGC_AGGR_MAX)                     /* molhiv EGC-M 224 / H4 / B4 add, mean, max */      \
  ROW(6, 8, 1, EGC_AGGR_SYMNORM)                                              /* molhiv EGC-S 296 / H8 / B4 symadd */              \
  ROW(5, 8, 1, EGC_AGGR_SYMNORM)                                              /* zinc / CIFAR EGC-S 168, arxiv EGC-S 184 / H8 / B4 */ \
  ROW(6, 4, 3, EGC_AGGR_SYMNORM, EGC_AGGR_MAX, EGC_AGGR_MEAN)                 /* arxiv EGC-M 136 / H4 / B4 symadd, max, mean */    \
  ROW(5, 4, 3, EGC_AGGR_SUM, EGC_AGGR_STD, EGC_AGGR_MAX)                      /* zinc EGC-M 124 / H4 / B4 add, std, max */         \
  ROW(5, 4, 3, EGC_AGGR_SYMNORM, EGC_AGGR_STD, EGC_AGGR_MAX)                  /* CIFAR EGC-M 128 / H4 / B4 symadd, std, max */     \
  ROW(4, 8, 4, EGC_AGGR_SUM, EGC_AGGR_MEAN, EGC_AGGR_MAX, EGC_AGGR_SYMNORM)   /* EGConv north star */                              \
  ROW(4, 8, 3, EGC_AGGR_SYMNORM, EGC_AGGR_MAX, EGC_AGGR_MEAN)                 /* EfficientGraphConv EGC-M */                       \
  ROW(4, 8, 1, EGC_AGGR_SYMNORM)                                              /* EGC-S */
// ROW(LPR_LOG2, HT, AT): the same kernel with the list read at run time.  These triples ARE the head / aggregator counts the
// register form serves (with other counts the LDS kernel is faster): 16 lanes a row with H = 8 (the d = 128 layers); 32 and 64
// lanes with the trained nets' H4 x 3 aggregators and H8 x 1 (hyperparameters.md: 124 ... 296 wide, 24 ... 56 slots).
#define EGC_BWD_DST_TRIPLES(ROW) ROW(6, 4, 3) ROW(6, 8, 1) ROW(5, 4, 3) ROW(5, 8, 1) ROW(4, 8, 4) ROW(4, 8, 3) ROW(4, 8, 1)
// ROW(flags): bwd_src_kernel<1, SRC_STATIC | flags>, the shipped layer kinds with records and -- on low-degree batches, where
// no records are built -- with the arg-byte form
#define EGC_BWD_SRC_FLAGS(ROW)                                                                               \
  ROW(SRC_T | SRC_X | SRC_YL)                              /* add+mean+max (molhiv EGC-M) */                  \
  ROW(SRC_T | SRC_S | SRC_X | SRC_YL)                      /* symadd+max+mean */                              \
  ROW(SRC_T | SRC_V | SRC_X | SRC_YL)                      /* add+std+max (zinc EGC-M) */                     \
  ROW(SRC_T | SRC_S | SRC_V | SRC_X | SRC_YL)              /* symadd+std+max (CIFAR EGC-M) */                 \
  ROW(SRC_T | SRC_S | SRC_X | SRC_XL | SRC_YL)             /* EGConv sum+mean+max+symnorm */                  \
  ROW(SRC_T | SRC_S | SRC_X | SRC_XL | SRC_YL | SRC_REC)   /* EGConv sum+mean+max+symnorm (north star) */     \
  ROW(SRC_T | SRC_S | SRC_X | SRC_YL | SRC_REC)            /* EfficientGraphConv symadd+max+mean */           \
  ROW(SRC_S | SRC_YL)                                      /* EfficientGraphConv symadd (EGC-S) */            \
  ROW(SRC_S | SRC_XL | SRC_YL)                             /* EGConv symnorm */                               \
  ROW(SRC_T | SRC_X | SRC_REC)                             /* relational EGC: mean+max, raw */                \
  ROW(SRC_T | SRC_V | SRC_X | SRC_YL | SRC_REC)            /* EfficientGraphConv add+std+max (zinc EGC-M) */  \
  ROW(SRC_T | SRC_S | SRC_V | SRC_X | SRC_YL | SRC_REC)    /* symadd+std+max (CIFAR EGC-M) */                 \
  ROW(SRC_T | SRC_X | SRC_YL | SRC_REC)                    /* add+mean+max (molhiv EGC-M) */
// slots per lane of arg_extrema_kernel, bwd_records_kernel and the run-time bwd_src_kernel
#define EGC_BWD_NS(ROW) ROW(1) ROW(2) ROW(3) ROW(4)

// Rows of a list that carry a key (agg 0: of the triples).  The plan asks "== 1", and every row's own key answers 1: the rows
// are disjoint, their order carries no meaning.
constexpr int bwd_dst_rows(int lg, int ht, int at, unsigned agg) {
  int n = 0;
#define EGC_ROW(LG, HT, AT, ...) n += (lg == LG && ht == HT && at == AT && agg == bwd_agg_pack(__VA_ARGS__)) ? 1 : 0;
  EGC_BWD_DST_LISTS(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(LG, HT, AT) n += (lg == LG && ht == HT && at == AT && agg == 0u) ? 1 : 0;
  EGC_BWD_DST_TRIPLES(EGC_ROW)
#undef EGC_ROW
  return n;
}
constexpr int bwd_src_rows(unsigned fl) {
  int n = 0;
#define EGC_ROW(FL) n += (fl == (SRC_STATIC | (FL))) ? 1 : 0;
  EGC_BWD_SRC_FLAGS(EGC_ROW)
#undef EGC_ROW
  return n;
}
#define EGC_ROW(LG, HT, AT, ...)                                                                                                 \
  static_assert(bwd_dst_rows(LG, HT, AT, bwd_agg_pack(__VA_ARGS__)) == 1 && bwd_agg_count(__VA_ARGS__) == AT && bwd_dst_rows(LG, HT, AT, 0u) == 1, \
                "a compiled list: once, AT aggregators, beside its run-time triple");
EGC_BWD_DST_LISTS(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(LG, HT, AT) static_assert(bwd_dst_rows(LG, HT, AT, 0u) == 1, "a run-time triple: once");
EGC_BWD_DST_TRIPLES(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(FL) static_assert(bwd_src_rows(SRC_STATIC | (FL)) == 1, "a compiled flag word: once");
EGC_BWD_SRC_FLAGS(EGC_ROW)
#undef EGC_ROW

// The run-time switches (diagnostics): read on every call, here and nowhere else.
struct BwdSwitches {
  bool generic;        // EGC_BWD_GENERIC: the LDS destination kernel and the run-time source kernel, whatever the layer
  bool no_rec;         // EGC_BWD_NO_REC: no per-entry records
  bool rec_separate;   // EGC_BWD_REC_SEPARATE: records by bwd_records_kernel also behind the register form
};
inline BwdSwitches bwd_switches() {
  return {env_on("EGC_BWD_GENERIC"), env_on("EGC_BWD_NO_REC"), env_on("EGC_BWD_REC_SEPARATE")};
}

// The workspace: tables T, S, V, X, N of [n, ldb] floats, then one 64-byte record per entry and extremum (max first).
// A record holds REC_ITEMS (value, column) pairs; an entry that receives more is marked REC_OVERFLOW and the source side reads
// the destination's whole X row and int32 arg row for it on top of the record.  An entry receives ldb / degree columns on
// average: 4.6 on the ogbn-arxiv graph at 64 basis columns, but 108 on a molhiv batch at 224 (two entries per row) -- there
// EVERY record overflowed, the source kernel fetched 282 MB per launch for 110 MB of payload (FETCH_SIZE, round 6) and the
// destination kernel spent a fifth of its time building records nobody could use.  Records only where they mostly fit.
struct BwdWorkspace {
  int extrema;            // of max and min, how many the layer has
  bool records;           // the rule: records are built for this layer on this graph (if the caller's workspace holds them)
  size_t tables, total;   // egc_backward_workspace_bytes / egc_backward_workspace_bytes_for (tables: a multiple of 256)
};
inline BwdWorkspace bwd_workspace(const egc_layer* layer, int64_t n, int64_t e, const BwdSwitches& sw) {
  const int ldb = layer_bases_ld(layer);
  int mx = 0, mn = 0;
  for (int t = 0; t < layer->num_aggrs && t < EGC_MAX_AGGRS; ++t) {
    if (layer->aggrs[t] == EGC_AGGR_MAX) mx = 1;
    if (layer->aggrs[t] == EGC_AGGR_MIN) mn = 1;
  }
  BwdWorkspace w = {mx + mn, false, (((size_t)5 * (size_t)n * ldb * sizeof(float) + 255) & ~(size_t)255) + 256, 0};
  w.records = w.extrema > 0 && e > 0 && ldb <= 256 && (uint64_t)e * 64ull < (uint64_t)OOB && !sw.no_rec &&
              (double)ldb * (double)std::max<int64_t>(n, 1) <= (double)REC_FIT_COLUMNS * (double)e;
  w.total = w.tables + (w.records ? (size_t)w.extrema * (size_t)e * 64 : 0);
  return w;
}
// LDS words of one record builder (records_from_columns) over up to `entries` entries of a row: count | offset | values | column
// bytes (+ the over-read of the last list)
constexpr int rec_group_u32(int ldb, int entries) { return 2 * entries + ldb + ldb / 4 + 4; }

// The arg pass of the training forward (arg_extrema_kernel<ns>): lane group per row behind the chunk blocks.
struct ArgPlan {
  int status;   // EGC_OK, or EGC_ERR_UNSUPPORTED: more than four slots a lane
  int lpr_log2, ns, chunk_blocks;
  unsigned grid;
};
inline ArgPlan arg_plan(int slots, int64_t n, int64_t n_edges, int64_t n_chunks) {
  const LaneGroup lg = lane_group(slots);
  const int cb = plan_chunk_blocks(n, n_edges, n_chunks);
  return {lg.ns <= 4 ? EGC_OK : EGC_ERR_UNSUPPORTED, lg.lpr_log2, lg.ns, cb, (unsigned)(cb + ceil_div(n, (int64_t)4 * (64 >> lg.lpr_log2)))};
}

struct BwdCounts {
  int64_t n, n_src;             // destination rows, source rows
  int64_t d_edges, d_chunks;    // destination-side graph: entries, host-known chunk count or -1
  int64_t t_edges, t_chunks;    // transposed graph
  size_t workspace_bytes;
  bool d_has_plan;              // the destination-side graph carries a long-row plan (the records of hub rows need it)
};
enum BwdRecMode { BWD_REC_OFF, BWD_REC_FUSED, BWD_REC_SEPARATE };
struct BwdPlan {
  // size_status: EGC_ERR_WORKSPACE, or EGC_ERR_UNSUPPORTED for n ldb 4 beyond 32-bit buffer offsets -- the entry point answers these
  // before its remaining pointer checks, as it always has; status: that, or EGC_ERR_UNSUPPORTED of a launch (refusal: which)
  int size_status, status;
  const char* refusal;
  int ldb, slots, H, B, A, L, Ls, F_g, F_out, W, aggr[EGC_MAX_AGGRS], stat_slot[5], stat_k;
  // tables: T always (need_t: some aggregator is linear in the plain messages), S / V / X / N at 1 .. 4 x table_floats if there
  int need_t;
  bool has_s, has_v, has_x, has_n;
  size_t table_floats;
  BwdWorkspace ws;
  BwdRecMode rec_mode;         // off also where the rule says yes and the workspace does not hold the records / no destination plan
  size_t rec_offset;           // bytes: the first record array; the second rec_entry_bytes behind it
  unsigned rec_entry_bytes;    // of one array; 0 = off
  // destination: bwd_dst_fast_kernel<dst_lpr_log2, H, A, agg> (agg 0: run-time list), else bwd_dst_kernel with wpb wavefronts
  bool fast, p2;               // p2: a basis spans a power-of-two number of lanes (butterfly), else the shares meet through LDS
  int dst_lpr_log2, wpb, lds_floats_per_wave, dst_group_floats, dst_row_blocks, rec_chunk_blocks;
  unsigned agg, dst_grid, dst_threads;
  size_t dst_lds;
  // records: bwd_records_kernel<rec_ns>, once per extremum; grid 0: fused, nothing to launch
  int rec_ns, rec_group_u32, rec_blocks, rec_short_rows;
  unsigned rec_grid;
  size_t rec_lds;
  // source: bwd_src_kernel<src_ns, src_flags> (src_flags 0: run-time form)
  int src_lpr_log2, src_ns, src_chunk_blocks;
  unsigned src_flags, src_grid;
};

inline BwdPlan bwd_plan(const egc_layer* layer, const BwdCounts& c, const BwdSwitches& sw) {
  BwdPlan p = {};
  p.refusal = "";
  auto refuse = [&](int status, const char* why) {   // the first refusal stands
    if (p.status == EGC_OK) { p.status = status; p.refusal = why; }
  };
  p.ldb = layer_bases_ld(layer); p.slots = p.ldb / 4;
  p.H = layer->num_heads; p.B = layer->num_bases; p.A = layer->num_aggrs;
  p.L = layer->out_channels / p.H; p.Ls = layer_basis_stride(layer);
  p.F_g = p.B * p.Ls; p.F_out = layer->out_channels; p.W = p.H * p.B * p.A;
  for (int t = 0; t < p.A; ++t) {
    const int g = p.aggr[t] = layer->aggrs[t];
    if (g == EGC_AGGR_SYMNORM) p.has_s = true;
    if (g == EGC_AGGR_VAR || g == EGC_AGGR_STD) p.has_v = true;
    if (g == EGC_AGGR_SUM || g == EGC_AGGR_MEAN || g == EGC_AGGR_VAR || g == EGC_AGGR_STD) p.need_t = 1;
  }
  p.stat_k = stat_layout(p.aggr, p.A, p.stat_slot);
  p.has_x = p.stat_slot[STAT_MX] >= 0; p.has_n = p.stat_slot[STAT_MN] >= 0;
  p.table_floats = (size_t)c.n * p.ldb;
  p.ws = bwd_workspace(layer, c.n, c.d_edges, sw);
  if (c.workspace_bytes < p.ws.tables) refuse(EGC_ERR_WORKSPACE, "workspace");
  if ((uint64_t)c.n * (uint64_t)p.ldb * 4ull > (uint64_t)OOB) refuse(EGC_ERR_UNSUPPORTED, "offsets");
  p.size_status = p.status;
  // per-entry records when the caller's workspace holds them (egc_backward_workspace_bytes_for)
  const bool rec = p.ws.records && c.d_has_plan && c.workspace_bytes >= p.ws.total;
  p.rec_offset = p.ws.tables;
  p.rec_entry_bytes = rec ? (unsigned)((uint64_t)c.d_edges * 64ull) : 0u;

  // destination.  The LDS form's strips per wavefront (agg [A][ldb], g [F_out], w' [W], d w' [W]) must fit whichever form runs.
  p.lds_floats_per_wave = p.A * p.ldb + ((p.F_out + 3) & ~3) + 2 * ((p.W + 3) & ~3);
  p.wpb = (size_t)4 * p.lds_floats_per_wave * sizeof(float) > 48 * 1024 ? 1 : 4;
  p.dst_lds = (size_t)p.wpb * p.lds_floats_per_wave * sizeof(float);
  if (p.dst_lds > BWD_LDS_MAX) refuse(EGC_ERR_UNSUPPORTED, "lds");
  // register-resident form when the layout allows (see bwd_dst_fast_kernel) and its head / aggregator counts are compiled
  const int P = p.Ls / 4;
  p.p2 = (P & (P - 1)) == 0;
  p.dst_lpr_log2 = lane_group(p.slots).lpr_log2;
  p.fast = !sw.generic && (p.Ls & 3) == 0 && p.ldb == p.B * p.Ls && P >= 1 && P <= 16 && (p.B & (p.B - 1)) == 0 && p.slots <= 64 &&
           p.A <= 4 && p.H <= BWD_HMAX && (!p.p2 || p.H % P == 0 || p.H < P) && layer->weight_act != EGC_ACT_SOFTMAX &&
           bwd_dst_rows(p.dst_lpr_log2, p.H, p.A, 0u) == 1;
  p.rec_mode = !rec ? BWD_REC_OFF : (p.fast && !sw.rec_separate) ? BWD_REC_FUSED : BWD_REC_SEPARATE;
  const bool fused = p.rec_mode == BWD_REC_FUSED;
  const int d_chunk_blocks = plan_chunk_blocks(c.n, c.d_edges, c.d_chunks);
  if (p.fast) {
    const int lpr = 1 << p.dst_lpr_log2, G = 64 / lpr;
    const unsigned packed = BWD_STATIC | pack_aggr_codes(p.aggr, p.A);
    p.agg = (layer->weight_act == EGC_ACT_NONE && bwd_dst_rows(p.dst_lpr_log2, p.H, p.A, packed) == 1) ? packed : 0u;
    // per lane group: the strips of g and w' (+ the transposed d w' shares of a basis that is not a power-of-two number of lanes
    // wide: [H A][lpr + 1]); afterwards the record builder's, 64 entries per group in the row role, 256 per WAVEFRONT in the
    // hub-chunk role of the trailing blocks
    p.dst_group_floats = std::max(((p.H * p.Ls + 3) & ~3) + ((p.W + 3) & ~3) + (p.p2 ? 0 : p.H * p.A * (lpr + 1)),
                                  fused ? std::max(rec_group_u32(p.ldb, 64), (rec_group_u32(p.ldb, 256) + G - 1) / G) : 0);
    p.dst_lds = (size_t)4 * G * p.dst_group_floats * sizeof(float);
    if (p.dst_lds > BWD_LDS_MAX) refuse(EGC_ERR_UNSUPPORTED, "lds_fast");
    p.dst_row_blocks = (int)ceil_div(c.n, (int64_t)4 * G);
    p.rec_chunk_blocks = fused ? d_chunk_blocks : 0;
    p.dst_grid = (unsigned)(p.dst_row_blocks + p.rec_chunk_blocks);
    p.dst_threads = 256;
  } else {
    p.dst_grid = (unsigned)ceil_div(c.n, p.wpb);
    p.dst_threads = (unsigned)p.wpb * 64;
  }
  if (rec) {   // behind the destination kernel: 16 lanes per short row, 16 rows per block, behind the chunk blocks
    p.rec_ns = std::min((p.slots + 15) / 16, 4);
    p.rec_group_u32 = rec_group_u32(p.ldb, 64);
    p.rec_blocks = d_chunk_blocks;
    p.rec_short_rows = fused ? 0 : 1;
    p.rec_grid = fused ? 0u : (unsigned)(p.rec_blocks + ceil_div(c.n, (int64_t)16));
    p.rec_lds = (size_t)16 * p.rec_group_u32 * sizeof(unsigned);
  }
  // source: lane group per source row behind the chunk blocks of the transposed graph
  const LaneGroup lg = lane_group(p.slots);
  p.src_lpr_log2 = lg.lpr_log2; p.src_ns = lg.ns;
  p.src_chunk_blocks = plan_chunk_blocks(c.n_src, c.t_edges, c.t_chunks);
  p.src_grid = (unsigned)(p.src_chunk_blocks + ceil_div(c.n_src, (int64_t)4 * (64 >> lg.lpr_log2)));
  const unsigned fl = SRC_STATIC | (p.need_t ? SRC_T : 0u) | (p.has_s ? SRC_S : 0u) | (p.has_v ? SRC_V : 0u) | (p.has_x ? SRC_X : 0u) |
                      (p.has_n ? SRC_N : 0u) | (layer->agg_set == EGC_SET_LOOPED ? SRC_XL : 0u) |
                      (layer->sym_set == EGC_SET_LOOPED ? SRC_YL : 0u) | (rec ? SRC_REC : 0u);
  p.src_flags = (!sw.generic && p.src_ns == 1 && bwd_src_rows(fl) == 1) ? fl : 0u;
  if (p.src_ns > 4) refuse(EGC_ERR_UNSUPPORTED, "slots");
  return p;
}

}  // namespace egc
