// Host side of the one-launch batch kernel (fused_tile_kernel, egc_fused_tile_dev.h), both directions, one definition each: the
// constants its host and device code share, the three packed operands' layouts as values (the pack kernels write through them, the
// byte queries answer from them, the kernel reads them), and one plan per direction -- form and envelope, chunk quantum and range,
// the derived fields of FusedTileArgs, the LDS image, the tile test a launch and its capacity query both ask, the grid rule and the
// run-time switches.  egc_fused_tile.hip, egc_fused_tile_wide.inc and the egc_batch_fused_* entry points follow it and decide
// nothing but which compiled configuration runs.  Plain C++: tests/fused_tile_plan runs it all.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#include "egc_plain.h"

namespace egc {

constexpr int FT_THREADS = 1024;
constexpr int FT_WAVES = FT_THREADS / 64;
constexpr int FT_MFMA_WAVES = 12;       // 16-column tiles of the virtual column space [bases (ldb) | weightings (W)]
constexpr int FT_FIRST_HELPER = 12;     // wavefronts 12-15: x rows -> planes
constexpr int FT_HELPER_THREADS = (FT_WAVES - FT_FIRST_HELPER) * 64;
constexpr int FT_KP = 128;              // k extent of the register-resident weight tiles (F_in <= 128, zero beyond)
constexpr int FT_CHUNK = 16;            // rows per GEMM step (one MFMA tile)
constexpr int FT_WORKER_THREADS = FT_FIRST_HELPER * 64;
constexpr int FT_EDGE_REGS = 4;         // edges per worker thread kept in registers (16:16 packed local ids)
constexpr int FT_CSR_WAVES = 3;         // helper wavefronts 12-14 build the tiles' CSR (15 plans the tiles)
constexpr int FT_PER = 3;               // rows per lane of the one-wavefront scan: 3 x 64 >= 16 FT_RING
constexpr int FT_RING = 10;             // 16-row chunks of x a tile may have: the helpers hold them all in registers (80 VGPRs)
static_assert(FT_PER * 64 >= FT_CHUNK * FT_RING, "the scan covers a whole tile");
constexpr int FT_MAX_NODES = 2048;      // local ids are 16-bit, the scan is one wavefront
constexpr int FT_NV = FT_MFMA_WAVES * 16;
constexpr int FT_PLANE_BYTES = FT_CHUNK * FT_KP * 2;     // one plane of one chunk
constexpr int FT_PBUF = 3;                                // chunk buffers: the helpers stage two chunks ahead of the workers' MFMAs
constexpr int FT_PLANES_BYTES = FT_PBUF * 2 * FT_PLANE_BYTES;  // [3 buffers][2 planes]
constexpr int FT_EMAX = 65535;          // edges of a tile: 16-bit cursors of the CSR build
// The backward form: at most FTB_K2 = ldb + H B 4 columns of [d bases | d w'] (six k-steps of 32) against FT_KP = 128 output
// features (eight tiles of 16); the kernel keeps eight 16-row chunks of x in flight -- six at H = 8, where the LDS image (d bases
// next to bases and w') holds no more than 96 rows anyway and the static configuration's helpers give the registers of the other
// two to their working set
constexpr int FTB_K2 = 192;
constexpr int FTB_EMAX = 16384;
constexpr int ftb_ring(int H) { return H == 8 ? 6 : 8; }
// ... its second GEMM: d rows of K2 columns as two fp16 planes, rows padded by 16 bytes
constexpr int FTB_ROW_BYTES = FTB_K2 * 2 + 16;             // (25 sixteen-byte pieces: conflict-free A-operand reads)
constexpr int FTB_PLANE_BYTES = FT_CHUNK * FTB_ROW_BYTES;  // one plane of one 16-row chunk
constexpr int FTB_PBUF_BYTES = 2 * FTB_PLANE_BYTES;        // [2 planes]
constexpr int FTB_PLANES_BYTES = 2 * FTB_PBUF_BYTES;       // [2 buffers]: 25,600 bytes (the first GEMM's three buffers take 24,576)
// The WIDE form (egc_fused_tile_wide.inc: 128 < F_in <= 320 or more than 192 virtual columns -- the reference's 168 / 224 / 296 /
// 300 / 304-wide batched nets, run_pretrained.sh:7-48): 32-row GEMM chunks on v_mfma_f32_32x32x16_f16, one 32-column tile per
// worker (at most 12: 384 virtual columns), the weight fragments streamed from L2 per k-step (a 320 x 384 operand does not fit the
// register files), x staged in k-slabs of 128 through two plane buffers.
constexpr int FTW_CH = 32;                                 // rows per GEMM chunk
constexpr int FTW_PP = 10;                                 // 16-byte pieces of x per helper thread and chunk: 8 threads per row, F_in <= 320
constexpr int FTW_MAX_FIN = 8 * FTW_PP * 4;
constexpr int FTW_SLAB = 128;                              // k per staged slab
constexpr int FTW_LDX = FTW_SLAB + 8;                      // halves per plane row in LDS (+ 16 bytes: conflict-free A-operand reads)
constexpr int FTW_PLANE_BYTES = FTW_CH * FTW_LDX * 2;      // one plane of one slab
constexpr int FTW_PBUF_BYTES = 2 * FTW_PLANE_BYTES;        // [2 planes]
constexpr int FTW_PLANES_BYTES = 2 * FTW_PBUF_BYTES;       // [2 buffers]
constexpr int FTW_MAXCH = FT_CHUNK * FT_RING / FTW_CH;     // chunks of a tile (160 rows)
constexpr int FTW_MAX_CT = FT_MFMA_WAVES;                  // 32-column tiles
constexpr int FT_DBS_POISON = 0x7fffffff;                  // backward: the tile's fixed-point scale when its g or w' holds an Inf / NaN
constexpr size_t FT_LDS_BUDGET = 160 * 1024 - 256;

// ---------------------------------------------------------------------------------------------
// A packed operand: [tile of TW columns][k-step of 512 / TW][plane][lane][8] halves, then a tail of floats.  One fragment
// ([lane][8], one KiB) is the B operand of an MFMA as it is loaded: lane TW (k % KW / 8) + column % TW holds k = KW s + 8 (lane / TW)
// ..+7 of column TW ct + lane % TW -- TW = 16, KW = 32 for v_mfma_f32_16x16x32_f16, TW = 32, KW = 16 for v_mfma_f32_32x32x16_f16.
// Tail: the columns' inverse scales, then (bias_at > 0) their biases from float bias_at on.
// ---------------------------------------------------------------------------------------------
constexpr int FT_FRAG = 64 * 8;   // halves of a fragment
struct FtPacked {
  int tw, tiles, ksteps, tail_floats, bias_at;
  constexpr int columns() const { return tiles * tw; }                   // pack blocks: one per (virtual) column
  constexpr int k_rows() const { return ksteps * (FT_FRAG / tw); }
  constexpr int64_t tile_halves() const { return (int64_t)ksteps * 2 * FT_FRAG; }
  constexpr int64_t tail_at() const { return (int64_t)tiles * ksteps * 2 * FT_FRAG; }   // in halves
  constexpr size_t bytes() const { return (size_t)tail_at() * 2 + (size_t)tail_floats * sizeof(float); }
};
// the high plane's half of (column v, row k); the low plane's: FT_FRAG further
template <int TW>
constexpr int64_t ft_frag_index(unsigned v, unsigned k, int ksteps) {
  constexpr unsigned KW = FT_FRAG / TW;
  return ((((int64_t)(v / TW) * ksteps + (k / KW)) * 2) * 64 + TW * ((k % KW) >> 3) + (v % TW)) * 8 + (k & 7);
}
// narrow forward: 12 tiles x k = 128, float col_inv[192], col_bias[192]
constexpr FtPacked ft_packed_narrow() { return {16, FT_MFMA_WAVES, FT_KP / 32, 2 * FT_NV, FT_NV}; }
// wide forward: n_ct tiles of 32 x k = 16 k16 (a tile's k-steps contiguous: the kernel streams them in order), col_inv[384], col_bias[384]
constexpr FtPacked ft_packed_wide(int n_ct, int k16) { return {32, n_ct, k16, 2 * FTW_MAX_CT * 32, FTW_MAX_CT * 32}; }
// transposed (backward, d x = d W^T): 8 tiles of 16 output features x k = FTB_K2 image columns, col_inv[128]
constexpr FtPacked ft_packed_t() { return {16, FT_KP / 16, FTB_K2 / 32, FT_KP, 0}; }

// ---------------------------------------------------------------------------------------------
// The plan.  FtLayer: the layer fields it reads (egc_fused_tile.hip fills it from AggArgs).
// ---------------------------------------------------------------------------------------------
struct FtLayer {
  int H, B, A, L, Ls, ldb, slots, W, act, aggr[EGC_MAX_AGGRS];
  int f_in;
  bool with_post;
};
enum FtForm { FT_FORM_NONE = 0, FT_FORM_NARROW = 1, FT_FORM_WIDE = 2 };

constexpr int ft_ldbp(int ldb) { return (ldb + 31) & ~31; }       // WIDE: ldb rounded up to 32, the first virtual column of the weightings
constexpr int ft_p0(int Ls) { return ((Ls >> 2) + 1) / 2; }       // rows of more than 64 slots: the first pass's slots of every basis

inline bool ft_narrow_shape(const FtLayer& a) {
  return a.f_in >= 4 && a.f_in <= FT_KP && (a.f_in & 3) == 0 && a.ldb + a.W <= FT_NV && a.slots <= 64 && a.A <= AMAX;
}
// the WIDE form's envelope: F_in <= 320, at most 12 column tiles of 32 (bases padded to a multiple of 32, then the weightings)
inline bool ft_wide_shape(const FtLayer& a) {
  if (a.slots > 64 && (a.slots > 128 || a.B * ft_p0(a.Ls) > 64)) return false;    // two passes of at most 64 lanes
  return a.f_in >= 4 && a.f_in <= FTW_MAX_FIN && (a.f_in & 3) == 0 && ft_ldbp(a.ldb) + a.W <= FTW_MAX_CT * 32 && a.A <= AMAX;
}
// the backward's: the d = 128 / 64 layers (B = 4 bases of 16 channels, H = 4 or 8, F_in <= 128), sum / mean / max / symnorm, no
// weight nonlinearity
inline bool ftb_shape(const FtLayer& a) {
  if (!ft_narrow_shape(a) || a.act != EGC_ACT_NONE) return false;
  if (a.B != 4 || a.L != 16 || a.Ls != 16 || a.ldb != 64 || (a.H != 4 && a.H != 8)) return false;
  for (int k = 0; k < a.A; ++k)
    if (a.aggr[k] != EGC_AGGR_SUM && a.aggr[k] != EGC_AGGR_MEAN && a.aggr[k] != EGC_AGGR_MAX && a.aggr[k] != EGC_AGGR_SYMNORM) return false;
  return true;
}

struct FtPlan {
  FtForm form;               // FT_FORM_NONE: outside the envelope, every other field 0
  bool bwd;
  int quantum, max_chunks;   // tile_nodes: a multiple of quantum (rows per GEMM chunk), at most max_chunks of them
  int max_emax;
  // FusedTileArgs' derived fields
  int n_ct;                  // column tiles in use
  int n_slabs, k16, ldbp;    // WIDE: k-slabs of x, k-steps of 16 (padded with zero fragments to the kernel's ring of four), see ft_ldbp
  int w_aw, wl_floats;       // floats per (h, b) block of a weightings row in LDS (4; WIDE: A when A < 3), and per row
  int nsets, p0;             // rows of more than 64 slots: two passes
  unsigned magic0, magic1;
  int k2;                    // backward: columns of the d rows, ldb + H B 4
  // the image's inputs
  int ldb, bias_floats, bias_strips;
  FtPacked packed, packed_t; // the forward operand of this form; backward: the transposed one
};

inline FtPlan ft_plan_of(const FtLayer& a, FtForm form, bool bwd) {
  FtPlan p = {};
  if (form == FT_FORM_NONE) return p;
  const bool wide = form == FT_FORM_WIDE;
  p.form = form; p.bwd = bwd;
  p.quantum = wide ? FTW_CH : FT_CHUNK;
  p.max_chunks = bwd ? ftb_ring(a.H) : wide ? FTW_MAXCH : FT_RING;
  p.max_emax = bwd ? FTB_EMAX : FT_EMAX;
  p.ldbp = ft_ldbp(a.ldb);
  p.n_ct = wide ? (p.ldbp + a.W + 31) / 32 : (a.ldb + a.W + 15) / 16;
  p.n_slabs = (a.f_in + FTW_SLAB - 1) / FTW_SLAB;
  p.k16 = (((a.f_in + 15) / 16) + 3) & ~3;
  p.w_aw = (wide && a.A < 3) ? a.A : 4;
  p.wl_floats = a.H * a.B * p.w_aw;
  p.nsets = a.slots > 64 ? 2 : 1;
  p.p0 = ft_p0(a.Ls);
  p.magic0 = agg_magic(std::max(1, p.p0));
  p.magic1 = agg_magic(std::max(1, (a.Ls >> 2) - p.p0));
  p.k2 = a.ldb + a.H * a.B * 4;
  p.ldb = a.ldb;
  p.bias_floats = bias_strip_floats(a.H, a.Ls);
  p.bias_strips = (a.with_post && !bwd) ? 2 : 1;
  p.packed = wide ? ft_packed_wide(p.n_ct, p.k16) : ft_packed_narrow();
  if (bwd) p.packed_t = ft_packed_t();
  return p;
}
inline FtPlan ft_plan(const FtLayer& a) {
  return ft_plan_of(a, ft_narrow_shape(a) ? FT_FORM_NARROW : ft_wide_shape(a) ? FT_FORM_WIDE : FT_FORM_NONE, false);
}
inline FtPlan ftb_plan(const FtLayer& a) { return ft_plan_of(a, ftb_shape(a) ? FT_FORM_NARROW : FT_FORM_NONE, true); }

// The LDS image of a tile of `tcap` rows and `emax` edges: byte offsets, and the total.
struct FtLds {
  size_t total;
  int off_rec, off_planes, off_rowinv, off_bases, off_wt;
  int off_col, off_rowptr, off_cnt, off_dis;   // the CSR areas of an even tile; csr_stride bytes further: those of an odd tile
  int csr_stride;
  int off_db, off_rowinv2;                     // backward form
};
inline FtLds ft_image(const FtPlan& p, int tcap, int emax) {
  FtLds L = {};
  const bool wide = p.form == FT_FORM_WIDE;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  size_t at = up16((size_t)p.bias_strips * p.bias_floats * sizeof(float));
  L.off_rec = (int)at; at += 128;
  L.off_planes = (int)at; at += wide ? FTW_PLANES_BYTES : (p.bwd ? std::max(FT_PLANES_BYTES, FTB_PLANES_BYTES) : FT_PLANES_BYTES);
  L.off_rowinv = (int)at; at += wide ? up16(2 * FTW_CH * sizeof(float)) : up16(FT_PBUF * FT_CHUNK * sizeof(float));
  if (p.bwd) { L.off_rowinv2 = (int)at; at += up16(2 * FT_CHUNK * sizeof(float)); }
  L.off_bases = (int)at; at += up16((size_t)(tcap + 1) * p.ldb * 4);   // (+ the all-zero row absent entries read)
  L.off_wt = (int)at; at += up16((size_t)tcap * p.wl_floats * 4);
  if (p.bwd) { L.off_db = (int)at; at += up16((size_t)(tcap + 1) * p.ldb * 8); }   // d bases as 64-bit fixed point (+ a row absent entries would address)
  const size_t csr0 = at;
  L.off_col = (int)at; at += up16((size_t)emax * 2);
  L.off_rowptr = (int)at; at += up16((size_t)(tcap + 1) * 4);
  L.off_cnt = (int)at; at += up16((size_t)tcap * 4);      // (with rowptr: one 16-bit counter, then cursor, per CSR wavefront and row)
  L.off_dis = (int)at; at += up16((size_t)tcap * 4);
  L.csr_stride = (int)(at - csr0);
  at += L.csr_stride;       // the second set: tile it + 1's CSR is built while tile it's is being read
  L.total = at;
  return L;
}

// May a launch run tiles of `tcap` rows and `emax` edges?  EGC_ERR_UNSUPPORTED: a layer outside the envelope; EGC_ERR_INVALID:
// tcap not a multiple of the quantum within its range, emax outside [0, max_emax]; EGC_ERR_UNSUPPORTED: the image beyond the LDS.
inline int ft_tile_ok(const FtPlan& p, int tcap, int emax, FtLds* image = nullptr) {
  if (p.form == FT_FORM_NONE) return EGC_ERR_UNSUPPORTED;
  if (tcap < p.quantum || tcap > p.quantum * p.max_chunks || tcap % p.quantum != 0 || emax < 0 || emax > p.max_emax) return EGC_ERR_INVALID;
  const FtLds L = ft_image(p, tcap, emax);
  if (image != nullptr) *image = L;
  return L.total <= FT_LDS_BUDGET ? EGC_OK : EGC_ERR_UNSUPPORTED;
}
// rows of the largest tile a launch runs at `emax` edges; 0 = none
inline int ft_capacity(const FtPlan& p, int emax) {
  int best = 0;
  for (int tcap = p.quantum; p.form != FT_FORM_NONE && tcap <= p.quantum * p.max_chunks; tcap += p.quantum) {
    if (ft_tile_ok(p, tcap, emax) == EGC_OK) best = tcap; else break;
  }
  return best;
}

// The run-time switches (diagnostics): read on every call, here and nowhere else.
struct FtSwitches {
  bool static_cfg;   // EGC_NO_STATIC_CFG unset: a layer that equals a compiled-in configuration runs it
  int64_t grid;      // EGC_FT_GRID (at least 1), else 256: one workgroup per CU
};
inline FtSwitches ft_switches() {
  const char* e = getenv("EGC_FT_GRID");
  return {!env_on("EGC_NO_STATIC_CFG"), e != nullptr ? std::max(1, atoi(e)) : 256};
}
// one workgroup per CU at most; fewer when the batch is small (a workgroup's share: at least ~16 nodes, at least one graph)
inline unsigned ft_grid(const FtSwitches& sw, int64_t n_graphs, int64_t n_nodes) {
  return (unsigned)std::min({sw.grid, std::max<int64_t>(1, n_graphs), std::max<int64_t>(1, n_nodes / 16)});
}

}  // namespace egc
