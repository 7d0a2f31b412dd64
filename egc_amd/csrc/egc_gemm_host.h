// Host side of the packed basis transform  [bases | weightings] = x @ wcat (+ bcat)  (egc_gemm_bf16x3.hip, egc_gemm_f16x2.hip,
// egc_gemm_f16x2k.hip), one definition each.  gemm_plan: which kernel family serves a shape (its planes are packed in its own
// fragment order and no other family reads them, so pack and launch read the SAME plan), ldb, NV, KS, column tiles, pack bytes;
// EGC_GEMM_24BIT is read there and nowhere else.  gemm_bf16x3_launches / gemm_longk_launches: instance, grid, threads and LDS of
// every launch -- the launchers follow them, and the plan asks the latter whether every launch fits.  gemm_for_row_ranges: row
// ranges below 2 GiB.  gemm_sizes_ok / gemm_pointers_ok: the entry points' checks.  Plain C++: tests/gemm_plan runs it all.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "egc_hip.h"

namespace egc {

constexpr int GEMM_KT = 32;                  // k per packed staging step
constexpr size_t GEMM_LDS_MAX = 160 * 1024;  // LDS of one CU
constexpr int KROWS = 16;                    // long k: rows of an x tile = one MFMA row block
constexpr int XBM = 128;                     // LDS-staged bf16x3 kernel: rows per block
constexpr int XBN = 192;                     // ... virtual columns per block (6 MFMA tiles)
constexpr int XLD = 40;                      // ... LDS row stride in bf16 (80 B: conflict-free ds_read_b128 of 16-byte k-runs)
constexpr int WS_ROWS = 32;                  // weight-stationary bf16x3 kernel: rows per tile

inline int64_t gemm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// row tiles of a launch; EGC_ERR_INVALID: more than a 32-bit tile walk (or a grid dimension) holds
inline int gemm_row_tiles(int64_t M, int rows, int& n_tiles) {
  const int64_t n = gemm_cdiv(M, rows);
  n_tiles = (int)n;
  return n >= ((int64_t)1 << 31) ? EGC_ERR_INVALID : EGC_OK;
}
inline int gemm_grid(int per_cu, int n_tiles) { return std::min(256 * per_cu, n_tiles); }   // persistent blocks on 256 CUs

template <class L> struct GemmLaunches { int status, n; L l[2]; };   // status: EGC_OK, or why the shape cannot be launched

// ---- long k (egc_gemm_f16x2k.hip): column tiles of 16, x tiles of KROWS rows brought in by `stagers` wavefronts, R pieces of 16 bytes per
// thread (at most 16), into a ring of `ring` raw tiles of slot_bytes.
enum GemmLongKForm {
  LONGK_TWO_TILES,   // spec kernel, TPW = 2: helpers move x, every multiplier owns two column tiles; one launch over all tiles
  LONGK_ROLES,       // spec kernel: up to four helpers move and split x next to one multiplier per column tile
  LONGK_ALL_IN_ONE   // every wavefront requests, splits and multiplies
};
struct GemmLongKLaunch {
  int status;         // EGC_OK, or EGC_ERR_UNSUPPORTED: this form does not fit
  GemmLongKForm form;
  int waves;          // template instance: 12 or 16 wavefronts (the register budget of a wavefront)
  int tile0, tiles;   // column tiles [tile0, tile0 + tiles) of this launch, on `mult` multiplier wavefronts
  int mult, per_cu;   // per_cu: workgroups per CU the grid is sized for
  int LDX, R, slot_bytes, ring, threads;
  size_t lds;
};

inline GemmLongKLaunch gemm_longk_form(GemmLongKForm form, int K, int NT, int waves, int tile0, int tiles, int mult, int stagers) {
  const int KS = (K + GEMM_KT - 1) / GEMM_KT, sthreads = stagers * 64;
  GemmLongKLaunch g = {EGC_OK, form, waves, tile0, tiles, mult, 1};
  // row stride of the planes in fp16: the B fragments are ds_read_b128 of lanes (row j = lane & 15, k piece lane >> 4);
  // with 32 KS + 16 every one of the instruction's four 16-lane groups touches 16 distinct 4-bank slots
  // (32 KS + 8 leaves five 2-way conflicts per group)
  g.LDX = 32 * KS + 16;
  // next to the ring: planes [2 buffers][2 planes][KROWS][LDX] fp16, row scales, [16 NT][2] column scale / bias
  const size_t fixed = (size_t)4 * KROWS * g.LDX * sizeof(uint16_t) + (2 * KROWS + 2 * 16 * NT) * sizeof(float);
  g.R = (int)gemm_cdiv((int64_t)KROWS * (K / 4), sthreads);
  g.slot_bytes = g.R * sthreads * 16;
  // depth of the raw-tile ring: what the LDS holds next to the planes, at most 4 (and within the counted wait's range)
  g.ring = (int)std::min<size_t>(4, (GEMM_LDS_MAX - fixed) / (size_t)g.slot_bytes);
  if (form != LONGK_ALL_IN_ONE) {
    g.threads = (mult + stagers) * 64;
    while (g.ring > 2 && (g.ring - 2) * g.R > 32) --g.ring;
    if (g.ring < 2 || g.R > 16) g.status = EGC_ERR_UNSUPPORTED;
  } else {
    g.threads = sthreads;
    const size_t lds2 = (size_t)2 * g.slot_bytes + fixed;
    if (lds2 > GEMM_LDS_MAX || g.R > 16) g.status = EGC_ERR_UNSUPPORTED;
    // workgroups per CU: as many as the LDS holds, within about five wavefronts per SIMD (the KS <= 9 kernels use up to
    // 102 registers).  Short k leaves room for two (F_in = 192, 8 column tiles: 59 KB of LDS each), and the second one's
    // matrix work covers the first one's barrier and split: 66.9 -> 50.1 us for the 192 -> 128 gradient GEMM at
    // N = 169,343 (a third workgroup that does not fit measured 57 us: uneven CUs).
    g.per_cu = (int)std::min<size_t>(GEMM_LDS_MAX / lds2, (size_t)(20 / tiles));
    if (KS > 9 || g.per_cu < 1) g.per_cu = 1;
    if (g.per_cu > 1) g.ring = 2;   // a workgroup that shares its CU keeps 2
    while (g.ring > 2 && ((g.ring - 2) * (g.R + 1) + 4 > 32 || (size_t)g.ring * g.slot_bytes + fixed > GEMM_LDS_MAX)) --g.ring;
    g.ring = std::max(g.ring, 2);
  }
  g.lds = (size_t)g.ring * g.slot_bytes + fixed;
  return g;
}

// Every launch of a GEMM over k = K against NT column tiles.
inline GemmLaunches<GemmLongKLaunch> gemm_longk_launches(int K, int NT) {
  GemmLaunches<GemmLongKLaunch> r = {EGC_ERR_UNSUPPORTED, 0, {}};
  const int KS = (K + GEMM_KT - 1) / GEMM_KT;
  if (KS < 5 || KS > 12 || NT < 1) return r;
  // 17 - 20 column tiles (224 / H4 / B4 with three aggregators forward: 14 + 3; the d x GEMM of 296 / H8 / B4: 19): ONE launch
  // with two tiles per multiplier (K <= 224: 16 KS weight registers fit twelve wavefronts).  From nine tiles on the two-tile
  // form is also the faster single launch (half the operand reads per product, five to eight multipliers and as many wavefronts
  // left to move and split x: 3 - 20 % at 9 - 16 tiles and 169 k rows, same bits; at eight tiles and fewer two workgroups of the
  // all-in-one kernel per CU win: 60.6 against 67.0 us at 192 -> 128).
  if (KS <= 7 && NT >= 9 && NT <= 20) {
    r.l[0] = gemm_longk_form(LONGK_TWO_TILES, K, NT, 12, 0, NT, (NT + 1) / 2, 12 - (NT + 1) / 2);
    if (r.l[0].status == EGC_OK) { r.status = EGC_OK; r.n = 1; return r; }
  }
  // more than 16 column tiles (e.g. 224/H4/B4 with three aggregators: 14 + 3; 300/H4/B4: 19 + 3; 304/H8/B8: 20 + 4): two
  // launches over half of the tiles each -- x is read twice, which still beats the LDS-staged bf16x3 kernel 2 x
  r.n = NT <= 16 ? 1 : 2;
  for (int l = 0, t0 = 0; l < r.n; ++l) {
    const int tiles = (NT - t0 + (r.n - l) - 1) / (r.n - l);
    // up to 9 column tiles: 12 wavefronts (168 registers), 3-4 of them helpers; more: 16 wavefronts (128 registers) with
    // 16 - tiles helpers (none at 16 tiles: the kernel in which every wavefront does everything)
    const int waves = tiles <= 9 ? 12 : 16, nh = std::min(waves - tiles, 4);
    r.l[l] = gemm_longk_form(LONGK_ALL_IN_ONE, K, NT, waves, t0, tiles, tiles, tiles);
    // where two workgroups of the all-in-one kernel share a CU -- short k, few column tiles -- that form stays: 52.7 against
    // 62.3 us at 184 -> 96 + 32, N = 169,343
    if (nh >= 2 && r.l[l].per_cu < 2) {
      const GemmLongKLaunch roles = gemm_longk_form(LONGK_ROLES, K, NT, waves, t0, tiles, tiles, nh);
      if (roles.status == EGC_OK) r.l[l] = roles;
    }
    if (r.l[l].status != EGC_OK) return r;
    t0 += tiles;
  }
  r.status = EGC_OK;
  return r;
}

// Shapes served by the long-k kernels: 128 < F_in <= 384, at most 32 column tiles of 16 (two launches beyond 16), every launch fits.
inline bool gemm_longk_shape(int f_in, int NT) {
  if (f_in <= 128 || f_in > 384 || (f_in & 3) != 0 || NT < 1 || NT > 32) return false;
  const int per_launch = NT <= 16 ? NT : (NT + 1) / 2, narrow = NT <= 16 ? NT : NT / 2;
  if ((f_in + 31) / 32 == 12 && per_launch > 12) return false;  // 96 weight registers do not fit four wavefronts per SIMD
  // a narrow GEMM over a long k -- the dx GEMM of a layer with few input features -- has too few wavefronts to stage its tile
  // by themselves: its narrower launch must fit the all-in-one form too, whichever form runs (bf16x3 kernels otherwise)
  return gemm_longk_form(LONGK_ALL_IN_ONE, f_in, NT, 16, 0, narrow, narrow, narrow).status == EGC_OK &&
         gemm_longk_launches(f_in, NT).status == EGC_OK;
}

// ---- the plan
enum GemmLayout { GEMM_BF16X3, GEMM_F16X2, GEMM_F16X2K };
struct GemmPlan {
  bool valid;          // f_in > 0, f_g > 0, w_cols >= 0
  int f_in, f_g, w_cols;
  GemmLayout layout;   // fragment order of the packed planes = the family that runs
  int ldb, NV, KS;     // bases row stride, virtual columns (multiple of 32), k-steps of 32 (every family counts them alike)
  int TB, NT;          // long k: column tiles of 16 that hold the bases / all column tiles
  size_t pack_bytes[3], pack_bytes_max;   // by layout; what egc_basis_pack_bytes answers (it is asked before any flag is known)
};

// Shapes served by the fp16x2 register-stationary kernel.
// (a wavefront's 32 columns lie in `bases` or in `weightings`: ldb % 32 == 0 -- or there are no weightings at all, as in the d x
// GEMM of the 168- and 184-wide nets, [d bases | d weightings] (128 columns) x wcat^T -> 168 / 184: round 6, 117.7 -> ~60 us at
// CIFAR b2048 against the three-plane kernel those shapes took before)
inline bool gemm_f16x2_shape(int f_in, int ldb, int NV, int w_cols) {
  return f_in > 96 && f_in <= 128 && f_in % 4 == 0 && NV == 192 && (ldb % 32 == 0 || w_cols == 0);
}

// flags & EGC_GEMM_24BIT: operands split into THREE bf16 planes (24 significand bits: nothing of an fp32 operand is
// dropped) whatever the shape -- the fp16x2 forms keep 22 bits, which layers with std / var amplify (egc_hip.h)
inline GemmPlan gemm_plan(int f_in, int f_g, int w_cols, int flags) {
  GemmPlan p = {f_in > 0 && f_g > 0 && w_cols >= 0, f_in, f_g, w_cols};
  if (!p.valid) return p;
  p.ldb = (f_g + 3) & ~3;
  p.NV = (p.ldb + w_cols + 31) & ~31;
  p.KS = (f_in + GEMM_KT - 1) / GEMM_KT;
  p.TB = (p.ldb + 15) / 16, p.NT = p.TB + (w_cols + 15) / 16;
  const bool fp16 = (flags & EGC_GEMM_24BIT) == 0;
  p.layout = fp16 && gemm_f16x2_shape(f_in, p.ldb, p.NV, w_cols) ? GEMM_F16X2 : fp16 && gemm_longk_shape(f_in, p.NT) ? GEMM_F16X2K : GEMM_BF16X3;
  p.pack_bytes[GEMM_BF16X3] = (size_t)p.KS * 3 * p.NV * GEMM_KT * sizeof(uint16_t);
  p.pack_bytes[GEMM_F16X2] = (size_t)p.KS * 2 * p.NV * GEMM_KT * sizeof(uint16_t) + (size_t)p.NV * sizeof(float);
  p.pack_bytes[GEMM_F16X2K] = (size_t)p.NT * p.KS * 2 * 64 * 8 * sizeof(uint16_t) + (size_t)p.NT * 16 * sizeof(float);
  p.pack_bytes_max = std::max(std::max(p.pack_bytes[0], p.pack_bytes[1]), p.pack_bytes[2]);
  return p;
}

// ---- bf16x3
struct GemmBf16x3Launch {
  int ksub;       // > 0: basis_gemm_ws_kernel<ksub>, the weights stay in registers as 2 | 4 | 6 | 8 sub-steps of 16 k; else
  int nt;         // basis_gemm_bf16x3_kernel<vec4, nt>: nt = 7 | 6 | 4 column tiles per block, or 0 = a run-time count
  bool vec4;      // x is read in 16-byte pieces (F_in % 4 == 0, x 16-byte aligned)
  int vblock0;    // staged: first 192-column block of the launch
  unsigned grid_x, grid_y;
  int threads, pieces, n_tiles;   // weight-stationary: 16-byte pieces of an x tile (at most 4 per thread), row tiles the grid walks
  size_t lds;            // weight-stationary: dynamic; staged: the kernel's own static allocation
};

inline GemmLaunches<GemmBf16x3Launch> gemm_bf16x3_launches(int64_t M, int f_in, int NV, bool vec4) {
  GemmLaunches<GemmBf16x3Launch> r = {};
  if (f_in <= 128 && NV <= 256) {  // weight-stationary form (<= 8 wavefronts of 32 columns)
    GemmBf16x3Launch& g = r.l[0];
    g = {f_in <= 32 ? 2 : f_in <= 64 ? 4 : f_in <= 96 ? 6 : 8, 0, vec4, 0, 0, 1, 2 * NV};
    g.pieces = WS_ROWS * (16 * g.ksub) / 4;
    if (g.threads * 4 >= g.pieces) {   // (else: too few wavefronts to stage a tile: the LDS-staged kernel)
      r.status = gemm_row_tiles(M, WS_ROWS, g.n_tiles);
      r.n = r.status == EGC_OK;
      g.lds = (size_t)2 * 3 * WS_ROWS * (16 * g.ksub + 8) * sizeof(uint16_t);
      // persistent grid: enough blocks to fill the chip a few times over, each walks tiles with stride gridDim
      g.grid_x = (unsigned)gemm_grid(NV <= 128 ? 4 : 2, g.n_tiles);
      return r;
    }
  }
  int mblocks;
  if ((r.status = gemm_row_tiles(M, XBM, mblocks)) != EGC_OK) return r;
  auto staged = [&](int nt, unsigned grid_y, int vblock0) {
    r.l[r.n++] = {0, nt, vec4, vblock0, (unsigned)mblocks, grid_y, 256, 0, 0, (size_t)3 * (XBM + (nt == 7 ? 224 : XBN)) * XLD * sizeof(uint16_t)};
  };
  const int full = NV / XBN;   // column blocks of the full 192 columns; a narrower remainder block follows
  if (NV == 224 && vec4) { staged(7, 1, 0); return r; }   // 193..224 columns: one 7-tile block, one pass over x
  if (full > 0) staged(6, (unsigned)full, 0);
  if (NV % XBN != 0) staged(vec4 && NV - full * XBN == 128 ? 4 : 0, 1, full);   // a 128-column remainder (or GEMM): pipelined too
  return r;
}

// ---- row ranges.  The fp16x2 kernels address x, bases and weightings through 32-bit buffer offsets (and drop masked stores at offset 2^31 +
// scalar row offset): row ranges of less than 2 GiB per array, whole row tiles each, are launched one after another.
// f(r0, rows) -> status.  EGC_GEMM_MAX_ROWS (tests) lowers the bound.
template <class F>
int gemm_for_row_ranges(int64_t M, int64_t widest, int tile_rows, F&& f) {
  const int64_t whole = ~(int64_t)(tile_rows - 1);
  int64_t max_rows = ((int64_t)0x7FFFFFF0 / (4 * widest)) & whole;
  if (const char* e = getenv("EGC_GEMM_MAX_ROWS")) max_rows = std::max<int64_t>(tile_rows, atoll(e) & whole);
  for (int64_t r0 = 0; r0 < M; r0 += max_rows)
    if (const int st = f(r0, std::min(max_rows, M - r0)); st != EGC_OK) return st;
  return EGC_OK;
}

// ---- the entry points' checks
inline bool gemm_sizes_ok(int64_t n_nodes, int f_in, int f_g, int w_cols, int ldb) {
  return n_nodes >= 0 && f_in > 0 && f_g > 0 && w_cols >= 0 && ldb == ((f_g + 3) & ~3);
}
inline bool gemm_pointers_ok(const void* x, const void* packed, const void* bases, const void* weightings, int w_cols) {
  return x != nullptr && packed != nullptr && bases != nullptr && (w_cols == 0 || weightings != nullptr);
}

}  // namespace egc
