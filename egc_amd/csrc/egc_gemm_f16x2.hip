// Basis transform + weightings Linear on the fp16 matrix cores with fp32-level accuracy (gfx950), for the
// shapes whose whole weight matrix fits the register files of one block (F_in <= 128, 192 virtual columns:
// the north-star layer).
//
//     [bases | weightings] = x[N,F_in] @ [bases_weight | comb.weight^T]  (+ comb.bias)
//
// Reference behaviour replaced: torch.matmul(x, bases_weight) (experiments/layers.py:97-101,
// optimized_layers.py:180) and comb_weights(x) (layers.py:110, optimized_layers.py:182).
//
// Split: every x row and every weight column is first scaled by a power of two so that its largest
// magnitude lies in [1, 2) (exact), then written as
//     xs = xh + 2^-11 xl,     ws = wh + 2^-11 wl        (xh = fp16(xs), xl = fp16(2^11 (xs - xh)))
// fp16 carries an 11-bit significand, so the two planes hold ~22 bits and the remainder is < 2^-22 of the
// row / column maximum; xl and wl are stored pre-multiplied by 2^11 so that they stay normal numbers.
// Three products are accumulated in fp32 on v_mfma_f32_32x32x16_f16,
//     acc0 = xh wh,     acc1 = xh wl + xl wh,     result = 2^ex 2^ew (acc0 + 2^-11 acc1),
// the dropped xl*wl term and the plane remainders are ~2^-22 relative: the result is within a few fp32
// roundings of the reference's fp32 GEMM (parity tests: <= 1e-5).  Three MFMAs per k-step instead of the
// six of the bf16x3 split (egc_gemm_bf16x3.hip) put this GEMM back under its 217 MB of HBM traffic.
//
// Structure: persistent blocks of 12 wavefronts (one per CU), 64-row x tiles double-buffered in LDS as two
// fp16 planes, wavefront (ct, rt) owns column tile ct of row half rt and keeps BOTH planes of its weight tile in registers for the
// whole kernel; all global traffic through buffer instructions; LDS-only barriers (details at the kernel).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "egc_common.h"
#include "egc_gemm_host.h"
#include "egc_gemm_split.h"

namespace egc {

constexpr int F16X2_KP = 128;          // k extent of the register-resident weight block (F_in <= 128, zero beyond F_in)

// packed[column tile][k-step][plane][lane][8] (fp16 bits, the MFMA B fragments as they are loaded) followed by float inv_scale[NV].  One wavefront per virtual column
// (runs once per parameter update -- every step when training): lanes stride over k, the column maximum is a
// wavefront all-reduce.
__global__ void __launch_bounds__(64) pack_f16x2_kernel(const float* __restrict__ wcat, int64_t rs, int64_t cs, int K, int F_g,
                                                        int W, int ldb, int NV, int KS, u16* __restrict__ packed) {
  const int v = blockIdx.x;
  const int lane = threadIdx.x;
  const int src = (v < F_g) ? v : ((v < ldb || v >= ldb + W) ? -1 : v - ldb + F_g);
  unsigned amax = 0;
  if (src >= 0)
    for (int k = lane; k < K; k += 64) amax = max(amax, __float_as_uint(wcat[k * rs + src * cs]) & 0x7fffffffu);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, d));
  const F16x2ColScale col = f16x2_col_scale(amax);
  for (int k = lane; k < KS * GEMM_KT; k += 64) {
    const F16x2Bits b = f16x2_pack_split((src >= 0 && k < K) ? wcat[k * rs + src * cs] * col.scale : 0.f);
    // fragment order: the B operand of k-step s (16 k), plane p, column tile ct is 64 lanes x 8 halves, lane
    // 32 (k % 16 / 8) + column % 32 -- a wavefront of the GEMM fetches it as ONE contiguous KiB (with the planes laid
    // out [k-slab][plane][column][32 k] every lane's 16 bytes sat in a line of their own, and the 196 KB of weight
    // loads of a block took ~3 us of its prologue)
    const int64_t base = ((((int64_t)(v >> 5) * (F16X2_KP / 16) + (k >> 4)) * 2) * 64 + 32 * ((k & 15) >> 3) + (v & 31)) * 8 + (k & 7);
    packed[base] = b.h;
    packed[base + 64 * 8] = b.l;
  }
  if (lane == 0) reinterpret_cast<float*>(packed + (int64_t)KS * 2 * NV * GEMM_KT)[v] = col.inv;
}

// What bounds this kernel is each SIMD's vector issue port and its matrix pipe TOGETHER: a VALU instruction
// holds the port for 4 cycles, a v_mfma_f32_32x32x16_f16 for 8 and the pipe for 32 (MI355X_MICROARCH.md,
// constants table), so a tile runs at the pipe's pace only if about six vector instructions sit behind every
// MFMA, everywhere in the loop.  The vector work of a tile is about 150 instructions per wavefront (split of
// the next tile ~25 per 16-byte piece, scale/bias/store of the outputs ~68) against 24 MFMAs, so:
//   * a block is 12 wavefronts = 6 column tiles x 2 row halves of a 64-row x tile, one block per CU, 3
//     wavefronts per SIMD (two 6-wavefront blocks per CU do not become co-resident: measured);
//   * the epilogue of tile i is deferred into the MFMA loop of tile i+1: only t = acc0 + 2^-11 acc1 is formed
//     right after the loop (16 registers carried across the barrier), scaling, bias and stores follow beside
//     k-steps 0-3 of the next tile; the split of tile i+2 sits beside k-steps 4-7;
//   * no packed-f32 arithmetic (slower than two scalar operations next to MFMAs), |x| maxima through source
//     modifiers, the row exponent by integer operations, the low plane by one mixed-precision fma per element.
//
// x reaches the CU by LDS-DMA (buffer_load_dwordx4 ... lds: no VGPR destination) into a ring of two raw fp32
// tiles per block: registers cannot hold a prefetch deep enough to cover HBM latency (measured with one tile
// of register prefetch: 19 GB/s per CU).  Every thread later reads back exactly the 16-byte pieces its own
// wavefront requested -- ordered by that wavefront's counted vmcnt alone -- splits them into the fp16 planes
// and the wavefront immediately re-arms the slot with the tile three ahead: 64 KB per CU always in flight.
constexpr int F16X2_THREADS = 768;      // 6 column tiles x 2 row halves
constexpr int F16X2_ROWS = 64;
constexpr int F16X2_LDX = F16X2_KP + 8;
constexpr int F16X2_RAW_BYTES = F16X2_ROWS * F16X2_KP * 4;                  // one raw fp32 tile
constexpr int F16X2_PLANE_BYTES = 2 * 2 * F16X2_ROWS * F16X2_LDX * 2;       // two buffers x two planes
constexpr int F16X2_STORES_PER_TILE = 16;  // per wavefront (vmcnt arithmetic below)
constexpr int F16X2_CNT_SLOTS = 8;         // ring of per-row 1 / max(cnt, 1) of the folded form (a tile's slot lives 5 tiles)
constexpr int F16X2_LDS_BYTES = F16X2_PLANE_BYTES + 2 * F16X2_RAW_BYTES + 3 * F16X2_ROWS * 4 + (F16X2_CNT_SLOTS * F16X2_ROWS + 4) * 4;

// Folded weightings (FM >= 0: egc_layer_forward_packed with sum and mean in the aggregator list, egc_hip.h).  mean = sum /
// max(cnt, 1) over the same entries, so  w_sum sum + w_mean mean = (w_sum + w_mean / max(cnt, 1)) sum:  the GEMM writes
// H B (A - 1) weightings per row, the sum column carrying the mean's weighting, and the aggregate forms no mean.  In the
// HBA order the A = 4 weightings of a (h, b) pair are one lane quad of a wavefront, FM is the mean's place in it: one DPP
// broadcast inside the quad and one fma per element fold them, the mean lane's store is dropped and the others close ranks
// (output column 3 pair + a - (a > FM)).  cnt comes from the graph's deg^-1/2 table of the aggregators' edge set (dis^-2 =
// cnt exactly after rounding to an integer, for rows of fewer than 2^20 entries), brought in by LDS-DMA like the x tiles
// and turned into the aggregate's own rcp(max(cnt, 1)) once per tile.

#define EGC_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

template <int FM>
__global__ void __launch_bounds__(F16X2_THREADS) basis_gemm_f16x2_kernel(const float* __restrict__ x,
                                                                          const u16* __restrict__ packed,
                                                                          const float* __restrict__ bcat, int64_t M, int K,
                                                                          int W, float* __restrict__ bases, int ldb,
                                                                          float* __restrict__ weightings, int NV,
                                                                          int rows_per_block, const float* __restrict__ dis,
                                                                          int fold_s) {
  constexpr int KP = F16X2_KP;
  constexpr int KSUB = KP / 16;         // 16-k MFMA steps
  constexpr int LDX = F16X2_LDX;
  constexpr int ROWS = F16X2_ROWS;
  constexpr int XBUF = 2 * ROWS * LDX;  // fp16 elements of one x buffer (2 planes)
  constexpr int nthreads = F16X2_THREADS;
  extern __shared__ __attribute__((aligned(16))) u16 smem_h2[];
  u16* xs = smem_h2;                                                             // [2][2][ROWS][LDX] fp16 planes
  char* raw = reinterpret_cast<char*>(smem_h2) + F16X2_PLANE_BYTES;              // [2][ROWS][KP] fp32 ring
  // inverse row scales of tile t live in row_inv[t % 3]: tile t-1's are still being read by its deferred
  // epilogue while the split of tile t+1 writes its own
  float* row_inv = reinterpret_cast<float*>(raw + 2 * F16X2_RAW_BYTES);          // [3][ROWS]
  float* icnt = row_inv + 3 * ROWS;                   // FM >= 0: [F16X2_CNT_SLOTS][ROWS] dis, then 1 / max(cnt, 1), of tile t at t % 8
  float* zero4 = icnt + F16X2_CNT_SLOTS * ROWS;  // 16 zero bytes: what the lanes other than the sum lanes fold with
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = wave % 6, rt = wave / 6;                       // column tile, 32-row half of the x tile
  const int l31 = lane & 31, hh = lane >> 5;
  const int cb = 32 * ct;
  // A block owns a CONTIGUOUS row range of M / gridDim rows (its last tile is partial: the DMA and the stores of the
  // rows beyond the range are dropped by range checks, and the loop is bound by those bytes): every block moves the
  // same bytes.  (Whole 64-row tiles dealt round-robin left 86 of 256 blocks with an 11th tile at config 2.)
  const int64_t row_lo = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row_hi = row_lo + rows_per_block < M ? row_lo + rows_per_block : M;
  const int n_tiles = (int)((row_hi - row_lo + F16X2_ROWS - 1) / F16X2_ROWS);

  f16x8 wf[KSUB][2];
  float col_inv, col_bias;
  // 16-byte pieces of a tile: piece pc = tid + 768 i  <->  (row pc / 32, k 4 (pc % 32)); i = 2 exists for
  // wavefronts 0-7 only (2048 pieces)
  constexpr unsigned GOOB = 0xFFFFFFF0u;  // out-of-range offset: loads return 0 -- no branches
  constexpr unsigned SOOB = 0x80000000u;  // same for the stores, which add a scalar offset (host: buffers < 2 GiB)
  const u32x4 rx = {(unsigned)(uintptr_t)x, (unsigned)((uintptr_t)x >> 32) & 0xffffu, (unsigned)(M * K * 4), 0x00020000u};
  // this wavefront's 32 columns lie either in `bases` or in `weightings` (host: ldb % 32 == 0, or W == 0: every tile in `bases`)
  const bool to_bases = cb < ldb;
  const int wcol_v = cb - ldb + l31;                  // weightings column of this lane (to_bases == false)
  const int qa = wcol_v & 3;                          // FM >= 0: place in the (h, b) pair's quad
  const int W_out = FM >= 0 ? W / 4 * 3 : W;          // row length of the weightings written
  const __amdgpu_buffer_rsrc_t ro =
      to_bases ? __builtin_amdgcn_make_buffer_rsrc((void*)bases, 0, (unsigned)(row_hi * ldb * 4), 0x00020000)
               : __builtin_amdgcn_make_buffer_rsrc((void*)weightings, 0, (unsigned)(row_hi * (int64_t)W_out * 4), 0x00020000);
  const int out_ld = to_bases ? ldb : W_out;
  const int out_col = to_bases ? cb + l31 : FM >= 0 ? 3 * (wcol_v >> 2) + qa - (qa > FM ? 1 : 0) : wcol_v;
  const bool col_ok = to_bases ? out_col < ldb : (wcol_v < W && (FM < 0 || qa != FM));
  const bool is_sum = FM >= 0 && !to_bases && qa == fold_s;
  const u32x4 rd = {(unsigned)(uintptr_t)dis, (unsigned)((uintptr_t)dis >> 32) & 0xffffu, (unsigned)(M * 4), 0x00020000u};
  const unsigned icnt_lds = (unsigned)(uintptr_t)icnt;
  const unsigned raw_lds = (unsigned)(uintptr_t)raw;  // LDS byte address of the ring
  const bool third = wave < 8;

  // one LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global offsets to 1 KiB of contiguous LDS
  auto dma_piece = [&](int tile, int slot, int i) {
    const int pc = tid + nthreads * i;
    const int row = pc >> 5;
    const int k4 = (pc & 31) * 4;
    const int64_t gm = row_lo + (int64_t)tile * ROWS + row;
    const bool ok = (tile < n_tiles) & (gm < row_hi) & (k4 < K);
    const unsigned voff = ok ? (unsigned)((gm * K + k4) * 4) : GOOB;
    const unsigned dst =
        __builtin_amdgcn_readfirstlane(raw_lds + slot * F16X2_RAW_BYTES + (wave * 64 + nthreads * i) * 16);  // wave-uniform
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(dst), "s"(rx)
                 : "memory");
  };
  // FM >= 0: the tile's 64 dis values (one dword per lane) -> its slot of the count ring, by wavefront 8 (one of the
  // wavefronts with two x pieces per tile: its DMA group then has three operations, like those of wavefronts 0-7)
  auto dma_cnt = [&](int tile) {
    const int64_t gm = row_lo + (int64_t)tile * ROWS + lane;
    const bool ok = (tile < n_tiles) & (gm < row_hi);
    const unsigned voff = ok ? (unsigned)(gm * 4) : GOOB;
    const unsigned dst = __builtin_amdgcn_readfirstlane(icnt_lds + (tile & (F16X2_CNT_SLOTS - 1)) * ROWS * 4);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(dst), "s"(rd)
                 : "memory");
  };
  auto dma_tile = [&](int tile, int slot) {
    dma_piece(tile, slot, 0);
    dma_piece(tile, slot, 1);
    if (third) dma_piece(tile, slot, 2);
    if (FM >= 0 && wave == 8) dma_cnt(tile);
  };
  // dis -> 1 / max(cnt, 1) in place (wavefront 8, once its own DMA of the slot has retired): cnt = dis^-2 rounded to an integer,
  // then the aggregate's own reciprocal.  dis == 0 (no entries, or rows past the range) gives 0.
  auto cnt_inverse = [&](int tile) {
    float* p = icnt + (tile & (F16X2_CNT_SLOTS - 1)) * ROWS + lane;
    const float d = *p;
    const float c = __builtin_rintf(__builtin_amdgcn_rcpf(d * d));
    *p = __builtin_amdgcn_rcpf(fmaxf(c, 1.f));
  };
  // A row is 32 consecutive pieces = one half wavefront: its largest magnitude is an all-reduce over 32 lanes, on the bit
  // patterns of the non-negative |maxima|
  auto row_amax = [&](const float4 v) -> unsigned { return row_group_umax<32>(__float_as_uint(f16x2_abs_max4(v))); };
  auto split_store = [&](int buf, int ri, int i, const float4 v, unsigned amax) {
    const int pc = tid + nthreads * i;
    const int row = pc >> 5;
    const int k4 = (pc & 31) * 4;
    const unsigned e = f16x2_row_exp(amax);
    const F16x2RowScale sc = f16x2_row_scale(e);
    const F16x2Planes p = f16x2_split4(v, sc);
    u16* dst = xs + buf * XBUF + row * LDX + k4;
    *reinterpret_cast<u32x2*>(dst) = p.hi;
    *reinterpret_cast<u32x2*>(dst + ROWS * LDX) = p.lo;
    row_inv[ri * ROWS + row] = __uint_as_float(e);  // 2^e; all 32 lanes of the row write the same word: no branch
  };
  auto raw_piece = [&](int slot, int i) -> float4 {
    return *reinterpret_cast<const float4*>(raw + slot * F16X2_RAW_BYTES + (tid + nthreads * i) * 16);
  };
  auto stage = [&](int buf, int ri, int slot, int i) {
    const float4 v = raw_piece(slot, i);
    split_store(buf, ri, i, v, row_amax(v));
  };
  // A operands (x): lane -> row 32 rt + l31, k = 16 s + 8 hh .. + 7
  auto frag = [&](int buf, int s, f16x8& xh, f16x8& xl) {
    const u16* xb = xs + buf * XBUF + (32 * rt + l31) * LDX + 16 * s + 8 * hh;
    xh = *reinterpret_cast<const f16x8*>(xb);
    xl = *reinterpret_cast<const f16x8*>(xb + ROWS * LDX);
  };
  f32x16 acc0, acc1, t;   // t: previous tile's acc0 + 2^-11 acc1, waiting for its scales
  auto mfma_step = [&](int s, const f16x8 xh, const f16x8 xl) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wf[s][0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wf[s][0], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wf[s][1], acc1, 0, 0, 0);
  };
  // D layout (x as the A operand): lane -> column cb + l31, rows 8 j + 4 hh + i: one dword store writes two
  // full 128-byte lines.  (With x as B a lane would hold 4 consecutive columns of one row and a dwordx4 store
  // would touch 32 lines: the stores, not the arithmetic, then set the tile time.)  Rows past M fall outside
  // the buffer and are dropped by its range check; the row part of the address is a scalar offset.
  auto epilogue = [&](unsigned voff, int j, const float* rinv_t, const float* icnt_t) {
    const float4 ri = *reinterpret_cast<const float4*>(rinv_t + 32 * rt + 8 * j + 4 * hh);
    // 2^ex 2^ew (acc0 + 2^-11 acc1) + bias; the scale product is a power of two, so the fma rounds once
    float v0 = __builtin_fmaf(t[4 * j], col_inv * ri.x, col_bias);
    float v1 = __builtin_fmaf(t[4 * j + 1], col_inv * ri.y, col_bias);
    float v2 = __builtin_fmaf(t[4 * j + 2], col_inv * ri.z, col_bias);
    float v3 = __builtin_fmaf(t[4 * j + 3], col_inv * ri.w, col_bias);
    if constexpr (FM >= 0) {
      if (!to_bases) {  // (wave-uniform) sum lane += mean lane's weighting x 1 / max(cnt, 1); the other lanes add 0 x it
        const float4 ic = *reinterpret_cast<const float4*>(is_sum ? icnt_t + 32 * rt + 8 * j + 4 * hh : zero4);
        constexpr int QP = FM | (FM << 2) | (FM << 4) | (FM << 6);  // quad_perm: every lane reads lane FM of its quad
        v0 = __builtin_fmaf(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v0), QP, 0xf, 0xf, false)), ic.x, v0);
        v1 = __builtin_fmaf(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v1), QP, 0xf, 0xf, false)), ic.y, v1);
        v2 = __builtin_fmaf(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v2), QP, 0xf, 0xf, false)), ic.z, v2);
        v3 = __builtin_fmaf(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v3), QP, 0xf, 0xf, false)), ic.w, v3);
      }
    }
    const int so = (8 * j) * out_ld * 4;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v0), ro, voff, so, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v1), ro, voff, so + out_ld * 4, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v2), ro, voff, so + 2 * out_ld * 4, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v3), ro, voff, so + 3 * out_ld * 4, 0);
  };
  auto out_offset = [&](int tile, bool valid) -> unsigned {
    return (valid & col_ok) ? (unsigned)(((row_lo + (int64_t)tile * ROWS + 32 * rt + 4 * hh) * out_ld + out_col) * 4) : SOOB;
  };
#define EGC_PIN __builtin_amdgcn_sched_barrier(0)

  constexpr int stride = 1;   // (tiles of this block's own range, in order)
  int tile = 0;
  if (n_tiles <= 0) return;
  if (FM >= 0 && tid < 4) zero4[tid] = 0.f;   // (made visible by the barrier before the loop)
  if (K < KP) {  // columns k >= K of a tile are out of range for the DMA and must read as 0
    for (int i = tid; i < 2 * F16X2_RAW_BYTES / 16; i += nthreads) reinterpret_cast<u32x4*>(raw)[i] = u32x4{0, 0, 0, 0};
    lds_barrier();
  }
  // first two tiles on their way before anything else: the weight loads below overlap their latency
  dma_tile(tile, 0);
  dma_tile(tile + stride, 1);
  // both planes of this wavefront's 128 x 32 weight block, as B operands of v_mfma_f32_32x32x16_f16:
  // lane -> column cb + l31, k = 16 s + 8 hh .. + 7
#pragma unroll
  for (int s = 0; s < KSUB; ++s)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      wf[s][p] = *reinterpret_cast<const f16x8*>(packed + ((((int64_t)ct * KSUB + s) * 2 + p) * 64 + lane) * 8);   // one KiB per wavefront
    }
  // every output element of a lane belongs to ONE column (cb + l31): its inverse scale and bias stay in registers
  col_inv = reinterpret_cast<const float*>(packed + (int64_t)(KP / GEMM_KT) * 2 * NV * GEMM_KT)[cb + l31];
  const int wcol = cb + l31 - ldb;
  col_bias = (bcat != nullptr && wcol >= 0 && wcol < W) ? bcat[wcol] : 0.f;
  EGC_VMCNT(0);
  // the compiler counts only its own loads: let it retire the weight loads HERE (the counter is already zero),
  // or its waits in the first tile would also drain the DMAs issued below
  asm volatile("" : "+v"(wf[0][0]), "+v"(wf[0][1]), "+v"(wf[1][0]), "+v"(wf[1][1]), "+v"(wf[2][0]), "+v"(wf[2][1]),
               "+v"(wf[3][0]), "+v"(wf[3][1]), "+v"(wf[4][0]), "+v"(wf[4][1]), "+v"(wf[5][0]), "+v"(wf[5][1]),
               "+v"(wf[6][0]), "+v"(wf[6][1]), "+v"(wf[7][0]), "+v"(wf[7][1]), "+v"(col_inv), "+v"(col_bias));
  stage(0, 0, 0, 0);
  stage(0, 0, 0, 1);
  if (third) stage(0, 0, 0, 2);
  dma_tile(tile + 2 * stride, 0);
  lds_barrier();
  int buf = 0;
  int ri_cur = 0;                 // row_inv slot of the tile being multiplied (tile index mod 3)
  unsigned prev_off = SOOB;       // no previous tile yet: its stores are dropped
  const float* prev_ri = row_inv;
  const float* prev_ic = icnt;
#pragma unroll
  for (int r = 0; r < 16; ++r) t[r] = 0.f;
  // In the loop every wavefront issues, per tile, F16X2_STORES_PER_TILE stores (k-steps 0-3) and then 3
  // (wavefronts 0-7) or 2 (8-11) DMA pieces (k-step 7), always in this order, and the counter retires them in
  // order.  When the pieces of the next tile are read (k-step 4), the operations issued after the DMA of piece
  // i are the rest of that DMA group, one whole tile of stores + DMA, and this tile's stores:
  //     piece 0: (2|1) + 16 + (3|2) + 16 = 37 | 35     piece 1: (1|0) + 16 + (3|2) + 16 = 36 | 34
  //     piece 2 (wavefronts 0-7 only):   0 + 16 +  3    + 16 = 35
  // A smaller count is always safe: one wait for 34 covers every piece of every wavefront.  (Folded form: wavefront 8 issues
  // the tile's count DMA after its two x pieces, so its pieces sit at 2 + 16 + 3 + 16 = 37 and 1 + 16 + 3 + 16 = 36.  Tile t's count
  // DMA, issued in iteration t - 3, is read after the wait of iteration t, with 16 + 3 + 16 + 3 + 16 = 54 operations behind it.)
  static_assert(F16X2_STORES_PER_TILE == 16, "vmcnt count below");
  for (; tile < n_tiles; tile += stride) {
    const int slot = buf ^ 1;  // ring slot of the next tile (tile index parity == plane buffer parity)
    const int ri_next = ri_cur == 2 ? 0 : ri_cur + 1;
    f16x8 xh, xl, yh, yl;
    frag(buf, 0, xh, xl);
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    // k-steps 0-3: the previous tile leaves
    frag(buf, 1, yh, yl);
    mfma_step(0, xh, xl);
    epilogue(prev_off, 0, prev_ri, prev_ic);
    EGC_PIN;
    frag(buf, 2, xh, xl);
    mfma_step(1, yh, yl);
    epilogue(prev_off, 1, prev_ri, prev_ic);
    EGC_PIN;
    frag(buf, 3, yh, yl);
    mfma_step(2, xh, xl);
    epilogue(prev_off, 2, prev_ri, prev_ic);
    EGC_PIN;
    frag(buf, 4, xh, xl);
    mfma_step(3, yh, yl);
    epilogue(prev_off, 3, prev_ri, prev_ic);
    EGC_PIN;
    // k-steps 4-7: the next tile is split and staged, its ring slot re-armed
    EGC_VMCNT(34);
    if (FM >= 0 && wave == 8) cnt_inverse(tile);   // (this tile's dis arrived with the DMA of three tiles ago)
    frag(buf, 5, yh, yl);
    mfma_step(4, xh, xl);
    stage(buf ^ 1, ri_next, slot, 0);
    EGC_PIN;
    frag(buf, 6, xh, xl);
    mfma_step(5, yh, yl);
    stage(buf ^ 1, ri_next, slot, 1);
    EGC_PIN;
    frag(buf, 7, yh, yl);
    mfma_step(6, xh, xl);
    if (third) stage(buf ^ 1, ri_next, slot, 2);
    EGC_PIN;
    mfma_step(7, yh, yl);
    dma_tile(tile + 3 * stride, slot);
    EGC_PIN;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = __builtin_fmaf(acc1[r], 1.f / 2048.f, acc0[r]);
    prev_off = out_offset(tile, true);
    prev_ri = row_inv + ri_cur * ROWS;
    prev_ic = icnt + (tile & (F16X2_CNT_SLOTS - 1)) * ROWS;
    ri_cur = ri_cur == 2 ? 0 : ri_cur + 1;
    lds_barrier();
    buf ^= 1;
  }
  epilogue(prev_off, 0, prev_ri, prev_ic);
  epilogue(prev_off, 1, prev_ri, prev_ic);
  epilogue(prev_off, 2, prev_ri, prev_ic);
  epilogue(prev_off, 3, prev_ri, prev_ic);
  EGC_VMCNT(0);  // no DMA may still be writing this block's LDS when it is handed to the next block
}

int f16x2_pack(const float* wcat, int64_t rs, int64_t cs, const GemmPlan& p, void* packed, hipStream_t stream) {
  pack_f16x2_kernel<<<p.NV, 64, 0, stream>>>(wcat, rs, cs, p.f_in, p.f_g, p.w_cols, p.ldb, p.NV, p.KS, (u16*)packed);
  EGC_LAUNCH_CHECK("pack_f16x2_kernel");
  return EGC_OK;
}

int f16x2_launch(const float* x, const void* packed, const float* bcat, int64_t M, const GemmPlan& p, float* bases,
                 float* weightings, hipStream_t stream, const float* dis, int fold_s, int fold_m) {
  const int K = p.f_in, W = p.w_cols, ldb = p.ldb, NV = p.NV;
  if (p.layout != GEMM_F16X2 || !aligned16(x)) return EGC_ERR_UNSUPPORTED;   // (the kernel's shapes: gemm_f16x2_shape)
  const bool fold = fold_m >= 0;
  if (fold && (dis == nullptr || W % 32 != 0 || fold_m > 3 || fold_s < 0 || fold_s > 3 || fold_s == fold_m)) return EGC_ERR_INVALID;
  const int W_out = fold ? W / 4 * 3 : W;
  static_assert(F16X2_LDS_BYTES <= 160 * 1024, "LDS of one CU");
  return gemm_for_row_ranges(M, std::max(std::max(K, ldb), W), F16X2_ROWS, [&](int64_t r0, int64_t rows) -> int {
    int n_tiles;
    if (const int st = gemm_row_tiles(rows, F16X2_ROWS, n_tiles); st != EGC_OK) return st;
    const int grid = gemm_grid(1, n_tiles);  // one 12-wavefront block per CU (registers: 3 wavefronts per SIMD)
    const int rows_per_block = (int)((rows + grid - 1) / grid);   // contiguous, equal row ranges
    // one instantiation per place of the mean in the quad (FM) and the plain form (FM = -1)
    auto launch = [&](auto fm) -> int {
      EGC_ALLOW_DYNAMIC_LDS(&basis_gemm_f16x2_kernel<fm()>, 160 * 1024, "f16x2");
      basis_gemm_f16x2_kernel<fm()><<<grid, F16X2_THREADS, (size_t)F16X2_LDS_BYTES, stream>>>(
          x + r0 * K, (const u16*)packed, bcat, rows, K, W, bases + r0 * ldb, ldb, weightings != nullptr ? weightings + r0 * W_out : nullptr,
          NV, rows_per_block, fold ? dis + r0 : nullptr, fold ? fold_s : -1);
      EGC_LAUNCH_CHECK("basis_gemm_f16x2_kernel");
      return EGC_OK;
    };
    switch (fold_m) {
      case 0: return launch(std::integral_constant<int, 0>{});
      case 1: return launch(std::integral_constant<int, 1>{});
      case 2: return launch(std::integral_constant<int, 2>{});
      case 3: return launch(std::integral_constant<int, 3>{});
      default: return launch(std::integral_constant<int, -1>{});
    }
  });
}

}  // namespace egc
