// Basis transform + weightings Linear for F_in > 128 on the fp16 matrix cores with fp32-level accuracy (gfx950):
// the register-stationary fp16x2 scheme of egc_gemm_f16x2.hip carried to long k (128 < F_in <= 384) -- the
// reference's ogbn-mag layers (352 wide, mag/models.py:23-53) and its other trained nets (136 ... 304 wide).
//
//     [bases | weightings] = x[N,F_in] @ [bases_weight | comb.weight^T]  (+ comb.bias)
//
// Reference behaviour replaced: torch.matmul(x, bases_weight) (experiments/layers.py:97-101,
// optimized_layers.py:180) and comb_weights(x) (layers.py:110, optimized_layers.py:182).
//
// Numerics: exactly those of egc_gemm_f16x2.hip -- every x row and weight column scaled by a power of two so that
// its largest magnitude lies in [1, 2), xs = xh + 2^-11 xl in two fp16 planes (same for w), three products
// (xh wh, xh wl + xl wh) accumulated in fp32, result 2^ex 2^ew (acc0 + 2^-11 acc1): ~2^-22 relative.
//
// What changes with long k is WHERE the weights can live.  [F_in x 208 columns] in two fp16 planes is 293 KB at the
// ogbn-mag shape: no LDS holds it and a 32-column register block (176 registers) leaves no room for anything else,
// which is why the bf16x3 kernel re-stages the weights from L2 every k-step and ends up LDS-bandwidth bound (1.0 ms
// against 0.26 ms of HBM or MFMA time).  Here a wavefront owns SIXTEEN columns for the whole k range
// (v_mfma_f32_16x16x32_f16: 4 registers per plane and k-step of 32 -> 88 registers at F_in = 352) and one workgroup
// of up to 16 wavefronts covers up to 256 virtual columns: the weights are read from memory ONCE per workgroup.
// x arrives by LDS-DMA into a ring of two raw fp32 tiles of 16 rows (the row maximum needs the whole row before
// the first MFMA, so a tile is complete rows), is split into two fp16 planes (double-buffered) half a wavefront
// per row, and every wavefront multiplies the same 16 x F_in planes by its own weights: per tile and wavefront
// 3 KS MFMAs of 16 cycles against 2 KS LDS reads of 1 KB.  One barrier per tile: the split of tile t + 1 and
// the MFMAs of tile t sit between the same two barriers, so the vector work of one wavefront runs beside the matrix
// work of another.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "egc_common.h"
#include "egc_gemm_host.h"
#include "egc_gemm_split.h"

namespace egc {

// Virtual column space: column tiles of 16; tiles [0, TB) hold the bases columns (ldb of them, the rest of the last
// tile is padding that is never stored), tiles [TB, NT) the weightings columns.
struct KCols {
  int F_g, ldb, W, TB, NT;
  __host__ __device__ inline int source(int v) const {  // column of wcat behind virtual column v, or -1
    const int t = v >> 4;
    if (t < TB) return v < F_g ? v : -1;
    const int w = v - 16 * TB;
    return w < W ? F_g + w : -1;
  }
};

// packed: [NT][KS][2 planes][64 lanes][8] fp16 -- the A fragments of v_mfma_f32_16x16x32_f16 in register order
// (lane (i, kq) holds k = 32 s + 8 kq .. + 7 of column 16 t + i) -- followed by float inv_scale[16 NT].
// One wavefront per virtual column: lanes stride over k, the column maximum is a wavefront all-reduce.
__global__ void __launch_bounds__(64) pack_f16x2k_kernel(const float* __restrict__ wcat, int64_t rs, int64_t cs, int K,
                                                         KCols c, int KS, u16* __restrict__ packed) {
  const int v = blockIdx.x;
  const int lane = threadIdx.x;
  const int src = c.source(v);
  unsigned amax = 0;
  if (src >= 0)
    for (int k = lane; k < K; k += 64) amax = max(amax, __float_as_uint(wcat[k * rs + src * cs]) & 0x7fffffffu);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, d));
  const F16x2ColScale col = f16x2_col_scale(amax);
  const int t = v >> 4, i = v & 15;
  for (int k = lane; k < KS * 32; k += 64) {
    const F16x2Bits b = f16x2_pack_split((src >= 0 && k < K) ? wcat[k * rs + src * cs] * col.scale : 0.f);
    const int s = k >> 5, kq = (k >> 3) & 3, e = k & 7;
    const int64_t base = ((((int64_t)t * KS + s) * 2) * 64 + (kq * 16 + i)) * 8 + e;
    packed[base] = b.h;
    packed[base + 64 * 8] = b.l;
  }
  if (lane == 0) reinterpret_cast<float*>(packed + (int64_t)c.NT * KS * 2 * 64 * 8)[v] = col.inv;
}

template <int N>
__device__ inline void vmwait_k() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// wave-uniform runtime count (DMA wave-instructions per tile depend on F_in and the workgroup size)
__device__ inline void vmwait_rt(int n) {
  switch (n) {
    case 0: vmwait_k<0>(); break;   case 1: vmwait_k<1>(); break;   case 2: vmwait_k<2>(); break;
    case 3: vmwait_k<3>(); break;   case 4: vmwait_k<4>(); break;   case 5: vmwait_k<5>(); break;
    case 6: vmwait_k<6>(); break;   case 7: vmwait_k<7>(); break;   case 8: vmwait_k<8>(); break;
    case 9: vmwait_k<9>(); break;   case 10: vmwait_k<10>(); break; case 11: vmwait_k<11>(); break;
    case 12: vmwait_k<12>(); break; case 13: vmwait_k<13>(); break; case 14: vmwait_k<14>(); break;
    case 15: vmwait_k<15>(); break; case 16: vmwait_k<16>(); break; case 17: vmwait_k<17>(); break;
    case 18: vmwait_k<18>(); break; case 19: vmwait_k<19>(); break; case 20: vmwait_k<20>(); break;
    case 21: vmwait_k<21>(); break; case 22: vmwait_k<22>(); break; case 23: vmwait_k<23>(); break;
    case 24: vmwait_k<24>(); break; case 25: vmwait_k<25>(); break; case 26: vmwait_k<26>(); break;
    case 27: vmwait_k<27>(); break; case 28: vmwait_k<28>(); break; case 29: vmwait_k<29>(); break;
    case 30: vmwait_k<30>(); break; case 31: vmwait_k<31>(); break; case 32: vmwait_k<32>(); break;
    default: vmwait_k<0>(); break;
  }
}

template <int KS, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) basis_gemm_f16x2k_kernel(const float* __restrict__ x, const u16* __restrict__ packed,
                                                                      const float* __restrict__ bcat, int64_t M, int K,
                                                                      KCols c, float* __restrict__ bases,
                                                                      float* __restrict__ weightings, int n_tiles, int LDX,
                                                                      int R, int slot_bytes, int tile0, int ring,
                                                                      const float* __restrict__ addend) {
  extern __shared__ __attribute__((aligned(16))) char smem_k[];
  char* raw = smem_k;                                                    // [ring][slot_bytes] raw fp32 tiles (DMA ring)
  u16* xs = reinterpret_cast<u16*>(smem_k + ring * slot_bytes);          // [2 buffers][2 planes][KROWS][LDX] fp16
  float* row_inv = reinterpret_cast<float*>(xs + 4 * KROWS * LDX);       // [2 buffers][KROWS]
  float* colinfo = row_inv + 2 * KROWS;                                  // [16 NT][2]: inverse column scale, bias
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = tile0 + wave;                                           // this wavefront's column tile (a launch covers tiles tile0 .. tile0 + wavefronts - 1)
  const int j = lane & 15, quad = lane >> 4;
  const int K4 = K >> 2;                                                 // 16-byte pieces per row
  constexpr unsigned GOOB = 0xFFFFFFF0u;
  const u32x4 rx = {(unsigned)(uintptr_t)x, (unsigned)((uintptr_t)x >> 32) & 0xffffu, (unsigned)(M * K * 4), 0x00020000u};
  const unsigned raw_lds = (unsigned)(uintptr_t)raw;
  const unsigned magic_K4 = (unsigned)(((uint64_t)1 << 32) / (uint64_t)K4) + 1u;

  // one LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global offsets to 1 KiB of contiguous LDS
  auto dma_tile = [&](int tile, int slot) {
    for (int i = 0; i < R; ++i) {
      const int pc = tid + nthreads * i;
      const int row = (int)__umulhi((unsigned)pc, magic_K4);   // pc / K4 for pc < 2^16
      const int k4 = pc - row * K4;
      const int64_t gm = (int64_t)tile * KROWS + row;
      const bool ok = (tile < n_tiles) & (row < KROWS) & (gm < M);
      const unsigned voff = ok ? (unsigned)((gm * K + 4 * k4) * 4) : GOOB;
      const unsigned dst = __builtin_amdgcn_readfirstlane(raw_lds + slot * slot_bytes + (wave * 64 + nthreads * i) * 16);
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff), "s"(dst), "s"(rx)
                   : "memory");
    }
  };

  const int stride = gridDim.x;
  int tile = blockIdx.x;
  if (tile >= n_tiles) return;
  for (int r = 0; r < ring; ++r) dma_tile(tile + r * stride, r);    // `ring` tiles of x per CU in flight (two left HBM latency exposed: 3.8 TB/s)
  // zero the planes once: the k range [K, 32 KS) and the row padding are never written again
  for (int i = tid; i < 4 * KROWS * LDX / 8; i += nthreads) reinterpret_cast<u32x4*>(xs)[i] = u32x4{0, 0, 0, 0};

  // both planes of this wavefront's F_in x 16 weight block, as A operands
  f16x8 wf[KS][2];
  {
    const u16* src = packed + ((int64_t)ct * KS * 2 * 64 + lane) * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      wf[s][0] = *reinterpret_cast<const f16x8*>(src + (s * 2) * 64 * 8);
      wf[s][1] = *reinterpret_cast<const f16x8*>(src + (s * 2 + 1) * 64 * 8);
    }
  }
  // output addressing: lane (j, quad) holds, per row block, row 16 rb + j and virtual columns 16 ct + 4 quad .. + 3
  const bool to_bases = ct < c.TB;
  const int out_ld = to_bases ? c.ldb : c.W;
  const int col0 = to_bases ? 16 * ct + 4 * quad : 16 * (ct - c.TB) + 4 * quad;
  const int lim = to_bases ? c.ldb : c.W;
  float* outp = to_bases ? bases : weightings;
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)outp, 0, (unsigned)(M * out_ld * 4), 0x00020000);
  const float* inv_tab = reinterpret_cast<const float*>(packed + (int64_t)c.NT * KS * 2 * 64 * 8);
  // inverse column scales and biases live in LDS (8 registers less next to the 8 KS weight registers)
  for (int v = tid; v < 16 * c.NT; v += nthreads) {
    const int w = v - 16 * c.TB;
    colinfo[2 * v] = inv_tab[v];
    colinfo[2 * v + 1] = (w >= 0 && w < c.W && bcat != nullptr) ? bcat[w] : 0.f;
  }
  const bool vec_store = (out_ld & 3) == 0;
  // `addend` (the host passes it only where the bases rows are stored as 16-byte pieces): out = x W + addend on the bases columns --
  // the residual branch's gradient joining d x in the d x GEMM's store (one 16-byte load per lane and tile, requested right after
  // the barrier, ahead of the tile's DMA requests, by inline assembly: the compiler, which cannot see the DMAs, would wait for
  // everything)
  const bool add = addend != nullptr && to_bases;    // wave-uniform
  const u32x4 ra = {(unsigned)(uintptr_t)addend, (unsigned)((uintptr_t)addend >> 32) & 0xffffu, add ? (unsigned)(M * out_ld * 4) : 0u, 0x00020000u};
  vmwait_k<0>();
  // the compiler counts only its own loads: let it retire the weight loads HERE
#pragma unroll
  for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(wf[s][0]), "+v"(wf[s][1]));
  // the first tiles were requested before the weight loads: all have landed by now (vmcnt(0) above)
  lds_barrier();

  const int hw = tid >> 5;                    // half-wavefront index: one row of the tile per half-wavefront and pass
  const int hl = tid & 31;
  const int n_hw = nthreads >> 5;
  const int n_stores = vec_store ? 1 : 4;     // store instructions per tile and wavefront
  // raw fp32 rows of ring slot `rslot` -> the two fp16 planes of buffer `pbuf` + row scales
  auto split = [&](int rslot, int pbuf) {
    const char* rs = raw + rslot * slot_bytes;
    u16* xp = xs + pbuf * 2 * KROWS * LDX;
    for (int row = hw; row < KROWS; row += n_hw) {
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k4 = hl + 32 * i;
        if (k4 < K4) {
          const float4 v = *reinterpret_cast<const float4*>(rs + ((size_t)row * K4 + k4) * 16);
          m = fmaxf(m, f16x2_abs_max4(v));
        }
      }
      const unsigned e = f16x2_row_exp(row_group_umax<32>(__float_as_uint(m)));
      const F16x2RowScale sc = f16x2_row_scale(e);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k4 = hl + 32 * i;
        if (k4 < K4) {
          const float4 v = *reinterpret_cast<const float4*>(rs + ((size_t)row * K4 + k4) * 16);   // second read: 12 registers less
          const F16x2Planes p = f16x2_split4(v, sc);
          u16* dst = xp + row * LDX + 4 * k4;
          *reinterpret_cast<u32x2*>(dst) = p.hi;
          *reinterpret_cast<u32x2*>(dst + KROWS * LDX) = p.lo;
        }
      }
      if (hl == 0) row_inv[pbuf * KROWS + row] = __uint_as_float(e);  // 2^e
    }
  };
  split(0, 0);
  // One barrier per tile.  At the top of iteration t (tile t of this workgroup): ring slots (t + 1) % ring ... hold or await
  // the raw tiles t + 1 ... t + ring - 1, plane buffer t % 2 the split tile t.  After the barrier the slot t % ring is free
  // (everybody has split tile t) and is re-armed with tile t + ring at once; then the wavefronts split tile t + 1 into the
  // other plane buffer and multiply tile t, in whatever order they get there: the vector work of one wavefront runs beside
  // the matrix work of another.  The wait at the top is for this wavefront's own pieces of tile t + 1: behind them in the
  // (in-order) counter are the pieces of tiles t + 2 ... t + ring - 1 and the last tile's stores.
  int cur = 0, slot = 0;
  const int behind = (ring - 2) * (R + (add ? 1 : 0)) + n_stores;
  for (bool first = true; tile < n_tiles; tile += stride, first = false) {
    if (first) vmwait_k<0>(); else vmwait_rt(behind);
    lds_barrier();
    f4 av;                  // (no initial value: a second definition would be a copy the compiler may place ahead of the wait)
    asm volatile("" : "=v"(av));
    if (add) {
      const int64_t arow = (int64_t)tile * KROWS + j;
      const unsigned aoff = (arow < M && col0 + 3 < lim) ? (unsigned)((arow * out_ld + col0) * 4) : GOOB;
      asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(av) : "v"(aoff), "s"(ra) : "memory");
    }
    const int nslot = slot + 1 == ring ? 0 : slot + 1;
    split(nslot, cur ^ 1);
    dma_tile(tile + ring * stride, slot);
    slot = nslot;
    {
      f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const u16* xb = xs + cur * 2 * KROWS * LDX + j * LDX + 8 * quad;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const f16x8 xh = *reinterpret_cast<const f16x8*>(xb + 32 * s);
        const f16x8 xl = *reinterpret_cast<const f16x8*>(xb + KROWS * LDX + 32 * s);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s][0], xh, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s][0], xl, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s][1], xh, acc1, 0, 0, 0);
      }
      const float ri = row_inv[cur * KROWS + j];
      f4 cinv, cbias;
      {
        const float* ci = colinfo + 2 * (16 * ct + 4 * quad);
        const f4 c01 = *reinterpret_cast<const f4*>(ci), c23 = *reinterpret_cast<const f4*>(ci + 4);
        cinv = f4{c01[0], c01[2], c23[0], c23[2]};
        cbias = f4{c01[1], c01[3], c23[1], c23[3]};
      }
      const int64_t grow = (int64_t)tile * KROWS + j;
      f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = __builtin_fmaf(__builtin_fmaf(acc1[r], 1.f / 2048.f, acc0[r]), cinv[r] * ri, cbias[r]);
      // Every store instruction is always issued (masked lanes go out of the buffer's range): the counted wait at
      // the top of the loop relies on a fixed number of vector-memory operations per tile.
      const bool row_ok = grow < M;
      const unsigned off = (unsigned)((grow * out_ld + col0) * 4);
      if (add) {        // behind the addend's load in the counter: this iteration's R DMA requests
        vmwait_rt(R);
        asm volatile("" : "+v"(av));
        o += av;
      }
      if (vec_store) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, (row_ok && col0 + 3 < lim) ? off : GOOB, 0, 0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[r]), ro, (row_ok && col0 + r < lim) ? off + 4u * r : GOOB, 0, 0);
      }
    }
    cur ^= 1;
  }
  vmwait_k<0>();  // no DMA may still be writing this block's LDS when it is handed to the next block
}

// ---------------------------------------------------------------------------------------------------------------------
// The same GEMM with the wavefronts' ROLES separated (round 4; the form the ogbn-mag layer runs on).  In the kernel above
// every wavefront requests its pieces of x, splits a row and multiplies: next to the 8 KS registers of its weight tile there
// is no register left to request the next k-step's operands ahead, so every k-step pays the LDS latency (98 cycles per MFMA
// measured at 352 -> 176 + 32, against 16 of matrix pipe), and the split, the DMA issue and the products of a wavefront are
// serial (6,400 cycles per 16-row tile and wavefront: 3,200 products, 1,050 split, 570 DMA issue, 1,100 barrier).  Here
// wavefronts [0, nmf) only multiply -- the operands of k-step s + 1 in flight during the products of k-step s -- and
// `nh` further wavefronts only move x: LDS-DMA requests `ring` tiles ahead, the fp16x2 split of tile t + 1 while tile t is
// being multiplied (their registers are free: each row's pieces are read once and kept).  Same numerics, same packed weights.
// ---------------------------------------------------------------------------------------------------------------------
// TPW (round 6): column tiles per multiplier wavefront.  Two (32 columns, 16 KS weight registers: K <= 224 at twelve wavefronts) let ONE
// launch cover the 17 - 20 column tiles of the reference's 224-wide forward GEMM (224 + 48 columns) and 296-wide d x GEMM, which
// sixteen single-tile wavefronts cannot: x is read once, the per-tile pipeline (a barrier, a split, the LDS round trips of the
// operands) runs once instead of once per launch, and both tiles' products share every operand read.  `ntl`: column tiles of
// this launch; the multipliers are wavefronts [0, nmf), nmf = ceil(ntl / TPW).  Per tile the same products in the same order.
template <int KS, int WAVES, int TPW = 1>
__global__ void __launch_bounds__(WAVES * 64) basis_gemm_f16x2k_spec_kernel(const float* __restrict__ x, const u16* __restrict__ packed,
                                                                           const float* __restrict__ bcat, int64_t M, int K,
                                                                           KCols c, float* __restrict__ bases,
                                                                           float* __restrict__ weightings, int n_tiles, int LDX,
                                                                           int R, int slot_bytes, int tile0, int ring, int nmf,
                                                                           const float* __restrict__ addend, int ntl) {
  extern __shared__ __attribute__((aligned(16))) char smem_k[];
  char* raw = smem_k;                                                    // [ring][slot_bytes] raw fp32 tiles (DMA ring)
  u16* xs = reinterpret_cast<u16*>(smem_k + ring * slot_bytes);          // [2 buffers][2 planes][KROWS][LDX] fp16
  float* row_inv = reinterpret_cast<float*>(xs + 4 * KROWS * LDX);       // [2 buffers][KROWS]
  float* colinfo = row_inv + 2 * KROWS;                                  // [16 NT][2]: inverse column scale, bias
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_helper = wave >= nmf;
  const int K4 = K >> 2;                                                 // 16-byte pieces per row
  const int stride = gridDim.x;
  int tile = blockIdx.x;
  if (tile >= n_tiles) return;
  // zero the planes once: the k range [K, 32 KS) and the row padding are never written again
  for (int i = tid; i < 4 * KROWS * LDX / 8; i += nthreads) reinterpret_cast<u32x4*>(xs)[i] = u32x4{0, 0, 0, 0};
  {
    const float* inv_tab = reinterpret_cast<const float*>(packed + (int64_t)c.NT * KS * 2 * 64 * 8);
    for (int v = tid; v < 16 * c.NT; v += nthreads) {
      const int w = v - 16 * c.TB;
      colinfo[2 * v] = inv_tab[v];
      colinfo[2 * v + 1] = (w >= 0 && w < c.W && bcat != nullptr) ? bcat[w] : 0.f;
    }
  }

  if (is_helper) {
    // ================= the x movers =================
    const int ht = tid - nmf * 64;                 // thread index among the helpers
    const int hthreads = nthreads - nmf * 64;
    const int hwave = wave - nmf;
    constexpr unsigned GOOB = 0xFFFFFFF0u;
    const u32x4 rx = {(unsigned)(uintptr_t)x, (unsigned)((uintptr_t)x >> 32) & 0xffffu, (unsigned)(M * K * 4), 0x00020000u};
    const unsigned raw_lds = (unsigned)(uintptr_t)raw;
    const unsigned magic_K4 = (unsigned)(((uint64_t)1 << 32) / (uint64_t)K4) + 1u;
    // this thread's (up to 16) pieces of a tile: byte offset inside the tile, or out of range -- computed once (per tile and
    // piece the index arithmetic was a third of the helpers' time)
    unsigned poff[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pc = ht + hthreads * i;
      const int row = (int)__umulhi((unsigned)pc, magic_K4);   // pc / K4 for pc < 2^16
      const int k4 = pc - row * K4;
      poff[i] = (i < R && row < KROWS) ? (unsigned)((row * K + 4 * k4) * 4) : GOOB;
    }
    const int64_t tile_bytes = (int64_t)KROWS * K * 4;
    auto dma_tile = [&](int tl, int slot) {
      // rows beyond M fall outside the buffer (its range check drops them); a tile beyond the last one is not requested
      const bool tile_ok = tl < n_tiles;
      const unsigned tbase = (unsigned)((int64_t)tl * tile_bytes);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i < R) {     // wave-uniform
          const unsigned voff = (tile_ok && poff[i] != GOOB) ? tbase + poff[i] : GOOB;
          const unsigned dst = __builtin_amdgcn_readfirstlane(raw_lds + slot * slot_bytes + (hwave * 64 + hthreads * i) * 16);
          unsigned keep;
          asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                       : "=&s"(keep)
                       : "v"(voff), "s"(dst), "s"(rx)
                       : "memory");
        }
      }
    };
    const int hw = ht >> 5, hl = ht & 31, n_hw = hthreads >> 5;
    // raw fp32 rows of ring slot `rslot` -> the two fp16 planes of buffer `pbuf` + row scales; a half-wavefront per row,
    // the lane's (up to) three 16-byte pieces read once, together, and kept
    // (the rows of a half-wavefront -- up to four -- are processed TOGETHER: one row at a time is a chain of ~60 dependent
    // instructions on a wavefront that has its SIMD's vector unit almost to itself: 1,300 cycles per row measured)
    auto split = [&](int rslot, int pbuf) {
      const char* rs = raw + rslot * slot_bytes;
      u16* xp = xs + pbuf * 2 * KROWS * LDX;
      constexpr int RPH = 4;
      float4 v[RPH][3];
#pragma unroll
      for (int r = 0; r < RPH; ++r) {
        const int row = hw + r * n_hw;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int k4 = hl + 32 * i;
          // (unconditional reads of clamped addresses: a conditional LDS read becomes a branch with its own wait, and the
          // first form of this function spent its time in 112 branches; a clamped piece repeats one the maximum already holds)
          v[r][i] = *reinterpret_cast<const float4*>(rs + ((size_t)(row < KROWS ? row : KROWS - 1) * K4 + (k4 < K4 ? k4 : K4 - 1)) * 16);
        }
      }
      unsigned a[RPH];
#pragma unroll
      for (int r = 0; r < RPH; ++r) {
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          m = fmaxf(m, f16x2_abs_max4(v[r][i]));
        }
        a[r] = __float_as_uint(m);
      }
      row_group_umax<32>(a);
#pragma unroll
      for (int r = 0; r < RPH; ++r) {
        const int row = hw + r * n_hw;
        if (row < KROWS) {     // uniform in the half-wavefront
          const unsigned e = f16x2_row_exp(a[r]);
          const F16x2RowScale sc = f16x2_row_scale(e);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const int k4 = hl + 32 * i;
            if (k4 < K4) {
              const F16x2Planes p = f16x2_split4(v[r][i], sc);
              u16* dst = xp + row * LDX + 4 * k4;
              *reinterpret_cast<u32x2*>(dst) = p.hi;
              *reinterpret_cast<u32x2*>(dst + KROWS * LDX) = p.lo;
            }
          }
          if (hl == 0) row_inv[pbuf * KROWS + row] = __uint_as_float(e);  // 2^e
        }
      }
    };
    for (int r = 0; r < ring; ++r) dma_tile(tile + r * stride, r);
    vmwait_k<0>();
    lds_barrier();           // every helper's pieces of the first tiles have landed; the planes are zeroed, colinfo written
    split(0, 0);
    // At the top of iteration t: this wavefront's pieces of tile t + 1 must have landed; behind them in the (in-order)
    // counter are only the pieces of tiles t + 2 ... t + ring - 1.
    int cur = 0, slot = 0;
    const int behind = (ring - 2) * R;
    for (; tile < n_tiles; tile += stride) {
      vmwait_rt(behind);
      lds_barrier();         // tile t split (all helpers), tile t + 1 landed, the workers done with plane buffer cur ^ 1
      const int nslot = slot + 1 == ring ? 0 : slot + 1;
      split(nslot, cur ^ 1);
      dma_tile(tile + ring * stride, slot);     // (slot held tile t: split in the previous iteration, before this barrier)
      slot = nslot;
      cur ^= 1;
    }
    vmwait_k<0>();  // no DMA may still be writing this block's LDS when it is handed to the next block
    return;
  }

  // ================= the multipliers =================
  const int j = lane & 15, quad = lane >> 4;
  constexpr unsigned GOOB = 0xFFFFFFF0u;
  int ct[TPW];
  bool live[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    live[u] = wave * TPW + u < ntl;                                    // (an odd tile count leaves the last wavefront's second tile idle:
    ct[u] = tile0 + (live[u] ? wave * TPW + u : wave * TPW);           //  it repeats its first tile and stores nothing)
  }
  f16x8 wf[TPW][KS][2];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const u16* src = packed + ((int64_t)ct[u] * KS * 2 * 64 + lane) * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      wf[u][s][0] = *reinterpret_cast<const f16x8*>(src + (s * 2) * 64 * 8);
      wf[u][s][1] = *reinterpret_cast<const f16x8*>(src + (s * 2 + 1) * 64 * 8);
    }
  }
  bool to_bases[TPW], vec_store[TPW], add[TPW];
  int out_ld[TPW], col0[TPW], lim[TPW];
  __amdgpu_buffer_rsrc_t ro[TPW], ra[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    to_bases[u] = ct[u] < c.TB;
    out_ld[u] = to_bases[u] ? c.ldb : c.W;
    col0[u] = to_bases[u] ? 16 * ct[u] + 4 * quad : 16 * (ct[u] - c.TB) + 4 * quad;
    lim[u] = live[u] ? (to_bases[u] ? c.ldb : c.W) : 0;                // (an idle tile: every column out of range)
    float* outp = to_bases[u] ? bases : weightings;
    ro[u] = __builtin_amdgcn_make_buffer_rsrc((void*)outp, 0, (unsigned)(M * out_ld[u] * 4), 0x00020000);
    vec_store[u] = (out_ld[u] & 3) == 0;
    // `addend`: as in the kernel above; the multipliers issue no DMA, so the compiler's own count of this load is right
    add[u] = addend != nullptr && to_bases[u] && live[u];              // wave-uniform
    ra[u] = __builtin_amdgcn_make_buffer_rsrc((void*)(add[u] ? addend : outp), 0, add[u] ? (unsigned)(M * out_ld[u] * 4) : 0u, 0x00020000);
  }
  vmwait_k<0>();
#pragma unroll
  for (int u = 0; u < TPW; ++u)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(wf[u][s][0]), "+v"(wf[u][s][1]));
  lds_barrier();
  int cur = 0;
  for (; tile < n_tiles; tile += stride) {
    lds_barrier();
    f4 av[TPW], acc0[TPW], acc1[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      av[u] = acc0[u] = acc1[u] = f4{0.f, 0.f, 0.f, 0.f};
      if (add[u]) {
        const int64_t arow = (int64_t)tile * KROWS + j;
        av[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(
                                               ra[u], (arow < M && col0[u] + 3 < lim[u]) ? (unsigned)((arow * out_ld[u] + col0[u]) * 4) : GOOB, 0, 0));
      }
    }
    const u16* xb = xs + cur * 2 * KROWS * LDX + j * LDX + 8 * quad;
    // PF operand sets in rotation: the operands of k-step s + PF - 1 are requested before the products of k-step s, and the
    // order is pinned (left alone the scheduler folds the sets back into one and waits for a read two MFMAs after issuing it)
    // (two tiles: six products per operand pair, and the registers are the weights'; K > 320 at sixteen wavefronts: the third set
    // was paid for in spilled weight registers -- 12 / 20 at KS = 11 / 12 --, 570 -> 540 us at the ogbn-mag shape without it)
    constexpr int PF = (TPW == 1 && KS <= 10) ? 3 : 2;
    f16x8 xh[PF], xl[PF];
#pragma unroll
    for (int p = 0; p < PF - 1; ++p)
      if (p < KS) {
        xh[p] = *reinterpret_cast<const f16x8*>(xb + 32 * p);
        xl[p] = *reinterpret_cast<const f16x8*>(xb + KROWS * LDX + 32 * p);
      }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s + PF - 1 < KS) {
        xh[(s + PF - 1) % PF] = *reinterpret_cast<const f16x8*>(xb + 32 * (s + PF - 1));
        xl[(s + PF - 1) % PF] = *reinterpret_cast<const f16x8*>(xb + KROWS * LDX + 32 * (s + PF - 1));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < TPW; ++u) acc0[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][s][0], xh[s % PF], acc0[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < TPW; ++u) acc1[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][s][0], xl[s % PF], acc1[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < TPW; ++u) acc1[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u][s][1], xh[s % PF], acc1[u], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float ri = row_inv[cur * KROWS + j];
    const int64_t grow = (int64_t)tile * KROWS + j;
    const bool row_ok = grow < M;
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      f4 cinv, cbias;
      {
        const float* ci = colinfo + 2 * (16 * ct[u] + 4 * quad);
        const f4 c01 = *reinterpret_cast<const f4*>(ci), c23 = *reinterpret_cast<const f4*>(ci + 4);
        cinv = f4{c01[0], c01[2], c23[0], c23[2]};
        cbias = f4{c01[1], c01[3], c23[1], c23[3]};
      }
      f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = __builtin_fmaf(__builtin_fmaf(acc1[u][r], 1.f / 2048.f, acc0[u][r]), cinv[r] * ri, cbias[r]);
      const unsigned off = (unsigned)((grow * out_ld[u] + col0[u]) * 4);
      if (add[u]) o += av[u];
      if (vec_store[u]) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro[u], (row_ok && col0[u] + 3 < lim[u]) ? off : GOOB, 0, 0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[r]), ro[u], (row_ok && col0[u] + r < lim[u]) ? off + 4u * r : GOOB, 0, 0);
      }
    }
    cur ^= 1;
  }
}

static KCols kcols(const GemmPlan& p) { return KCols{p.f_g, p.ldb, p.w_cols, p.TB, p.NT}; }

int f16x2k_pack(const float* wcat, int64_t rs, int64_t cs, const GemmPlan& p, void* packed, hipStream_t stream) {
  pack_f16x2k_kernel<<<p.NT * 16, 64, 0, stream>>>(wcat, rs, cs, p.f_in, kcols(p), p.KS, (u16*)packed);
  EGC_LAUNCH_CHECK("pack_f16x2k_kernel");
  return EGC_OK;
}

// One launch as gemm_longk_launches describes it (egc_gemm_host.h).  The instances compiled: the all-in-one kernel and the kernel
// of multipliers and helpers with 12 and 16 wavefronts, and for KS <= 7 (16 KS weight registers fit twelve wavefronts) the
// latter with two column tiles per multiplier.
template <int KS>
static int launch_ks(const GemmLongKLaunch& g, const float* x, const u16* packed, const float* bcat, int64_t M, int K, const KCols& c,
                     float* bases, float* weightings, const float* addend, hipStream_t stream) {
  int n_tiles;
  if (const int st = gemm_row_tiles(M, KROWS, n_tiles); st != EGC_OK) return st;
  const int grid = gemm_grid(g.per_cu, n_tiles);
  auto all = [&](auto waves) -> int {
    auto kern = &basis_gemm_f16x2k_kernel<KS, waves()>;
    EGC_ALLOW_DYNAMIC_LDS(kern, 160 * 1024, "f16x2");
    kern<<<grid, g.threads, g.lds, stream>>>(x, packed, bcat, M, K, c, bases, weightings, n_tiles, g.LDX, g.R, g.slot_bytes, g.tile0, g.ring,
                                            addend);
    EGC_LAUNCH_CHECK("basis_gemm_f16x2k_kernel");
    return EGC_OK;
  };
  auto spec = [&](auto waves, auto tpw) -> int {
    auto kern = &basis_gemm_f16x2k_spec_kernel<KS, waves(), tpw()>;
    EGC_ALLOW_DYNAMIC_LDS(kern, 160 * 1024, "f16x2 spec");
    kern<<<grid, g.threads, g.lds, stream>>>(x, packed, bcat, M, K, c, bases, weightings, n_tiles, g.LDX, g.R, g.slot_bytes, g.tile0, g.ring,
                                            g.mult, addend, g.tiles);
    EGC_LAUNCH_CHECK("basis_gemm_f16x2k_spec_kernel");
    return EGC_OK;
  };
  constexpr std::integral_constant<int, 12> w12;
  constexpr std::integral_constant<int, 16> w16;
  if (g.form == LONGK_TWO_TILES) {
    if constexpr (KS <= 7) return spec(w12, std::integral_constant<int, 2>{});
    return EGC_ERR_UNSUPPORTED;
  }
  if (g.form == LONGK_ROLES) return g.waves == 12 ? spec(w12, std::integral_constant<int, 1>{}) : spec(w16, std::integral_constant<int, 1>{});
  return g.waves == 12 ? all(w12) : all(w16);
}

int f16x2k_launch(const float* x, const void* packed, const float* bcat, int64_t M, const GemmPlan& p, float* bases,
                  float* weightings, hipStream_t stream, const float* addend) {
  const int K = p.f_in, ldb = p.ldb, W = p.w_cols;
  if (!aligned16(x) || !aligned16(bases) || (W > 0 && (W & 3) == 0 && !aligned16(weightings))) return EGC_ERR_UNSUPPORTED;
  if (addend != nullptr && (!aligned16(addend) || (ldb & 3) != 0)) return EGC_ERR_UNSUPPORTED;
  const auto ls = gemm_longk_launches(K, p.NT);
  if (ls.status != EGC_OK) return ls.status;
  const KCols c = kcols(p);
  return gemm_for_row_ranges(M, std::max(std::max(K, ldb), W), KROWS, [&](int64_t r0, int64_t rows) -> int {
    for (int l = 0; l < ls.n; ++l) {
      auto run = [&](auto ks) {
        return launch_ks<ks()>(ls.l[l], x + r0 * K, (const u16*)packed, bcat, rows, K, c, bases + r0 * ldb,
                               weightings != nullptr ? weightings + r0 * W : nullptr, addend != nullptr ? addend + r0 * ldb : nullptr, stream);
      };
      int st;
      switch (p.KS) {   // (gemm_longk_launches admits 5 .. 12)
        case 5: st = run(std::integral_constant<int, 5>{}); break;     case 6: st = run(std::integral_constant<int, 6>{}); break;
        case 7: st = run(std::integral_constant<int, 7>{}); break;     case 8: st = run(std::integral_constant<int, 8>{}); break;
        case 9: st = run(std::integral_constant<int, 9>{}); break;     case 10: st = run(std::integral_constant<int, 10>{}); break;
        case 11: st = run(std::integral_constant<int, 11>{}); break;   default: st = run(std::integral_constant<int, 12>{});
      }
      if (st != EGC_OK) return st;
    }
    return EGC_OK;
  });
}

}  // namespace egc
