// Shared between the split-precision GEMM translation units (egc_gemm_bf16x3.hip, egc_gemm_f16x2.hip, egc_gemm_f16x2k.hip)
// and the fused tile kernels (egc_fused_tile_dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "egc_common.h"
#include "egc_gemm_host.h"

namespace egc {

// ---- the fp16x2 split: the numerics of every fp16x2 GEMM (egc_gemm_f16x2.hip header) ----
// A weight column or an x row is scaled by a power of two that puts its largest magnitude in [1, 2), then written as
// s = h + 2^-11 l, h = fp16(s), l = fp16(2^11 (s - h)); the products recombine as 2^ex 2^ew (acc0 + 2^-11 acc1).

struct F16x2ColScale { float scale, inv; };
// biased exponent of a weight column's largest magnitude (sign cleared) -> (scale, inverse scale), both exact powers of two
__device__ inline F16x2ColScale f16x2_col_scale(unsigned amax_bits) {
  unsigned be = amax_bits >> 23;
  be = be > 253u ? 253u : be;           // huge / inf / nan: keep the scale a normal number (values propagate)
  return {__uint_as_float((254u - be) << 23),
          __uint_as_float(be << 23)};   // be == 0 (all-zero or denormal column): the results flush to 0
}

struct F16x2Bits { u16 h, l; };
// one scaled weight -> the fp16 bits of its h plane and of its 2^11-scaled l plane
__device__ inline F16x2Bits f16x2_pack_split(float w) {
  const _Float16 h = (_Float16)w;
  const _Float16 l = (_Float16)((w - (float)h) * 2048.f);
  return {__builtin_bit_cast(u16, h), __builtin_bit_cast(u16, l)};
}

// exponent field of an x row's largest magnitude (bit pattern), kept where both 2^-e and 2^(11-e) are normal numbers (rows
// below 2^-113 are scaled by 2^114 only and keep fewer bits; rows above 2^126 overflow as they would in fp32); 2^e is the
// row's inverse scale
__device__ inline unsigned f16x2_row_exp(unsigned amax_bits) {
  const unsigned e = amax_bits & 0x7f800000u;
  return min(max(e, 13u << 23), 253u << 23);
}

struct F16x2RowScale { float sc, sc2k; };   // 2^-e, 2^(11-e)
__device__ inline F16x2RowScale f16x2_row_scale(unsigned e) {
  return {__uint_as_float(0x7f000000u - e), __uint_as_float(0x7f000000u + (11u << 23) - e)};
}

struct F16x2Planes { u32x2 hi, lo; };
// four floats of a row -> packed fp16 pairs of the h plane and of the 2^11-scaled l plane (element 0 low)
template <class V>
__device__ inline F16x2Planes f16x2_split4(const V v, const F16x2RowScale s) {
  const float sc = s.sc, sc2k = s.sc2k;
  const f16x2 h01 = __builtin_convertvector(f32x2{v.x * sc, v.y * sc}, f16x2);
  const f16x2 h23 = __builtin_convertvector(f32x2{v.z * sc, v.w * sc}, f16x2);
  // (xs - h) * 2^11 = fma(h, -2^11, x * 2^(11-e)): one mixed-precision fma, rounded once to fp16
  f16x2 l01, l23;
  l01[0] = (_Float16)__builtin_fmaf((float)h01[0], -2048.f, v.x * sc2k);
  l01[1] = (_Float16)__builtin_fmaf((float)h01[1], -2048.f, v.y * sc2k);
  l23[0] = (_Float16)__builtin_fmaf((float)h23[0], -2048.f, v.z * sc2k);
  l23[1] = (_Float16)__builtin_fmaf((float)h23[1], -2048.f, v.w * sc2k);
  return {u32x2{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)},
          u32x2{__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23)}};
}

// largest |.| of four floats, through source modifiers (two instructions; asm because the compiler canonicalises every
// fmax operand)
template <class V>
__device__ inline float f16x2_abs_max4(const V v) {
  float m;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|\n\tv_max_f32 %0, |%4|, %0" : "=&v"(m) : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
  return m;
}

// maximum of a non-negative bit pattern over each group of LANES consecutive lanes (8, 16 or 32): DPP steps inside the rows
// of 16, one cross-row exchange for 32.  NaNs drop out of the row maxima and propagate through the products instead.  N
// values reduce step by step side by side (their chains interleaved: one value at a time is a chain of dependent
// instructions).
template <int LANES, int N>
__device__ inline void row_group_umax(unsigned (&a)[N]) {
  static_assert(LANES == 8 || LANES == 16 || LANES == 32, "row group of 8, 16 or 32 lanes");
#pragma unroll
  for (int r = 0; r < N; ++r) a[r] = max(a[r], (unsigned)__builtin_amdgcn_update_dpp(0, (int)a[r], 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
#pragma unroll
  for (int r = 0; r < N; ++r) a[r] = max(a[r], (unsigned)__builtin_amdgcn_update_dpp(0, (int)a[r], 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
#pragma unroll
  for (int r = 0; r < N; ++r) a[r] = max(a[r], (unsigned)__builtin_amdgcn_update_dpp(0, (int)a[r], 0x141, 0xf, 0xf, true));  // row_half_mirror
  if (LANES >= 16) {
#pragma unroll
    for (int r = 0; r < N; ++r) a[r] = max(a[r], (unsigned)__builtin_amdgcn_update_dpp(0, (int)a[r], 0x140, 0xf, 0xf, true));  // row_mirror
  }
  if (LANES >= 32) {
#pragma unroll
    for (int r = 0; r < N; ++r) a[r] = max(a[r], (unsigned)__builtin_amdgcn_ds_swizzle((int)a[r], 0x401F));                    // lane ^ 16
  }
}
template <int LANES>
__device__ inline unsigned row_group_umax(unsigned a) {
  unsigned v[1] = {a};
  row_group_umax<LANES>(v);
  return v[0];
}

// ---- host: the families' pack and launch, each for the shapes to which gemm_plan (egc_gemm_host.h) gives its layout ----
// (rs, cs): floats between consecutive k / consecutive columns of the source: (f_g + w_cols, 1) for wcat [f_in][f_g + w_cols],
// (1, ld) for its transpose stored [f_g + w_cols][ld]
int f16x2_pack(const float* wcat, int64_t rs, int64_t cs, const GemmPlan& p, void* packed, hipStream_t stream);
// dis != nullptr and 0 <= fold_m <= 3 (W % 32 == 0, HBA weightings of A = 4 aggregators): the folded form -- the mean
// weighting at place fold_m of a (h, b) pair's quad joins the sum weighting at fold_s through 1 / max(cnt, 1) of the row,
// cnt = dis^-2; `weightings` then has W / 4 * 3 columns (egc_gemm_f16x2.hip)
int f16x2_launch(const float* x, const void* packed, const float* bcat, int64_t M, const GemmPlan& p, float* bases,
                 float* weightings, hipStream_t stream, const float* dis = nullptr, int fold_s = -1, int fold_m = -1);
// egc_basis_transform_packed_ex in the folded form above; EGC_ERR_UNSUPPORTED where the shape / flags take another kernel
int basis_transform_packed_folded(const float* x, const void* packed, const float* bcat, int64_t n_nodes, int32_t f_in,
                                  int32_t f_g, int32_t w_cols, int32_t flags, float* bases, int32_t ldb, float* weightings,
                                  const float* dis, int fold_s, int fold_m, hipStream_t stream);

// the long-k fp16x2 kernels (egc_gemm_f16x2k.hip): 128 < F_in <= 384, at most 32 column tiles of 16 in one or two launches
int f16x2k_pack(const float* wcat, int64_t rs, int64_t cs, const GemmPlan& p, void* packed, hipStream_t stream);
// addend (or nullptr): [M][ldb] added to the bases columns in the store
int f16x2k_launch(const float* x, const void* packed, const float* bcat, int64_t M, const GemmPlan& p, float* bases,
                  float* weightings, hipStream_t stream, const float* addend = nullptr);

}  // namespace egc
