// Shared host/device helpers for libegc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "egc_hip.h"
#include "egc_plain.h"   // ceil_div, the layer's strides, the long-row plan's capacities: shared with the HIP-free planners

#define EGC_WAVE 64

namespace egc {

// Records the message returned by egc_last_error().
void set_last_error(const char* what, hipError_t err);

#define EGC_HIP_TRY(expr)                          \
  do {                                             \
    hipError_t _e = (expr);                        \
    if (_e != hipSuccess) {                        \
      ::egc::set_last_error(#expr, _e);            \
      return EGC_ERR_HIP;                          \
    }                                              \
  } while (0)

#define EGC_LAUNCH_CHECK(name)                     \
  do {                                             \
    hipError_t _e = hipGetLastError();             \
    if (_e != hipSuccess) {                        \
      ::egc::set_last_error(name, _e);             \
      return EGC_ERR_HIP;                          \
    }                                              \
  } while (0)

// Allow `bytes` of dynamic LDS (beyond the default 64 KiB) for one kernel instance, once per process: the flag is a static of
// the expansion, so inside a launcher template there is one per kernel instance.  Returns EGC_ERR_HIP from the caller on failure.
#define EGC_ALLOW_DYNAMIC_LDS(kernel, bytes, what)                                                              \
  do {                                                                                                          \
    static bool _allowed = false;                                                                               \
    if (!_allowed) {                                                                                            \
      hipError_t _e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),                                \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes));            \
      if (_e != hipSuccess) {                                                                                   \
        ::egc::set_last_error("hipFuncSetAttribute(" what ")", _e);                                             \
        return EGC_ERR_HIP;                                                                                     \
      }                                                                                                         \
      _allowed = true;                                                                                          \
    }                                                                                                           \
  } while (0)

// vector types of the kernels (MFMA operands and accumulators, packed fp16 / bf16, 8- and 16-byte LDS pieces)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL access of the
// wavefront (s_waitcnt vmcnt(0)): in a streaming kernel that drains the stores of the tile just finished and the prefetch of
// the next one at every barrier -- microseconds of HBM latency per tile.  The tiles exchanged between wavefronts live in LDS,
// so lgkmcnt(0) + s_barrier is all that is needed.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A lane's four adjacent columns c .. c + 3 of a row of `width` floats, p pointing at column c (every kernel that gives a lane
// four columns: the baseline layers, the encoders, the readouts): one 16-byte access (VEC: width, strides and pointers are
// multiples of 16 bytes) or 4-byte ones of the columns that exist.  NT: non-temporal loads (data read once: the readouts' x).
template <bool VEC, bool NT = false>
__device__ inline f4 tm_load(const float* __restrict__ p, int c, int width) {
  if (VEC) return NT ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(p)) : *reinterpret_cast<const f4*>(p);
  f4 v = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < width) v[j] = NT ? __builtin_nontemporal_load(p + j) : p[j];
  return v;
}

template <bool VEC>
__device__ inline void tm_store(float* __restrict__ p, int c, int width, f4 v) {
  if (VEC) {
    *reinterpret_cast<f4*>(p) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < width) p[j] = v[j];
}

// the same four columns of an int32 row (edge ids, CSR positions); a column that does not exist reads as -1
typedef int i4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ inline i4 tm_load_i(const int32_t* __restrict__ p, int c, int width) {
  if (VEC) return *reinterpret_cast<const i4*>(p);
  i4 v = i4{-1, -1, -1, -1};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < width) v[j] = p[j];
  return v;
}

template <bool VEC>
__device__ inline void tm_store_i(int32_t* __restrict__ p, int c, int width, i4 v) {
  if (VEC) {
    *reinterpret_cast<i4*>(p) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < width) p[j] = v[j];
}

// egc_backward.hip: CSR positions of the first entries attaining each row's max / min (training forward)
int arg_extrema(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb, const float* stats,
                const int32_t* cnt, int32_t* arg_max, int32_t* arg_min, unsigned* arg8_max, unsigned* arg8_min,
                hipStream_t stream);

// egc_readout.hip: the segmented readout's forward launch (op = EGC_READOUT_*; arguments already validated)
int launch_segment_reduce(const float* x, const int64_t* seg_ptr, int64_t n_segments, int64_t n_rows, int32_t width,
                          int32_t op, float* out, int32_t* arg, hipStream_t stream);

}  // namespace egc
