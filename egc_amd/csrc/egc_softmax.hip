// Output head and loss of the classification nets: row log-softmax (with the row arg-max), its backward, and the fused
// selected-row NLL loss forward / backward.  gfx950 only, float32.  The reference ends every node-classification net with
// `conv(x)[:, :349].log_softmax(-1)`, `out[train_idx]`, `F.nll_loss(out, y[train_idx])` (mag/models.py:68-69 with
// mag/configs.py:34-35; arxiv/norm_models.py:42-43 with arxiv/configs.py:53-54; rmag/configs.py:35-36) and the graph-level
// ones with F.cross_entropy (cifar/configs.py:57): a strided softmax, a row gather, the loss, and in backward two zero
// fills, an index-put, the softmax backward and a slice backward -- about ten passes over the logits.  The loss needs the
// selected rows alone: here the forward reads them once, the backward reads them once more and writes the gradient once,
// in the padded [N, ld] layout of the logits.  ignore_index and class weights are NOT supported (the reference uses neither).
//
// Rows hold n_classes columns inside a row stride ld >= n_classes.  Columns n_classes .. ld-1 are never read; the backward
// forms write them as zeros.
//
// Mapping.  A row belongs to a group of G lanes, G the power of two >= ceil(n_classes / 4), 64 at the most; a lane holds
// 4 K elements of the row in registers, K = ceil(n_classes / (4 G)) <= 4 (n_classes <= EGC_SOFTMAX_MAX_CLASSES): 16 rows
// per wavefront at 10 classes, 4 at 40, one wavefront per row from 129 classes on.  Max, sum and the store therefore cost
// one read of x.  A workgroup of 256 threads owns SM_CHUNK = 128 consecutive rows; group s of its 256 / G groups takes the
// rows chunk0 + s, chunk0 + s + 256 / G, ... ascending and requests its next row before it reduces the current one.
// Vector form (row stride % 4 == 0, pointers 16-byte aligned): lane l holds columns 4 (l + k G) .. + 3, k < K, as 16-byte
// accesses; the piece that straddles n_classes is read column by column.  Scalar form: lane l holds columns l + G e,
// e < 4 K, so a wavefront's 4-byte accesses are adjacent.  Lanes combine with xor shuffles (no LDS): after every level
// both partners hold a + b and b + a, the same bits, so all lanes of a group end with one value.
//
// Order rules.  Row sums (sum of exp, sum of g): a lane adds its elements in ascending column order, then the xor levels
// G/2, G/4, .., 1 -- a function of n_classes alone.  Arg-max: the FIRST maximal column (strict compare in ascending
// column order inside a lane; across lanes the larger value, the smaller column on a tie).  Loss: group s adds
// cnt[r] * (x[r, y[r]] - lse[r]) over its rows ascending; the workgroup's 256 / G group sums are added four adjacent ones
// per lane, ascending, then by the 64-lane xor levels: that is partial[chunk].  A second launch of one workgroup adds
// partial[t], partial[t + 256], ... ascending in thread t, then the 256 thread sums in the same way.  No float atomics:
// the loss is a function of the inputs and shapes alone.  Longest add chain: 128 G / 256 + 9 + ceil(chunks / 256) + 9.
#include "egc_common.h"

#include <math.h>

namespace egc {

constexpr int SM_CHUNK = 128;   // rows of a workgroup
constexpr int SM_BLOCK = 256;

// column of element e of lane l
template <bool VEC>
__device__ inline int sm_col(int l, int G, int e) {
  return VEC ? 4 * (l + (e >> 2) * G) + (e & 3) : l + G * e;
}

// a lane's 4 K elements of one row (columns >= n_cols: `fill`, nothing is read there)
template <bool VEC, int K>
__device__ inline void sm_load(const float* __restrict__ row, int l, int G, int n_cols, float fill, float (&v)[4 * K]) {
  if (VEC) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = 4 * (l + k * G);
      if (c + 3 < n_cols) {
        const f4 t = *reinterpret_cast<const f4*>(row + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * k + j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * k + j] = c + j < n_cols ? row[c + j] : fill;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) {
      const int c = l + G * e;
      v[e] = c < n_cols ? row[c] : fill;
    }
  }
}

// a lane's elements into columns [0, limit) of a row, then zeros into [4 K G, ld): with the caller's zeros in the
// elements past n_classes, every column of [0, ld) is written once.  VEC: limit % 4 == 0 and ld % 4 == 0.
template <bool VEC, int K>
__device__ inline void sm_store(float* __restrict__ row, int l, int G, int limit, int ld, const float (&v)[4 * K]) {
  if (VEC) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = 4 * (l + k * G);
      if (c < limit)
        __builtin_nontemporal_store(f4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]}, reinterpret_cast<f4*>(row + c));
    }
    for (int c = 4 * (K * G + l); c < ld; c += 4 * G)
      __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(row + c));
  } else {
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) {
      const int c = l + G * e;
      if (c < limit) __builtin_nontemporal_store(v[e], row + c);
    }
    for (int c = 4 * K * G + l; c < ld; c += G) __builtin_nontemporal_store(0.f, row + c);
  }
}

__device__ inline float sm_group_max(float v, int G) {
  for (int m = G >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

__device__ inline float sm_group_sum(float v, int G) {
  for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// lse = m + log(sum exp(v - m)) of the group's row (elements past n_classes hold -inf: exp gives 0)
template <int K>
__device__ inline float sm_lse(const float (&v)[4 * K], int G) {
  float m = v[0];
#pragma unroll
  for (int e = 1; e < 4 * K; ++e) m = fmaxf(m, v[e]);
  m = sm_group_max(m, G);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4 * K; ++e) s += expf(v[e] - m);
  s = sm_group_sum(s, G);
  return m + logf(s);
}

// the 256 values of s_part (one per thread; unused slots hold 0) in the fixed order of the header; valid in wavefront 0
__device__ inline float sm_block_sum(const float* s_part) {
  const int lane = threadIdx.x & 63;
  float a = s_part[4 * lane];
#pragma unroll
  for (int j = 1; j < 4; ++j) a += s_part[4 * lane + j];
  return sm_group_sum(a, 64);
}

#define SM_GROUP_INDEX                                                                                  \
  const int G = 1 << gl, s = (int)threadIdx.x >> gl, l = (int)threadIdx.x & (G - 1), subs = SM_BLOCK >> gl; \
  const int64_t r0 = (int64_t)blockIdx.x * SM_CHUNK, r1 = min(r0 + SM_CHUNK, n_rows)

template <bool VEC, int K>
__global__ void __launch_bounds__(SM_BLOCK) log_softmax_forward_kernel(const float* __restrict__ x, int64_t n_rows, int n_classes,
                                                                       int ld, int gl, float* __restrict__ out,
                                                                       float* __restrict__ lse, int32_t* __restrict__ amax) {
  SM_GROUP_INDEX;
  float cur[4 * K], nxt[4 * K];
  int64_t r = r0 + s;
  if (r < r1) sm_load<VEC, K>(x + r * ld, l, G, n_classes, -INFINITY, cur);
#pragma unroll 1
  for (; r < r1; r += subs) {
    if (r + subs < r1) sm_load<VEC, K>(x + (r + subs) * ld, l, G, n_classes, -INFINITY, nxt);
    if (amax != nullptr) {
      float bm = cur[0];
      int bi = sm_col<VEC>(l, G, 0);
#pragma unroll
      for (int e = 1; e < 4 * K; ++e) {
        const bool take = cur[e] > bm;
        bm = take ? cur[e] : bm;
        bi = take ? sm_col<VEC>(l, G, e) : bi;
      }
      for (int m = G >> 1; m > 0; m >>= 1) {
        const float om = __shfl_xor(bm, m);
        const int oi = __shfl_xor(bi, m);
        const bool take = om > bm || (om == bm && oi < bi);
        bm = take ? om : bm;
        bi = take ? oi : bi;
      }
      if (l == 0) amax[r] = bi;
    }
    const float L = sm_lse<K>(cur, G);
    if (l == 0 && lse != nullptr) lse[r] = L;
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cur[e] -= L;
    sm_store<VEC, K>(out + r * n_classes, l, G, n_classes, 0, cur);
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cur[e] = nxt[e];
  }
}

template <bool VEC, int K>
__global__ void __launch_bounds__(SM_BLOCK) log_softmax_backward_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                                        int64_t n_rows, int n_classes, int ld, int gl,
                                                                        float* __restrict__ dx) {
  SM_GROUP_INDEX;
  float cg[4 * K], co[4 * K], ng[4 * K], no[4 * K];
  int64_t r = r0 + s;
  if (r < r1) {
    sm_load<VEC, K>(g + r * n_classes, l, G, n_classes, 0.f, cg);
    sm_load<VEC, K>(out + r * n_classes, l, G, n_classes, -INFINITY, co);
  }
#pragma unroll 1
  for (; r < r1; r += subs) {
    if (r + subs < r1) {
      sm_load<VEC, K>(g + (r + subs) * n_classes, l, G, n_classes, 0.f, ng);
      sm_load<VEC, K>(out + (r + subs) * n_classes, l, G, n_classes, -INFINITY, no);
    }
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) sum += cg[e];
    sum = sm_group_sum(sum, G);
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cg[e] = sm_col<VEC>(l, G, e) < n_classes ? cg[e] - expf(co[e]) * sum : 0.f;
    sm_store<VEC, K>(dx + r * ld, l, G, ld, ld, cg);
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cg[e] = ng[e], co[e] = no[e];
  }
}

template <bool VEC, int K>
__global__ void __launch_bounds__(SM_BLOCK) nll_forward_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                               const int32_t* __restrict__ cnt, int64_t n_rows, int n_classes,
                                                               int ld, int gl, float* __restrict__ lse,
                                                               float* __restrict__ partial, int32_t* __restrict__ host_flag) {
  __shared__ float s_part[SM_BLOCK];
  SM_GROUP_INDEX;
  s_part[threadIdx.x] = 0.f;
  float cur[4 * K], nxt[4 * K];
  float acc = 0.f;
  bool bad = false;
  int64_t r = r0 + s;
  int cc = r < r1 ? (cnt != nullptr ? cnt[r] : 1) : 0;
  if (cc > 0) sm_load<VEC, K>(x + r * ld, l, G, n_classes, -INFINITY, cur);
#pragma unroll 1
  for (; r < r1; r += subs) {
    const int64_t rn = r + subs;
    const int cn = rn < r1 ? (cnt != nullptr ? cnt[rn] : 1) : 0;
    if (cn > 0) sm_load<VEC, K>(x + rn * ld, l, G, n_classes, -INFINITY, nxt);
    float L = 0.f;
    if (cc > 0) {   // (the same for every lane of the group)
      const int64_t label = y[r];
      const bool ok = label >= 0 && label < n_classes;   // outside: never an address; nothing added, flag raised
      const float xy = ok ? x[r * ld + label] : 0.f;
      L = sm_lse<K>(cur, G);
      if (ok) acc += (float)cc * (xy - L);
      bad |= !ok;
    }
    if (l == 0) lse[r] = L;
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cur[e] = nxt[e];
    cc = cn;
  }
  if (bad && l == 0 && host_flag != nullptr) *(volatile int32_t*)host_flag = 1;   // sticky, host-visible
  __syncthreads();
  if (l == 0) s_part[s] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    const float t = sm_block_sum(s_part);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
  }
}

// loss = -(sum of the chunk sums) [/ M], one workgroup; M = *total, or n_rows when every row counts once
__global__ void __launch_bounds__(SM_BLOCK) nll_finalize_kernel(const float* __restrict__ partial, int64_t n_chunks,
                                                                const int64_t* __restrict__ total, int64_t n_rows, int mean,
                                                                float* __restrict__ loss) {
  __shared__ float s_part[SM_BLOCK];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n_chunks; i += SM_BLOCK) a += partial[i];
  s_part[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < 64) {
    const float t = sm_block_sum(s_part);
    if (threadIdx.x == 0) {
      const float m = (float)(total != nullptr ? *total : n_rows);
      *loss = mean ? -(t / m) : -t;
    }
  }
}

template <bool VEC, int K>
__global__ void __launch_bounds__(SM_BLOCK) nll_backward_kernel(const float* __restrict__ x, const int64_t* __restrict__ y,
                                                                const int32_t* __restrict__ cnt, const int64_t* __restrict__ total,
                                                                const float* __restrict__ lse, const float* __restrict__ grad_loss,
                                                                int64_t n_rows, int n_classes, int ld, int gl, int mean,
                                                                float* __restrict__ dx) {
  SM_GROUP_INDEX;
  const float g0 = *grad_loss;
  const float m = mean ? (float)(total != nullptr ? *total : n_rows) : 1.f;
  float cur[4 * K], nxt[4 * K];
  int64_t r = r0 + s;
  // a row takes part when it is selected and its label is a class (the forward reported the others)
  int64_t label = r < r1 ? y[r] : -1;
  int cc = r < r1 && label >= 0 && label < n_classes ? (cnt != nullptr ? cnt[r] : 1) : 0;
  if (cc > 0) sm_load<VEC, K>(x + r * ld, l, G, n_classes, -INFINITY, cur);
#pragma unroll 1
  for (; r < r1; r += subs) {
    const int64_t rn = r + subs;
    const int64_t label_n = rn < r1 ? y[rn] : -1;
    const int cn = rn < r1 && label_n >= 0 && label_n < n_classes ? (cnt != nullptr ? cnt[rn] : 1) : 0;
    if (cn > 0) sm_load<VEC, K>(x + rn * ld, l, G, n_classes, -INFINITY, nxt);
    if (cc > 0) {
      const float L = lse[r];
      const float w = mean ? (g0 * (float)cc) / m : g0 * (float)cc;
#pragma unroll
      for (int e = 0; e < 4 * K; ++e) {
        const int c = sm_col<VEC>(l, G, e);
        cur[e] = c < n_classes ? w * (expf(cur[e] - L) - (c == (int)label ? 1.f : 0.f)) : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4 * K; ++e) cur[e] = 0.f;
    }
    sm_store<VEC, K>(dx + r * ld, l, G, ld, ld, cur);
#pragma unroll
    for (int e = 0; e < 4 * K; ++e) cur[e] = nxt[e];
    cc = cn;
    label = label_n;
  }
}

__global__ void __launch_bounds__(SM_BLOCK) selection_count_kernel(const int64_t* __restrict__ index, int64_t n_index,
                                                                   int64_t n_rows, int32_t* __restrict__ cnt,
                                                                   unsigned long long* __restrict__ total,
                                                                   int32_t* __restrict__ host_flag) {
  const int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
  bool valid = false;
  if (i < n_index) {
    const int64_t v = index[i];
    valid = v >= 0 && v < n_rows;   // outside: never an address
    if (valid) atomicAdd(&cnt[v], 1);
    else if (host_flag != nullptr) *(volatile int32_t*)host_flag = 1;
  }
  const unsigned long long b = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(total, (unsigned long long)__popcll(b));
}

struct SmShape {
  int gl, k;
  int64_t chunks;
};

static int sm_shape(int64_t n_rows, int32_t n_classes, int32_t ld, SmShape* sh) {
  if (n_rows < 0 || n_classes <= 0 || ld < n_classes) return EGC_ERR_INVALID;
  if (n_classes > EGC_SOFTMAX_MAX_CLASSES) return EGC_ERR_UNSUPPORTED;
  const int q = (n_classes + 3) / 4;
  sh->gl = 0;
  while ((1 << sh->gl) < q && sh->gl < 6) ++sh->gl;
  sh->k = (q + (1 << sh->gl) - 1) >> sh->gl;
  sh->chunks = ceil_div(n_rows, SM_CHUNK);
  if (sh->chunks >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  return EGC_OK;
}

// KERNEL<vec, K><<<chunks, 256>>>(args) for the run-time K in 1..4
#define SM_LAUNCH(KERNEL, ...)                                                                         \
  do {                                                                                                 \
    const unsigned grid = (unsigned)sh.chunks;                                                         \
    if (vec) {                                                                                         \
      if (sh.k == 1) KERNEL<true, 1><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                      \
      else if (sh.k == 2) KERNEL<true, 2><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                 \
      else if (sh.k == 3) KERNEL<true, 3><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                 \
      else KERNEL<true, 4><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                                \
    } else {                                                                                           \
      if (sh.k == 1) KERNEL<false, 1><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                     \
      else if (sh.k == 2) KERNEL<false, 2><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                \
      else if (sh.k == 3) KERNEL<false, 3><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                \
      else KERNEL<false, 4><<<grid, SM_BLOCK, 0, stream>>>(__VA_ARGS__);                               \
    }                                                                                                  \
    EGC_LAUNCH_CHECK(#KERNEL);                                                                         \
  } while (0)

}  // namespace egc

using namespace egc;

int egc_log_softmax_forward_f32(const float* x, int64_t n_rows, int32_t n_classes, int32_t ld, float* out, float* lse,
                                int32_t* argmax, egc_stream_t stream_) {
  SmShape sh;
  if (int rc = sm_shape(n_rows, n_classes, ld, &sh)) return rc;
  if (n_rows == 0) return EGC_OK;
  if (x == nullptr || out == nullptr) return EGC_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (ld & 3) == 0 && (n_classes & 3) == 0 && aligned16(x) && aligned16(out);
  SM_LAUNCH(log_softmax_forward_kernel, x, n_rows, n_classes, ld, sh.gl, out, lse, argmax);
  return EGC_OK;
}

int egc_log_softmax_backward_f32(const float* grad_out, const float* out, int64_t n_rows, int32_t n_classes, int32_t ld,
                                 float* d_x, egc_stream_t stream_) {
  SmShape sh;
  if (int rc = sm_shape(n_rows, n_classes, ld, &sh)) return rc;
  if (n_rows == 0) return EGC_OK;
  if (grad_out == nullptr || out == nullptr || d_x == nullptr) return EGC_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (ld & 3) == 0 && (n_classes & 3) == 0 && aligned16(grad_out) && aligned16(out) && aligned16(d_x);
  SM_LAUNCH(log_softmax_backward_kernel, grad_out, out, n_rows, n_classes, ld, sh.gl, d_x);
  return EGC_OK;
}

int egc_row_selection_count(const int64_t* index, int64_t n_index, int64_t n_rows, int32_t* cnt, int64_t* total,
                            int32_t* host_flag, egc_stream_t stream_) {
  if (n_index < 0 || n_rows < 0 || total == nullptr || (cnt == nullptr && n_rows > 0) || (index == nullptr && n_index > 0))
    return EGC_ERR_INVALID;
  const int64_t blocks = ceil_div(n_index, SM_BLOCK);
  if (blocks >= ((int64_t)1 << 31) || n_index >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;   // cnt is int32
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows > 0) EGC_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)n_rows * sizeof(int32_t), stream));
  EGC_HIP_TRY(hipMemsetAsync(total, 0, sizeof(int64_t), stream));
  if (n_index == 0) return EGC_OK;
  selection_count_kernel<<<(unsigned)blocks, SM_BLOCK, 0, stream>>>(index, n_index, n_rows, cnt,
                                                                    reinterpret_cast<unsigned long long*>(total), host_flag);
  EGC_LAUNCH_CHECK("selection_count_kernel");
  return EGC_OK;
}

size_t egc_nll_log_softmax_workspace_bytes(int64_t n_rows, int32_t n_classes) {
  SmShape sh;
  if (sm_shape(n_rows, n_classes, n_classes, &sh) != EGC_OK) return 0;
  return (size_t)(sh.chunks > 0 ? sh.chunks : 1) * sizeof(float);
}

int egc_nll_log_softmax_forward_f32(const float* x, const int64_t* y, const int32_t* cnt, const int64_t* total, int64_t n_rows,
                                    int32_t n_classes, int32_t ld, int32_t mean, float* loss, float* lse, void* workspace,
                                    size_t workspace_bytes, int32_t* host_flag, egc_stream_t stream_) {
  SmShape sh;
  if (int rc = sm_shape(n_rows, n_classes, ld, &sh)) return rc;
  if (loss == nullptr || (cnt != nullptr && total == nullptr)) return EGC_ERR_INVALID;
  if (n_rows > 0 && (x == nullptr || y == nullptr || lse == nullptr)) return EGC_ERR_INVALID;
  if (workspace == nullptr || !aligned_to(workspace, 4) ||
      workspace_bytes < egc_nll_log_softmax_workspace_bytes(n_rows, n_classes))
    return EGC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* partial = static_cast<float*>(workspace);
  if (n_rows > 0) {
    const bool vec = (ld & 3) == 0 && aligned16(x);
    SM_LAUNCH(nll_forward_kernel, x, y, cnt, n_rows, n_classes, ld, sh.gl, lse, partial, host_flag);
  }
  nll_finalize_kernel<<<1, SM_BLOCK, 0, stream>>>(partial, sh.chunks, cnt != nullptr ? total : nullptr, n_rows, mean != 0, loss);
  EGC_LAUNCH_CHECK("nll_finalize_kernel");
  return EGC_OK;
}

int egc_nll_log_softmax_backward_f32(const float* x, const int64_t* y, const int32_t* cnt, const int64_t* total,
                                     const float* lse, const float* grad_loss, int64_t n_rows, int32_t n_classes, int32_t ld,
                                     int32_t mean, float* d_x, egc_stream_t stream_) {
  SmShape sh;
  if (int rc = sm_shape(n_rows, n_classes, ld, &sh)) return rc;
  if (n_rows == 0) return EGC_OK;
  if (x == nullptr || y == nullptr || lse == nullptr || grad_loss == nullptr || d_x == nullptr ||
      (cnt != nullptr && total == nullptr))
    return EGC_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (ld & 3) == 0 && aligned16(x) && aligned16(d_x);
  SM_LAUNCH(nll_backward_kernel, x, y, cnt, cnt != nullptr ? total : nullptr, lse, grad_loss, n_rows, n_classes, ld, sh.gl,
            mean != 0, d_x);
  return EGC_OK;
}
