// The optimizer step of every net of the reference -- torch.optim.Adam(params, lr, weight_decay=wd), zinc/configs.py,
// mol/configs.py, cifar/configs.py, code/configs.py, exp_config.py -- for ALL tensors of a parameter group as one launch.
// gfx950 only.  ABI and arithmetic: include/egc_optim.h; DESIGN.md section 3.33.
//
// torch composes the step from a dozen _foreach_* launches per chunk of tensors; the nets here have 35-70 tensors of a few
// hundred KB in all, so the step is bound by launches, not by the 7 arrays it streams.  One kernel, one workgroup of 256
// threads per 1024 elements of a tensor (a tensor without elements still has one, which counts its step):
//   * The per-tensor descriptors (p, g, state offset, step offset, numel) and the prefix sums of the tensors' workgroup
//     counts are kernel ARGUMENTS, by value.  GraphedStep records the backward with fresh gradient buffers from the graph's
//     pool, so the addresses differ from call to call; a device-side pointer table would have to be uploaded from pageable
//     host memory, which a capture refuses.  Arguments are copied at the launch call and recorded with the node.  Their
//     4 KB hold EGC_ADAM_MAX_TENSORS = 120 tensors at 32 bytes each; more tensors are further launches.
//   * A workgroup finds its tensor by bisection over the prefix sums: uniform scalar loads from the argument segment.
//   * Thread 0 reads the workgroup's step word, computes lr / (1 - beta1^t) and sqrt(1 - beta2^t) in float64 (beta^t by
//     repeated squaring over the bits of the integer t: exact to a few ulp of a double, no libm pow), rounds each once and
//     hands them over in LDS; the other threads load their elements meanwhile.  It writes t back: one writer per word.
//   * p, g, m, v move as one 16-byte access per thread where p and g are 16-byte aligned (the state slices always are), as
//     4-byte accesses for a tensor that is not (a view at an odd offset) and for the last partial quad.
// Bound by: launch latency and one dependent chain step word -> float64 factors -> barrier; 28 bytes per element of traffic.
// No atomics, every word has one writer, the element arithmetic is one fixed sequence of float32 operations (the build
// passes -ffp-contract=off; sqrtf and / are correctly rounded): results are bit-reproducible.
#include <atomic>

#include "egc_common.h"
#include "egc_optim.h"

namespace egc {

constexpr int ADAM_THREADS = 256;
static_assert(EGC_ADAM_BLOCK_ELEMS == ADAM_THREADS * 4, "one quad per thread");

struct AdamArgs {   // by value in the kernel arguments
  float* p[EGC_ADAM_MAX_TENSORS];
  float* g[EGC_ADAM_MAX_TENSORS];
  uint32_t state_off[EGC_ADAM_MAX_TENSORS];
  uint32_t step_off[EGC_ADAM_MAX_TENSORS];
  int32_t numel[EGC_ADAM_MAX_TENSORS];
  uint32_t prefix[EGC_ADAM_MAX_TENSORS + 1];   // workgroups in front of tensor k; prefix[n] = the grid
  float* m;
  float* v;
  int32_t* steps;
  const double* lr;
  double beta1, beta2;
  float b1, omb1, b2, omb2;   // beta and 1 - beta (taken in float64), rounded once on the host
  float eps, wd;
  int32_t n, zero;
};
static_assert(sizeof(AdamArgs) <= 4096, "the descriptors must fit HIP's 4 KB of kernel arguments");

__device__ inline double adam_powi(double x, int t) {   // x^t, t >= 0
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= x;
    x *= x;
    t >>= 1;
  }
  return r;
}

struct AdamFactors {
  float step_size, sqrt_bc2;
};

__device__ inline void adam_update(float& p, float& m, float& v, float g, const AdamArgs& a, AdamFactors f) {
  if (a.wd != 0.f) g = g + a.wd * p;
  m = a.b1 * m + a.omb1 * g;
  v = a.b2 * v + a.omb2 * (g * g);
  const float denom = sqrtf(v) / f.sqrt_bc2 + a.eps;
  p = p - f.step_size * (m / denom);
}

__global__ void __launch_bounds__(ADAM_THREADS) adam_kernel(const AdamArgs a) {
  __shared__ AdamFactors shared;
  const unsigned b = blockIdx.x;
  int lo = 0, hi = a.n;   // prefix[lo] <= b < prefix[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.prefix[mid] <= b) lo = mid;
    else hi = mid;
  }
  const int k = lo;
  const unsigned w = b - a.prefix[k];
  const int tid = (int)threadIdx.x;
  const int numel = a.numel[k];
  float* __restrict__ p = a.p[k];
  float* __restrict__ g = a.g[k];
  float* __restrict__ m = a.m + a.state_off[k];
  float* __restrict__ v = a.v + a.state_off[k];
  if (tid == 0) {
    int32_t* word = a.steps + (size_t)a.step_off[k] + w;
    const int t = *word + 1;
    const double lr = *a.lr;
    AdamFactors f;
    f.step_size = (float)(lr / (1.0 - adam_powi(a.beta1, t)));
    f.sqrt_bc2 = (float)sqrt(1.0 - adam_powi(a.beta2, t));
    shared = f;
    *word = t;
  }
  const int64_t i0 = (int64_t)w * EGC_ADAM_BLOCK_ELEMS + tid * 4;   // < 2^31 + 1024
  const bool quad = i0 + 4 <= numel && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  f4 pv = f4{0.f, 0.f, 0.f, 0.f}, gv = pv, mv = pv, vv = pv;
  if (quad) {   // in flight while thread 0 works out the factors
    pv = *reinterpret_cast<const f4*>(p + i0);
    gv = *reinterpret_cast<const f4*>(g + i0);
    mv = *reinterpret_cast<const f4*>(m + i0);
    vv = *reinterpret_cast<const f4*>(v + i0);
  }
  __syncthreads();   // the one barrier, outside every branch: `quad` differs between the lanes of a tensor's last workgroup
  const AdamFactors f = shared;
  if (quad) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], mj = mv[j], vj = vv[j];
      adam_update(pj, mj, vj, gv[j], a, f);
      pv[j] = pj;
      mv[j] = mj;
      vv[j] = vj;
    }
    *reinterpret_cast<f4*>(p + i0) = pv;
    *reinterpret_cast<f4*>(m + i0) = mv;
    *reinterpret_cast<f4*>(v + i0) = vv;
    if (a.zero) *reinterpret_cast<f4*>(g + i0) = f4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + j;
      if (i < numel) {
        float pj = p[i], mj = m[i], vj = v[i];
        adam_update(pj, mj, vj, g[i], a, f);
        p[i] = pj;
        m[i] = mj;
        v[i] = vj;
        if (a.zero) g[i] = 0.f;
      }
    }
  }
}

static inline int64_t adam_blocks(int64_t numel) {
  const int64_t b = ceil_div(numel, (int64_t)EGC_ADAM_BLOCK_ELEMS);
  return b > 0 ? b : 1;
}

static std::atomic<int64_t> g_adam_launches{0};

}  // namespace egc

using namespace egc;

int32_t egc_adam_max_tensors(void) { return EGC_ADAM_MAX_TENSORS; }

int64_t egc_adam_launches(int64_t n_tensors) {
  return n_tensors > 0 ? ceil_div(n_tensors, (int64_t)EGC_ADAM_MAX_TENSORS) : 0;
}

int64_t egc_adam_launch_count(void) { return g_adam_launches.load(std::memory_order_relaxed); }

int64_t egc_adam_plan(const int64_t* numels, int64_t n_tensors, int32_t* blocks_out, int64_t* state_offsets_out) {
  if (n_tensors < 0 || (n_tensors > 0 && (numels == nullptr || blocks_out == nullptr || state_offsets_out == nullptr))) return -1;
  int64_t total = 0;
  for (int64_t k = 0; k < n_tensors; ++k) {
    if (numels[k] < 0 || numels[k] >= ((int64_t)1 << 31)) return -1;
    blocks_out[k] = (int32_t)adam_blocks(numels[k]);
    state_offsets_out[k] = total;
    total += ceil_div(numels[k], (int64_t)4) * 4;
    if (total >= ((int64_t)1 << 32)) return -1;
  }
  return total;
}

int egc_adam_step_f32(const egc_adam_tensor* tensors, int64_t n_tensors, float* exp_avg, float* exp_avg_sq, int32_t* steps,
                      const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, int32_t zero_grads,
                      egc_stream_t stream_) {
  if (n_tensors < 0) return EGC_ERR_INVALID;
  if (n_tensors == 0) return EGC_OK;
  if (tensors == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || steps == nullptr || lr_dev == nullptr)
    return EGC_ERR_INVALID;
  if (!aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned_to(steps, 4) || !aligned_to(lr_dev, 8)) return EGC_ERR_INVALID;
  for (int64_t k = 0; k < n_tensors; ++k) {   // everything is checked before anything is launched
    const egc_adam_tensor& t = tensors[k];
    if (t.numel < 0 || t.numel >= ((int64_t)1 << 31)) return EGC_ERR_INVALID;
    if (t.numel > 0 && (t.p == nullptr || t.g == nullptr)) return EGC_ERR_INVALID;
    if (!aligned_to(t.p, 4) || !aligned_to(t.g, 4) || t.state_offset % 4 != 0) return EGC_ERR_INVALID;
  }
  AdamArgs a = {};
  a.m = exp_avg;
  a.v = exp_avg_sq;
  a.steps = steps;
  a.lr = lr_dev;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.b1 = (float)beta1;
  a.omb1 = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  a.zero = zero_grads != 0;
  hipStream_t stream = (hipStream_t)stream_;
  for (int64_t k0 = 0; k0 < n_tensors; k0 += EGC_ADAM_MAX_TENSORS) {
    const int n = (int)(n_tensors - k0 < EGC_ADAM_MAX_TENSORS ? n_tensors - k0 : EGC_ADAM_MAX_TENSORS);
    uint32_t grid = 0;
    for (int k = 0; k < n; ++k) {
      const egc_adam_tensor& t = tensors[k0 + k];
      a.p[k] = t.p;
      a.g[k] = t.g;
      a.state_off[k] = t.state_offset;
      a.step_off[k] = t.step_offset;
      a.numel[k] = (int32_t)t.numel;
      a.prefix[k] = grid;
      grid += (uint32_t)adam_blocks(t.numel);   // as egc_adam_plan counts them; at most 120 * 2^21
    }
    a.prefix[n] = grid;
    a.n = n;
    adam_kernel<<<grid, ADAM_THREADS, 0, stream>>>(a);
    EGC_LAUNCH_CHECK("adam_kernel");
    g_adam_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return EGC_OK;
}
