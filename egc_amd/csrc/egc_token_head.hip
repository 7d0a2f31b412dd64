// The token head of the reference's ogbg-code net, fused with its loss: T Linear maps of the pooled graph rows onto a
// vocabulary, the mean cross-entropy over the T positions, the arg-max of every position, and the backward of all of it.
// gfx950 only, float32.  The reference writes (code/models.py:95-98, 121-125 with code/configs.py:63-66, 94)
//     preds = [nn.Linear(hidden, 5002)(x) for _ in range(5)]              x = pooled [G, hidden]
//     loss  = sum(F.cross_entropy(preds[i], y_arr[:, i]) for i in range(5)) / 5
//     pred  = torch.argmax(preds[i], dim=1)
// which at G = 128 is a [128, 5 x 5002] logits array written and re-read several times and thirty launches.  Here nothing of
// size [G, V] exists: only x, W_t, b_t, y, one lse per (row, token) and the three gradients cross HBM.
//
// Decomposition.  The T V columns are cut into slabs of TH_SLAB = 64 columns of ONE token (the last slab of a token is
// short); workgroup w of n_wg owns the consecutive slabs [w spw, (w + 1) spw) (th_plan: spw = ceil(slabs / 256), n_wg =
// ceil(slabs / spw): every workgroup has work, none has more than spw slabs).  A workgroup is 8 wavefronts; it stages a
// slab's weight rows in LDS (zero rows past V, zero columns past K up to the next multiple of 16) and walks the rows of x in
// blocks of 128, wavefront v taking rows 16 v .. 16 v + 15 of a block.
//
// Logits: v_mfma_f32_16x16x4_f32, exact float32 products, bitwise an fma chain.  A lane takes 16 bytes of its x row and of
// its W row at k = 16 s + 4 (lane / 16) .. + 3 and feeds element e of both to MFMA e of step s, so the four k of one MFMA are
// 16 s + e + {0, 4, 8, 12}: logit[g, c] is ONE fma chain over a fixed permutation of k that is the same for every row and
// column (two columns with equal weights get equal bits), followed by one add of the bias.
//
// Forward.  Per slab and row: m = max, s = sum exp(logit - m) (a lane adds its 4 columns ascending, then the 16 lanes of a
// row over the xor distances 1, 2, 4, 8), the first maximal column, and the label's logit where the label lies in the slab.
// th_combine_kernel, one thread per (row, token): M = max of the slab maxima, S = sum over slabs ascending of s_i exp(m_i - M),
// lse = M + log S, arg-max = the arg-max of the FIRST slab whose maximum equals M; term = lse - logit[label] (0 and the sticky
// flag for a label outside [0, V)).  th_finalize_kernel, one workgroup: thread t adds term[t], term[t + 256], ... ascending
// (term index = row T + token), the 256 thread sums are added four adjacent ones per lane, ascending, then over the xor
// distances 32 .. 1; *loss = sum / float(G T).  Longest chain of adds: ceil(G T / 256) + 3 + 6.  No float atomics.
//
// Backward.  Loop order: row block (128 rows) outermost, the workgroup's slabs inside.  Per (block, slab):
//   1. the logit tile again, g = sc (exp(logit - lse) - [c == y]) with sc = grad_loss / float(G T), into LDS [128][64];
//   2. dW^T tile = x^T g over the block's rows on the matrix cores (wavefront v owns the k tiles v, v + 8, v + 16 and all four
//      column tiles; rows in the fixed order 16 (s / 4) + (s % 4) + {0, 4, 8, 12}, s = 0 .. 31), stored as 16-byte pieces of
//      dW_t rows; db = the column's sum over the block's rows ascending.  The first row block WRITES, a later one adds its sum
//      to what is there: at G <= 128 every element is written exactly once, and at any G only its owner touches it;
//   3. dx tile += g W over the slab's columns, 16 rows x all K per wavefront in accumulators that live across the slabs.
// After its slabs the workgroup writes its share of dx [128 rows, K] to partial[w]; th_dx_reduce_kernel adds the n_wg
// partials ascending.  Two runs give the same bits.
//
// Bytes at G = 128, K = 304, V = 5002, T = 5 (395 slabs, spw = 2, n_wg = 198): W 30.4 MB read once per pass, dW 30.4 MB
// written once, dx partials 198 x 155.6 KB = 30.8 MB written and read once -- the price of keeping dW complete inside its
// owner; x (155.6 KB) is re-read per slab from L2.  Flops: 1.95 G forward, 5.84 G backward (157 TFLOP/s: 12 and 37 us).
#include "egc_common.h"

#include <math.h>

namespace egc {
namespace {

constexpr int TH_SLAB = EGC_TOKEN_HEAD_SLAB;
constexpr int TH_WAVES = 8, TH_THREADS = 64 * TH_WAVES, TH_ROWS = 16 * TH_WAVES;   // 512 threads, 128 rows per block
constexpr int TH_MAX_K = EGC_TOKEN_HEAD_MAX_IN, TH_KT = TH_MAX_K / 16;                               // k tiles of the dx accumulators
constexpr int TH_GP = TH_SLAB + 4;        // pitch of the g tile: rows 4 apart and rows 1 apart with columns 4 apart hit distinct banks
constexpr int TH_CUS = 256;
constexpr int TH_BLOCK = 256;             // threads of the combine / finalize / reduce kernels
static_assert(TH_SLAB == 64, "four 16-column MFMA tiles per slab");

struct ThPtrs {
  const float* w[EGC_TOKEN_HEAD_MAX_SEQ];
  const float* b[EGC_TOKEN_HEAD_MAX_SEQ];
  float* dw[EGC_TOKEN_HEAD_MAX_SEQ];
  float* db[EGC_TOKEN_HEAD_MAX_SEQ];
};

// slab width, slabs per workgroup, partial count, LDS and workspace layout: the one owner (query and both launchers)
struct ThPlan {
  int kp, pw;            // K rounded up to 16; LDS pitch of a weight row (pw % 64 == 20: the 16-byte reads of 16 rows and the
                         // 4-byte reads of rows 4 apart both spread over all banks)
  int spt, slabs, spw, n_wg;
  size_t lds_fwd, lds_bwd;
  size_t off_recs, off_reci, off_ylog, off_term;   // float offsets of the forward's arrays (recm at 0)
  size_t bytes;          // max(forward, backward) workspace
};

static int th_plan(int64_t G, int32_t K, int64_t V, int32_t T, ThPlan* p) {
  if (G < 0 || K <= 0 || V <= 0 || T <= 0) return EGC_ERR_INVALID;
  if ((K & 3) != 0 || K > TH_MAX_K || T > EGC_TOKEN_HEAD_MAX_SEQ || V > (1 << 30) || G > (int64_t)1 << 30) return EGC_ERR_UNSUPPORTED;
  p->kp = (K + 15) / 16 * 16;
  p->pw = p->kp + ((20 - p->kp % 64) + 64) % 64;
  p->spt = (int)ceil_div(V, (int64_t)TH_SLAB);
  const int64_t slabs = (int64_t)T * p->spt;
  if (slabs >= (1 << 30)) return EGC_ERR_UNSUPPORTED;
  p->slabs = (int)slabs;
  p->spw = (int)ceil_div(slabs, (int64_t)TH_CUS);
  p->n_wg = (int)ceil_div(slabs, (int64_t)p->spw);
  p->lds_fwd = (size_t)TH_SLAB * p->pw * sizeof(float);
  p->lds_bwd = p->lds_fwd + (size_t)TH_ROWS * TH_GP * sizeof(float);
  const size_t rec = (size_t)slabs * (size_t)G, gt = (size_t)G * T;
  p->off_recs = rec;
  p->off_reci = 2 * rec;
  p->off_ylog = 3 * rec;
  p->off_term = 3 * rec + gt;
  const size_t fwd = (3 * rec + 2 * gt) * sizeof(float);
  const size_t bwd = (size_t)p->n_wg * (size_t)G * K * sizeof(float);
  const size_t need = fwd > bwd ? fwd : bwd;
  p->bytes = need < 16 ? 16 : (need + 15) / 16 * 16;
  return EGC_OK;
}

constexpr size_t TH_LDS_FWD_MAX = (size_t)TH_SLAB * (TH_MAX_K + 20) * sizeof(float);
constexpr size_t TH_LDS_BWD_MAX = TH_LDS_FWD_MAX + (size_t)TH_ROWS * TH_GP * sizeof(float);

template <typename P>
__device__ inline P th_pick(P const (&a)[EGC_TOKEN_HEAD_MAX_SEQ], int t) {
  P r = a[0];
#pragma unroll
  for (int i = 1; i < EGC_TOKEN_HEAD_MAX_SEQ; ++i) r = t == i ? a[i] : r;
  return r;
}

// rows c0 .. c0 + 63 of W [V][K] into wl [64][pw]: zeros in rows past V and in columns K .. kp - 1
__device__ inline void th_load_slab(float* __restrict__ wl, const float* __restrict__ W, int c0, int V, int K, int kp, int pw) {
  const int q4 = kp >> 2, total = TH_SLAB * q4;
  constexpr int U = 6;   // pieces of a thread in flight at once: the slab is two round trips to memory, not ten
  for (int base = threadIdx.x; base < total; base += U * TH_THREADS) {
    f4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * TH_THREADS, c = idx / q4, q = idx - c * q4;
      v[u] = f4{0.f, 0.f, 0.f, 0.f};
      if (idx < total && c0 + c < V && 4 * q < K) v[u] = *reinterpret_cast<const f4*>(W + (int64_t)(c0 + c) * K + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * TH_THREADS, c = idx / q4, q = idx - c * q4;
      if (idx < total) *reinterpret_cast<f4*>(wl + c * pw + 4 * q) = v[u];
    }
  }
}

// acc[j][r] = sum_k x[r0 + 4 (lane / 16) + r][k] W[c0 + 16 j + lane % 16][k] (rows past G: 0), the fma chain of the header
__device__ inline void th_logits(const float* __restrict__ x, int64_t r0, int64_t G, int K, int kp, const float* __restrict__ wl,
                                 int pw, int m, int kk, f4 (&acc)[4]) {
  const int64_t row = r0 + m;
  const bool rok = row < G;
  const float* xr = x + (rok ? row : 0) * K + 4 * kk;
  const float* wr = wl + m * pw + 4 * kk;
  const int steps = kp >> 4;
#pragma unroll 4
  for (int s = 0; s < steps; ++s) {
    f4 a = f4{0.f, 0.f, 0.f, 0.f};
    if (rok && 16 * s + 4 * kk < K) a = *reinterpret_cast<const f4*>(xr + 16 * s);
    f4 b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f4*>(wr + 16 * j * pw + 16 * s);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[j][e], acc[j], 0, 0, 0);
  }
}

#define TH_SLAB_INDEX                                                                              \
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, m = lane & 15, kk = lane >> 4;          \
  const int s0 = (int)blockIdx.x * spw, s1 = min(s0 + spw, slabs)

__global__ void __launch_bounds__(TH_THREADS) th_forward_kernel(const float* __restrict__ x, ThPtrs p, const int64_t* __restrict__ y,
                                                                int64_t G, int K, int V, int T, int kp, int pw, int spt, int slabs,
                                                                int spw, float* __restrict__ recm, float* __restrict__ recs,
                                                                int32_t* __restrict__ reci, float* __restrict__ ylog) {
  extern __shared__ float lds[];   // [TH_SLAB][pw]
  TH_SLAB_INDEX;
  for (int slab = s0; slab < s1; ++slab) {
    const int tok = slab / spt, sl = slab - tok * spt, c0 = sl * TH_SLAB;
    const float* bias = th_pick(p.b, tok);
    lds_barrier();   // the previous slab's reads are done
    th_load_slab(lds, th_pick(p.w, tok), c0, V, K, kp, pw);
    lds_barrier();
    float bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bj[j] = c0 + 16 * j + m < V ? bias[c0 + 16 * j + m] : 0.f;
    for (int64_t r0 = 16 * wave; r0 < G; r0 += TH_ROWS) {
      f4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
      th_logits(x, r0, G, K, kp, lds, pw, m, kk, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + 4 * kk + r;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c0 + 16 * j + m < V ? acc[j][r] + bj[j] : -INFINITY;
        float bm = v[0];
        int bi = c0 + m;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
          const bool take = v[j] > bm;
          bm = take ? v[j] : bm;
          bi = take ? c0 + 16 * j + m : bi;
        }
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
          const float om = __shfl_xor(bm, d);
          const int oi = __shfl_xor(bi, d);
          const bool take = om > bm || (om == bm && oi < bi);
          bm = take ? om : bm;
          bi = take ? oi : bi;
        }
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) e += c0 + 16 * j + m < V ? expf(v[j] - bm) : 0.f;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) e += __shfl_xor(e, d);
        if (row < G) {
          if (m == 0) {
            const int64_t at = (int64_t)slab * G + row;
            recm[at] = bm;
            recs[at] = e;
            reci[at] = bi;
          }
          if (y != nullptr) {
            const int64_t label = y[row * T + tok];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (label == c0 + 16 * j + m && label < V) ylog[row * T + tok] = v[j];   // one lane of one slab
          }
        }
      }
    }
  }
}

// one thread per (row, token): the slab records in ascending slab order
__global__ void __launch_bounds__(TH_BLOCK) th_combine_kernel(const float* __restrict__ recm, const float* __restrict__ recs,
                                                              const int32_t* __restrict__ reci, const float* __restrict__ ylog,
                                                              const int64_t* __restrict__ y, int64_t G, int V, int T, int spt,
                                                              float* __restrict__ lse, int32_t* __restrict__ argmax,
                                                              float* __restrict__ term, int32_t* __restrict__ host_flag) {
  const int64_t i = (int64_t)blockIdx.x * TH_BLOCK + threadIdx.x;
  if (i >= G * T) return;
  const int64_t g = i / T;
  const int tok = (int)(i - g * T);
  const int64_t base = (int64_t)tok * spt * G + g;
  float M = recm[base];
  int32_t I = reci[base];
  for (int sl = 1; sl < spt; ++sl) {
    const float m2 = recm[base + (int64_t)sl * G];
    if (m2 > M) {
      M = m2;
      I = reci[base + (int64_t)sl * G];
    }
  }
  if (argmax != nullptr) argmax[i] = I;
  if (lse == nullptr && y == nullptr) return;
  float S = 0.f;
  for (int sl = 0; sl < spt; ++sl) S += recs[base + (int64_t)sl * G] * expf(recm[base + (int64_t)sl * G] - M);
  const float L = M + logf(S);
  if (lse != nullptr) lse[i] = L;
  if (y != nullptr) {
    const int64_t label = y[i];
    const bool ok = label >= 0 && label < V;   // outside: never an address; nothing added, flag raised
    term[i] = ok ? L - ylog[i] : 0.f;
    if (!ok && host_flag != nullptr) *(volatile int32_t*)host_flag = 1;   // sticky, host-visible
  }
}

// *loss = (sum of the n terms in the fixed order of the header) / float(n); n == 0 gives NaN as torch's mean does
__global__ void __launch_bounds__(TH_BLOCK) th_finalize_kernel(const float* __restrict__ term, int64_t n, float* __restrict__ loss) {
  __shared__ float s_part[TH_BLOCK];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += TH_BLOCK) a += term[i];
  s_part[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    float v = s_part[4 * lane];
#pragma unroll
    for (int j = 1; j < 4; ++j) v += s_part[4 * lane + j];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) *loss = v / (float)n;
  }
}

__global__ void __launch_bounds__(TH_THREADS) th_backward_kernel(const float* __restrict__ x, ThPtrs p, const int64_t* __restrict__ y,
                                                                 const float* __restrict__ lse, const float* __restrict__ grad_loss,
                                                                 int64_t G, int K, int V, int T, int kp, int pw, int spt, int slabs,
                                                                 int spw, float* __restrict__ partial, int want_dx, int want_dw,
                                                                 int want_db) {
  extern __shared__ float lds[];   // [TH_SLAB][pw] weights, then [TH_ROWS][TH_GP] g
  TH_SLAB_INDEX;
  float* wl = lds;
  float* gl = lds + TH_SLAB * pw;
  const int nkt = kp >> 4;
  const float sc = *grad_loss / (float)(G * T);
  for (int64_t sb0 = 0; sb0 < G; sb0 += TH_ROWS) {
    f4 dxa[TH_KT];
#pragma unroll
    for (int j = 0; j < TH_KT; ++j) dxa[j] = f4{0.f, 0.f, 0.f, 0.f};
    for (int slab = s0; slab < s1; ++slab) {
      const int tok = slab / spt, sl = slab - tok * spt, c0 = sl * TH_SLAB;
      const float* bias = th_pick(p.b, tok);
      lds_barrier();   // the previous slab's reads of both tiles are done
      th_load_slab(wl, th_pick(p.w, tok), c0, V, K, kp, pw);
      lds_barrier();
      {  // 1. g tile
        f4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
        const int64_t r0 = sb0 + 16 * wave;
        th_logits(x, r0, G, K, kp, wl, pw, m, kk, acc);
        float bj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bj[j] = c0 + 16 * j + m < V ? bias[c0 + 16 * j + m] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = r0 + 4 * kk + r;
          const bool rok = row < G;
          const int64_t label = rok ? y[row * T + tok] : -1;
          const float L = rok ? lse[row * T + tok] : 0.f;
          const bool ok = rok && label >= 0 && label < V;   // a label outside the classes: a zero gradient row
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int col = c0 + 16 * j + m;
            float gv = 0.f;
            if (ok && col < V) gv = sc * (expf((acc[j][r] + bj[j]) - L) - (col == label ? 1.f : 0.f));
            gl[(16 * wave + 4 * kk + r) * TH_GP + 16 * j + m] = gv;
          }
        }
      }
      lds_barrier();
      if (want_dw) {  // 2. dW^T tiles [k][c] = sum over the block's rows of x[row][k] g[row][c]
        f4 dwa[3][4];
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
#pragma unroll
          for (int i = 0; i < 4; ++i) dwa[jj][i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < TH_ROWS / 4; ++s) {   // (eight steps' loads of x in flight: the product waits on L2 otherwise)
          const int rowl = 16 * (s >> 2) + 4 * kk + (s & 3);   // the four rows of a step are 4 apart: conflict-free reads of g
          const int64_t row = sb0 + rowl;
          float a[3], b[4];
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) {
            const int k = 16 * (wave + TH_WAVES * jj) + m;
            a[jj] = (row < G && k < K) ? x[row * K + k] : 0.f;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) b[i] = gl[rowl * TH_GP + 16 * i + m];
#pragma unroll
          for (int jj = 0; jj < 3; ++jj)
            if (wave + TH_WAVES * jj < nkt) {
#pragma unroll
              for (int i = 0; i < 4; ++i) dwa[jj][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], b[i], dwa[jj][i], 0, 0, 0);
            }
        }
        float* dW = th_pick(p.dw, tok);
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int col = c0 + 16 * i + m, k = 16 * (wave + TH_WAVES * jj) + 4 * kk;   // register r is k + r
            if (col < V && k < K) {
              f4* dst = reinterpret_cast<f4*>(dW + (int64_t)col * K + k);
              f4 v = dwa[jj][i];
              if (sb0 > 0) v = *dst + v;
              *dst = v;
            }
          }
      }
      if (want_db && t < TH_SLAB && c0 + t < V) {
        float sum = 0.f;
        for (int rowl = 0; rowl < TH_ROWS; ++rowl) sum += gl[rowl * TH_GP + t];
        float* db = th_pick(p.db, tok);
        db[c0 + t] = sb0 > 0 ? db[c0 + t] + sum : sum;
      }
      if (want_dx) {  // 3. dx tile [row][k] += sum over the slab's columns of g[row][c] W[c][k]
#pragma unroll 1
        for (int s = 0; s < TH_SLAB / 4; ++s) {
          const int c = 16 * (s >> 2) + 4 * kk + (s & 3);   // columns 4 apart: conflict-free reads of the weight rows
          const float a = gl[(16 * wave + m) * TH_GP + c];
          const float* wrow = wl + c * pw + m;
#pragma unroll
          for (int j = 0; j < TH_KT; ++j)
            if (j < nkt) dxa[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wrow[16 * j], dxa[j], 0, 0, 0);
        }
      }
    }
    if (want_dx) {
      float* out = partial + ((int64_t)blockIdx.x * G + sb0 + 16 * wave + 4 * kk) * K;
#pragma unroll
      for (int j = 0; j < TH_KT; ++j)
        if (j < nkt) {
          const int k = 16 * j + m;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (sb0 + 16 * wave + 4 * kk + r < G && k < K) out[(int64_t)r * K + k] = dxa[j][r];
        }
    }
  }
}

// dx = partial[0] + partial[1] + ... ascending, 16 bytes per thread
__global__ void __launch_bounds__(TH_BLOCK) th_dx_reduce_kernel(const float* __restrict__ partial, int n_wg, int64_t n4,
                                                                float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * TH_BLOCK + threadIdx.x;
  if (i >= n4) return;
  const f4* p = reinterpret_cast<const f4*>(partial) + i;
  f4 s = p[0];
#pragma unroll 8
  for (int w = 1; w < n_wg; ++w) s += p[(int64_t)w * n4];
  reinterpret_cast<f4*>(dx)[i] = s;
}

}  // namespace
}  // namespace egc

using namespace egc;

size_t egc_token_head_workspace_bytes(int64_t n_rows, int32_t in_features, int32_t n_classes, int32_t seq_len) {
  ThPlan p;
  if (th_plan(n_rows, in_features, n_classes, seq_len, &p) != EGC_OK) return 0;
  return p.bytes;
}

int egc_token_head_forward_f32(const float* x, const float* const* weights, const float* const* biases, const int64_t* y,
                               int64_t n_rows, int32_t in_features, int32_t n_classes, int32_t seq_len, float* loss, float* lse,
                               int32_t* argmax, void* workspace, size_t workspace_bytes, int32_t* host_flag,
                               egc_stream_t stream_) {
  ThPlan pl;
  if (int rc = th_plan(n_rows, in_features, n_classes, seq_len, &pl)) return rc;
  if (weights == nullptr || biases == nullptr) return EGC_ERR_INVALID;
  const bool train = y != nullptr || (n_rows == 0 && loss != nullptr);   // (no row: an empty y has no address)
  if (train ? (loss == nullptr || (n_rows > 0 && lse == nullptr)) : (n_rows > 0 && argmax == nullptr)) return EGC_ERR_INVALID;
  ThPtrs ptrs = {};
  for (int t = 0; t < seq_len; ++t) {
    if (weights[t] == nullptr || biases[t] == nullptr) return EGC_ERR_INVALID;
    if (!aligned16(weights[t])) return EGC_ERR_UNSUPPORTED;
    ptrs.w[t] = weights[t];
    ptrs.b[t] = biases[t];
  }
  if (n_rows > 0 && x == nullptr) return EGC_ERR_INVALID;
  if (!aligned16(x)) return EGC_ERR_UNSUPPORTED;
  if (workspace == nullptr || !aligned16(workspace) || workspace_bytes < pl.bytes) return EGC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* ws = static_cast<float*>(workspace);
  float* term = ws + pl.off_term;
  if (n_rows > 0) {
    EGC_ALLOW_DYNAMIC_LDS(&th_forward_kernel, TH_LDS_FWD_MAX, "th_forward_kernel");
    th_forward_kernel<<<(unsigned)pl.n_wg, TH_THREADS, pl.lds_fwd, stream>>>(
        x, ptrs, y, n_rows, in_features, n_classes, seq_len, pl.kp, pl.pw, pl.spt, pl.slabs, pl.spw, ws, ws + pl.off_recs,
        reinterpret_cast<int32_t*>(ws + pl.off_reci), ws + pl.off_ylog);
    EGC_LAUNCH_CHECK("th_forward_kernel");
    const int64_t gt = n_rows * seq_len;
    th_combine_kernel<<<(unsigned)ceil_div(gt, (int64_t)TH_BLOCK), TH_BLOCK, 0, stream>>>(
        ws, ws + pl.off_recs, reinterpret_cast<const int32_t*>(ws + pl.off_reci), ws + pl.off_ylog, y, n_rows, n_classes, seq_len,
        pl.spt, lse, argmax, term, host_flag);
    EGC_LAUNCH_CHECK("th_combine_kernel");
  }
  if (train) {
    th_finalize_kernel<<<1, TH_BLOCK, 0, stream>>>(term, n_rows * seq_len, loss);
    EGC_LAUNCH_CHECK("th_finalize_kernel");
  }
  return EGC_OK;
}

int egc_token_head_backward_f32(const float* x, const float* const* weights, const float* const* biases, const int64_t* y,
                                const float* lse, const float* grad_loss, int64_t n_rows, int32_t in_features, int32_t n_classes,
                                int32_t seq_len, float* d_x, float* const* d_weights, float* const* d_biases, void* workspace,
                                size_t workspace_bytes, egc_stream_t stream_) {
  ThPlan pl;
  if (int rc = th_plan(n_rows, in_features, n_classes, seq_len, &pl)) return rc;
  if (weights == nullptr || biases == nullptr || grad_loss == nullptr) return EGC_ERR_INVALID;
  ThPtrs ptrs = {};
  for (int t = 0; t < seq_len; ++t) {
    if (weights[t] == nullptr || biases[t] == nullptr) return EGC_ERR_INVALID;
    if ((d_weights != nullptr && d_weights[t] == nullptr) || (d_biases != nullptr && d_biases[t] == nullptr)) return EGC_ERR_INVALID;
    if (!aligned16(weights[t]) || (d_weights != nullptr && !aligned16(d_weights[t]))) return EGC_ERR_UNSUPPORTED;
    ptrs.w[t] = weights[t];
    ptrs.b[t] = biases[t];
    ptrs.dw[t] = d_weights != nullptr ? d_weights[t] : nullptr;
    ptrs.db[t] = d_biases != nullptr ? d_biases[t] : nullptr;
  }
  if (n_rows > 0 && (x == nullptr || y == nullptr || lse == nullptr)) return EGC_ERR_INVALID;
  if (!aligned16(x) || !aligned16(d_x)) return EGC_ERR_UNSUPPORTED;
  if (workspace == nullptr || !aligned16(workspace) || workspace_bytes < pl.bytes) return EGC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows == 0) {   // no row: the parameters' gradients are zeros, d_x is empty
    for (int t = 0; t < seq_len; ++t) {
      if (d_weights != nullptr) EGC_HIP_TRY(hipMemsetAsync(d_weights[t], 0, (size_t)n_classes * in_features * sizeof(float), stream));
      if (d_biases != nullptr) EGC_HIP_TRY(hipMemsetAsync(d_biases[t], 0, (size_t)n_classes * sizeof(float), stream));
    }
    return EGC_OK;
  }
  if (d_x == nullptr && d_weights == nullptr && d_biases == nullptr) return EGC_OK;
  float* partial = static_cast<float*>(workspace);
  EGC_ALLOW_DYNAMIC_LDS(&th_backward_kernel, TH_LDS_BWD_MAX, "th_backward_kernel");
  th_backward_kernel<<<(unsigned)pl.n_wg, TH_THREADS, pl.lds_bwd, stream>>>(
      x, ptrs, y, lse, grad_loss, n_rows, in_features, n_classes, seq_len, pl.kp, pl.pw, pl.spt, pl.slabs, pl.spw, partial,
      d_x != nullptr, d_weights != nullptr, d_biases != nullptr);
  EGC_LAUNCH_CHECK("th_backward_kernel");
  if (d_x != nullptr) {
    const int64_t n4 = n_rows * in_features / 4;
    th_dx_reduce_kernel<<<(unsigned)ceil_div(n4, (int64_t)TH_BLOCK), TH_BLOCK, 0, stream>>>(partial, pl.n_wg, n4, d_x);
    EGC_LAUNCH_CHECK("th_dx_reduce_kernel");
  }
  return EGC_OK;
}
