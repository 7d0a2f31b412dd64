// The graph-level MLP head of the reference's batched nets, fused with its loss: pool -> mlp([h, h/2, h/4, out]) -> loss, where
// experiments/utils.py:30-40 builds mlp as Linear -> BatchNorm1d -> ReLU -> Dropout(0) per hidden layer and a final Linear, and
// the loss is F.l1_loss (zinc/configs.py:48-50), F.binary_cross_entropy_with_logits over the labelled entries
// (mol/configs.py:64-68) or none (the caller's own; cifar/configs.py:57 takes egc_nll_log_softmax).  gfx950 only, float32.
// sizes = [K0, K1, .., K_{L-1}, OUT]: L Linears (1 <= L <= EGC_HEAD_MAX_LINEARS), L - 1 of them followed by a BatchNorm; any
// positive widths <= EGC_HEAD_MAX_WIDTH (no multiple-of-4 requirement: nothing here moves 16 bytes of global memory at a
// time), OUT <= EGC_HEAD_MAX_OUT, 2 <= G <= EGC_HEAD_MAX_ROWS rows in training.
//
// Launch structure (every dependency on all rows is a launch boundary or the arrival counter of egc_bn_column.h: the block whose
// agent-scope fetch_add finds all others arrived reads their partials after an acquire fence and re-zeroes the counter; no
// grid barrier, no spin wait, no cooperative launch, no float atomics):
//   training forward   L launches of hd_linear_kernel, one per Linear.  Launch l reads its input rows (x, or z_{l-1} with
//                      a = relu(z scale + shift) applied on load), writes z_l = a W_l^T + b_l; a hidden layer's launch also
//                      writes float64 column partials of z_l per row block, and its last block turns them into stats_l (mean,
//                      biased variance, 1/std), affine_l (scale, shift) and the running statistics (num_batches_tracked is
//                      bumped there too).  The final launch writes out [G, OUT] and, with a fused loss, per-block float64 loss
//                      partials that its last block adds into {loss, labelled count}.
//   evaluation forward ONE launch of hd_eval_kernel: a block carries its 16 rows through all layers in LDS; the running
//                      statistics are folded into scale / shift per column by the block itself (float64, as the tail does).
//   training backward  L launches of hd_backward_rows_kernel, from the top layer down, and ONE hd_param_grad_kernel.
//                      Row pass of layer l: forms dz_l for its 16 rows (the top layer: d out of the fused loss, or the caller's
//                      gradient; a hidden layer: dz = c_g g + c_h z + c_1 from the g_l the pass above wrote), then
//                      d a = dz_l W_l.  Layer 1: that is d x.  Otherwise g_{l-1} = d a * [pre > 0] is written with float64
//                      partials of sum g and sum g z per row block, and the last block turns them into d gamma, d beta and
//                      the three coefficients of layer l - 1.
//                      hd_param_grad_kernel: one block per 16 x 16 tile of every dW_l = dz_l^T a_{l-1}; a_{l-1} is formed
//                      again from z_{l-1} and affine_{l-1} on load; the tiles of the first k columns also produce d b_l.
//   That is L launches forward (1 in evaluation) and L + 1 backward (L when no parameter needs a gradient).  No [G, K] array
//   exists beyond z_l, g_l and dz_l; no activation and no mask is stored: the ReLU decision is the float32 expression
//   fl(fl(z * scale) + shift) > 0 wherever it is needed.
//
// Tiling.  hd_linear_kernel: a block of 256 threads owns 16 rows x 64 output columns (grid: row blocks x column tiles); thread
// t owns row t / 16 and the four columns 4 (t % 16) .. + 3.  The input rows sit in LDS at full width, the weights pass
// through LDS in chunks of 32 along the reduction.  The row passes own 16 rows and walk the column tiles themselves.
//
// Orders (two runs give the same bits):
//   product       every output element is ONE float32 fma chain over the reduction index ascending (exact products, zeros
//                 past the end add nothing), then one add of the bias (forward).
//   column sums   float64.  A row block adds its 16 rows ascending.  The last block adds the row blocks' partials: lane
//                 j = 0 .. 7 takes the partials j, j + 8, .. ascending, then the eight lane sums are added ascending.
//   loss          float64 terms.  A row block adds, per column, its rows ascending, then the columns ascending.  The last
//                 block: lane j = 0 .. 63 takes the blocks j, j + 64, .. ascending, then the lane sums ascending;
//                 loss = float(sum / count).  The stand-alone losses: thread j = 0 .. 255 takes the elements j, j + 256, ..
//                 ascending, then the thread sums ascending.
//   dW, db        one fma chain (db: one chain of adds) over all G rows ascending.
#include "egc_bn_column.h"
#include "egc_common.h"

#include <atomic>
#include <math.h>

namespace egc {
namespace {

constexpr int HD_ROWS = EGC_HEAD_ROW_TILE, HD_COLS = 64, HD_RED = 32, HD_THREADS = 256;
constexpr int HD_PA = EGC_HEAD_MAX_WIDTH + 4;   // LDS pitch of an activation row
constexpr int HD_PW = HD_COLS + 4;              // LDS pitch of a weight chunk row
constexpr int HD_LANES = 8, HD_GCOLS = 32;      // the last block's column totals: 32 columns x 8 partial lanes at a time
constexpr int HD_PT = 16, HD_PCHUNK = 256;      // parameter gradients: 16 x 16 tile, 256 rows staged at a time
static_assert(HD_ROWS == 16 && HD_THREADS == 16 * 16, "thread t owns row t / 16");
static_assert(EGC_HEAD_MAX_OUT <= HD_COLS, "the final Linear is one column tile");

std::atomic<int64_t> g_head_launches{0};
inline void launched() { g_head_launches.fetch_add(1, std::memory_order_relaxed); }

// the ReLU decision's argument: two roundings, never contracted
__device__ inline float hd_pre(float z, float scale, float shift) { return __fadd_rn(__fmul_rn(z, scale), shift); }

// 16 rows r0 .. of in [G][K] into al [16][HD_PA]: relu(z scale + shift) with affine [2][K], zeros past G and in K .. K + 3
__device__ inline void hd_fill(float* __restrict__ al, const float* __restrict__ in, const float* __restrict__ affine, int64_t r0,
                               int64_t G, int K) {
  const int kp = (K + 3) & ~3;
  for (int idx = threadIdx.x; idx < HD_ROWS * kp; idx += HD_THREADS) {
    const int r = idx / kp, k = idx - r * kp;
    float v = 0.f;
    if (r0 + r < G && k < K) {
      v = in[(r0 + r) * K + k];
      if (affine != nullptr) {
        const float pre = hd_pre(v, affine[k], affine[K + k]);
        v = pre > 0.f ? pre : 0.f;
      }
    }
    al[r * HD_PA + k] = v;
  }
}

// acc[j] = sum over red = 0 .. R - 1 ascending of al[t / 16][red] * w(red, c0 + 4 (t % 16) + j), one fma chain per element.
// TRANS: w(red, col) = W[col * ld + red] (forward: W is [C][R]); else w(red, col) = W[red * ld + col] (backward: W is [R][C]).
// Columns past C give 0.  al holds zeros in R .. round-up-4(R).  Begins with a barrier: al and wl may have just been written.
template <bool TRANS>
__device__ inline f4 hd_tile_mm(const float* __restrict__ al, const float* __restrict__ W, int ld, int R, int C, int c0,
                                float* __restrict__ wl) {
  const int t = threadIdx.x, r = t >> 4, c4 = t & 15;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  constexpr int PER = HD_RED * HD_COLS / HD_THREADS;
  float wv[PER];   // the next chunk on its way while this one is multiplied
  auto fetch = [&](int red0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = t + HD_THREADS * i;
      const int rr = TRANS ? (idx & (HD_RED - 1)) : (idx >> 6), cc = TRANS ? (idx >> 5) : (idx & (HD_COLS - 1));
      const int red = red0 + rr, col = c0 + cc;
      wv[i] = (red < R && col < C) ? (TRANS ? W[(int64_t)col * ld + red] : W[(int64_t)red * ld + col]) : 0.f;
    }
  };
  fetch(0);
  for (int red0 = 0; red0 < R; red0 += HD_RED) {
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = t + HD_THREADS * i;
      const int rr = TRANS ? (idx & (HD_RED - 1)) : (idx >> 6), cc = TRANS ? (idx >> 5) : (idx & (HD_COLS - 1));
      wl[rr * HD_PW + cc] = wv[i];
    }
    __syncthreads();
    if (red0 + HD_RED < R) fetch(red0 + HD_RED);
    const int lim = min(HD_RED, R - red0);
    for (int rr = 0; rr < lim; rr += 4) {
      const f4 a = *reinterpret_cast<const f4*>(al + r * HD_PA + red0 + rr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f4 w = *reinterpret_cast<const f4*>(wl + (rr + e) * HD_PW + 4 * c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(a[e], w[j], acc[j]);
      }
    }
  }
  return acc;
}

// A row block's float64 column sums of a and a * b over the 16 rows ascending, from two LDS tiles [16][HD_PW] (ta, tb):
// partials[block][0][col] = sum ta, partials[block][1][col] = sum ta * tb
__device__ inline void hd_block_moments(const float* ta, const float* tb, int c0, int cols, int block, double* partials) {
  const int t = threadIdx.x;
  if (t < HD_COLS && c0 + t < cols) {
    double s1 = 0.0, s2 = 0.0;
    for (int rr = 0; rr < HD_ROWS; ++rr) {
      const double a = (double)ta[rr * HD_PW + t];
      s1 += a;
      s2 += a * (double)tb[rr * HD_PW + t];
    }
    store_partial(partials + ((int64_t)block * 2) * cols + c0 + t, s1);
    store_partial(partials + ((int64_t)block * 2 + 1) * cols + c0 + t, s2);
  }
}

// The last block: totals of the columns cbase .. cbase + 31 over n_p partial blocks in the header's order; valid in the
// threads t < 32 (column cbase + t).  All threads of the block call it.
__device__ inline void hd_col_totals(const double* __restrict__ partials, int n_p, int cols, int cbase,
                                     double (&red)[2][HD_LANES][HD_GCOLS + 1], double& t1, double& t2) {
  const int cl = threadIdx.x & (HD_GCOLS - 1), pl = threadIdx.x >> 5, col = cbase + cl;
  double s1 = 0.0, s2 = 0.0;
  if (col < cols) {
    int p = pl;
    for (; p + 7 * HD_LANES < n_p; p += 8 * HD_LANES) {   // eight partials' loads in flight, added in the same order
      double a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a[u] = partials[((int64_t)(p + u * HD_LANES) * 2) * cols + col];
        b[u] = partials[((int64_t)(p + u * HD_LANES) * 2 + 1) * cols + col];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s1 += a[u];
        s2 += b[u];
      }
    }
    for (; p < n_p; p += HD_LANES) {
      s1 += partials[((int64_t)p * 2) * cols + col];
      s2 += partials[((int64_t)p * 2 + 1) * cols + col];
    }
  }
  __syncthreads();   // the previous group's totals have been read
  red[0][pl][cl] = s1;
  red[1][pl][cl] = s2;
  __syncthreads();
  t1 = t2 = 0.0;
  if (pl == 0)
    for (int k = 0; k < HD_LANES; ++k) {
      t1 += red[0][k][cl];
      t2 += red[1][k][cl];
    }
}

// one element of a loss in float64: its term and whether it counts
__device__ inline void hd_loss_term(int kind, float o_, float y_, double& term, double& cnt) {
  const double o = (double)o_, y = (double)y_;
  if (kind == EGC_HEAD_LOSS_L1) {
    term = fabs(o - y);
    cnt = 1.0;
  } else {
    const bool ok = y_ == y_;
    term = ok ? fmax(o, 0.0) - o * y + log1p(exp(-fabs(o))) : 0.0;
    cnt = ok ? 1.0 : 0.0;
  }
}

// d loss / d o of one element, rounded once: sc = grad_loss / count in float64
__device__ inline float hd_loss_grad(int kind, float o_, float y_, double sc) {
  const double o = (double)o_, y = (double)y_;
  if (kind == EGC_HEAD_LOSS_L1) return (float)(o > y ? sc : (o < y ? -sc : 0.0));
  if (!(y_ == y_)) return 0.f;
  return (float)((1.0 / (1.0 + exp(-o)) - y) * sc);
}

__device__ inline double hd_loss_scale(int kind, const float* grad_loss, const float* loss2, double n_elements) {
  return (double)*grad_loss / (kind == EGC_HEAD_LOSS_L1 ? n_elements : (double)loss2[1]);
}

struct HdLinear {
  const float* in;          // [G][K]: x, or the z of the layer below
  const float* in_affine;   // [2][K] of the layer below, or nullptr (x)
  const float* W;           // [N][K]
  const float* b;           // [N]
  float* z;                 // [G][N]: z_l, or out
  int64_t G;
  int K, N, hidden;
  // hidden layer: statistics
  double* partials;         // [row blocks][2][N]
  int* sync;
  const float* gamma;
  const float* beta;
  double eps, momentum;
  double* stats;            // [3][N]
  float* affine;            // [2][N]
  float* running_mean;
  float* running_var;
  int64_t* n_tracked;
  // final layer: loss
  int loss_kind;
  const float* y;           // [G][N]
  float* loss2;             // {loss, count}
  double* lpart;            // [row blocks][2]
};

__global__ void __launch_bounds__(HD_THREADS) hd_linear_kernel(HdLinear a) {
  __shared__ __attribute__((aligned(16))) float al[HD_ROWS * HD_PA];
  __shared__ __attribute__((aligned(16))) float wl[HD_RED * HD_PW];
  __shared__ double red[2][HD_LANES][HD_GCOLS + 1];
  __shared__ double s_tracked;
  const int t = threadIdx.x, r = t >> 4, c4 = t & 15;
  const int64_t r0 = (int64_t)blockIdx.x * HD_ROWS, row = r0 + r;
  const int c0 = (int)blockIdx.y * HD_COLS;
  const int n_blocks = (int)(gridDim.x * gridDim.y);
  hd_fill(al, a.in, a.in_affine, r0, a.G, a.K);
  const f4 acc = hd_tile_mm<true>(al, a.W, a.K, a.K, a.N, c0, wl);
  f4 z;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = c0 + 4 * c4 + j;
    const bool ok = row < a.G && col < a.N;
    z[j] = ok ? acc[j] + a.b[col] : 0.f;
    if (ok) a.z[row * a.N + col] = z[j];
  }
  if (a.hidden) {
    __syncthreads();   // the last chunk's reads of wl are done
    *reinterpret_cast<f4*>(wl + r * HD_PW + 4 * c4) = z;
    __syncthreads();
    hd_block_moments(wl, wl, c0, a.N, (int)blockIdx.x, a.partials);
    if (!arrive_last(a.sync, n_blocks)) return;
    if (t == 0) {   // nn.BatchNorm1d: the count first, the cumulative average then uses it
      double tracked = 1.0;
      if (a.running_mean != nullptr && a.n_tracked != nullptr) {
        const int64_t n = *a.n_tracked + 1;
        *a.n_tracked = n;
        tracked = (double)n;
      }
      s_tracked = tracked;
    }
    __syncthreads();
    for (int cbase = 0; cbase < a.N; cbase += HD_GCOLS) {
      double t1, t2;
      hd_col_totals(a.partials, (int)gridDim.x, a.N, cbase, red, t1, t2);
      if (t < HD_GCOLS && cbase + t < a.N)
        bn_forward_column(t1, t2, cbase + t, a.N, (double)a.G, a.gamma, a.beta, a.eps, a.stats, a.affine, a.running_mean,
                             a.running_var, a.momentum, s_tracked);
    }
    return;
  }
  if (a.loss_kind == EGC_HEAD_LOSS_NONE) return;
  // the final layer's loss: one column tile (N <= 64), so the row blocks are the blocks
  __syncthreads();   // al is free
  double* dt = reinterpret_cast<double*>(al);   // [16][64] terms, then [16][64] counts
  double* ct = dt + HD_ROWS * HD_COLS;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = 4 * c4 + j;
    double term = 0.0, cnt = 0.0;
    if (row < a.G && col < a.N) hd_loss_term(a.loss_kind, z[j], a.y[row * a.N + col], term, cnt);
    dt[r * HD_COLS + col] = term;
    ct[r * HD_COLS + col] = cnt;
  }
  __syncthreads();
  double s = 0.0, c = 0.0;
  if (t < HD_COLS)
    for (int rr = 0; rr < HD_ROWS; ++rr) {
      s += dt[rr * HD_COLS + t];
      c += ct[rr * HD_COLS + t];
    }
  __syncthreads();
  if (t < HD_COLS) {
    dt[t] = s;
    ct[t] = c;
  }
  __syncthreads();
  if (t == 0) {
    s = c = 0.0;
    for (int k = 0; k < HD_COLS; ++k) {
      s += dt[k];
      c += ct[k];
    }
    store_partial(a.lpart + 2 * (int64_t)blockIdx.x, s);
    store_partial(a.lpart + 2 * (int64_t)blockIdx.x + 1, c);
  }
  if (!arrive_last(a.sync, n_blocks)) return;
  s = c = 0.0;
  if (t < 64)
    for (int p = t; p < n_blocks; p += 64) {
      s += a.lpart[2 * (int64_t)p];
      c += a.lpart[2 * (int64_t)p + 1];
    }
  __syncthreads();
  if (t < 64) {
    dt[t] = s;
    ct[t] = c;
  }
  __syncthreads();
  if (t == 0) {
    s = c = 0.0;
    for (int k = 0; k < 64; ++k) {
      s += dt[k];
      c += ct[k];
    }
    a.loss2[0] = (float)(s / c);   // no labelled entry: 0 / 0 = NaN, torch's mean over an empty selection
    a.loss2[1] = (float)c;
  }
}

struct HdEval {
  const float* x;
  float* out;
  int64_t G;
  int L;
  int sizes[EGC_HEAD_MAX_LINEARS + 1];
  const float* W[EGC_HEAD_MAX_LINEARS];
  const float* b[EGC_HEAD_MAX_LINEARS];
  const float* gamma[EGC_HEAD_MAX_LINEARS];
  const float* beta[EGC_HEAD_MAX_LINEARS];
  const float* running_mean[EGC_HEAD_MAX_LINEARS];
  const float* running_var[EGC_HEAD_MAX_LINEARS];
  double eps[EGC_HEAD_MAX_LINEARS];
};

__global__ void __launch_bounds__(HD_THREADS) hd_eval_kernel(HdEval a) {
  __shared__ __attribute__((aligned(16))) float buf[2][HD_ROWS * HD_PA];
  __shared__ __attribute__((aligned(16))) float wl[HD_RED * HD_PW];
  const int t = threadIdx.x, r = t >> 4, c4 = t & 15;
  const int64_t r0 = (int64_t)blockIdx.x * HD_ROWS, row = r0 + r;
  hd_fill(buf[0], a.x, nullptr, r0, a.G, a.sizes[0]);
  for (int l = 0; l < a.L; ++l) {
    const float* cur = buf[l & 1];
    float* nxt = buf[(l + 1) & 1];
    const int K = a.sizes[l], N = a.sizes[l + 1];
    const bool hidden = l + 1 < a.L;
    for (int c0 = 0; c0 < N; c0 += HD_COLS) {
      const f4 acc = hd_tile_mm<true>(cur, a.W[l], K, K, N, c0, wl);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = c0 + 4 * c4 + j;
        if (col >= N) {
          if (hidden && col < ((N + 3) & ~3)) nxt[r * HD_PA + col] = 0.f;   // the zeros hd_tile_mm reads past N
          continue;
        }
        float v = acc[j] + a.b[l][col];
        if (hidden) {
          const double rstd = 1.0 / sqrt((double)a.running_var[l][col] + a.eps[l]);
          const double g = a.gamma[l] != nullptr ? (double)a.gamma[l][col] : 1.0;
          const double be = a.beta[l] != nullptr ? (double)a.beta[l][col] : 0.0;
          const float pre = hd_pre(v, (float)(g * rstd), (float)(be - (double)a.running_mean[l][col] * g * rstd));
          nxt[r * HD_PA + col] = pre > 0.f ? pre : 0.f;
        } else if (row < a.G) {
          a.out[row * N + col] = v;
        }
      }
    }
  }
}

struct HdRows {
  int64_t G;
  int N, Kin;               // dz [G][N], W [N][Kin]
  int top, loss_kind;
  const float* out;         // top with a loss: the forward's out, y, {loss, count}, the scalar grad_loss
  const float* y;
  const float* loss2;
  const float* grad;        // top: grad_loss (a loss) or the caller's d out [G][N] (none)
  float* dz;                // [G][N]: written (the top layer: only with a loss)
  const float* g;           // below the top: g_l [G][N] of the pass above, z_l and coef_l [5][N]
  const float* z;
  const float* coef;
  const float* W;
  int lower;                // 0: nothing below, 1: d x, 2: a hidden layer
  float* dx;                // [G][Kin]
  const float* z_lo;        // lower == 2: z, affine, stats, gamma of the layer below; g_lo [G][Kin] receives g
  const float* affine_lo;
  float* g_lo;
  double* partials;
  int* sync;
  const double* stats_lo;
  const float* gamma_lo;
  float* coef_lo;
};

__global__ void __launch_bounds__(HD_THREADS) hd_backward_rows_kernel(HdRows a) {
  __shared__ __attribute__((aligned(16))) float al[HD_ROWS * HD_PA];
  __shared__ __attribute__((aligned(16))) float wl[HD_RED * HD_PW];
  __shared__ double red[2][HD_LANES][HD_GCOLS + 1];
  const int t = threadIdx.x, r = t >> 4, c4 = t & 15;
  const int64_t r0 = (int64_t)blockIdx.x * HD_ROWS, row = r0 + r;
  const int np = (a.N + 3) & ~3;
  double sc = 0.0;
  if (a.top && a.loss_kind != EGC_HEAD_LOSS_NONE) sc = hd_loss_scale(a.loss_kind, a.grad, a.loss2, (double)a.G * (double)a.N);
  for (int idx = t; idx < HD_ROWS * np; idx += HD_THREADS) {
    const int rr = idx / np, c = idx - rr * np;
    float v = 0.f;
    if (r0 + rr < a.G && c < a.N) {
      const int64_t at = (r0 + rr) * a.N + c;
      if (a.top) {
        if (a.loss_kind == EGC_HEAD_LOSS_NONE) {
          v = a.grad[at];
        } else {
          v = hd_loss_grad(a.loss_kind, a.out[at], a.y[at], sc);
          a.dz[at] = v;
        }
      } else {
        v = __fadd_rn(__fadd_rn(__fmul_rn(a.coef[2 * a.N + c], a.g[at]), __fmul_rn(a.coef[3 * a.N + c], a.z[at])), a.coef[4 * a.N + c]);
        a.dz[at] = v;
      }
    }
    al[rr * HD_PA + c] = v;
  }
  if (a.lower == 0) return;
  for (int c0 = 0; c0 < a.Kin; c0 += HD_COLS) {
    const f4 acc = hd_tile_mm<false>(al, a.W, a.Kin, a.N, a.Kin, c0, wl);
    if (a.lower == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = c0 + 4 * c4 + j;
        if (row < a.G && col < a.Kin) a.dx[row * a.Kin + col] = acc[j];
      }
      continue;
    }
    f4 g = f4{0.f, 0.f, 0.f, 0.f}, zz = g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + 4 * c4 + j;
      if (row < a.G && col < a.Kin) {
        zz[j] = a.z_lo[row * a.Kin + col];
        g[j] = hd_pre(zz[j], a.affine_lo[col], a.affine_lo[a.Kin + col]) > 0.f ? acc[j] : 0.f;
        a.g_lo[row * a.Kin + col] = g[j];
      }
    }
    __syncthreads();   // the last chunk's reads of wl are done
    *reinterpret_cast<f4*>(wl + r * HD_PW + 4 * c4) = g;
    *reinterpret_cast<f4*>(wl + (HD_ROWS + r) * HD_PW + 4 * c4) = zz;
    __syncthreads();
    hd_block_moments(wl, wl + HD_ROWS * HD_PW, c0, a.Kin, (int)blockIdx.x, a.partials);
  }
  if (a.lower != 2) return;
  if (!arrive_last(a.sync, (int)gridDim.x)) return;
  for (int cbase = 0; cbase < a.Kin; cbase += HD_GCOLS) {
    double t1, t2;
    hd_col_totals(a.partials, (int)gridDim.x, a.Kin, cbase, red, t1, t2);
    if (t < HD_GCOLS && cbase + t < a.Kin)
      bn_backward_column(t1, t2, cbase + t, a.Kin, (double)a.G, a.stats_lo, a.gamma_lo, a.coef_lo, nullptr);
  }
}

struct HdParams {
  int64_t G;
  int L;
  int tile_end[EGC_HEAD_MAX_LINEARS];   // running count of 16 x 16 tiles through layer l
  int N[EGC_HEAD_MAX_LINEARS], K[EGC_HEAD_MAX_LINEARS];
  const float* dz[EGC_HEAD_MAX_LINEARS];       // [G][N]
  const float* in[EGC_HEAD_MAX_LINEARS];       // [G][K]: x or z of the layer below
  const float* in_affine[EGC_HEAD_MAX_LINEARS];
  float* dW[EGC_HEAD_MAX_LINEARS];
  float* db[EGC_HEAD_MAX_LINEARS];
};

__global__ void __launch_bounds__(HD_THREADS) hd_param_grad_kernel(HdParams a) {
  __shared__ float dzl[HD_PCHUNK * HD_PT];
  __shared__ float inl[HD_PCHUNK * HD_PT];
  int l = 0;
  while (l + 1 < a.L && (int)blockIdx.x >= a.tile_end[l]) ++l;
  const int tb = (int)blockIdx.x - (l > 0 ? a.tile_end[l - 1] : 0);
  const int N = a.N[l], K = a.K[l], nkt = (K + HD_PT - 1) / HD_PT;
  const int n0 = HD_PT * (tb / nkt), k0 = HD_PT * (tb % nkt);
  const float* __restrict__ dz = a.dz[l];
  const float* __restrict__ in = a.in[l];
  const float* __restrict__ aff = a.in_affine[l];
  const int t = threadIdx.x, hi = t >> 4, lo = t & 15;   // staging: row hi + 16 i, column lo; product: n = hi, k = lo
  const bool nok = n0 + lo < N, kok = k0 + lo < K;
  float sc = 1.f, sh = 0.f;
  if (aff != nullptr && kok) {
    sc = aff[k0 + lo];
    sh = aff[K + k0 + lo];
  }
  constexpr int PER = HD_PCHUNK / 16;
  float dv[PER], av[PER];
  auto load = [&](int64_t base) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t row = base + hi + 16 * i;
      dv[i] = (row < a.G && nok) ? dz[row * N + n0 + lo] : 0.f;
      float v = (row < a.G && kok) ? in[row * K + k0 + lo] : 0.f;
      if (aff != nullptr) {
        const float pre = hd_pre(v, sc, sh);
        v = (row < a.G && kok && pre > 0.f) ? pre : 0.f;
      }
      av[i] = v;
    }
  };
  float acc = 0.f, accb = 0.f;
  load(0);
  for (int64_t base = 0; base < a.G; base += HD_PCHUNK) {
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      dzl[(hi + 16 * i) * HD_PT + lo] = dv[i];
      inl[(hi + 16 * i) * HD_PT + lo] = av[i];
    }
    __syncthreads();
    if (base + HD_PCHUNK < a.G) load(base + HD_PCHUNK);
    const int rows = (int)min((int64_t)HD_PCHUNK, a.G - base);
    int rr = 0;
    for (; rr + 8 <= rows; rr += 8) {   // eight rows' LDS reads ahead of the one chain
      float d[8], v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        d[u] = dzl[(rr + u) * HD_PT + hi];
        v[u] = inl[(rr + u) * HD_PT + lo];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc = __builtin_fmaf(d[u], v[u], acc);
        accb += d[u];
      }
    }
    for (; rr < rows; ++rr) {
      const float d = dzl[rr * HD_PT + hi];
      acc = __builtin_fmaf(d, inl[rr * HD_PT + lo], acc);
      accb += d;
    }
  }
  if (n0 + hi < N && k0 + lo < K) a.dW[l][(int64_t)(n0 + hi) * K + k0 + lo] = acc;
  if (k0 == 0 && lo == 0 && n0 + hi < N && a.db[l] != nullptr) a.db[l][n0 + hi] = accb;
}

// the stand-alone losses: one block
__global__ void __launch_bounds__(HD_THREADS) hd_loss_forward_kernel(const float* __restrict__ out, const float* __restrict__ y,
                                                                     int64_t n, int kind, float* __restrict__ loss2) {
  __shared__ double ss[HD_THREADS], cs[HD_THREADS];
  double s = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += HD_THREADS) {
    double term, cnt;
    hd_loss_term(kind, out[i], y[i], term, cnt);
    s += term;
    c += cnt;
  }
  ss[threadIdx.x] = s;
  cs[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = c = 0.0;
    for (int k = 0; k < HD_THREADS; ++k) {
      s += ss[k];
      c += cs[k];
    }
    loss2[0] = (float)(s / c);
    loss2[1] = (float)c;
  }
}

__global__ void __launch_bounds__(HD_THREADS) hd_loss_backward_kernel(const float* __restrict__ out, const float* __restrict__ y,
                                                                      const float* __restrict__ grad_loss,
                                                                      const float* __restrict__ loss2, int64_t n, int kind,
                                                                      float* __restrict__ d_out) {
  const int64_t i = (int64_t)blockIdx.x * HD_THREADS + threadIdx.x;
  if (i >= n) return;
  d_out[i] = hd_loss_grad(kind, out[i], y[i], hd_loss_scale(kind, grad_loss, loss2, (double)n));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int hd_check(const egc_head* h, int64_t G) {
  if (h == nullptr || G < 0 || h->n_linears < 1) return EGC_ERR_INVALID;
  if (h->n_linears > EGC_HEAD_MAX_LINEARS) return EGC_ERR_UNSUPPORTED;
  const int L = h->n_linears;
  for (int i = 0; i <= L; ++i)
    if (h->sizes[i] < 1) return EGC_ERR_INVALID;
  for (int i = 0; i < L; ++i)
    if (h->sizes[i] > EGC_HEAD_MAX_WIDTH) return EGC_ERR_UNSUPPORTED;
  if (h->sizes[L] > EGC_HEAD_MAX_OUT || G > EGC_HEAD_MAX_ROWS) return EGC_ERR_UNSUPPORTED;
  for (int i = 0; i < L; ++i)
    if (h->weight[i] == nullptr || h->bias[i] == nullptr) return EGC_ERR_INVALID;
  for (int i = 0; i + 1 < L; ++i)
    if ((h->running_mean[i] == nullptr) != (h->running_var[i] == nullptr)) return EGC_ERR_INVALID;
  return EGC_OK;
}

int64_t hd_row_blocks(int64_t G) { return ceil_div(G, (int64_t)HD_ROWS); }

size_t hd_workspace_bytes(const egc_head* h, int64_t G) {
  int widest = 1;
  for (int i = 1; i < h->n_linears; ++i) widest = h->sizes[i] > widest ? h->sizes[i] : widest;
  const int64_t nb = hd_row_blocks(G) > 0 ? hd_row_blocks(G) : 1;
  return (size_t)nb * 2 * ((size_t)widest + 1) * sizeof(double);   // column partials, then the loss partials
}

int hd_loss_kind_ok(int32_t kind) {
  return kind == EGC_HEAD_LOSS_NONE || kind == EGC_HEAD_LOSS_L1 || kind == EGC_HEAD_LOSS_BCE_MASKED;
}

int hd_loss_forward(const float* out, const float* y, int64_t n, int kind, float* loss2, egc_stream_t stream_) {
  if (n < 0 || loss2 == nullptr || (n > 0 && (out == nullptr || y == nullptr))) return EGC_ERR_INVALID;
  if (n > (int64_t)EGC_HEAD_MAX_ROWS * EGC_HEAD_MAX_OUT) return EGC_ERR_UNSUPPORTED;
  hd_loss_forward_kernel<<<1, HD_THREADS, 0, (hipStream_t)stream_>>>(out, y, n, kind, loss2);
  EGC_LAUNCH_CHECK("hd_loss_forward_kernel");
  launched();
  return EGC_OK;
}

int hd_loss_backward(const float* out, const float* y, const float* grad_loss, const float* loss2, int64_t n, int kind,
                     float* d_out, egc_stream_t stream_) {
  if (n < 0 || grad_loss == nullptr || loss2 == nullptr || (n > 0 && (out == nullptr || y == nullptr || d_out == nullptr)))
    return EGC_ERR_INVALID;
  if (n > (int64_t)EGC_HEAD_MAX_ROWS * EGC_HEAD_MAX_OUT) return EGC_ERR_UNSUPPORTED;
  if (n == 0) return EGC_OK;
  hd_loss_backward_kernel<<<(unsigned)ceil_div(n, (int64_t)HD_THREADS), HD_THREADS, 0, (hipStream_t)stream_>>>(
      out, y, grad_loss, loss2, n, kind, d_out);
  EGC_LAUNCH_CHECK("hd_loss_backward_kernel");
  launched();
  return EGC_OK;
}

}  // namespace
}  // namespace egc

using namespace egc;

int64_t egc_head_launches(void) { return g_head_launches.load(std::memory_order_relaxed); }

size_t egc_head_workspace_bytes(const egc_head* head, int64_t n_rows) {
  if (hd_check(head, n_rows) != EGC_OK) return 0;
  return hd_workspace_bytes(head, n_rows);
}

int egc_head_forward_train_f32(const egc_head* h, const float* x, int64_t n_rows, int32_t loss_kind, const float* y, float* out,
                               float* loss2, void* workspace, size_t workspace_bytes, int32_t* sync, egc_stream_t stream_) {
  if (int rc = hd_check(h, n_rows)) return rc;
  const int L = h->n_linears;
  if (!hd_loss_kind_ok(loss_kind) || x == nullptr || out == nullptr || sync == nullptr) return EGC_ERR_INVALID;
  if (loss_kind != EGC_HEAD_LOSS_NONE && (y == nullptr || loss2 == nullptr)) return EGC_ERR_INVALID;
  if (n_rows < 1 || (L > 1 && n_rows < 2)) return EGC_ERR_INVALID;   // (nn.BatchNorm1d raises on one row in training mode)
  for (int i = 0; i + 1 < L; ++i) {
    if (h->z[i] == nullptr || h->stats[i] == nullptr || h->affine[i] == nullptr) return EGC_ERR_INVALID;
    if (h->running_mean[i] != nullptr && h->momentum[i] < 0.0 && h->num_batches_tracked[i] == nullptr) return EGC_ERR_INVALID;
  }
  if (workspace == nullptr || !aligned_to(workspace, 8) || workspace_bytes < hd_workspace_bytes(h, n_rows))
    return EGC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nb = hd_row_blocks(n_rows);
  double* partials = static_cast<double*>(workspace);
  for (int l = 0; l < L; ++l) {
    HdLinear a = HdLinear();
    a.in = l == 0 ? x : h->z[l - 1];
    a.in_affine = l == 0 ? nullptr : h->affine[l - 1];
    a.W = h->weight[l];
    a.b = h->bias[l];
    a.G = n_rows;
    a.K = h->sizes[l];
    a.N = h->sizes[l + 1];
    a.hidden = l + 1 < L;
    a.sync = sync;
    if (a.hidden) {
      a.z = h->z[l];
      a.partials = partials;
      a.gamma = h->gamma[l];
      a.beta = h->beta[l];
      a.eps = h->eps[l];
      a.momentum = h->momentum[l];
      a.stats = h->stats[l];
      a.affine = h->affine[l];
      a.running_mean = h->running_mean[l];
      a.running_var = h->running_var[l];
      a.n_tracked = h->num_batches_tracked[l];
    } else {
      a.z = out;
      a.loss_kind = loss_kind;
      a.y = y;
      a.loss2 = loss2;
      a.lpart = partials;
    }
    hd_linear_kernel<<<dim3((unsigned)nb, (unsigned)ceil_div(a.N, HD_COLS)), HD_THREADS, 0, stream>>>(a);
    EGC_LAUNCH_CHECK("hd_linear_kernel");
    launched();
  }
  return EGC_OK;
}

int egc_head_forward_eval_f32(const egc_head* h, const float* x, int64_t n_rows, float* out, egc_stream_t stream_) {
  if (int rc = hd_check(h, n_rows)) return rc;
  const int L = h->n_linears;
  for (int i = 0; i + 1 < L; ++i)
    if (h->running_mean[i] == nullptr) return EGC_ERR_INVALID;
  if (n_rows == 0) return EGC_OK;
  if (x == nullptr || out == nullptr) return EGC_ERR_INVALID;
  HdEval a = HdEval();
  a.x = x;
  a.out = out;
  a.G = n_rows;
  a.L = L;
  for (int i = 0; i <= L; ++i) a.sizes[i] = h->sizes[i];
  for (int i = 0; i < L; ++i) {
    a.W[i] = h->weight[i];
    a.b[i] = h->bias[i];
  }
  for (int i = 0; i + 1 < L; ++i) {
    a.gamma[i] = h->gamma[i];
    a.beta[i] = h->beta[i];
    a.running_mean[i] = h->running_mean[i];
    a.running_var[i] = h->running_var[i];
    a.eps[i] = h->eps[i];
  }
  hd_eval_kernel<<<(unsigned)hd_row_blocks(n_rows), HD_THREADS, 0, (hipStream_t)stream_>>>(a);
  EGC_LAUNCH_CHECK("hd_eval_kernel");
  launched();
  return EGC_OK;
}

int egc_head_backward_f32(const egc_head* h, const float* x, int64_t n_rows, int32_t loss_kind, const float* y, const float* out,
                          const float* loss2, const float* grad, float* d_x, int32_t want_params, void* workspace,
                          size_t workspace_bytes, int32_t* sync, egc_stream_t stream_) {
  if (int rc = hd_check(h, n_rows)) return rc;
  const int L = h->n_linears;
  if (!hd_loss_kind_ok(loss_kind) || x == nullptr || grad == nullptr || sync == nullptr) return EGC_ERR_INVALID;
  if (loss_kind != EGC_HEAD_LOSS_NONE && (y == nullptr || out == nullptr || loss2 == nullptr || h->dz[L - 1] == nullptr))
    return EGC_ERR_INVALID;
  if (n_rows < 1 || (L > 1 && n_rows < 2)) return EGC_ERR_INVALID;
  for (int i = 0; i + 1 < L; ++i)
    if (h->z[i] == nullptr || h->stats[i] == nullptr || h->affine[i] == nullptr || h->dz[i] == nullptr || h->g[i] == nullptr ||
        h->coef[i] == nullptr)
      return EGC_ERR_INVALID;
  if (want_params)
    for (int i = 0; i < L; ++i)
      if (h->d_weight[i] == nullptr || h->d_bias[i] == nullptr) return EGC_ERR_INVALID;
  if (workspace == nullptr || !aligned_to(workspace, 8) || workspace_bytes < hd_workspace_bytes(h, n_rows))
    return EGC_ERR_WORKSPACE;
  if (d_x == nullptr && !want_params) return EGC_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nb = hd_row_blocks(n_rows);
  const float* dz_top = loss_kind == EGC_HEAD_LOSS_NONE ? grad : h->dz[L - 1];
  for (int l = L - 1; l >= 0; --l) {
    HdRows a = HdRows();
    a.G = n_rows;
    a.N = h->sizes[l + 1];
    a.Kin = h->sizes[l];
    a.top = l == L - 1;
    a.loss_kind = loss_kind;
    a.out = out;
    a.y = y;
    a.loss2 = loss2;
    a.grad = grad;
    a.dz = h->dz[l];
    a.W = h->weight[l];
    if (!a.top) {
      a.g = h->g[l];
      a.z = h->z[l];
      a.coef = h->coef[l];
    }
    if (l == 0) {
      a.lower = d_x != nullptr ? 1 : 0;
      a.dx = d_x;
    } else {
      a.lower = 2;
      a.z_lo = h->z[l - 1];
      a.affine_lo = h->affine[l - 1];
      a.g_lo = h->g[l - 1];
      a.partials = static_cast<double*>(workspace);
      a.sync = sync;
      a.stats_lo = h->stats[l - 1];
      a.gamma_lo = h->gamma[l - 1];
      a.coef_lo = h->coef[l - 1];
    }
    if (a.lower == 0 && a.top && loss_kind == EGC_HEAD_LOSS_NONE) continue;   // nothing to form: dz is the caller's gradient
    hd_backward_rows_kernel<<<(unsigned)nb, HD_THREADS, 0, stream>>>(a);
    EGC_LAUNCH_CHECK("hd_backward_rows_kernel");
    launched();
  }
  if (want_params) {
    HdParams p = HdParams();
    p.G = n_rows;
    p.L = L;
    int tiles = 0;
    for (int l = 0; l < L; ++l) {
      p.N[l] = h->sizes[l + 1];
      p.K[l] = h->sizes[l];
      tiles += ceil_div(p.N[l], HD_PT) * ceil_div(p.K[l], HD_PT);
      p.tile_end[l] = tiles;
      p.dz[l] = l == L - 1 ? dz_top : h->dz[l];
      p.in[l] = l == 0 ? x : h->z[l - 1];
      p.in_affine[l] = l == 0 ? nullptr : h->affine[l - 1];
      p.dW[l] = h->d_weight[l];
      p.db[l] = h->d_bias[l];
    }
    hd_param_grad_kernel<<<(unsigned)tiles, HD_THREADS, 0, stream>>>(p);
    EGC_LAUNCH_CHECK("hd_param_grad_kernel");
    launched();
  }
  return EGC_OK;
}

int egc_l1_loss_forward_f32(const float* out, const float* y, int64_t n, float* loss2, egc_stream_t stream) {
  return hd_loss_forward(out, y, n, EGC_HEAD_LOSS_L1, loss2, stream);
}

int egc_l1_loss_backward_f32(const float* out, const float* y, const float* grad_loss, const float* loss2, int64_t n, float* d_out,
                             egc_stream_t stream) {
  return hd_loss_backward(out, y, grad_loss, loss2, n, EGC_HEAD_LOSS_L1, d_out, stream);
}

int egc_bce_masked_forward_f32(const float* out, const float* y, int64_t n, float* loss2, egc_stream_t stream) {
  return hd_loss_forward(out, y, n, EGC_HEAD_LOSS_BCE_MASKED, loss2, stream);
}

int egc_bce_masked_backward_f32(const float* out, const float* y, const float* grad_loss, const float* loss2, int64_t n,
                                float* d_out, egc_stream_t stream) {
  return hd_loss_backward(out, y, grad_loss, loss2, n, EGC_HEAD_LOSS_BCE_MASKED, d_out, stream);
}
