// Multi-aggregator neighbourhood aggregation of PNAConv (PyG 2.x, edge_dim = None, pre_layers = post_layers = 1) without its
// [E, 2 F] endpoint features, its [E, T F] messages, its four scatter passes and its [N, T, 12 F] scaled concatenation.  A tower's
// pre-transform acts on [x_i | x_j], so it splits as Mpnn's message Linear does (egc_mpnn.hip): with P = x Ms^T and
// Q = x Md^T + b_pre (two dense [N, W] arrays) the message of entry j -> i is h = P_j + Q_i, and over a row's n entries, per column,
//
//   SUM   S0 + float(n) * Q_i           S0 = sum of P[col]
//   MEAN  S0 / float(n) + Q_i
//   MIN   (min of P[col]) + Q_i         arg = the FIRST entry attaining it (strict <)
//   MAX   (max of P[col]) + Q_i         arg = the FIRST entry attaining it (strict >)
//   VAR   v = max(S2 / n - m1 * m1, 0)  s = P[col[first entry of the row]], S1 = sum of (P[col] - s), S2 = sum of (P[col] - s)^2,
//   STD   sqrt(v + 1e-5)                m1 = S1 / n; saved for the backward: mu = s + m1 and v
//
// and 0 (arg -1; STD sqrt(1e-5)) for a row without entries: Q_i is not added there.  The variance is the one of P alone (h differs
// from it by the row constant Q_i) about the row's first entry -- the EGC std aggregator's policy, not E[h^2] - E[h]^2 in float32.
// gfx950 only.  ONE gather pass over P whatever the list: a lane carries S0 (SUM / MEAN listed), S1 and S2 and the shift (VAR /
// STD listed), the running min and max with their positions (MIN / MAX listed) -- the kernels are instantiated per combination, so
// a list without VAR / STD loads no shift and one without MIN / MAX carries no positions.  SUM and MEAN come from the unshifted
// S0 so that their bits do not depend on what else is listed.
//
// Order rule: egc_row_chunks.h.  Inside a chunk every accumulator starts at 0 (+inf / -inf, position = the chunk's first entry)
// and takes the entries in order -- S0 = S0 + v;  d = v - s, S1 = S1 + d, S2 = S2 + d * d;  v < min, v > max strict -- and the
// row's value is chunk 0's with chunks 1, 2, ... merged in ascending order: plain addition for S0, S1, S2 (the shift s is the
// row's in every chunk), a strict compare for min / max, so the first chunk keeps a tie (a NaN is never selected).  Then, each
// one IEEE operation (-ffp-contract=off):  nf = float(n);  SUM = S0 + nf * q;  MEAN = S0 / nf + q;  MIN = mn + q;  MAX = mx + q;
// m1 = S1 / nf;  t = S2 / nf - m1 * m1;  v = t > 0 ? t : 0;  STD = sqrt(v + 1e-5f);  mu = s + m1.
//
// Backward, two launches after the chunk launch, no atomics, every element written once:
//   destination pass (one read of the row's gradients and saved statistics), nf = float(n), rows without entries give zeros:
//     d Q_i = ((nf * g_sum + g_mean) + g_min) + g_max                       (absent terms skipped, the accumulator starts at 0)
//     lin = g_sum + g_mean / nf;   c = g_var + g_std / (2 * sqrt(v_i + 1e-5f));   b_i = (2 * c) / nf;   a_i = lin - b_i * mu_i
//     (c = 0 in the columns whose saved variance v_i is exactly 0 -- a one-entry row, a row of equal entries: d v / d P_j =
//     2 (P_j - mu) / n is 0 there and PyG's relu'(0) = 0 says the same, while the two records would cancel b mu against P_j b at
//     1 / (2 sqrt(1e-5)) = 158 times the rounding error of either)
//   source pass over the TRANSPOSED CSR, entries in ascending forward position, chunked as above, four plain sums per column:
//     A = sum a_i,  B = sum b_i,  Mn = sum of g_min[i] where arg_min[i] names this edge (else 0),  Mx likewise, and
//     d P_j = ((A + P_j * B) + Mn) + Mx                                      (absent terms skipped; 0 for a row without entries)
//   since d v / d P_j = 2 (P_j - mu) / n, the var / std / mean / sum part of d P_j is sum_i a_i + P_j * sum_i b_i.
// The records a and b live in the caller's workspace, in front of the chunk partials.
//
// Mapping: egc_row_chunks.h, a batch is PN_AHEAD entries; edge positions are clamped to the entry count like row offsets.
//
// The scaler combine at the end of the file: out_i = base_i + sum_k f_k(d_i) Y_i[k D : (k + 1) D], d_i = max(n_i, 1), the factors
// formed per row in double and rounded once to float.
#include "egc_row_chunks.h"

namespace egc {

constexpr int PN_AHEAD = 8;
constexpr int PN_OPS = 6;

struct PnWalk {
  const int32_t* rowptr;   // the CSR walked: n_rows + 1 offsets
  const int32_t* col;      // n_edges entries: rows of `in`
  const float* in;         // forward: P, n_in_rows rows of ld_in floats
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_in, width, lanes;
};

struct PnAcc {
  f4 s0, s1, s2, mn, mx;
  i4 pmn, pmx;
};

// field f of slot g: [fields][slots][lanes] 16-byte pieces
__device__ inline float* pn_ws(float* ws, int f, int64_t slots, int64_t g, int lanes, int c) {
  return ws + (((int64_t)f * slots + g) * lanes) * 4 + c;
}

// ---------------------------------------------------------------------------------------------------------------- forward

// PN_AHEAD consecutive entries from p on (FULL: all of them exist; else those before p1, the others load entry p1 - 1 again and
// are not taken) folded into the accumulators in entry order
template <bool VEC, bool SUM, bool MOM2, bool EXT, bool FULL>
__device__ inline void pn_take_batch(PnAcc& A, const PnWalk& W, f4 shift, int64_t p, int64_t p1, int c) {
  constexpr int N = FULL ? PN_AHEAD : PN_AHEAD - 1;
  const int last_in = (int)W.n_in_rows - 1;
  int j[N];
  batch_rows<N, FULL>(j, W.col, p, p1, last_in);
  f4 v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = tm_load<VEC>(W.in + (int64_t)j[k] * W.ld_in + c, c, W.width);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const bool live = FULL || p + k < p1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = v[k][i];
      if (SUM) A.s0[i] = live ? A.s0[i] + x : A.s0[i];
      if (MOM2) {
        const float d = x - shift[i];
        A.s1[i] = live ? A.s1[i] + d : A.s1[i];
        A.s2[i] = live ? A.s2[i] + d * d : A.s2[i];
      }
      if (EXT) {
        const bool lt = live && x < A.mn[i], gt = live && x > A.mx[i];
        A.mn[i] = lt ? x : A.mn[i];
        A.pmn[i] = lt ? (int)(p + k) : A.pmn[i];
        A.mx[i] = gt ? x : A.mx[i];
        A.pmx[i] = gt ? (int)(p + k) : A.pmx[i];
      }
    }
  }
}

// the entries [p0, p1), p0 < p1, in order, from fresh accumulators
template <bool VEC, bool SUM, bool MOM2, bool EXT>
__device__ inline void pn_reduce_entries(PnAcc& A, const PnWalk& W, f4 shift, int64_t p0, int64_t p1, int c) {
  const float inf = __builtin_inff();
  A.s0 = A.s1 = A.s2 = f4{0.f, 0.f, 0.f, 0.f};
  A.mn = f4{inf, inf, inf, inf};
  A.mx = f4{-inf, -inf, -inf, -inf};
  A.pmn = A.pmx = i4{(int)p0, (int)p0, (int)p0, (int)p0};
  int64_t p = p0;
#pragma unroll 1
  for (; p + PN_AHEAD <= p1; p += PN_AHEAD) pn_take_batch<VEC, SUM, MOM2, EXT, true>(A, W, shift, p, p1, c);
  if (p < p1) pn_take_batch<VEC, SUM, MOM2, EXT, false>(A, W, shift, p, p1, c);
}

// the row's shift: its first entry's row of P
template <bool VEC>
__device__ inline f4 pn_shift(const PnWalk& W, int64_t p0, int c) {
  const int j = clamp_index(W.col[p0], (int)W.n_in_rows - 1);
  return tm_load<VEC>(W.in + (int64_t)j * W.ld_in + c, c, W.width);
}

// workspace fields in this order, those instantiated only: S0 | S1 S2 | min max pos_min pos_max
template <bool SUM, bool MOM2, bool EXT>
struct PnFields {
  static constexpr int s0 = 0, s1 = SUM ? 1 : 0, s2 = s1 + 1, mn = s1 + (MOM2 ? 2 : 0), mx = mn + 1, pmn = mn + 2, pmx = mn + 3;
  static constexpr int count = (SUM ? 1 : 0) + (MOM2 ? 2 : 0) + (EXT ? 4 : 0);
};

template <bool VEC, bool SUM, bool MOM2, bool EXT>
__global__ void __launch_bounds__(256) pna_chunks_kernel(const PnWalk W, int64_t slots, float* __restrict__ ws) {
  typedef PnFields<SUM, MOM2, EXT> F;
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  f4 shift = f4{0.f, 0.f, 0.f, 0.f};
  if (MOM2) {
    int64_t p0, p1;
    row_range(W.rowptr, W.n_edges, row, p0, p1);
    shift = pn_shift<VEC>(W, p0, c);
  }
  PnAcc A;
  pn_reduce_entries<VEC, SUM, MOM2, EXT>(A, W, shift, s0, s1, c);
  if (SUM) *reinterpret_cast<f4*>(pn_ws(ws, F::s0, slots, g, W.lanes, c)) = A.s0;
  if (MOM2) {
    *reinterpret_cast<f4*>(pn_ws(ws, F::s1, slots, g, W.lanes, c)) = A.s1;
    *reinterpret_cast<f4*>(pn_ws(ws, F::s2, slots, g, W.lanes, c)) = A.s2;
  }
  if (EXT) {
    *reinterpret_cast<f4*>(pn_ws(ws, F::mn, slots, g, W.lanes, c)) = A.mn;
    *reinterpret_cast<f4*>(pn_ws(ws, F::mx, slots, g, W.lanes, c)) = A.mx;
    *reinterpret_cast<i4*>(pn_ws(ws, F::pmn, slots, g, W.lanes, c)) = A.pmn;
    *reinterpret_cast<i4*>(pn_ws(ws, F::pmx, slots, g, W.lanes, c)) = A.pmx;
  }
}

struct PnOut {
  const float* Q;
  float* out;
  float* mu;               // NULL, or dense [n_rows, width]
  float* var;              // NULL, or dense [n_rows, width]
  int32_t* arg_min;        // NULL, or dense [n_rows, width]
  int32_t* arg_max;
  const int32_t* edge_id;  // NULL: the position
  int32_t ld_q, ld_out;
  int32_t blk[PN_OPS];     // the output block of EGC_PNA_SUM .. EGC_PNA_STD, -1: not listed
};

template <bool VEC, bool SUM, bool MOM2, bool EXT>
__global__ void __launch_bounds__(256) pna_aggregate_rows_kernel(const PnWalk W, const PnOut O, int64_t slots,
                                                                 float* __restrict__ ws) {
  typedef PnFields<SUM, MOM2, EXT> F;
  int64_t row, p0, p1;
  int c;
  group_lane(W.lanes, row, c);
  if (row >= W.n_rows) return;
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  f4 r[PN_OPS] = {zero, zero, zero, zero, zero, zero};
  f4 mu = zero;
  i4 emn = i4{-1, -1, -1, -1}, emx = emn;
  if (p1 > p0) {
    const f4 q = tm_load<VEC>(O.Q + row * O.ld_q + c, c, W.width);
    f4 shift = zero;
    if (MOM2) shift = pn_shift<VEC>(W, p0, c);
    PnAcc A;
    pn_reduce_entries<VEC, SUM, MOM2, EXT>(A, W, shift, p0, min(p0 + ROW_CHUNK, p1), c);
    if (p1 - p0 > ROW_CHUNK) {   // (n_part is 0 otherwise: the test only spares the short rows the division)
      int64_t first, n_part;
      row_partials(p0, p1, first, n_part);
#pragma unroll 2
      for (int64_t k = 0; k < n_part; ++k) {
        const int64_t g = first + k;
        if (SUM) A.s0 += *reinterpret_cast<const f4*>(pn_ws(ws, F::s0, slots, g, W.lanes, c));
        if (MOM2) {
          A.s1 += *reinterpret_cast<const f4*>(pn_ws(ws, F::s1, slots, g, W.lanes, c));
          A.s2 += *reinterpret_cast<const f4*>(pn_ws(ws, F::s2, slots, g, W.lanes, c));
        }
        if (EXT) {
          const f4 vn = *reinterpret_cast<const f4*>(pn_ws(ws, F::mn, slots, g, W.lanes, c));
          const f4 vx = *reinterpret_cast<const f4*>(pn_ws(ws, F::mx, slots, g, W.lanes, c));
          const i4 qn = *reinterpret_cast<const i4*>(pn_ws(ws, F::pmn, slots, g, W.lanes, c));
          const i4 qx = *reinterpret_cast<const i4*>(pn_ws(ws, F::pmx, slots, g, W.lanes, c));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool lt = vn[i] < A.mn[i], gt = vx[i] > A.mx[i];
            A.mn[i] = lt ? vn[i] : A.mn[i];
            A.pmn[i] = lt ? qn[i] : A.pmn[i];
            A.mx[i] = gt ? vx[i] : A.mx[i];
            A.pmx[i] = gt ? qx[i] : A.pmx[i];
          }
        }
      }
    }
    const float nf = (float)(p1 - p0);
    if (SUM) {
      r[EGC_PNA_SUM] = A.s0 + nf * q;
      r[EGC_PNA_MEAN] = A.s0 / nf + q;
    }
    if (EXT) {
      r[EGC_PNA_MIN] = A.mn + q;
      r[EGC_PNA_MAX] = A.mx + q;
      const int last_e = (int)W.n_edges - 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = min(max(A.pmn[i], 0), last_e), b = min(max(A.pmx[i], 0), last_e);
        emn[i] = O.edge_id != nullptr && O.arg_min != nullptr ? O.edge_id[a] : a;
        emx[i] = O.edge_id != nullptr && O.arg_max != nullptr ? O.edge_id[b] : b;
      }
    }
    if (MOM2) {
      const f4 m1 = A.s1 / nf;
      const f4 tt = A.s2 / nf - m1 * m1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = tt[i] > 0.f ? tt[i] : 0.f;
        r[EGC_PNA_VAR][i] = v;
        r[EGC_PNA_STD][i] = __builtin_sqrtf(v + 1e-5f);
      }
      mu = shift + m1;
    }
  } else if (MOM2) {
    const float e = __builtin_sqrtf(1e-5f);
    r[EGC_PNA_STD] = f4{e, e, e, e};
  }
#pragma unroll
  for (int op = 0; op < PN_OPS; ++op)
    if (O.blk[op] >= 0) tm_store<VEC>(O.out + row * O.ld_out + (int64_t)O.blk[op] * W.width + c, c, W.width, r[op]);
  if (MOM2 && O.mu != nullptr) tm_store<VEC>(O.mu + row * W.width + c, c, W.width, mu);
  if (MOM2 && O.var != nullptr) tm_store<VEC>(O.var + row * W.width + c, c, W.width, r[EGC_PNA_VAR]);
  if (EXT && O.arg_min != nullptr) tm_store_i<VEC>(O.arg_min + row * W.width + c, c, W.width, emn);
  if (EXT && O.arg_max != nullptr) tm_store_i<VEC>(O.arg_max + row * W.width + c, c, W.width, emx);
}

// --------------------------------------------------------------------------------------------------------------- backward

struct PnGrad {
  const int32_t* rowptr;   // forward rowptr, n_rows + 1
  const float* g;          // d agg, n_rows rows of ld_g floats
  const float* mu;         // dense [n_rows, width] (var / std listed)
  const float* var;        // dense [n_rows, width] (var / std listed): the forward's clamped variance
  float* dQ;               // NULL, or n_rows rows of ld_dq
  float* a;                // NULL, or the records: dense [n_rows, lanes * 4]
  float* b;
  int64_t n_rows, n_edges;
  int32_t ld_g, ld_dq, width, lanes;
  int32_t blk[PN_OPS];
};

template <bool VEC>
__global__ void __launch_bounds__(256) pna_backward_dst_kernel(const PnGrad G) {
  int64_t row, p0, p1;
  int c;
  group_lane(G.lanes, row, c);
  if (row >= G.n_rows) return;
  row_range(G.rowptr, G.n_edges, row, p0, p1);
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  f4 dq = zero, a = zero, b = zero;
  if (p1 > p0) {
    const float nf = (float)(p1 - p0);
    f4 g[PN_OPS];
#pragma unroll
    for (int op = 0; op < PN_OPS; ++op)
      g[op] = G.blk[op] >= 0 ? tm_load<VEC>(G.g + row * G.ld_g + (int64_t)G.blk[op] * G.width + c, c, G.width) : zero;
    if (G.blk[EGC_PNA_SUM] >= 0) {
      dq = dq + nf * g[EGC_PNA_SUM];
      a = a + g[EGC_PNA_SUM];
    }
    if (G.blk[EGC_PNA_MEAN] >= 0) {
      dq = dq + g[EGC_PNA_MEAN];
      a = a + g[EGC_PNA_MEAN] / nf;
    }
    if (G.blk[EGC_PNA_MIN] >= 0) dq = dq + g[EGC_PNA_MIN];
    if (G.blk[EGC_PNA_MAX] >= 0) dq = dq + g[EGC_PNA_MAX];
    if (G.a != nullptr && (G.blk[EGC_PNA_VAR] >= 0 || G.blk[EGC_PNA_STD] >= 0)) {
      const f4 v = tm_load<VEC>(G.var + row * G.width + c, c, G.width);
      f4 cc = zero;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (v[i] > 0.f) {
          if (G.blk[EGC_PNA_VAR] >= 0) cc[i] = cc[i] + g[EGC_PNA_VAR][i];
          if (G.blk[EGC_PNA_STD] >= 0) cc[i] = cc[i] + g[EGC_PNA_STD][i] / (2.f * __builtin_sqrtf(v[i] + 1e-5f));
        }
      }
      b = (2.f * cc) / nf;
      const f4 mu = tm_load<VEC>(G.mu + row * G.width + c, c, G.width);
      a = a - b * mu;
    }
  }
  if (G.dQ != nullptr) tm_store<VEC>(G.dQ + row * G.ld_dq + c, c, G.width, dq);
  if (G.a != nullptr) {   // (the records are padded to whole lanes: always one 16-byte store)
    *reinterpret_cast<f4*>(G.a + (row * G.lanes) * 4 + c) = a;
    if (G.b != nullptr) *reinterpret_cast<f4*>(G.b + (row * G.lanes) * 4 + c) = b;
  }
}

struct PnBack {
  const int32_t* rowptr;   // transposed CSR: n_rows (= sources) + 1 offsets
  const int32_t* col;      // destination of every transposed entry
  const int32_t* eid;      // forward CSR position of every transposed entry (NULL: its own position)
  const int32_t* f_eid;    // edge id of every forward CSR position (NULL: the position)
  const float* a;          // records, dense [n_in_rows, lanes * 4]; NULL: no sum / mean / var / std listed
  const float* b;          // NULL: no var / std listed
  const float* g_min;      // the MIN block of d agg (first column), NULL: not listed
  const float* g_max;
  const int32_t* arg_min;  // dense [n_in_rows, width]
  const int32_t* arg_max;
  const float* P;          // n_rows rows of ld_p (read when b != NULL)
  float* dP;
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_g, ld_p, ld_dp, width, lanes;
};

struct PnBAcc {
  f4 a, b, mn, mx;
};

template <bool VEC, bool MOM2, bool FULL>
__device__ inline void pn_back_batch(PnBAcc& A, const PnBack& W, int64_t p, int64_t p1, int c) {
  constexpr int N = FULL ? PN_AHEAD : PN_AHEAD - 1;
  const int last_in = (int)W.n_in_rows - 1, last_e = (int)W.n_edges - 1;
  const bool ext = W.g_min != nullptr || W.g_max != nullptr;
  int j[N], e[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int64_t q = batch_entry<FULL>(p, k, p1);
    j[k] = clamp_index(W.col[q], last_in);
    e[k] = ext && W.eid != nullptr ? clamp_index(W.eid[q], last_e) : (int)q;
  }
  if (ext && W.f_eid != nullptr) {
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = W.f_eid[e[k]];
  }
  if (W.a != nullptr) {
    f4 va[N], vb[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      va[k] = *reinterpret_cast<const f4*>(W.a + ((int64_t)j[k] * W.lanes) * 4 + c);
      if (MOM2) vb[k] = *reinterpret_cast<const f4*>(W.b + ((int64_t)j[k] * W.lanes) * 4 + c);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool live = FULL || p + k < p1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        A.a[i] = live ? A.a[i] + va[k][i] : A.a[i];
        if (MOM2) A.b[i] = live ? A.b[i] + vb[k][i] : A.b[i];
      }
    }
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float* __restrict__ g = side == 0 ? W.g_min : W.g_max;
    const int32_t* __restrict__ arg = side == 0 ? W.arg_min : W.arg_max;
    if (g == nullptr) continue;
    f4 v[N];
    i4 r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      v[k] = tm_load<VEC>(g + (int64_t)j[k] * W.ld_g + c, c, W.width);
      r[k] = tm_load_i<VEC>(arg + (int64_t)j[k] * W.width + c, c, W.width);
    }
    f4& acc = side == 0 ? A.mn : A.mx;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool live = FULL || p + k < p1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = r[k][i] == e[k] ? v[k][i] : 0.f;
        acc[i] = live ? acc[i] + x : acc[i];
      }
    }
  }
}

template <bool VEC, bool MOM2>
__device__ inline void pn_back_entries(PnBAcc& A, const PnBack& W, int64_t p0, int64_t p1, int c) {
  A.a = A.b = A.mn = A.mx = f4{0.f, 0.f, 0.f, 0.f};
  int64_t p = p0;
#pragma unroll 1
  for (; p + PN_AHEAD <= p1; p += PN_AHEAD) pn_back_batch<VEC, MOM2, true>(A, W, p, p1, c);
  if (p < p1) pn_back_batch<VEC, MOM2, false>(A, W, p, p1, c);
}

// workspace of the source pass: fields A | B | Mn | Mx, [4][slots][lanes] 16-byte pieces
template <bool VEC, bool MOM2>
__global__ void __launch_bounds__(256) pna_backward_chunks_kernel(const PnBack W, int64_t slots, float* __restrict__ ws) {
  int64_t g, row, s0, s1;
  int c;
  group_lane(W.lanes, g, c);
  if (g >= slots || !slot_chunk(W.rowptr, W.n_rows, W.n_edges, g, row, s0, s1)) return;
  PnBAcc A;
  pn_back_entries<VEC, MOM2>(A, W, s0, s1, c);
  *reinterpret_cast<f4*>(pn_ws(ws, 0, slots, g, W.lanes, c)) = A.a;
  if (MOM2) *reinterpret_cast<f4*>(pn_ws(ws, 1, slots, g, W.lanes, c)) = A.b;
  if (W.g_min != nullptr) *reinterpret_cast<f4*>(pn_ws(ws, 2, slots, g, W.lanes, c)) = A.mn;
  if (W.g_max != nullptr) *reinterpret_cast<f4*>(pn_ws(ws, 3, slots, g, W.lanes, c)) = A.mx;
}

template <bool VEC, bool MOM2>
__global__ void __launch_bounds__(256) pna_backward_src_kernel(const PnBack W, int64_t slots, float* __restrict__ ws) {
  int64_t row, p0, p1;
  int c;
  group_lane(W.lanes, row, c);
  if (row >= W.n_rows) return;
  row_range(W.rowptr, W.n_edges, row, p0, p1);
  f4 d = f4{0.f, 0.f, 0.f, 0.f};
  if (p1 > p0) {
    PnBAcc A;
    pn_back_entries<VEC, MOM2>(A, W, p0, min(p0 + ROW_CHUNK, p1), c);
    if (p1 - p0 > ROW_CHUNK) {   // (n_part is 0 otherwise: the test only spares the short rows the division)
      int64_t first, n_part;
      row_partials(p0, p1, first, n_part);
#pragma unroll 2
      for (int64_t k = 0; k < n_part; ++k) {
        const int64_t g = first + k;
        if (W.a != nullptr) A.a += *reinterpret_cast<const f4*>(pn_ws(ws, 0, slots, g, W.lanes, c));
        if (MOM2) A.b += *reinterpret_cast<const f4*>(pn_ws(ws, 1, slots, g, W.lanes, c));
        if (W.g_min != nullptr) A.mn += *reinterpret_cast<const f4*>(pn_ws(ws, 2, slots, g, W.lanes, c));
        if (W.g_max != nullptr) A.mx += *reinterpret_cast<const f4*>(pn_ws(ws, 3, slots, g, W.lanes, c));
      }
    }
    if (W.a != nullptr) d = A.a;
    if (MOM2) d = d + tm_load<VEC>(W.P + row * W.ld_p + c, c, W.width) * A.b;
    if (W.g_min != nullptr) d = d + A.mn;
    if (W.g_max != nullptr) d = d + A.mx;
  }
  tm_store<VEC>(W.dP + row * W.ld_dp + c, c, W.width, d);
}

// ---------------------------------------------------------------------------------------------------------- scaler combine

struct PnScale {
  const int32_t* rowptr;
  int64_t n_rows;
  double avg_lin, avg_log;
  int32_t n_scalers, dim, lanes;
  int32_t scalers[EGC_PNA_MAX_SCALERS];
};

// the factor of scaler `code` for a row of n entries: d = max(n, 1), formed in double, rounded once
__device__ inline float pn_factor(int code, int n, double avg_lin, double avg_log) {
  const double d = (double)max(n, 1);
  switch (code) {
    case EGC_PNA_AMPLIFICATION: return (float)(log(d + 1.0) / avg_log);
    case EGC_PNA_ATTENUATION: return (float)(avg_log / log(d + 1.0));
    case EGC_PNA_LINEAR: return (float)(d / avg_lin);
    case EGC_PNA_INVERSE_LINEAR: return (float)(avg_lin / d);
    default: return 1.f;
  }
}

// BACKWARD false: out = base + sum_k f_k Y[k]  (acc = base; acc = acc + f_k * Y_k in list order)
// BACKWARD true:  out[k] = f_k * g   (x = g [n, dim], out = d Y [n, S dim])
template <bool VEC, bool BACKWARD>
__global__ void __launch_bounds__(256) pna_scale_kernel(const PnScale S, const float* __restrict__ x, int ld_x,
                                                        const float* __restrict__ base, int ld_base, float* __restrict__ out,
                                                        int ld_out) {
  int64_t row;
  int c;
  group_lane(S.lanes, row, c);
  if (row >= S.n_rows) return;
  const int n = S.rowptr[row + 1] - S.rowptr[row];
  if (BACKWARD) {
    const f4 g = tm_load<VEC>(x + row * ld_x + c, c, S.dim);
    for (int k = 0; k < S.n_scalers; ++k)
      tm_store<VEC>(out + row * ld_out + (int64_t)k * S.dim + c, c, S.dim, pn_factor(S.scalers[k], n, S.avg_lin, S.avg_log) * g);
  } else {
    f4 acc = tm_load<VEC>(base + row * ld_base + c, c, S.dim);
    for (int k = 0; k < S.n_scalers; ++k)
      acc = acc + pn_factor(S.scalers[k], n, S.avg_lin, S.avg_log) * tm_load<VEC>(x + row * ld_x + (int64_t)k * S.dim + c, c, S.dim);
    tm_store<VEC>(out + row * ld_out + c, c, S.dim, acc);
  }
}

// ------------------------------------------------------------------------------------------------------------------- host

// blk[op] = the block of op in the list, -1 when absent; false: an unknown or duplicate op, an empty or overlong list
static bool pn_blocks(const int32_t* ops, int32_t n_ops, int32_t* blk) {
  for (int op = 0; op < PN_OPS; ++op) blk[op] = -1;
  if (ops == nullptr || n_ops < 1 || n_ops > PN_OPS) return false;
  for (int k = 0; k < n_ops; ++k) {
    if (ops[k] < 0 || ops[k] >= PN_OPS || blk[ops[k]] >= 0) return false;
    blk[ops[k]] = k;
  }
  return true;
}

struct PnNeeds {
  bool sum, mom2, ext;
  int fields;
};
static PnNeeds pn_needs(const int32_t* blk) {
  PnNeeds n;
  n.sum = blk[EGC_PNA_SUM] >= 0 || blk[EGC_PNA_MEAN] >= 0;
  n.mom2 = blk[EGC_PNA_VAR] >= 0 || blk[EGC_PNA_STD] >= 0;
  n.ext = blk[EGC_PNA_MIN] >= 0 || blk[EGC_PNA_MAX] >= 0;
  n.fields = (n.sum ? 1 : 0) + (n.mom2 ? 2 : 0) + (n.ext ? 4 : 0);
  return n;
}

template <bool VEC, bool SUM, bool MOM2, bool EXT>
static int pn_forward_launch(const PnWalk& W, const PnOut& O, int64_t slots, float* ws, hipStream_t stream) {
  if (slots > 0) {
    unsigned blocks;
    if (grid_blocks(slots * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
    pna_chunks_kernel<VEC, SUM, MOM2, EXT><<<blocks, 256, 0, stream>>>(W, slots, ws);
    EGC_LAUNCH_CHECK("pna_chunks_kernel");
  }
  unsigned blocks;
  if (grid_blocks(W.n_rows * W.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  pna_aggregate_rows_kernel<VEC, SUM, MOM2, EXT><<<blocks, 256, 0, stream>>>(W, O, slots, ws);
  EGC_LAUNCH_CHECK("pna_aggregate_rows_kernel");
  return EGC_OK;
}

template <bool VEC>
static int pn_forward_dispatch(const PnNeeds& n, const PnWalk& W, const PnOut& O, int64_t slots, float* ws, hipStream_t stream) {
  switch ((n.sum ? 1 : 0) | (n.mom2 ? 2 : 0) | (n.ext ? 4 : 0)) {
    case 1: return pn_forward_launch<VEC, true, false, false>(W, O, slots, ws, stream);
    case 2: return pn_forward_launch<VEC, false, true, false>(W, O, slots, ws, stream);
    case 3: return pn_forward_launch<VEC, true, true, false>(W, O, slots, ws, stream);
    case 4: return pn_forward_launch<VEC, false, false, true>(W, O, slots, ws, stream);
    case 5: return pn_forward_launch<VEC, true, false, true>(W, O, slots, ws, stream);
    case 6: return pn_forward_launch<VEC, false, true, true>(W, O, slots, ws, stream);
    default: return pn_forward_launch<VEC, true, true, true>(W, O, slots, ws, stream);
  }
}

template <bool VEC, bool MOM2>
static int pn_backward_src_launch(const PnBack& B, int64_t slots, float* ws, hipStream_t stream) {
  if (slots > 0) {
    unsigned blocks;
    if (grid_blocks(slots * B.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
    pna_backward_chunks_kernel<VEC, MOM2><<<blocks, 256, 0, stream>>>(B, slots, ws);
    EGC_LAUNCH_CHECK("pna_backward_chunks_kernel");
  }
  unsigned blocks;
  if (grid_blocks(B.n_rows * B.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  pna_backward_src_kernel<VEC, MOM2><<<blocks, 256, 0, stream>>>(B, slots, ws);
  EGC_LAUNCH_CHECK("pna_backward_src_kernel");
  return EGC_OK;
}

static inline size_t pn_record_bytes(int64_t n_rows, int32_t width) { return (size_t)n_rows * (size_t)((width + 3) / 4) * 16; }

}  // namespace egc

using namespace egc;

size_t egc_pna_aggregate_workspace_bytes(int64_t n_edges, int32_t width, const int32_t* ops, int32_t n_ops) {
  int32_t blk[PN_OPS];
  if (n_edges <= 0 || width <= 0 || !pn_blocks(ops, n_ops, blk)) return 0;
  return (size_t)chunk_slots(n_edges) * (size_t)((width + 3) / 4) * 16 * (size_t)pn_needs(blk).fields;
}

size_t egc_pna_aggregate_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t width) {
  if (n_rows <= 0 || width <= 0) return 0;
  const int64_t slots = n_edges > 0 ? chunk_slots(n_edges) : 0;
  return 2 * pn_record_bytes(n_rows, width) + (size_t)slots * (size_t)((width + 3) / 4) * 16 * 4;
}

int egc_pna_aggregate_f32(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, int64_t n_rows, int64_t n_edges,
                          int64_t n_src_rows, const float* P, int32_t ld_p, const float* Q, int32_t ld_q, int32_t width,
                          const int32_t* ops, int32_t n_ops, float* out, int32_t ld_out, int32_t* arg_min, int32_t* arg_max,
                          float* mu, float* var, void* workspace, size_t workspace_bytes, egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PnOut O = {};
  if (width <= 0 || n_rows < 0 || n_edges < 0 || n_src_rows < 0 || !pn_blocks(ops, n_ops, O.blk)) return EGC_ERR_INVALID;
  if (ld_p < width || ld_q < width || (int64_t)ld_out < (int64_t)n_ops * width) return EGC_ERR_INVALID;
  if (n_rows == 0) return EGC_OK;
  if (rowptr == nullptr || Q == nullptr || out == nullptr) return EGC_ERR_INVALID;
  if (n_edges > 0 && (col == nullptr || P == nullptr || n_src_rows == 0)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  const PnNeeds needs = pn_needs(O.blk);
  PnWalk W = {};
  W.rowptr = rowptr, W.col = col, W.in = P;
  W.n_rows = n_rows, W.n_edges = n_edges, W.n_in_rows = n_src_rows;
  W.ld_in = ld_p, W.width = width, W.lanes = (width + 3) / 4;
  O.Q = Q, O.out = out, O.ld_q = ld_q, O.ld_out = ld_out, O.edge_id = edge_id;
  O.mu = needs.mom2 ? mu : nullptr;
  O.var = needs.mom2 ? var : nullptr;
  O.arg_min = O.blk[EGC_PNA_MIN] >= 0 ? arg_min : nullptr;
  O.arg_max = O.blk[EGC_PNA_MAX] >= 0 ? arg_max : nullptr;
  const bool vec = all_mult4(width, ld_p, ld_q, ld_out) && all_aligned16(P, Q, out, O.arg_min, O.arg_max, O.mu, O.var);
  const int64_t slots = chunk_slots(n_edges);
  float* ws = static_cast<float*>(workspace);
  if (slots > 0 && !workspace_ok(ws, workspace_bytes, (size_t)slots * (size_t)W.lanes * 16 * (size_t)needs.fields))
    return EGC_ERR_WORKSPACE;
  return vec ? pn_forward_dispatch<true>(needs, W, O, slots, ws, stream) : pn_forward_dispatch<false>(needs, W, O, slots, ws, stream);
}

int egc_pna_aggregate_backward_f32(const int32_t* rowptr, const int32_t* edge_id, int64_t n_rows, const int32_t* t_rowptr,
                                   const int32_t* t_col, const int32_t* t_edge_id, int64_t n_src_rows, int64_t n_edges,
                                   const float* dagg, int32_t ld_dagg, const int32_t* ops, int32_t n_ops, int32_t width,
                                   const float* P, int32_t ld_p, const int32_t* arg_min, const int32_t* arg_max, const float* mu,
                                   const float* var, float* dP, int32_t ld_dp, float* dQ, int32_t ld_dq,
                                   void* workspace, size_t workspace_bytes, egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PnGrad G = {};
  if (width <= 0 || n_rows < 0 || n_edges < 0 || n_src_rows < 0 || !pn_blocks(ops, n_ops, G.blk)) return EGC_ERR_INVALID;
  if ((int64_t)ld_dagg < (int64_t)n_ops * width || (dP != nullptr && ld_dp < width) || (dQ != nullptr && ld_dq < width))
    return EGC_ERR_INVALID;
  const int64_t p_rows = dP != nullptr ? n_src_rows : 0, q_rows = dQ != nullptr ? n_rows : 0;
  if (p_rows == 0 && q_rows == 0) return EGC_OK;
  if (rowptr == nullptr || (n_rows > 0 && dagg == nullptr)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  const PnNeeds needs = pn_needs(G.blk);
  const bool has_min = G.blk[EGC_PNA_MIN] >= 0, has_max = G.blk[EGC_PNA_MAX] >= 0;
  const bool lin = needs.sum || needs.mom2;          // the a record exists
  const bool want_p = p_rows > 0;
  if (want_p) {
    if (t_rowptr == nullptr || (n_edges > 0 && (t_col == nullptr || n_rows == 0))) return EGC_ERR_INVALID;
    if (n_edges > 0 && ((has_min && arg_min == nullptr) || (has_max && arg_max == nullptr))) return EGC_ERR_INVALID;
    if (needs.mom2 && (mu == nullptr || var == nullptr || P == nullptr || ld_p < width)) return EGC_ERR_INVALID;
  }
  const int32_t lanes = (width + 3) / 4;
  const bool records = want_p && lin && n_rows > 0;
  const int64_t slots = want_p ? chunk_slots(n_edges) : 0;
  float* ws = static_cast<float*>(workspace);
  const size_t rec = pn_record_bytes(n_rows, width);
  if ((records || slots > 0) && !workspace_ok(ws, workspace_bytes, egc_pna_aggregate_backward_workspace_bytes(n_rows, n_edges, width)))
    return EGC_ERR_WORKSPACE;
  const bool vec = all_mult4(width, ld_dagg, ld_dp, ld_dq, ld_p) && all_aligned16(dagg, dP, dQ, P, arg_min, arg_max, mu, var);
  if (n_rows > 0 && (q_rows > 0 || records)) {
    G.rowptr = rowptr, G.g = dagg, G.mu = mu, G.var = var, G.dQ = dQ;
    G.a = records ? ws : nullptr;
    G.b = records && needs.mom2 ? ws + rec / 4 : nullptr;
    G.n_rows = n_rows, G.n_edges = n_edges;
    G.ld_g = ld_dagg, G.ld_dq = ld_dq, G.width = width, G.lanes = lanes;
    unsigned blocks;
    if (grid_blocks(n_rows * lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
    if (vec) pna_backward_dst_kernel<true><<<blocks, 256, 0, stream>>>(G);
    else pna_backward_dst_kernel<false><<<blocks, 256, 0, stream>>>(G);
    EGC_LAUNCH_CHECK("pna_backward_dst_kernel");
  }
  if (!want_p) return EGC_OK;
  PnBack B = {};
  B.rowptr = t_rowptr, B.col = t_col, B.eid = t_edge_id, B.f_eid = edge_id;
  B.a = records ? ws : nullptr;
  B.b = records && needs.mom2 ? ws + rec / 4 : nullptr;
  B.g_min = has_min && n_rows > 0 ? dagg + (int64_t)G.blk[EGC_PNA_MIN] * width : nullptr;
  B.g_max = has_max && n_rows > 0 ? dagg + (int64_t)G.blk[EGC_PNA_MAX] * width : nullptr;
  B.arg_min = arg_min, B.arg_max = arg_max, B.P = P, B.dP = dP;
  B.n_rows = n_src_rows, B.n_edges = n_edges, B.n_in_rows = n_rows;
  B.ld_g = ld_dagg, B.ld_p = ld_p, B.ld_dp = ld_dp, B.width = width, B.lanes = lanes;
  float* parts = ws != nullptr ? ws + 2 * (rec / 4) : nullptr;
  const bool mom2 = B.b != nullptr;
  if (vec) return mom2 ? pn_backward_src_launch<true, true>(B, slots, parts, stream) : pn_backward_src_launch<true, false>(B, slots, parts, stream);
  return mom2 ? pn_backward_src_launch<false, true>(B, slots, parts, stream) : pn_backward_src_launch<false, false>(B, slots, parts, stream);
}

static int pn_scale(bool backward, const int32_t* rowptr, int64_t n_rows, const int32_t* scalers, int32_t n_scalers, double avg_lin,
                    double avg_log, int32_t dim, const float* x, int32_t ld_x, const float* base, int32_t ld_base, float* out,
                    int32_t ld_out, hipStream_t stream) {
  if (dim <= 0 || n_rows < 0 || scalers == nullptr || n_scalers < 1 || n_scalers > EGC_PNA_MAX_SCALERS) return EGC_ERR_INVALID;
  PnScale S = {};
  for (int k = 0; k < n_scalers; ++k) {
    if (scalers[k] < 0 || scalers[k] > EGC_PNA_INVERSE_LINEAR) return EGC_ERR_INVALID;
    for (int m = 0; m < k; ++m)
      if (scalers[m] == scalers[k]) return EGC_ERR_INVALID;
    S.scalers[k] = scalers[k];
  }
  const int64_t wide = (int64_t)n_scalers * dim;
  if (backward ? (ld_x < dim || ld_out < wide) : (ld_x < wide || ld_base < dim || ld_out < dim)) return EGC_ERR_INVALID;
  if (n_rows == 0) return EGC_OK;
  if (rowptr == nullptr || x == nullptr || out == nullptr || (!backward && base == nullptr)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows)) return EGC_ERR_UNSUPPORTED;
  S.rowptr = rowptr, S.n_rows = n_rows, S.avg_lin = avg_lin, S.avg_log = avg_log;
  S.n_scalers = n_scalers, S.dim = dim, S.lanes = (dim + 3) / 4;
  const bool vec = all_mult4(dim, ld_x, ld_base, ld_out) && all_aligned16(x, base, out);
  unsigned blocks;
  if (grid_blocks(n_rows * S.lanes, 256, blocks) != EGC_OK) return EGC_ERR_UNSUPPORTED;
  if (backward) {
    if (vec) pna_scale_kernel<true, true><<<blocks, 256, 0, stream>>>(S, x, ld_x, base, ld_base, out, ld_out);
    else pna_scale_kernel<false, true><<<blocks, 256, 0, stream>>>(S, x, ld_x, base, ld_base, out, ld_out);
  } else {
    if (vec) pna_scale_kernel<true, false><<<blocks, 256, 0, stream>>>(S, x, ld_x, base, ld_base, out, ld_out);
    else pna_scale_kernel<false, false><<<blocks, 256, 0, stream>>>(S, x, ld_x, base, ld_base, out, ld_out);
  }
  EGC_LAUNCH_CHECK("pna_scale_kernel");
  return EGC_OK;
}

int egc_pna_scale_combine_f32(const int32_t* rowptr, int64_t n_rows, const int32_t* scalers, int32_t n_scalers, double avg_lin,
                              double avg_log, int32_t dim, const float* Y, int32_t ld_y, const float* base, int32_t ld_base,
                              float* out, int32_t ld_out, egc_stream_t stream) {
  return pn_scale(false, rowptr, n_rows, scalers, n_scalers, avg_lin, avg_log, dim, Y, ld_y, base, ld_base, out, ld_out,
                  (hipStream_t)stream);
}

int egc_pna_scale_combine_backward_f32(const int32_t* rowptr, int64_t n_rows, const int32_t* scalers, int32_t n_scalers,
                                       double avg_lin, double avg_log, int32_t dim, const float* g, int32_t ld_g, float* dY,
                                       int32_t ld_dy, egc_stream_t stream) {
  return pn_scale(true, rowptr, n_rows, scalers, n_scalers, avg_lin, avg_log, dim, g, ld_g, nullptr, 0, dY, ld_dy,
                  (hipStream_t)stream);
}
