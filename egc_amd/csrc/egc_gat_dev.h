// Device pieces that the attention kernels (egc_gatv2.hip, egc_gat.hip) share: the padded-group row mapping and its lane
// bookkeeping, the per-head sum across a group's lanes, the row loads and stores, the online-softmax state and the dropout
// mask.  Their host side (launch geometry, argument checks, the (S, VEC, SMALL) dispatch): egc_gat_host.h.
//
// Mapping: egc_row_chunks.h's, with the group padded.  A row's group is G = the power of two >= ceil(H C / 4) lanes, at most 64,
// so it lies inside one wavefront; for H C > 256 the group is a whole wavefront and a lane owns two quads of columns (S = 2
// slots, 256 columns apart).  "Virtual lane" v = lane + G * slot owns columns 4 v .. 4 v + 3.
//
// Order rule of a per-head sum over the head's C columns (gat_head_sums).  It depends on H and C only, never on where in the
// grid the row lands.
//   C >= 4: per virtual lane, a = its columns of the head of its FIRST column added in ascending column order, b = its later
//   columns (they belong to the next head) likewise.  The first virtual lane of a head's segment (the lanes whose first column
//   lies in the head) takes a = b(v - 1) + a when the head starts inside lane v - 1.  Then a Hillis-Steele inclusive scan over
//   the segment: for d = 1, 2, 4, ... < ceil(C / 4) + 1, a(v) = a(v) + a(v - d) where v - d is still in the segment (all lanes
//   read before any writes).  The head's sum is a of the segment's last lane.
//   C < 4: a head lies within virtual lanes v - 1 .. v + 1; every column adds the head's columns in ascending column order.
// Order rule of the online softmax (gat_state_take, gat_state_merge), per batch of live scores s_k and rows v_k:
// bm = max(m, the live scores in entry order); l = l * r + sum in entry order of exp(s_k - bm), acc likewise with
// exp(s_k - bm) * v_k, r = exp(m - bm) (1 when m == bm); m = bm.  Two states merge as M = max(m1, m2);
// l = l1 exp(m1 - M) + l2 exp(m2 - M), acc likewise.
//
// Attention dropout (the DROP instances of both files' kernels; PyG's F.dropout on alpha, per entry and head, the self entry
// included).  The mask is a pure function of (seed, entry, head): Philox4x32-10 (egc_philox.h) under the key (low, high 32 bits
// of the int64 seed, read on the device), counter (p, h >> 2, 0, 0) for the entry at position p of the FORWARD CSR and
// (i, h >> 2, 1, 0) for row i's self entry; head h takes output word h & 3 and is dropped iff word < threshold
// (= floor(p 2^32)).  A lane's quad of columns lies in at most two groups of four heads: one Philox call per slot, a second
// one only where the quad's first and last column fall into different groups (gat_keep_bits); no lane talks to another.
// Skipped entries keep their position.  Order rule with the mask: m, l and lse are those of the unmasked row, term for term;
// a dropped (entry, head) leaves out its term of acc and nothing else, the kept terms stay in entry order, and the forward
// multiplies by scale = 1 / (1 - p) ONCE, at the row's end: out = (acc / l) * scale.  The backward sums take the factor per
// entry, m' = scale or 0 (gat_keep_f4), as a factor of the term they add, in the order they had.
#pragma once
#include "egc_philox.h"
#include "egc_row_chunks.h"

namespace egc {

constexpr int GAT_AHEAD = 8;
constexpr int GAT_AHEAD_BWD = 4;
constexpr int GAT_SUM_BLOCK = 64;

struct GatWalk {
  const int32_t* rowptr;   // the CSR walked: n_rows + 1 offsets
  const int32_t* col;      // n_edges entries: rows of the gathered arrays
  const float* xl;         // forward / destination pass: gathered (n_in_rows rows); source pass: the row's own
  const float* xr;         // forward / destination pass: the row's own; source pass: gathered
  const float* att;        // [H C]
  const float* g;          // backward: d out.  destination pass: the row's own; source pass: gathered
  const float* out;        // destination pass: the forward's output
  const float* lse;        // backward: [n_nodes, H]
  const float* D;          // source pass: [n_nodes, H] (the destination pass writes it)
  int64_t n_rows, n_edges, n_in_rows;
  int32_t ld_xl, ld_xr, ld_g, ld_out;
  int32_t H, C, width, G, V, seg, self_loops;
  float slope;
};

template <int S>
struct GatLane {
  int base;            // wavefront lane of the group's lane 0
  int v[S], c[S];      // virtual lane and its first column
  int na[S];           // how many of the four columns belong to the head of the first one (C >= 4)
  int first_a[S];      // first virtual lane of that head's segment
  int last_a[S], last_b[S];
  bool prev_b[S];      // the segment's first lane, and the head starts inside the lane before
  int hd[S][4];        // head of every column (clamped to H - 1)
  bool head_first[S][4];   // the column is its head's first (and exists)
};

template <int S>
__device__ inline GatLane<S> gat_lane(const GatWalk& W, int lane_in_group) {
  GatLane<S> L;
  L.base = ((int)threadIdx.x & 63) & ~(W.G - 1);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int v = lane_in_group + W.G * s, c = 4 * v;
    L.v[s] = v, L.c[s] = c;
    const bool live = c < W.width;
    const int ha = live ? c / W.C : 0;
    const int end_a = (ha + 1) * W.C;
    L.na[s] = live ? min(4, end_a - c) : 4;
    L.first_a[s] = live ? (ha * W.C + 3) / 4 : v;
    L.last_a[s] = live ? (end_a - 1) / 4 : v;
    const int hb = min(ha + 1, W.H - 1);
    L.last_b[s] = live ? min(((hb + 1) * W.C - 1) / 4, W.V - 1) : v;
    L.prev_b[s] = live && v > 0 && v == L.first_a[s] && (ha * W.C) % 4 != 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = min((c + j) / W.C, W.H - 1);
      L.hd[s][j] = h;
      L.head_first[s][j] = c + j < W.width && c + j == h * W.C;
    }
  }
  return L;
}

// x of virtual lane src (0 <= src < V) of this group
template <int S>
__device__ inline float gat_vget(const GatWalk& W, const GatLane<S>& L, const float (&x)[S], int src) {
  const int lane = L.base + (src & (W.G - 1));
  float t = __shfl(x[0], lane);
  if (S == 2) {
    const float t1 = __shfl(x[S - 1], lane);
    t = src >= W.G ? t1 : t;
  }
  return t;
}

// out[s][j] = the sum of p over the columns of column (c[s] + j)'s head, in the order of the file header
template <int S, bool SMALL>
__device__ inline void gat_head_sums(const GatWalk& W, const GatLane<S>& L, const f4 (&p)[S], f4 (&out)[S]) {
  if (SMALL) {
    float q[S][12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[S];
#pragma unroll
      for (int s = 0; s < S; ++s) x[s] = p[s][j];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        q[s][j] = gat_vget<S>(W, L, x, max(L.v[s] - 1, 0));
        q[s][4 + j] = x[s];
        q[s][8 + j] = gat_vget<S>(W, L, x, min(L.v[s] + 1, W.V - 1));
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lo = L.hd[s][j] * W.C, hi = lo + W.C;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          const int cc = L.c[s] - 4 + t;
          sum = (cc >= lo && cc < hi) ? sum + q[s][t] : sum;
        }
        out[s][j] = sum;
      }
    return;
  }
  float a[S], b[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a[s] = p[s][0], b[s] = 0.f;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      a[s] = j < L.na[s] ? a[s] + p[s][j] : a[s];
      b[s] = j < L.na[s] ? b[s] : b[s] + p[s][j];
    }
  }
  float t[S];
#pragma unroll
  for (int s = 0; s < S; ++s) t[s] = gat_vget<S>(W, L, b, max(L.v[s] - 1, 0));
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] = L.prev_b[s] ? t[s] + a[s] : a[s];
#pragma unroll 1
  for (int d = 1; d < W.seg; d <<= 1) {
#pragma unroll
    for (int s = 0; s < S; ++s) t[s] = gat_vget<S>(W, L, a, max(L.v[s] - d, 0));
#pragma unroll
    for (int s = 0; s < S; ++s) a[s] = L.v[s] - d >= L.first_a[s] ? a[s] + t[s] : a[s];
  }
  float sa[S], sb[S];
#pragma unroll
  for (int s = 0; s < S; ++s) sa[s] = gat_vget<S>(W, L, a, L.last_a[s]), sb[s] = gat_vget<S>(W, L, a, L.last_b[s]);
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[s][j] = j < L.na[s] ? sa[s] : sb[s];
}

template <bool VEC>
__device__ inline f4 gat_load(const float* __restrict__ p, int c, int width) {
  if (VEC) return c < width ? *reinterpret_cast<const f4*>(p) : f4{0.f, 0.f, 0.f, 0.f};
  return tm_load<false>(p, c, width);
}

template <bool VEC>
__device__ inline void gat_store(float* __restrict__ p, int c, int width, f4 v) {
  if (VEC) {
    if (c < width) *reinterpret_cast<f4*>(p) = v;
    return;
  }
  tm_store<false>(p, c, width, v);
}

template <int S, bool VEC>
__device__ inline void gat_load_row(f4 (&v)[S], const float* __restrict__ base, int64_t row, int ld, const GatLane<S>& L, int width) {
#pragma unroll
  for (int s = 0; s < S; ++s) v[s] = gat_load<VEC>(base + row * ld + L.c[s], L.c[s], width);
}

// a per-(row, head) value for every column of the lane
template <int S>
__device__ inline void gat_load_heads(f4 (&v)[S], const float* __restrict__ a, int64_t row, const GatWalk& W, const GatLane<S>& L) {
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[s][j] = a[row * W.H + L.hd[s][j]];
}

__device__ inline f4 gat_exp(f4 x) { return f4{expf(x[0]), expf(x[1]), expf(x[2]), expf(x[3])}; }

// the score's activation and its derivative, per column
__device__ inline f4 gat_lrelu(f4 z, float slope) {
  f4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = z[i] > 0.f ? z[i] : slope * z[i];
  return r;
}

__device__ inline f4 gat_dlrelu(f4 z, float slope) {
  f4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = z[i] > 0.f ? 1.f : slope;
  return r;
}

// The DROP forms of the device functions take ONE more argument at the end (the mask's GatMask; a batch's keep bits) and the
// plain forms none: a parameter pack that is empty or holds that one argument.  So the plain instantiations are, token for
// token, what they were before there was a mask.  gat_only: the pack's one element.
template <class T>
__device__ inline const T& gat_only(const T& t) { return t; }

template <int S>
struct GatState {
  f4 m[S], l[S], acc[S];
};

template <int S>
__device__ inline void gat_state_init(GatState<S>& st) {
  const float ninf = -__builtin_inff();
#pragma unroll
  for (int s = 0; s < S; ++s) st.m[s] = f4{ninf, ninf, ninf, ninf}, st.l[s] = f4{0.f, 0.f, 0.f, 0.f}, st.acc[s] = st.l[s];
}

// one batch of N entries with scores e and rows v folded into the state (file header).  With one more argument, keep[N] (DROP):
// bit 4 s + j of keep[k] clear = entry k adds nothing to acc of column j of slot s; m and l never look at it.
template <int S, int N, class... Keep>
__device__ inline void gat_state_take(GatState<S>& st, const f4 (&e)[N][S], const f4 (&v)[N][S], const bool (&live)[N],
                                      const Keep&... keep) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f4 bm = st.m[s];
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) bm[i] = (live[k] && e[k][s][i] > bm[i]) ? e[k][s][i] : bm[i];
    f4 r = gat_exp(st.m[s] - bm);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = st.m[s][i] == bm[i] ? 1.f : r[i];
    f4 l = st.l[s] * r, acc = st.acc[s] * r;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      f4 w = gat_exp(e[k][s] - bm);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = live[k] ? w[i] : 0.f;
      l = l + w;
      if constexpr (sizeof...(Keep) == 0) {
        acc = acc + w * v[k][s];
      } else {
        const uint32_t bits = gat_only(keep...)[k];
        const f4 t = acc + w * v[k][s];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = (bits >> (4 * s + i)) & 1u ? t[i] : acc[i];
      }
    }
    st.m[s] = bm, st.l[s] = l, st.acc[s] = acc;
  }
}

template <int S>
__device__ inline void gat_state_merge(GatState<S>& st, const f4 (&m2)[S], const f4 (&l2)[S], const f4 (&acc2)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f4 bm, r1, r2;
#pragma unroll
    for (int i = 0; i < 4; ++i) bm[i] = m2[s][i] > st.m[s][i] ? m2[s][i] : st.m[s][i];
    r1 = gat_exp(st.m[s] - bm), r2 = gat_exp(m2[s] - bm);
#pragma unroll
    for (int i = 0; i < 4; ++i) r1[i] = st.m[s][i] == bm[i] ? 1.f : r1[i], r2[i] = m2[s][i] == bm[i] ? 1.f : r2[i];
    st.l[s] = st.l[s] * r1 + l2[s] * r2;
    st.acc[s] = st.acc[s] * r1 + acc2[s] * r2;
    st.m[s] = bm;
  }
}

// ------------------------------------------------------------------------------------------------------ attention dropout

struct GatDrop {
  const int64_t* seed;      // device scalar: the Philox key
  const int32_t* edge_id;   // source pass: the forward position of every entry of the transposed CSR
  uint32_t threshold;       // dropped iff word < threshold
  float scale;              // 1 / (1 - p)
};

// what the kernels hold of it: the key read, the rest copied
struct GatMask {
  uint32_t k0, k1, threshold;
  float scale;
  const int32_t* edge_id;
};

__device__ inline GatMask gat_mask(const GatDrop& R) {
  const uint64_t s = (uint64_t)*R.seed;
  return GatMask{(uint32_t)s, (uint32_t)(s >> 32), R.threshold, R.scale, R.edge_id};
}

// Bit 4 s + j: column c[s] + j of this lane keeps the entry of counter (c0, ., c2, 0) -- c0 = the entry's forward position and
// c2 = 0, or c0 = the row and c2 = 1 for the self entry.  The heads of a quad span at most two groups of four (file header).
template <int S>
__device__ inline uint32_t gat_keep_bits(const GatMask& X, const GatLane<S>& L, uint32_t c0, uint32_t c2) {
  uint32_t bits = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int g0 = L.hd[s][0] >> 2, g1 = L.hd[s][3] >> 2;
    uint32_t w0[4], w1[4];
    philox4x32_10(c0, (uint32_t)g0, c2, 0u, X.k0, X.k1, w0);
#pragma unroll
    for (int i = 0; i < 4; ++i) w1[i] = w0[i];
    if (g1 != g0) philox4x32_10(c0, (uint32_t)g1, c2, 0u, X.k0, X.k1, w1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = L.hd[s][j], i = h & 3;
      const bool first = (h >> 2) == g0;
      const uint32_t a = i == 0 ? w0[0] : i == 1 ? w0[1] : i == 2 ? w0[2] : w0[3];
      const uint32_t b = i == 0 ? w1[0] : i == 1 ? w1[1] : i == 2 ? w1[2] : w1[3];
      bits |= ((first ? a : b) >= X.threshold ? 1u : 0u) << (4 * s + j);
    }
  }
  return bits;
}

// keep[k] = gat_keep_bits of entry k of the batch that starts at forward position p (self: the self entry of `row`), one entry
// after the other in a loop that is NOT unrolled: unrolled, the N independent Philox chains hold their registers at once
// (60 to 90 VGPRs more than the plain instance, a wave per SIMD less), and the integer work is not what the kernel waits for.
template <int S, int N, bool FULL>
__device__ inline void gat_batch_keep(uint32_t (&keep)[N], const GatMask& X, const GatLane<S>& L, int64_t p, int64_t p1, int64_t row,
                                      bool self) {
  static_assert(8 * N <= 64 && S <= 2, "eight bits per entry in one 64-bit word");
  uint64_t packed = 0;
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    const uint32_t c0 = (uint32_t)(self ? row : batch_entry<FULL>(p, k, p1));
    packed |= (uint64_t)gat_keep_bits<S>(X, L, c0, self ? 1u : 0u) << (8 * k);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) keep[k] = (uint32_t)(packed >> (8 * k)) & 0xffu;
}

// the same for entries whose counters are pos[k] (the source pass: forward positions read from t_edge_id; self: c2 = 1)
template <int S, int N>
__device__ inline void gat_batch_keep_at(uint32_t (&keep)[N], const GatMask& X, const GatLane<S>& L, const uint32_t (&pos)[N], bool self) {
  static_assert(8 * N <= 64 && S <= 2, "eight bits per entry in one 64-bit word");
  uint64_t packed = 0;
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    uint32_t c0 = pos[0];
#pragma unroll
    for (int i = 1; i < N; ++i) c0 = k == i ? pos[i] : c0;
    packed |= (uint64_t)gat_keep_bits<S>(X, L, c0, self ? 1u : 0u) << (8 * k);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) keep[k] = (uint32_t)(packed >> (8 * k)) & 0xffu;
}

// m' of slot s: scale where kept, 0 where dropped
__device__ inline f4 gat_keep_f4(uint32_t bits, int s, float scale) {
  f4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (bits >> (4 * s + i)) & 1u ? scale : 0.f;
  return r;
}

}  // namespace egc
