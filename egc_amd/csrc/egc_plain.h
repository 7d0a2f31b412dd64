// The plain host arithmetic every planner and launcher shares: no HIP header, no device code.  egc_common.h and
// egc_aggregate_dev.h include it; egc_backward_host.h and egc_fused_tile_host.h (and tests/backward_plan, tests/fused_tile_plan,
// compiled without HIP) build on it.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "egc_hip.h"

namespace egc {

constexpr unsigned OOB = 0xFFFFFFF0u;  // any offset >= num_records makes a buffer load return 0

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// THE alignment predicate of every launcher (a null pointer counts as aligned); bytes: a power of two
static inline bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
static inline bool aligned16(const void* p) { return aligned_to(p, 16); }

// THE reading of an on/off switch of the environment: on iff set to anything but "" / "0", as
// egc_amd._C.env_flag reads it; read on every call
static inline bool env_on(const char* name) {
  const char* v = getenv(name);
  return v != nullptr && v[0] != '\0' && !(v[0] == '0' && v[1] == '\0');
}

constexpr int AMAX = 4;     // aggregators supported by the register-resident combine

// floor(2^32 / d) + 1: q / d == umulhi(q, magic) for the q < 2^16 the kernels divide
inline unsigned agg_magic(int d) { return (unsigned)(((uint64_t)1 << 32) / (uint64_t)d) + 1u; }

// floats of the epilogue's bias strip in LDS: the (padded) head layout [h][Ls] (>= F_out floats)
constexpr int bias_strip_floats(int H, int Ls) { return (H * Ls + 3) & ~3; }

// floats between consecutive bases of a `bases` row (egc_layer.basis_stride; 0 = contiguous)
static inline int layer_basis_stride(const egc_layer* L) {
  const int len = L->out_channels / L->num_heads;
  return L->basis_stride > len ? L->basis_stride : len;
}

// floats of a `bases` row (what the exported egc_bases_ld answers for a layer with heads)
static inline int layer_bases_ld(const egc_layer* L) { return (L->num_bases * layer_basis_stride(L) + 3) & ~3; }

static inline bool layer_uses_symnorm(const egc_layer* L) {
  for (int t = 0; t < L->num_aggrs; ++t)
    if (L->aggrs[t] == EGC_AGGR_SYMNORM) return true;
  return false;
}

// Long-row plan layout (int32 words), shared by egc_csr_prepare and the aggregate kernels:
//   [0] n_long   [1] n_chunks   [2] cap_long   [3] cap_chunks
//   [4 .. 4+cap_long)                 long_row[s]      row id of long-row slot s
//   [.. +cap_long)                    long_chunk0[s]   first chunk slot of that row
//   [.. +cap_chunks)                  chunk_slot[c]    long-row slot the chunk belongs to
//   [.. +cap_chunks)                  chunk_begin[c]   first CSR entry of the chunk
struct PlanCaps {
  int64_t cap_long;
  int64_t cap_chunks;
};
static inline PlanCaps plan_caps(int64_t n_nodes, int64_t n_edges) {
  PlanCaps c;
  c.cap_long = n_edges / (EGC_LONG_ROW_THRESHOLD + 1) + 1;
  if (c.cap_long > n_nodes + 1) c.cap_long = n_nodes + 1;
  c.cap_chunks = n_edges / EGC_LONG_ROW_CHUNK + c.cap_long;
  return c;
}
// chunk slots a launch has to cover: the host-known chunk count of the graph (egc_graph.n_chunks) where it is one, else the capacity
static inline int64_t plan_chunks(const PlanCaps& c, int64_t n_chunks) {
  return (n_chunks >= 0 && n_chunks <= c.cap_chunks) ? n_chunks : c.cap_chunks;
}
// ... and the leading blocks of a grid that take them, one wavefront of a 256-thread block per chunk
static inline int plan_chunk_blocks(int64_t n_rows, int64_t n_edges, int64_t n_chunks) {
  return (int)ceil_div(plan_chunks(plan_caps(n_rows, n_edges), n_chunks), 4);
}

// Lane group of the kernels that give a row 16, 32 or 64 lanes (arg_extrema_kernel, bwd_src_kernel, bwd_dst_fast_kernel): the
// smallest of them that holds the row's 16-byte slots, and the slots a lane then owns (more than one beyond 64 slots).
struct LaneGroup {
  int lpr_log2, ns;
};
static inline LaneGroup lane_group(int slots) {
  int lg = 4;
  while ((1 << lg) < slots && lg < 6) ++lg;
  return {lg, (slots + (1 << lg) - 1) >> lg};
}

// an aggregator list as one word: 3 bits per code, first aggregator in the low bits (what the compiled-in configurations of
// the forward -- StCfg's AGG, agg_pack -- and of the backward -- bwd_agg_pack -- are matched against)
static inline unsigned pack_aggr_codes(const int* aggr, int A) {
  unsigned pk = 0;
  for (int t = 0; t < A; ++t) pk |= (unsigned)aggr[t] << (3 * t);
  return pk;
}

enum { STAT_SUM = 0, STAT_SQ = 1, STAT_MX = 2, STAT_MN = 3, STAT_WS = 4 };

// Which raw statistics a layer's aggregator list needs (shared by the forward store and the backward load).
static inline int stat_layout(const int* aggr, int A, int (&slot)[5]) {
  bool need[5] = {false, false, false, false, false};
  for (int t = 0; t < A; ++t) {
    switch (aggr[t]) {
      case EGC_AGGR_SUM: case EGC_AGGR_MEAN: need[STAT_SUM] = true; break;
      case EGC_AGGR_VAR: case EGC_AGGR_STD: need[STAT_SUM] = need[STAT_SQ] = true; break;
      case EGC_AGGR_MAX: need[STAT_MX] = true; break;
      case EGC_AGGR_MIN: need[STAT_MN] = true; break;
      default: need[STAT_WS] = true; break;
    }
  }
  int k = 0;
  for (int s = 0; s < 5; ++s) slot[s] = need[s] ? k++ : -1;
  return k;
}

}  // namespace egc
