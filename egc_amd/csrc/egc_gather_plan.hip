// Gather plan of a static graph (egc_hip.h: egc_gather_plan_build): col and edge_dis of every CSR entry in ONE word, which the
// inference aggregate (egc_aggregate_fast.hip, PLAN form) streams instead of the two arrays.  Built once per graph and edge set.
//
// Why: the aggregate is bound by the bytes that leave the XCD L2s.  Per entry it streams col (4 B) and
// edge_dis (4 B), yet edge_dis[p] = dis[col[p]] is one of a few hundred distinct floats -- the source id and an index into the
// table of those floats fit one word.  The word sits at the entry's CSR position: rows are found through rowptr as ever.
#include <algorithm>
#include <atomic>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "egc_common.h"

namespace egc {

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int64_t pad4(int64_t x) { return (x + 3) & ~(int64_t)3; }

struct GpLayout {   // int32 offsets into the plan
  int64_t table, entries, end;
};
inline GpLayout gp_layout(int64_t n, int64_t e) {
  GpLayout l;
  l.table = EGC_GP_HEADER_INTS;
  l.entries = l.table + pad4(std::max<int64_t>(n, 1));
  l.end = l.entries + pad4(std::max<int64_t>(e, 1));
  return l;
}

// bits of an entry that hold the source id: ceil(log2(n)), at least 1 and at least `min_bits`
__host__ __device__ inline int gp_col_bits(int64_t n, int min_bits) {
  int b = 1;
  while (((int64_t)1 << b) < n && b < 32) ++b;
  return b > min_bits ? b : min_bits;
}
// one packed word while the table's indices fit the bits above the source id
__host__ __device__ inline int gp_form(int cb, int64_t n_table) {
  return (cb < 32 && n_table <= ((int64_t)1 << (32 - cb))) ? EGC_GP_PACKED : EGC_GP_UNFIT;
}

struct GpWs {   // byte offsets into the workspace
  size_t dbits, dbits_sorted, flags, pos, src_idx, temp, temp_bytes, total;
};

hipError_t gp_ws(int64_t n, GpWs* w) {
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  size_t sort_b = 0, scan_b = 0;   // each primitive asked with the size it is called with
  hipError_t st = rocprim::radix_sort_keys(nullptr, sort_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, nn, 0u, 32u, (hipStream_t)0);
  if (st != hipSuccess) return st;
  st = rocprim::exclusive_scan(nullptr, scan_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, nn + 1, rocprim::plus<uint32_t>(),
                               (hipStream_t)0);
  if (st != hipSuccess) return st;
  const size_t arr = align256((nn + 1) * sizeof(uint32_t));
  size_t o = 0;
  auto take = [&](size_t& f) { f = o; o += arr; };
  take(w->dbits); take(w->dbits_sorted); take(w->flags); take(w->pos); take(w->src_idx);
  w->temp = o;
  w->temp_bytes = align256(std::max(sort_b, scan_b));
  w->total = o + w->temp_bytes + 256;
  return hipSuccess;
}

// ---- kernels ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gp_dis_bits_kernel(int n, const float* __restrict__ dis, uint32_t* __restrict__ bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) bits[i] = __float_as_uint(dis[i]);
}

__global__ void __launch_bounds__(256) gp_unique_flags_kernel(int n, const uint32_t* __restrict__ sorted, uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  flags[i] = (i < n && (i == 0 || sorted[i] != sorted[i - 1])) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) gp_unique_put_kernel(int n, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos, uint32_t* __restrict__ table) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && flags[i] != 0u) table[pos[i]] = sorted[i];
}

// The header, and the index of every source's dis value in the table (lower bound on the bit patterns: the table holds exactly
// these values).
__global__ void __launch_bounds__(256) gp_src_index_kernel(int n, const float* __restrict__ dis, const uint32_t* __restrict__ table,
                                                           const uint32_t* __restrict__ pos, int cb, uint32_t* __restrict__ src_idx,
                                                           int32_t* __restrict__ header) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n_table = (int)pos[n];
  if (i == 0) {
    header[EGC_GP_TABLE_SIZE] = n_table;
    header[EGC_GP_COL_BITS] = cb;
    header[EGC_GP_FORM] = gp_form(cb, n_table);
  }
  if (i >= n) return;
  const uint32_t v = __float_as_uint(dis[i]);
  int lo = 0, hi = n_table;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] < v) lo = mid + 1; else hi = mid;
  }
  src_idx[i] = (uint32_t)lo;
}

// entries[p] = col[p] | index(dis[col[p]]) << cb, where the form is packed (pos[n] = the table's size: the same decision as the
// header's, taken without reading what another workgroup of the previous launch wrote last)
__global__ void __launch_bounds__(256) gp_pack_kernel(int64_t e, int n, const int32_t* __restrict__ col, const uint32_t* __restrict__ src_idx,
                                                      const uint32_t* __restrict__ pos, int cb, uint32_t* __restrict__ entries) {
  if (gp_form(cb, (int64_t)pos[n]) != EGC_GP_PACKED) return;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < e; p += (int64_t)gridDim.x * 256) {
    const int j = col[p];
    entries[p] = (uint32_t)j | ((j >= 0 && j < n ? src_idx[j] : 0u) << cb);
  }
}

}  // namespace

}  // namespace egc

using namespace egc;

static std::atomic<int64_t> g_plan_launches{0};

namespace egc {
void gather_plan_launched() { g_plan_launches.fetch_add(1, std::memory_order_relaxed); }
}  // namespace egc

extern "C" {

int64_t egc_gather_plan_launches(void) { return g_plan_launches.load(std::memory_order_relaxed); }

int32_t egc_gather_plan_form(int64_t n_nodes, int64_t n_table, int32_t min_col_bits) {
  if (n_nodes < 0 || n_table < 0 || min_col_bits < 0 || min_col_bits > 32) return 0;
  const int cb = gp_col_bits(n_nodes, min_col_bits);
  return gp_form(cb, n_table) | (cb << 8);
}

int64_t egc_gather_plan_offset(int64_t n_nodes, int64_t n_edges, int32_t part) {
  if (n_nodes < 0 || n_edges < 0) return -1;
  const GpLayout l = gp_layout(n_nodes, n_edges);
  switch (part) {
    case 0: return l.table;
    case 1: return l.entries;
    case 2: return l.end;
    default: return -1;
  }
}

size_t egc_gather_plan_bytes(int64_t n_nodes, int64_t n_edges) {
  if (n_nodes < 0 || n_edges < 0) return 0;
  return (size_t)gp_layout(n_nodes, n_edges).end * sizeof(int32_t);
}

size_t egc_gather_plan_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
  if (n_nodes < 0 || n_edges < 0) return 0;
  GpWs w;
  if (gp_ws(n_nodes, &w) != hipSuccess) return 0;
  return w.total;
}

int egc_gather_plan_build(const egc_graph* graph, int32_t edge_set, int32_t min_col_bits, int32_t* plan, size_t plan_bytes,
                          void* workspace, size_t workspace_bytes, egc_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (graph == nullptr || plan == nullptr) return EGC_ERR_INVALID;
  const int64_t n = graph->n_nodes, e = graph->n_edges;
  if (n <= 0 || e < 0 || n >= ((int64_t)1 << 31) - 1 || e >= ((int64_t)1 << 31) - 1) return EGC_ERR_INVALID;
  if (graph->n_src_rows > 0 && graph->n_src_rows != n) return EGC_ERR_UNSUPPORTED;   // square graphs only
  if (e > 0 && graph->col == nullptr) return EGC_ERR_INVALID;
  if (edge_set != EGC_SET_RAW && edge_set != EGC_SET_LOOPED) return EGC_ERR_INVALID;
  if (min_col_bits < 0 || min_col_bits > 32) return EGC_ERR_INVALID;
  const float* dis = edge_set == EGC_SET_LOOPED ? graph->dis_looped : graph->dis_raw;
  if (dis == nullptr) return EGC_ERR_INVALID;
  const GpLayout l = gp_layout(n, e);
  if (plan_bytes < (size_t)l.end * sizeof(int32_t)) return EGC_ERR_INVALID;
  GpWs w;
  EGC_HIP_TRY(gp_ws(n, &w));
  if (workspace == nullptr || workspace_bytes < w.total) return EGC_ERR_WORKSPACE;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  auto u32 = [&](size_t off) { return (uint32_t*)(ws + off); };
  void* temp = ws + w.temp;
  const int cb = gp_col_bits(n, min_col_bits);
  const int nb = (int)ceil_div(n, (int64_t)256), nb1 = (int)ceil_div(n + 1, (int64_t)256);
  uint32_t* table = (uint32_t*)(plan + l.table);
  uint32_t* entries = (uint32_t*)(plan + l.entries);

  EGC_HIP_TRY(hipMemsetAsync(plan, 0, EGC_GP_HEADER_INTS * sizeof(int32_t), stream));
  // the distinct dis values: sort the bit patterns, mark the first of each run, scan, put
  gp_dis_bits_kernel<<<nb, 256, 0, stream>>>((int)n, dis, u32(w.dbits));
  EGC_LAUNCH_CHECK("gp_dis_bits_kernel");
  size_t tb = w.temp_bytes;
  EGC_HIP_TRY(rocprim::radix_sort_keys(temp, tb, (const uint32_t*)u32(w.dbits), u32(w.dbits_sorted), (size_t)n, 0u, 32u, stream));
  gp_unique_flags_kernel<<<nb1, 256, 0, stream>>>((int)n, u32(w.dbits_sorted), u32(w.flags));
  EGC_LAUNCH_CHECK("gp_unique_flags_kernel");
  tb = w.temp_bytes;
  EGC_HIP_TRY(rocprim::exclusive_scan(temp, tb, (const uint32_t*)u32(w.flags), u32(w.pos), 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), stream));
  gp_unique_put_kernel<<<nb, 256, 0, stream>>>((int)n, u32(w.dbits_sorted), u32(w.flags), u32(w.pos), table);
  EGC_LAUNCH_CHECK("gp_unique_put_kernel");
  // every source's index, the header, the packed words
  gp_src_index_kernel<<<nb, 256, 0, stream>>>((int)n, dis, table, u32(w.pos), cb, u32(w.src_idx), plan);
  EGC_LAUNCH_CHECK("gp_src_index_kernel");
  if (e > 0) {
    gp_pack_kernel<<<(int)std::min<int64_t>(ceil_div(e, (int64_t)256), 2048), 256, 0, stream>>>(e, (int)n, graph->col, u32(w.src_idx), u32(w.pos),
                                                                                                  cb, entries);
    EGC_LAUNCH_CHECK("gp_pack_kernel");
  }
  return EGC_OK;
}

}  // extern "C"
