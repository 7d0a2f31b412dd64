// Device-side collation of a mini-batch out of a dataset that lives in device memory, into the static padded buffers a
// recorded training step reads.  gfx950 only.  In the reference the batch comes from PyG's DataLoader -- per-graph Python
// collation on the CPU, then `batch.to(device)` (zinc/configs.py:53-67, mol/configs.py:52-70, cifar/configs.py:66-82,
// code/configs.py:47-69); here one call writes the whole padded batch, with no host work, so that it records into the
// step's hipGraph.  Layout of every output: include/egc_hip.h (egc_collate), DESIGN.md section 3.31.
//
// Two launches, whatever the number of fields.
//   1. collate_header_kernel, ONE workgroup of 1024 threads.  Slot i of the batch is graph ids[i] (or perm[cursor * G + i],
//      cursor and permutation length read on the device).  In passes of 1024 slots: a thread loads its graph's node and
//      edge range (an id outside [0, M) is an empty slot and raises bit 1), the counts go through a block-wide inclusive
//      scan in LDS (int64, Hillis-Steele, carried from pass to pass), and the capacity cut is read off the prefix sums:
//      they are monotone, so "the first graph that does not fit and every graph after it" is { i : incl_n[i] > n_pad - 1 or
//      incl_e[i] > e_pad }, and the one slot whose predecessor still fits names the cause (bits 2 / 4).  Written: ptr,
//      edge_ptr, the three counts, counts, graph_mask, inv_g, the per-slot record (source node offset, source edge offset,
//      source graph or -1) in the workspace, the bumped cursor, the status bits and host_flag.
//   2. collate_copy_kernel, destination-driven: every output element has exactly one writer and the padding needs no
//      second pass.  The grid is cut on the host from n_pad, e_pad and G alone (never from the batch) into workgroups of
//      256 destination rows, 1024 destination edge columns and 256 graph slots.  A row / edge workgroup stages ptr /
//      edge_ptr (at most 4098 entries, as int32: n_pad and e_pad are below 2^31) in LDS and each thread bisects there for
//      the slot that owns its row or column.  Node fields: the workgroup keeps the source row of each of its 256 rows in
//      LDS (-1: padding), then walks every field in units of 16, 8 or 4 bytes -- the widest that divides the row size and
//      both base addresses, chosen on the host, so that a unit never leaves its row and source and destination units are
//      aligned alike whatever row a graph starts at; consecutive lanes take consecutive destination units, which are
//      consecutive source units inside a graph.  Edges: both rows read as int64, the slot's node offset added.  Graph
//      fields: a gathered row or the field's fill element.
// Bound by: launch and dependent-load latency, not bandwidth -- the molhiv batch of 2,048 graphs moves about 6 MB, a
// microsecond of HBM time; the header launch is a chain of two dependent loads and twenty LDS barriers per pass, the copy
// launch one staging round, a bisection in LDS and one gather.  Plain C++ stores throughout, no float atomics; the one
// integer atomic is an LDS `or` that gathers the header's status bits.
#include "egc_common.h"

namespace egc {

constexpr int COL_HDR_THREADS = 1024;   // slots per pass of the header's scan
constexpr int COL_THREADS = 256;        // copy workgroup; destination rows / graph slots per workgroup
constexpr int COL_EDGE_COLS = 1024;     // destination edge columns per workgroup
constexpr int COL_NO_CUT = 0x7fffffff;

struct ColArgs {   // by value in the kernel arguments: nothing to upload, records into a hipGraph as it is
  egc_collate_store st;
  egc_collate_out out;
  const int64_t* ids;
  int64_t n_ids;
  const int64_t* perm;
  const int64_t* perm_len;
  int64_t* cursor;
  int64_t* ws;   // [3 G]: source node offset | source edge offset | source graph (-1: none) per slot
  int32_t* host_flag;
  int64_t n_pad, e_pad;
  int32_t G;
  int32_t n_node, n_graph;
  int32_t node_unit[EGC_COLLATE_MAX_FIELDS];
  egc_collate_field node[EGC_COLLATE_MAX_FIELDS];
  egc_collate_field graph[EGC_COLLATE_MAX_FIELDS];
};

__global__ void __launch_bounds__(COL_HDR_THREADS) collate_header_kernel(ColArgs a) {
  __shared__ int64_t sn[COL_HDR_THREADS], se[COL_HDR_THREADS];
  __shared__ int64_t cut_n, cut_e;
  __shared__ int cut_slot, flags;
  const int tid = (int)threadIdx.x, G = a.G;
  const int64_t M = a.st.n_graphs;
  const int64_t* ids = a.ids;
  int64_t k = a.n_ids, next_cursor = 0;
  if (ids == nullptr) {   // cursor mode: full batches only (drop-last); past the last one, back to 0
    int64_t len = *a.perm_len;
    len = len < 0 ? 0 : (len > M ? M : len);
    const int64_t batches = len / G;
    int64_t c = *a.cursor;
    if (c < 0 || c >= batches) c = 0;
    ids = a.perm + c * G;
    k = batches > 0 ? G : 0;
    next_cursor = c + 1;
  }
  if (tid == 0) {
    cut_slot = COL_NO_CUT;
    cut_n = cut_e = 0;
    flags = 0;
  }
  __syncthreads();   // (also: every thread has read the cursor before thread 0 writes it below)
  const int64_t cap_n = a.n_pad - 1, cap_e = a.e_pad;
  int64_t carry_n = 0, carry_e = 0;
#pragma unroll 1
  for (int base = 0; base < G; base += COL_HDR_THREADS) {
    const int slot = base + tid;
    int64_t n = 0, e = 0, src_n = 0, src_e = 0, gid = -1;
    if (slot < k) {
      const int64_t id = ids[slot];
      if (id >= 0 && id < M) {
        src_n = a.st.node_ptr[id];
        src_e = a.st.edge_ptr[id];
        n = a.st.node_ptr[id + 1] - src_n;
        e = a.st.edge_ptr[id + 1] - src_e;
        n = n < 0 ? 0 : n;
        e = e < 0 ? 0 : e;
        gid = id;
      } else {
        atomicOr(&flags, 1);
      }
    }
    sn[tid] = n;
    se[tid] = e;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < COL_HDR_THREADS; off <<= 1) {
      const int64_t vn = tid >= off ? sn[tid - off] : 0, ve = tid >= off ? se[tid - off] : 0;
      __syncthreads();
      sn[tid] += vn;
      se[tid] += ve;
      __syncthreads();
    }
    const int64_t incl_n = carry_n + sn[tid], incl_e = carry_e + se[tid];
    const int64_t excl_n = incl_n - n, excl_e = incl_e - e;
    carry_n += sn[COL_HDR_THREADS - 1];
    carry_e += se[COL_HDR_THREADS - 1];
    const bool fail = incl_n > cap_n || incl_e > cap_e;
    if (fail && !(excl_n > cap_n || excl_e > cap_e)) {   // the first slot that does not fit: one thread in the whole call
      cut_slot = slot;
      cut_n = excl_n;
      cut_e = excl_e;
      atomicOr(&flags, (incl_n > cap_n ? 2 : 0) | (incl_e > cap_e ? 4 : 0));
    }
    __syncthreads();   // the cut is visible; sn / se are free for the next pass
    if (slot < G) {
      const bool valid = slot < k && slot < cut_slot;
      a.out.ptr[slot] = slot < cut_slot ? excl_n : cut_n;
      a.out.edge_ptr[slot] = slot < cut_slot ? excl_e : cut_e;
      a.out.counts[slot] = valid && n > 0 ? (float)n : 1.f;
      a.out.graph_mask[slot] = valid ? 1.f : 0.f;
      a.ws[slot] = valid ? src_n : 0;
      a.ws[G + slot] = valid ? src_e : 0;
      a.ws[2 * (int64_t)G + slot] = valid ? gid : -1;
    }
  }
  if (tid == 0) {
    const bool cut = cut_slot != COL_NO_CUT;
    const int64_t n_valid = cut ? cut_n : carry_n, e_valid = cut ? cut_e : carry_e;
    const int64_t g_valid = cut ? (int64_t)cut_slot : k;
    a.out.ptr[G] = n_valid;
    a.out.ptr[G + 1] = a.n_pad;
    a.out.edge_ptr[G] = e_valid;
    a.out.edge_ptr[G + 1] = a.e_pad;
    *a.out.n_valid = n_valid;
    *a.out.e_valid = e_valid;
    *a.out.g_valid = g_valid;
    a.out.counts[G] = 1.f;
    a.out.graph_mask[G] = 0.f;
    *a.out.inv_g = (float)(1.0 / (double)(g_valid > 0 ? g_valid : 1));
    if (a.ids == nullptr) *a.cursor = next_cursor;
    if (flags != 0) {
      *a.out.status |= flags;   // sticky until BatchCollator.check() clears it; one workgroup, stream-ordered: no race
      if (a.host_flag != nullptr) *(volatile int32_t*)a.host_flag = 1;
    }
  }
}

// the slot s in [0, G] with p[s] <= r < p[s + 1]  (p[0] = 0 <= r < p[G + 1]; empty slots repeat their offset and are skipped)
__device__ inline int col_slot_of(const int32_t* p, int G, int32_t r) {
  int lo = 0, hi = G + 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// `total` units of sizeof(T) bytes, `upr` of them per row, for the workgroup's rows: dst is the first of these rows;
// row_src[i] is the source row of local row i, or -1 = write `fill`
template <typename T>
__device__ inline void col_copy_units(const char* __restrict__ src, char* __restrict__ dst, int64_t row_bytes, unsigned upr,
                                      unsigned total, const int64_t* row_src, T fill) {
  for (unsigned i = threadIdx.x; i < total; i += COL_THREADS) {
    const unsigned rl = i / upr;
    const int64_t sr = row_src[rl];
    T v = fill;
    if (sr >= 0) v = *reinterpret_cast<const T*>(src + sr * row_bytes + (size_t)(i - rl * upr) * sizeof(T));
    *reinterpret_cast<T*>(dst + (size_t)i * sizeof(T)) = v;
  }
}

__global__ void __launch_bounds__(COL_THREADS) collate_copy_kernel(ColArgs a, int node_blocks, int edge_blocks) {
  __shared__ int32_t sp[EGC_COLLATE_MAX_GRAPHS + 2];
  __shared__ int64_t row_src[COL_THREADS];
  const int tid = (int)threadIdx.x, G = a.G;
  const int b = (int)blockIdx.x;
  if (b < node_blocks + edge_blocks) {
    const int64_t* p = b < node_blocks ? a.out.ptr : a.out.edge_ptr;
    for (int i = tid; i < G + 2; i += COL_THREADS) sp[i] = (int32_t)p[i];
    __syncthreads();
  }
  if (b < node_blocks) {
    const int64_t r0 = (int64_t)b * COL_THREADS, r = r0 + tid;
    int64_t sr = -1;
    if (r < a.n_pad) {
      const int s = col_slot_of(sp, G, (int32_t)r);   // G: the spare graph that owns the padding rows
      if (s < G) sr = a.ws[s] + (r - sp[s]);
      a.out.batch[r] = s;
    }
    row_src[tid] = sr;
    __syncthreads();
    const unsigned rows = (unsigned)(a.n_pad - r0 < COL_THREADS ? a.n_pad - r0 : COL_THREADS);
#pragma unroll 1
    for (int f = 0; f < a.n_node; ++f) {
      const int64_t rb = a.node[f].row_bytes;
      const char* src = static_cast<const char*>(a.node[f].src);
      char* dst = static_cast<char*>(a.node[f].dst) + r0 * rb;
      const unsigned unit = (unsigned)a.node_unit[f], upr = (unsigned)rb / unit;
      if (unit == 16) col_copy_units<u32x4>(src, dst, rb, upr, rows * upr, row_src, u32x4{0u, 0u, 0u, 0u});
      else if (unit == 8) col_copy_units<uint64_t>(src, dst, rb, upr, rows * upr, row_src, (uint64_t)0);
      else col_copy_units<uint32_t>(src, dst, rb, upr, rows * upr, row_src, 0u);
    }
  } else if (b < node_blocks + edge_blocks) {
    const int64_t c0 = (int64_t)(b - node_blocks) * COL_EDGE_COLS;
    const int64_t* ei0 = a.st.edge_index;
    const int64_t* ei1 = a.st.edge_index + a.st.n_edges_all;
#pragma unroll
    for (int j = 0; j < COL_EDGE_COLS / COL_THREADS; ++j) {
      const int64_t c = c0 + j * COL_THREADS + tid;
      if (c < a.e_pad) {
        const int s = col_slot_of(sp, G, (int32_t)c);
        int64_t v0 = a.n_pad - 1, v1 = a.n_pad - 1;   // padding: self-loops on the last row
        if (s < G) {
          const int64_t sc = a.ws[G + s] + (c - sp[s]), off = a.out.ptr[s];
          v0 = ei0[sc] + off;
          v1 = ei1[sc] + off;
        }
        a.out.edge_index[c] = v0;
        a.out.edge_index[a.e_pad + c] = v1;
      }
    }
  } else {
    const int s0 = (b - node_blocks - edge_blocks) * COL_THREADS;
    row_src[tid] = s0 + tid < G ? a.ws[2 * (int64_t)G + s0 + tid] : -1;   // slot G, the spare graph: the fill
    __syncthreads();
    const unsigned slots = (unsigned)(G + 1 - s0 < COL_THREADS ? G + 1 - s0 : COL_THREADS);
#pragma unroll 1
    for (int f = 0; f < a.n_graph; ++f) {
      const int64_t rb = a.graph[f].row_bytes;
      const char* src = static_cast<const char*>(a.graph[f].src);
      char* dst = static_cast<char*>(a.graph[f].dst) + (int64_t)s0 * rb;
      const unsigned unit = (unsigned)a.graph[f].elem_bytes, upr = (unsigned)rb / unit;
      if (unit == 8) col_copy_units<uint64_t>(src, dst, rb, upr, slots * upr, row_src, a.graph[f].fill_bits);
      else col_copy_units<uint32_t>(src, dst, rb, upr, slots * upr, row_src, (uint32_t)a.graph[f].fill_bits);
    }
  }
}


static int col_check_field(const egc_collate_field& f) {
  if (f.src == nullptr || f.dst == nullptr) return EGC_ERR_INVALID;
  if (f.elem_bytes != 4 && f.elem_bytes != 8) return EGC_ERR_UNSUPPORTED;
  if (f.row_bytes <= 0 || f.row_bytes % f.elem_bytes != 0) return EGC_ERR_INVALID;
  if (f.row_bytes > EGC_COLLATE_MAX_ROW_BYTES) return EGC_ERR_UNSUPPORTED;
  if (!aligned_to(f.src, (uintptr_t)f.elem_bytes) || !aligned_to(f.dst, (uintptr_t)f.elem_bytes)) return EGC_ERR_INVALID;
  return EGC_OK;
}

}  // namespace egc

using namespace egc;

size_t egc_collate_workspace_bytes(int32_t batch_size) {
  if (batch_size <= 0 || batch_size > EGC_COLLATE_MAX_GRAPHS) return 0;
  return (size_t)batch_size * 3 * sizeof(int64_t);
}

int egc_collate(const egc_collate_store* store, const egc_collate_fields* fields, const egc_collate_out* out,
                const int64_t* ids, int64_t n_ids, const int64_t* perm, const int64_t* perm_len, int64_t* cursor,
                int32_t batch_size, int64_t n_pad, int64_t e_pad, void* workspace, size_t workspace_bytes,
                int32_t* host_flag, egc_stream_t stream_) {
  if (store == nullptr || fields == nullptr || out == nullptr) return EGC_ERR_INVALID;
  if (store->node_ptr == nullptr || store->edge_ptr == nullptr || store->n_graphs < 0 || store->n_edges_all < 0 ||
      (store->edge_index == nullptr && store->n_edges_all > 0))
    return EGC_ERR_INVALID;
  if (out->edge_index == nullptr || out->batch == nullptr || out->ptr == nullptr || out->edge_ptr == nullptr ||
      out->n_valid == nullptr || out->e_valid == nullptr || out->g_valid == nullptr || out->counts == nullptr ||
      out->graph_mask == nullptr || out->inv_g == nullptr || out->status == nullptr)
    return EGC_ERR_INVALID;
  if (batch_size <= 0 || n_pad < 1 || e_pad < 1) return EGC_ERR_INVALID;
  if (batch_size > EGC_COLLATE_MAX_GRAPHS || n_pad >= ((int64_t)1 << 31) || e_pad >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  if (ids != nullptr ? (n_ids < 1 || n_ids > batch_size) : (perm == nullptr || perm_len == nullptr || cursor == nullptr))
    return EGC_ERR_INVALID;
  if (fields->n_node < 0 || fields->n_graph < 0) return EGC_ERR_INVALID;
  if (fields->n_node > EGC_COLLATE_MAX_FIELDS || fields->n_graph > EGC_COLLATE_MAX_FIELDS) return EGC_ERR_UNSUPPORTED;
  if (workspace == nullptr || !aligned_to(workspace, 8) || workspace_bytes < egc_collate_workspace_bytes(batch_size))
    return EGC_ERR_WORKSPACE;
  ColArgs a = {};
  a.st = *store;
  a.out = *out;
  a.ids = ids;
  a.n_ids = n_ids;
  a.perm = perm;
  a.perm_len = perm_len;
  a.cursor = cursor;
  a.ws = static_cast<int64_t*>(workspace);
  a.host_flag = host_flag;
  a.n_pad = n_pad;
  a.e_pad = e_pad;
  a.G = batch_size;
  a.n_node = fields->n_node;
  a.n_graph = fields->n_graph;
  for (int f = 0; f < fields->n_node; ++f) {
    const egc_collate_field& fd = fields->node[f];
    if (int rc = col_check_field(fd)) return rc;
    a.node[f] = fd;
    int unit = 4;   // the widest access that divides the row and both base addresses: a unit never leaves its row
    if (fd.row_bytes % 16 == 0 && aligned16(fd.src) && aligned16(fd.dst)) unit = 16;
    else if (fd.row_bytes % 8 == 0 && aligned_to(fd.src, 8) && aligned_to(fd.dst, 8)) unit = 8;
    a.node_unit[f] = unit;
  }
  for (int f = 0; f < fields->n_graph; ++f) {
    if (int rc = col_check_field(fields->graph[f])) return rc;
    a.graph[f] = fields->graph[f];
  }
  const int64_t node_blocks = ceil_div(n_pad, (int64_t)COL_THREADS), edge_blocks = ceil_div(e_pad, (int64_t)COL_EDGE_COLS);
  const int64_t graph_blocks = fields->n_graph > 0 ? ceil_div((int64_t)batch_size + 1, (int64_t)COL_THREADS) : 0;
  hipStream_t stream = (hipStream_t)stream_;
  collate_header_kernel<<<1, COL_HDR_THREADS, 0, stream>>>(a);
  collate_copy_kernel<<<(unsigned)(node_blocks + edge_blocks + graph_blocks), COL_THREADS, 0, stream>>>(a, (int)node_blocks,
                                                                                                        (int)edge_blocks);
  EGC_LAUNCH_CHECK("collate kernels");
  return EGC_OK;
}
