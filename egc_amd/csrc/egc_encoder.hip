// Node encoders: out[n] = ((W_0[idx[n,0]] + W_1[idx[n,1]]) + W_2[idx[n,2]]) + ... over T embedding tables, forward and
// backward.  gfx950 only.  The reference starts every batched net with `x = self.embedding(batch.x)`, embedding =
// nn.Embedding (zinc/models.py:28-29,62-63) | AtomEncoder, nine tables (mol/pna_style_models.py:33-34,66-69) |
// ASTNodeEncoder, three tables and a clamp of the depth index (code/models.py:27-45,104-112), followed by
// `x = self.in_feat_dropout(x)`.
//
// Forward, one launch.  ceil(width / 4) lanes form the group of a node, 256 / lanes groups a workgroup (block = lanes x
// groups, so a thread finds its node and columns without a division by the run-time lane count); a lane owns four
// adjacent columns, reads the node's T indices (one contiguous piece of idx, the same addresses for the whole group)
// and the T table rows (tables total a few MB: L2), adds them in
// ascending table order with one IEEE add each (-ffp-contract=off) and stores once, non-temporally.  An index outside
// [0, R_t) after the clamp is never used as an address: that table contributes a zero row and the sticky host_flag is
// raised.  Optional dropout in the store: out = keep ? sum * scale : 0.
//
// Backward, two launches, no atomics of any kind.  d W_t[v] is a sum of rows of d_out over { n : idx[n,t] = v }: a
// scatter-add whose lists run from nothing to N / 2 rows (a two-row table).  The rows of d_out are the contribution
// rows themselves, so nothing is stored first; what is needed is every destination's list in a fixed order.
//   1. encoder_partial_kernel, one 256-thread workgroup per (table t, chunk c of ENC_CHUNK = 256 consecutive nodes):
//      thread i holds the key of node 256 c + i.  An all-pairs compare over the 256 keys in LDS gives every thread its
//      rank inside its list, the list's length and its first member; one packed scan over the lists' heads gives each
//      list a start in `order` and an ordinal.  order[start + rank] = i groups the chunk's nodes by key, ascending n
//      inside a list, with no counters and no dependence on R_t.  Lane groups then sum one list each, rows ascending,
//      RD_AHEAD loads in flight, and store the sum as partial row  slot = base(t, c) + ordinal.  The workgroup also
//      writes its column of map[ΣR_t][n_chunks]: the slot of every key it met, -1 for every other row of table t.
//   2. encoder_reduce_kernel, one lane group per destination row (t, v): walks map[(t, v)][0 .. n_chunks) and adds the
//      partial rows that exist in ascending chunk order; writes the row of d W_t (zeros when no node indexed it).
// Summation order of every element: ((g[n_1] + g[n_2]) + ...) inside a chunk, n ascending, then ((p[c_1] + p[c_2]) + ...),
// c ascending -- a function of idx and the shapes alone.  Every element of every d W_t is written exactly once.
// Chunk size: the longest chain is max(ENC_CHUNK, N / ENC_CHUNK) dependent adds, 256 / 207 for the molhiv batch of 52,771
// nodes; partial rows are at most n_chunks * sum_t min(ENC_CHUNK, R_t).
// Traffic: a workgroup serves ONE table, so every row of d_out (and of the mask) is read T times -- once from memory, T - 1
// times from the caches when N F 4 bytes fit the Infinity Cache (62 MB for molhiv at 296).
#include "egc_common.h"

namespace egc {

constexpr int ENC_CHUNK = 256;      // nodes per workgroup of the backward's first pass = its thread count
constexpr int ENC_RD_AHEAD = 8;     // rows requested before the first add that consumes them
constexpr int ENC_FWD_BATCH = 4;    // table rows requested together in the forward

struct EncTables {   // by value in the kernel arguments: nothing to upload, records into a hipGraph as it is
  const float* w[EGC_ENCODER_MAX_TABLES];
  float* dw[EGC_ENCODER_MAX_TABLES];
  int32_t rows[EGC_ENCODER_MAX_TABLES];
  int32_t clamp[EGC_ENCODER_MAX_TABLES];
  int32_t row_offset[EGC_ENCODER_MAX_TABLES + 1];    // prefix sums of rows
  int32_t slot_offset[EGC_ENCODER_MAX_TABLES + 1];   // prefix sums of min(ENC_CHUNK, rows): partial rows per chunk
};

// keep ? v * scale : 0 for a lane's four columns (mask bytes of row r; nullptr: no dropout)
template <bool VEC>
__device__ inline f4 enc_drop(f4 v, const uint8_t* __restrict__ keep, float scale, int64_t r, int width, int c) {
  if (keep == nullptr) return v;
  const uint8_t* k = keep + r * width + c;
  uint32_t m = 0;
  if (VEC) {
    m = *reinterpret_cast<const uint32_t*>(k);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < width) m |= (uint32_t)k[j] << (8 * j);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = ((m >> (8 * j)) & 0xffu) ? v[j] * scale : 0.f;
  return v;
}

// the row of table t that node n indexes, or -1 (outside the table after the clamp: nothing is addressed with it)
__device__ inline int enc_key(const int64_t* __restrict__ idx, int64_t n, int n_tables, int t, int rows, int clamp) {
  int64_t v = idx[n * n_tables + t];
  if (clamp >= 0 && v > clamp) v = clamp;
  return (v >= 0 && v < rows) ? (int)v : -1;
}

template <bool VEC>
__global__ void __launch_bounds__(256) encoder_forward_kernel(EncTables tb, int n_tables, const int64_t* __restrict__ idx,
                                                              int64_t n_rows, int width, int lanes,
                                                              const uint8_t* __restrict__ keep, float keep_scale,
                                                              float* __restrict__ out, int32_t* __restrict__ host_flag) {
  // block = (lanes, 256 / lanes): x is the lane of a node's group, y the node -- no division by a run-time lane count
  const int64_t n = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  if (n >= n_rows) return;
  const int c = (int)threadIdx.x * 4;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  bool bad = false;
#pragma unroll 1
  for (int t0 = 0; t0 < n_tables; t0 += ENC_FWD_BATCH) {
    f4 v[ENC_FWD_BATCH];
#pragma unroll
    for (int k = 0; k < ENC_FWD_BATCH; ++k) {
      const int t = min(t0 + k, n_tables - 1);   // past the last table: the last one again, not taken
      const int key = enc_key(idx, n, n_tables, t, tb.rows[t], tb.clamp[t]);
      bad |= key < 0;
      v[k] = key >= 0 ? tm_load<VEC>(tb.w[t] + (int64_t)key * width + c, c, width) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < ENC_FWD_BATCH; ++k) {
      if (t0 + k == 0) acc = v[k];   // the reference's 0 + e_0 is exact
      else if (t0 + k < n_tables) acc += v[k];
    }
  }
  if (bad && c == 0 && host_flag != nullptr) *(volatile int32_t*)host_flag = 1;   // sticky, host-visible
  acc = enc_drop<VEC>(acc, keep, keep_scale, n, width, c);
  float* p = out + n * width + c;
  if (VEC) __builtin_nontemporal_store(acc, reinterpret_cast<f4*>(p));
  else tm_store<false>(p, c, width, acc);
}

// partial rows in front of the rows of workgroup (t, chunk): every table owns n_chunks * min(ENC_CHUNK, rows) of them
__device__ inline int64_t enc_slot_base(const EncTables& tb, int t, int64_t chunk, int64_t n_chunks) {
  return (int64_t)tb.slot_offset[t] * n_chunks + chunk * (tb.slot_offset[t + 1] - tb.slot_offset[t]);
}

template <bool VEC>
__global__ void __launch_bounds__(ENC_CHUNK) encoder_partial_kernel(EncTables tb, int n_tables,
                                                                     const int64_t* __restrict__ idx, int64_t n_rows,
                                                                     int width, int lanes, const float* __restrict__ d_out,
                                                                     const uint8_t* __restrict__ keep, float keep_scale,
                                                                     float* __restrict__ partial, int32_t* __restrict__ map,
                                                                     int64_t n_chunks) {
  __shared__ int s_key[ENC_CHUNK];
  __shared__ int s_scan[2][ENC_CHUNK];
  __shared__ int s_start[ENC_CHUNK];               // by head thread: first position of its list in s_order
  __shared__ unsigned short s_order[ENC_CHUNK];    // the chunk's nodes grouped by key, ascending inside a list
  __shared__ int s_list[ENC_CHUNK];                // by ordinal: start | length << 16  (length <= 256 needs 9 bits)
  const int i = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int t = blockIdx.y;
  const int64_t n = chunk * ENC_CHUNK + i;
  const int rows = tb.rows[t];
  const int key = n < n_rows ? enc_key(idx, n, n_tables, t, rows, tb.clamp[t]) : -1;
  s_key[i] = key;
  // this workgroup's column of the map: -1 everywhere, the lists' slots below (after the barrier: same addresses)
  int32_t* mcol = map + (int64_t)tb.row_offset[t] * n_chunks + chunk;
  for (int v = i; v < rows; v += ENC_CHUNK) mcol[(int64_t)v * n_chunks] = -1;
  __syncthreads();
  int rank = 0, count = 0, head = i;
#pragma unroll 8
  for (int j = 0; j < ENC_CHUNK; ++j) {
    const bool m = s_key[j] == key;
    head = (m && count == 0) ? j : head;
    count += m;
    rank += (m && j < i);
  }
  const bool is_head = key >= 0 && rank == 0;
  // one inclusive scan over (list length << 16 | 1) of the heads: starts in the high half, ordinals in the low half
  const int mine = is_head ? (count << 16 | 1) : 0;
  s_scan[0][i] = mine;
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int d = 1; d < ENC_CHUNK; d <<= 1) {
    const int v = s_scan[cur][i] + (i >= d ? s_scan[cur][i - d] : 0);
    s_scan[cur ^ 1][i] = v;
    cur ^= 1;
    __syncthreads();
  }
  const int excl = s_scan[cur][i] - mine;
  const int n_lists = s_scan[cur][ENC_CHUNK - 1] & 0xffff;
  const int64_t base = enc_slot_base(tb, t, chunk, n_chunks);
  if (is_head) {
    s_start[i] = excl >> 16;
    s_list[excl & 0xffff] = (excl >> 16) | count << 16;
    mcol[(int64_t)key * n_chunks] = (int32_t)(base + (excl & 0xffff));
  }
  __syncthreads();
  if (key >= 0) s_order[s_start[head] + rank] = (unsigned short)i;
  __syncthreads();
  // one lane group per list, rows ascending
  const int g = i / lanes, n_groups = ENC_CHUNK / lanes;
  if (g >= n_groups) return;
  const int c = (i - g * lanes) * 4;
  const int64_t row0 = chunk * ENC_CHUNK;
#pragma unroll 1
  for (int l = g; l < n_lists; l += n_groups) {
    const int start = s_list[l] & 0xffff, len = s_list[l] >> 16;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k0 = 0; k0 < len; k0 += ENC_RD_AHEAD) {
      f4 v[ENC_RD_AHEAD];
#pragma unroll
      for (int k = 0; k < ENC_RD_AHEAD; ++k) {   // past the end: the last row again, not taken
        const int64_t r = row0 + s_order[start + min(k0 + k, len - 1)];
        v[k] = enc_drop<VEC>(tm_load<VEC>(d_out + r * width + c, c, width), keep, keep_scale, r, width, c);
      }
#pragma unroll
      for (int k = 0; k < ENC_RD_AHEAD; ++k) {
        if (k0 + k == 0) acc = v[k];
        else if (k0 + k < len) acc += v[k];
      }
    }
    tm_store<VEC>(partial + (base + l) * width + c, c, width, acc);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) encoder_reduce_kernel(EncTables tb, int n_tables, int width, int lanes,
                                                             const float* __restrict__ partial,
                                                             const int32_t* __restrict__ map, int64_t n_chunks) {
  const int64_t th = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t d = th / lanes;
  if (d >= tb.row_offset[n_tables]) return;
  const int c = (int)(th - d * lanes) * 4;
  int t = 0;
  while (t + 1 < n_tables && d >= tb.row_offset[t + 1]) ++t;
  const int32_t* m = map + d * n_chunks;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  bool any = false;
#pragma unroll 1
  for (int64_t c0 = 0; c0 < n_chunks; c0 += ENC_RD_AHEAD) {
    int32_t slot[ENC_RD_AHEAD];
    f4 v[ENC_RD_AHEAD];
#pragma unroll
    for (int k = 0; k < ENC_RD_AHEAD; ++k) slot[k] = c0 + k < n_chunks ? m[c0 + k] : -1;
#pragma unroll
    for (int k = 0; k < ENC_RD_AHEAD; ++k)
      v[k] = slot[k] >= 0 ? tm_load<VEC>(partial + (int64_t)slot[k] * width + c, c, width) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < ENC_RD_AHEAD; ++k) {
      if (slot[k] >= 0) {
        acc = any ? acc + v[k] : v[k];
        any = true;
      }
    }
  }
  tm_store<VEC>(tb.dw[t] + (d - tb.row_offset[t]) * width + c, c, width, acc);
}

static inline int64_t enc_chunks(int64_t n_rows) { return ceil_div(n_rows, ENC_CHUNK); }

// bytes of the partial rows in front of the map (a multiple of 16)
static inline size_t enc_partial_bytes(int64_t n_chunks, int64_t slots_per_chunk, int32_t width) {
  return ((size_t)n_chunks * slots_per_chunk * width * sizeof(float) + 15) & ~(size_t)15;
}

static int enc_check_shape(int64_t n_rows, int32_t n_tables, int64_t total_rows, int32_t width) {
  if (n_rows < 0 || n_tables <= 0 || total_rows < n_tables || width <= 0) return EGC_ERR_INVALID;
  if (n_tables > EGC_ENCODER_MAX_TABLES || total_rows > EGC_ENCODER_MAX_TABLE_ROWS || width > EGC_ENCODER_MAX_WIDTH ||
      n_rows >= ((int64_t)1 << 31) - ENC_CHUNK || enc_chunks(n_rows) * total_rows >= ((int64_t)1 << 31))
    return EGC_ERR_UNSUPPORTED;
  return EGC_OK;
}

// the by-value table block from the caller's host arrays; total rows in *total
static int enc_tables(const int32_t* table_rows, const int32_t* clamp, int32_t n_tables, int32_t width, int64_t n_rows,
                      EncTables* tb, int64_t* total) {
  if (n_tables <= 0 || table_rows == nullptr) return EGC_ERR_INVALID;
  if (n_tables > EGC_ENCODER_MAX_TABLES) return EGC_ERR_UNSUPPORTED;
  *tb = EncTables{};
  int64_t sum = 0, slots = 0;
  for (int t = 0; t < n_tables; ++t) {
    if (table_rows[t] <= 0) return EGC_ERR_INVALID;
    tb->rows[t] = table_rows[t];
    tb->clamp[t] = clamp != nullptr ? clamp[t] : -1;
    sum += table_rows[t];
    slots += table_rows[t] < ENC_CHUNK ? table_rows[t] : ENC_CHUNK;
    if (sum > EGC_ENCODER_MAX_TABLE_ROWS) return EGC_ERR_UNSUPPORTED;
    tb->row_offset[t + 1] = (int32_t)sum;
    tb->slot_offset[t + 1] = (int32_t)slots;
  }
  *total = sum;
  return enc_check_shape(n_rows, n_tables, sum, width);
}

}  // namespace egc

using namespace egc;

int egc_encoder_forward_f32(const float* const* tables, const int32_t* table_rows, const int32_t* clamp, int32_t n_tables,
                            const int64_t* idx, int64_t n_rows, int32_t width, const uint8_t* keep, float keep_scale,
                            float* out, int32_t* host_flag, egc_stream_t stream_) {
  EncTables tb;
  int64_t total;
  if (tables == nullptr) return EGC_ERR_INVALID;
  if (int rc = enc_tables(table_rows, clamp, n_tables, width, n_rows, &tb, &total)) return rc;
  bool vec = (width & 3) == 0 && aligned16(out) && aligned_to(keep, 4);
  for (int t = 0; t < n_tables; ++t) {
    if (tables[t] == nullptr) return EGC_ERR_INVALID;
    tb.w[t] = tables[t];
    vec = vec && aligned16(tables[t]);
  }
  if (n_rows == 0) return EGC_OK;
  if (idx == nullptr || out == nullptr) return EGC_ERR_INVALID;
  const int lanes = (width + 3) / 4;
  const dim3 block((unsigned)lanes, (unsigned)(256 / lanes));   // lanes <= 256 by EGC_ENCODER_MAX_WIDTH
  const int64_t blocks = ceil_div(n_rows, block.y);
  if (blocks >= ((int64_t)1 << 31)) return EGC_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  if (vec)
    encoder_forward_kernel<true><<<(unsigned)blocks, block, 0, stream>>>(tb, n_tables, idx, n_rows, width, lanes, keep,
                                                                         keep_scale, out, host_flag);
  else
    encoder_forward_kernel<false><<<(unsigned)blocks, block, 0, stream>>>(tb, n_tables, idx, n_rows, width, lanes, keep,
                                                                          keep_scale, out, host_flag);
  EGC_LAUNCH_CHECK("encoder_forward_kernel");
  return EGC_OK;
}

size_t egc_encoder_workspace_bytes(int64_t n_rows, int32_t n_tables, int64_t total_table_rows, int32_t width) {
  if (enc_check_shape(n_rows, n_tables, total_table_rows, width) != EGC_OK || n_rows == 0) return 0;
  const int64_t n_chunks = enc_chunks(n_rows);
  // sum_t min(ENC_CHUNK, R_t) from the two numbers the caller has: at most every row, at most a chunk per table
  const int64_t slots = total_table_rows < (int64_t)ENC_CHUNK * n_tables ? total_table_rows : (int64_t)ENC_CHUNK * n_tables;
  return enc_partial_bytes(n_chunks, slots, width) + (size_t)n_chunks * total_table_rows * sizeof(int32_t);
}

int egc_encoder_backward_f32(const float* d_out, const uint8_t* keep, float keep_scale, const int64_t* idx, int64_t n_rows,
                             int32_t width, const int32_t* table_rows, const int32_t* clamp, int32_t n_tables,
                             float* const* d_tables, void* workspace, size_t workspace_bytes, egc_stream_t stream_) {
  EncTables tb;
  int64_t total;
  if (d_tables == nullptr) return EGC_ERR_INVALID;
  if (int rc = enc_tables(table_rows, clamp, n_tables, width, n_rows, &tb, &total)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  for (int t = 0; t < n_tables; ++t) {
    if (d_tables[t] == nullptr) return EGC_ERR_INVALID;
    tb.dw[t] = d_tables[t];
  }
  if (n_rows == 0) {   // nobody indexes anything: zeros, and no workspace
    for (int t = 0; t < n_tables; ++t)
      EGC_HIP_TRY(hipMemsetAsync(d_tables[t], 0, (size_t)table_rows[t] * width * sizeof(float), stream));
    return EGC_OK;
  }
  if (d_out == nullptr || idx == nullptr) return EGC_ERR_INVALID;
  if (workspace == nullptr || !aligned16(workspace) ||
      workspace_bytes < egc_encoder_workspace_bytes(n_rows, n_tables, total, width))
    return EGC_ERR_WORKSPACE;
  const int64_t n_chunks = enc_chunks(n_rows);
  const int64_t slots = total < (int64_t)ENC_CHUNK * n_tables ? total : (int64_t)ENC_CHUNK * n_tables;
  float* partial = static_cast<float*>(workspace);
  int32_t* map = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + enc_partial_bytes(n_chunks, slots, width));
  const int lanes = (width + 3) / 4;
  bool vec = (width & 3) == 0 && aligned16(d_out) && aligned_to(keep, 4);
  for (int t = 0; t < n_tables; ++t) vec = vec && aligned16(d_tables[t]);
  const dim3 grid1((unsigned)n_chunks, (unsigned)n_tables);
  const int64_t blocks2 = ceil_div(total * lanes, 256);
  if (vec) {
    encoder_partial_kernel<true><<<grid1, ENC_CHUNK, 0, stream>>>(tb, n_tables, idx, n_rows, width, lanes, d_out, keep,
                                                                   keep_scale, partial, map, n_chunks);
    encoder_reduce_kernel<true><<<(unsigned)blocks2, 256, 0, stream>>>(tb, n_tables, width, lanes, partial, map, n_chunks);
  } else {
    encoder_partial_kernel<false><<<grid1, ENC_CHUNK, 0, stream>>>(tb, n_tables, idx, n_rows, width, lanes, d_out, keep,
                                                                    keep_scale, partial, map, n_chunks);
    encoder_reduce_kernel<false><<<(unsigned)blocks2, 256, 0, stream>>>(tb, n_tables, width, lanes, partial, map, n_chunks);
  }
  EGC_LAUNCH_CHECK("encoder_backward kernels");
  return EGC_OK;
}
