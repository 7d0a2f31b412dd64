/*
 * egc_hip.h -- C ABI of libegc_hip.so: the MI355X (gfx950) native hot path of the EGC layer.
 *
 * This is the drop-in boundary.  The reference
 * (shyam196/egc) is pure Python; its layer classes reach native code only
 * through third-party torch extensions.  Each entry point below names the
 * reference call site(s) whose native work it replaces.  All pointers are
 * DEVICE pointers unless stated otherwise; all float tensors are fp32,
 * contiguous, row-major; indices handed IN are int64 (PyG edge_index), indices
 * held by the library's CSR are int32.  No torch types cross this boundary.
 * Nothing here allocates, frees or synchronises: every launch goes to the
 * caller's stream and is safe to capture into a hipGraph.
 *
 * Error convention: every function returns an egc_status (0 = ok).  The Python
 * host (egc_amd/_C.py) turns non-zero codes into RuntimeError, mirroring
 * TORCH_CHECK failures of the torch_scatter / torch_sparse ops it replaces.
 */
#ifndef EGC_HIP_H
#define EGC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* egc_stream_t; /* a hipStream_t */

typedef enum {
  EGC_OK = 0,
  EGC_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, unknown enum, shape limits) */
  EGC_ERR_WORKSPACE = 2,   /* caller workspace too small */
  EGC_ERR_HIP = 3,         /* a HIP runtime call / launch failed; see egc_last_error() */
  EGC_ERR_UNSUPPORTED = 4  /* valid request outside the implemented envelope */
} egc_status;

/* Aggregators: union of layers.py:154-159 (add, mean, max, min, symadd, var, std) and
 * optimized_layers.py:92-94 (sum, mean, symnorm, min, max, var, std). */
typedef enum {
  EGC_AGGR_SUM = 0, EGC_AGGR_MEAN = 1, EGC_AGGR_MAX = 2, EGC_AGGR_MIN = 3,
  EGC_AGGR_VAR = 4, EGC_AGGR_STD = 5, EGC_AGGR_SYMNORM = 6
} egc_aggr;

/* Which edge set an aggregator reduces over (SURVEY.md 8a note 2):
 *   RAW    -- the CSR entries as given (duplicates and self-loops included);
 *   LOOPED -- the CSR entries minus every self-loop, plus exactly one self-loop per node
 *             (what gcn_norm / add_remaining_self_loops / fill_diag produce). */
typedef enum { EGC_SET_RAW = 0, EGC_SET_LOOPED = 1 } egc_edge_set;

/* Column order of the per-node weightings row:
 *   HBA: column = h*B*A + b*A + a   (EfficientGraphConv, layers.py:127-129)
 *   HAB: column = h*A*B + a*B + b   (EGConv, optimized_layers.py:195-202) */
typedef enum { EGC_LAYOUT_HBA = 0, EGC_LAYOUT_HAB = 1 } egc_weight_layout;

/* Nonlinearity on the weightings (layers.py:112-125, optimized_layers.py:183-184).
 * SOFTMAX is over the joint B*A axis per head. */
typedef enum { EGC_ACT_NONE = 0, EGC_ACT_SOFTMAX = 1, EGC_ACT_SIGMOID = 2, EGC_ACT_HARDTANH = 3 } egc_weight_act;

#define EGC_MAX_AGGRS 8
#define EGC_MAX_BASIS_WIDTH 1024   /* B * (F_out / H) */
#define EGC_MAX_WEIGHT_WIDTH 2048  /* H * B * A */
#define EGC_MAX_OUT_CHANNELS 2048

/* Rows with more than EGC_LONG_ROW_THRESHOLD entries are handled by whole wavefronts, in chunks of
 * EGC_LONG_ROW_CHUNK entries by separate wavefronts and merged (degree-skew handling). */
#define EGC_LONG_ROW_THRESHOLD 64
#define EGC_LONG_ROW_CHUNK 256

/* ------------------------------------------------------------------------------------------
 * Graph: CSR keyed by DESTINATION, entries of one row kept in input (edge_index) order.
 * Replaces torch_sparse.SparseTensor storage (rowptr / col; experiments/utils.py:107-113),
 * the gather index of MessagePassing.propagate and the degree pass of gcn_norm.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int64_t n_nodes;
  int64_t n_edges;
  const int32_t* rowptr;      /* [n_nodes+1] */
  const int32_t* col;         /* [n_edges] source node of each entry */
  const int32_t* edge_id;     /* [n_edges] position of the entry in the input edge list; may be NULL */
  const float* dis_raw;       /* [n_nodes] indeg^-1/2 over RAW entries (0 where indeg==0); NULL if unused */
  const float* dis_looped;    /* [n_nodes] (non-self indeg + 1)^-1/2; NULL if unused */
  const int32_t* max_index;   /* device scalar: largest node id present in edge_index (-1 if none) */
  const int32_t* plan;        /* [egc_plan_ints(n_nodes,n_edges)] long-row work plan from egc_csr_prepare */
  int64_t n_chunks;           /* HOST copy of plan[1] (number of long-row chunks) if the caller has read it
                                 back, else -1: the launch is then sized for the plan's capacity */
  int64_t n_src_rows;         /* rows of the tables that `col` indexes (bases, dis_*): n_nodes on one GPU; in a
                                 vertex-partitioned run the owned rows come first and the halo rows received
                                 from other ranks follow (n_src_rows >= n_nodes).  0 means n_nodes.  A rectangular
                                 adjacency between two node types (relational EGC, rmag/models.py:131-134) may have
                                 any n_src_rows > 0, with the RAW edge set and without symnorm. */
  const float* edge_dis_raw;  /* [n_edges] dis_raw[col[p]] per CSR entry, or NULL: the source-side deg^-1/2 factor of the
                                 symnorm weight laid out in traversal order (egc_csr_edge_dis), so that the aggregate
                                 kernel streams it instead of gathering 4 bytes per entry; the weight itself,
                                 dis[src] * dis[dst], is still formed in the kernel */
  const float* edge_dis_looped; /* [n_edges] the same for dis_looped, or NULL */
  const int32_t* gather_plan_raw;    /* egc_gather_plan_build(EGC_SET_RAW) of a STATIC graph, or NULL = no plan: col and
                                        edge_dis_raw of every entry in ONE word, which the inference aggregate streams instead */
  const int32_t* gather_plan_looped; /* the same for EGC_SET_LOOPED, or NULL */
  int32_t gather_plan_form_raw;      /* HOST copies of two header words of the plans, read back once by the caller:
                                        header[EGC_GP_FORM] | header[EGC_GP_COL_BITS] << 8; 0 = no plan */
  int32_t gather_plan_form_looped;
  /* The library reads every field of this struct: a caller ZERO-INITIALISES it (egc_graph g = {0};) and then fills in what it
   * has, so that fields it does not know -- the trailing ones a newer header adds -- mean "absent". */
} egc_graph;

/* int32 words the caller must allocate for egc_graph.plan. */
int64_t egc_plan_ints(int64_t n_nodes, int64_t n_edges);

/* Bytes of scratch egc_coo_to_csr needs (device). */
size_t egc_coo_to_csr_workspace_bytes(int64_t n_nodes, int64_t n_edges);

/* COO (edge_index[0]=src, edge_index[1]=dst, int64, any order, duplicates and self-loops allowed)
 * -> CSR by destination with a STABLE order inside each row.  Replaces the per-call
 * index_select/scatter index handling of MessagePassing.propagate (layers.py:191-193,
 * optimized_layers.py:191-193) and ToSparseTensor (experiments/utils.py:95-113).
 * Writes rowptr[n_nodes+1], col[n_edges], edge_id[n_edges], max_index[1].
 * Returns EGC_ERR_INVALID if n_nodes or n_edges >= 2^31.  Out-of-range node ids are NOT detected by this entry
 * (egc_coo_to_csr_checked is the one the host side of this repository calls). */
int egc_coo_to_csr(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes,
                   int32_t* rowptr, int32_t* col, int32_t* edge_id, int32_t* max_index,
                   void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* The same conversion with every node id RANGE-CHECKED, as egc_graph_build does it: an edge whose source is outside
 * [0, n_src_rows) (0 = n_nodes) or whose destination is outside [0, n_nodes) is dropped -- it sorts behind the last row,
 * rowptr[n_nodes] is the number of edges kept, col / edge_id behind it are defined (0 / undefined order) and never
 * referenced by a row -- and two flags are raised: *status (device int32, written by every call: 0 or 1) and, when
 * given, *host_flag = 1 (a STICKY word in host-visible memory, e.g. hipHostMalloc'ed: never cleared by the library, so
 * the host can poll it without synchronising the stream and report the error at its next call -- the reference's PyG
 * path raises at index_select, optimized_layers.py:191-193).  Same workspace as egc_coo_to_csr. */
int egc_coo_to_csr_checked(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes, int64_t n_src_rows,
                           int32_t* rowptr, int32_t* col, int32_t* edge_id, int32_t* max_index, int32_t* status,
                           int32_t* host_flag, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* One call for a per-batch graph: COO -> CSR by destination (stable inside a row) + both deg^-1/2 tables + their
 * per-entry copies + the long-row plan, in five launches and without a library sort -- what egc_coo_to_csr +
 * egc_csr_prepare + egc_csr_edge_dis produce in a dozen (five launches: histogram, block sums, scan, scatter, rows).  Replaces the same reference call sites (per-batch
 * index handling of MessagePassing.propagate: zinc/models.py:60-74, mol/pna_style_models.py:64-79,
 * cifar/models.py:61-75; gcn_norm's degree pass).  Node ids are RANGE-CHECKED here: an edge whose source is outside
 * [0, n_src_rows) or whose destination is outside [0, n_nodes) is dropped and *status (device int32, written by
 * every call: 0 or 1) is set -- the PyG path behind optimized_layers.py:191-193 raises on such an index; the host side
 * reads the flag at its next synchronisation point (CSRGraph.check_indices); host_flag (may be NULL) is the sticky
 * host-visible word of egc_coo_to_csr_checked, polled without a synchronisation.  rowptr[n_nodes] is then the number
 * of edges kept; col / edge_id / edge_dis_* behind it are written with harmless values (0 / INT32_MAX / 0), and
 * egc_csr_transposed_coo emits (-1, -1) for those positions, which the transposed graph's build drops again.
 * n_src_rows = 0 means n_nodes.  dis_* / edge_dis_* may be NULL (skipped).
 * Workspace: egc_graph_build_workspace_bytes() bytes, zero-filled before its FIRST use; every call leaves ALL of it
 * zero again, so one buffer (of the largest size needed) serves graphs of any size on the same stream.  Scratch:
 * egc_graph_build_scratch_bytes() bytes, any content (sort area of rows longer than 4096 entries).
 * Limits: n_nodes, n_edges < 2^30. */
size_t egc_graph_build_workspace_bytes(int64_t n_nodes, int64_t n_edges);
size_t egc_graph_build_scratch_bytes(int64_t n_edges);
int egc_graph_build(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes, int64_t n_src_rows,
                    int32_t* rowptr, int32_t* col, int32_t* edge_id, int32_t* max_index, float* dis_raw,
                    float* dis_looped, float* edge_dis_raw, float* edge_dis_looped, int32_t* plan, int32_t* status,
                    int32_t* host_flag, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                    egc_stream_t stream);

/* Degree statistics + long-row plan for an existing CSR.  Replaces gcn_norm's degree scatter and
 * pow(-0.5) (layers.py:173-178, optimized_layers.py:131-137) -- the per-edge weight
 * dis[src]*dis[dst] is formed inside the aggregate kernel, never materialised.
 * dis_raw / dis_looped may be NULL (skipped). */
int egc_csr_prepare(int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* col,
                    float* dis_raw, float* dis_looped, int32_t* plan, egc_stream_t stream);

/* The CSR as the COO input of its TRANSPOSE's build: out_src[p] = the row that holds entry p, out_dst[p] = col[p]
 * (int64, as egc_graph_build / egc_coo_to_csr take them).  The backward's source-side pass walks the transposed graph
 * (autograd of the gather behind MessagePassing.propagate, optimized_layers.py:191-193); entry order is kept, so
 * the transposed graph's edge_id is the CSR position the arg comparisons need. */
int egc_csr_transposed_coo(int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* col, int64_t* out_src,
                           int64_t* out_dst, egc_stream_t stream);

/* Per-entry copies of the source-side deg^-1/2 (egc_graph.edge_dis_*): out[p] = dis[col[p]].  Call after the
 * dis_* arrays are final (on a vertex partition: after their halo entries have arrived).  Either pair may be NULL. */
int egc_csr_edge_dis(int64_t n_edges, const int32_t* col, const float* dis_raw, const float* dis_looped,
                     float* edge_dis_raw, float* edge_dis_looped, egc_stream_t stream);

/* Gather plan of a STATIC graph (egc_graph.gather_plan_*): per CSR entry the inference aggregate streams col (4 B) and
 * edge_dis (4 B), yet edge_dis[p] = dis[col[p]] is one of a few hundred distinct floats.  The plan holds both in one word per
 * entry, at the entry's CSR position (rows are found through rowptr as ever) -- built once per graph and edge set, on the
 * device, no synchronisation:
 *   header   EGC_GP_HEADER_INTS words (EGC_GP_* below)
 *   table    the distinct values of the edge set's deg^-1/2 table, ascending by bit pattern: table[index] IS dis[source]
 *   entries  [n_edges] words: bits [0, cb) = col[p], the bits above = index of dis[col[p]] in `table`
 * cb = max(ceil(log2(n_nodes)), 1, min_col_bits) (min_col_bits > 0 only widens it: tests).  Where the distinct values do not
 * fit the 32 - cb spare bits the header says EGC_GP_UNFIT, `entries` is not written, and a launch given that form walks col
 * and edge_dis as it does without a plan.  Requires a square graph (n_src_rows == n_nodes) whose dis table of `edge_set` is
 * final: rebuild the plan whenever that table changes. */
#define EGC_GP_HEADER_INTS 16
#define EGC_GP_FORM 0            /* EGC_GP_PACKED / EGC_GP_UNFIT */
#define EGC_GP_COL_BITS 1        /* cb */
#define EGC_GP_TABLE_SIZE 2      /* distinct dis values */
#define EGC_GP_PACKED 1
#define EGC_GP_UNFIT 2
size_t egc_gather_plan_bytes(int64_t n_nodes, int64_t n_edges);
size_t egc_gather_plan_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int egc_gather_plan_build(const egc_graph* graph, int32_t edge_set, int32_t min_col_bits, int32_t* plan, size_t plan_bytes,
                          void* workspace, size_t workspace_bytes, egc_stream_t stream);
/* The builder's decision as a host function: header[EGC_GP_FORM] | header[EGC_GP_COL_BITS] << 8 of a plan over n_nodes sources
 * whose dis table has n_table distinct values: packed iff cb < 32 and n_table <= 2^(32 - cb). */
int32_t egc_gather_plan_form(int64_t n_nodes, int64_t n_table, int32_t min_col_bits);
/* int32 offset of a part of the plan (0 table, 1 entries; 2 = the plan's end): a function of the sizes alone */
int64_t egc_gather_plan_offset(int64_t n_nodes, int64_t n_edges, int32_t part);
/* Launches of the aggregate's PLAN form issued by this process so far (a diagnostic: tests assert that a launch took the form). */
int64_t egc_gather_plan_launches(void);

/* Vertex-partitioned runs (the reference is single-device, so there is no call site to cite beyond the
 * gather of MessagePassing.propagate this distributes): out[k][0..width) = table[idx[k]][0..width) -- the SEND PACK of
 * the halo all-to-all-v (the rows of `bases` other ranks read, grouped by destination rank), one launch.  width and ld
 * (row stride of table, floats) multiples of 4; table and out 16-byte aligned; idx int64 row ids. */
int egc_gather_rows_f32(const float* table, int64_t ld, const int64_t* idx, int64_t n_rows, int32_t width, float* out,
                        egc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layer description (the arguments of EfficientGraphConv.__init__ layers.py:13-27 /
 * EGConv.__init__ optimized_layers.py:74-86 that shape the computation).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t in_channels;
  int32_t out_channels;
  int32_t num_heads;
  int32_t num_bases;
  int32_t num_aggrs;
  int32_t aggrs[EGC_MAX_AGGRS];   /* egc_aggr codes, in the layer's aggregator order */
  int32_t agg_set;                /* egc_edge_set for sum/mean/max/min/var/std */
  int32_t sym_set;                /* egc_edge_set for symnorm */
  int32_t loops_all_nodes;        /* LOOPED self-loop for every node (1) or only ids <= *max_index (0):
                                     add_remaining_self_loops without num_nodes, optimized_layers.py:164 */
  int32_t weight_layout;          /* egc_weight_layout */
  int32_t weight_act;             /* egc_weight_act */
  int32_t basis_stride;           /* floats from one basis to the next inside a `bases` row: 0 (or L = F_out / H)
                                     = contiguous, as torch.matmul(x, bases_weight) lays them out; a multiple of 4
                                     >= L = each basis padded with zero columns to 16-byte slots, which lets the
                                     register-resident kernels serve L that is not a multiple of 4 (the caller pads
                                     bases_weight with zero columns; egc_bases_ld() reports the row length) */
} egc_layer;

/* Leading dimension (floats) the library wants for the `bases` intermediate: B*L rounded up to 4. */
int32_t egc_bases_ld(const egc_layer* layer);

/* Step 1 -- basis transform + weightings Linear as ONE fp32 MFMA GEMM:
 *   [bases | weightings] = x[N,F_in] @ wcat[F_in, F_g+W]  (+ bcat on the W columns)
 * Replaces torch.matmul(x, bases_weight) (layers.py:97-101, optimized_layers.py:180) and
 * comb_weights(x) (layers.py:110, optimized_layers.py:182).
 * wcat = [bases_weight (F_in x F_g) | comb.weight^T (F_in x W)] row-major; bcat = comb.bias [W] or NULL.
 * bases is written with leading dimension ldb (>= F_g, pad columns zeroed); weightings dense [N,W]. */
int egc_basis_transform_f32(const float* x, const float* wcat, const float* bcat, int64_t n_nodes,
                            int32_t f_in, int32_t f_g, int32_t w_cols, float* bases, int32_t ldb,
                            float* weightings, egc_stream_t stream);

/* Step 1, fast form -- the same GEMM on the 16-bit matrix cores with fp32-level accuracy (split precision).
 * North-star shapes (96 < F_in <= 128, F_g % 32 == 0, 192 padded output columns): every x row and every
 * weight column is scaled by a power of two and split into two fp16 planes (22 significand bits); three
 * cross products are accumulated in fp32 by v_mfma_f32_32x32x16_f16 (egc_gemm_f16x2.hip).  Other shapes:
 * three bf16 planes per operand, six products on v_mfma_f32_32x32x16_bf16 (egc_gemm_bf16x3.hip).  Either way
 * the dropped terms are of the order of one fp32 rounding of |x||w| (parity tests: <= 1e-5 of the output scale).
 * The weight planes are produced once per parameter update by egc_basis_pack into a caller buffer of
 * egc_basis_pack_bytes() bytes (opaque; its layout depends on the shape); egc_basis_transform_packed then
 * has the contract of egc_basis_transform_f32 (same reference call sites) with `packed` in place of `wcat`.
 * On the fp16 path egc_basis_transform_packed needs x 16-byte aligned (EGC_ERR_UNSUPPORTED otherwise). */
size_t egc_basis_pack_bytes(int32_t f_in, int32_t f_g, int32_t w_cols);
int egc_basis_pack(const float* wcat, int32_t f_in, int32_t f_g, int32_t w_cols, void* packed,
                   size_t packed_bytes, egc_stream_t stream);
/* Operand precision of the split GEMM.  flags = 0: as above (fp16x2, 22 significand bits, where the shape has that
 * kernel).  EGC_GEMM_24BIT: three bf16 planes per operand for EVERY shape -- all 24 bits of an fp32 operand survive.
 * Rounds 2-3 ran layers with `std` / `var` on it: var = E[x^2] - E[x]^2 cancels on (nearly) constant neighbourhoods and
 * std = sqrt(relu(var) + 1e-5) (layers.py:203-216) then amplifies what the GEMM dropped from `bases` 158x.  Since round 4
 * the aggregate kernels accumulate the variance about the row's first entry -- E[(x - s)^2] - (E[x] - s)^2, the same number
 * without the cancellation -- and such layers sit within 7e-7 of the float64 value with either operand precision (the
 * float32 formula itself: up to 3.7e-4), so egc_layer_gemm_flags(layer) is 0 for every layer; EGC_GEMM_STDVAR_24BIT=1 in the
 * environment makes it EGC_GEMM_24BIT for std / var layers again.  Pass its value to BOTH calls of a layer (pack and
 * transform must agree); egc_layer_forward_packed applies it by itself, so its `packed` must come from egc_basis_pack_ex
 * with the same flags.  Cost of the 24-bit form at the 128-wide shapes: 63-70 us instead of 40 us per GEMM at ogbn-arxiv
 * size. */
#define EGC_GEMM_24BIT 1
int32_t egc_layer_gemm_flags(const egc_layer* layer);
int egc_basis_pack_ex(const float* wcat, int32_t f_in, int32_t f_g, int32_t w_cols, int32_t flags, void* packed,
                      size_t packed_bytes, egc_stream_t stream);
int egc_basis_transform_packed_ex(const float* x, const void* packed, const float* bcat, int64_t n_nodes, int32_t f_in,
                                  int32_t f_g, int32_t w_cols, int32_t flags, float* bases, int32_t ldb,
                                  float* weightings, egc_stream_t stream);
/* egc_basis_pack of a matrix given TRANSPOSED: wt [f_g + w_cols][ld >= f_in] row-major holds wcat^T (element (k, c) of
 * wcat at wt[c * ld + k]).  The gradient w.r.t. x is [d bases | d weightings] @ wcat^T -- a basis transform whose
 * "wcat" is the transpose of the layer's own operand: this packs it where it lies (no transposed copy per step). */
int egc_basis_pack_transposed(const float* wt, int64_t ld, int32_t f_in, int32_t f_g, int32_t w_cols, void* packed,
                              size_t packed_bytes, egc_stream_t stream);
int egc_basis_transform_packed(const float* x, const void* packed, const float* bcat, int64_t n_nodes,
                               int32_t f_in, int32_t f_g, int32_t w_cols, float* bases, int32_t ldb,
                               float* weightings, egc_stream_t stream);
/* egc_basis_transform_packed_ex with bases = x W + bases_addend (round 6): bases_addend [n_nodes][ldb], 16-byte aligned, joins the
 * bases columns in the kernel's store.  The gradient of a residual block  x + f(conv(x))  w.r.t. x is the layer's d x GEMM plus the
 * upstream gradient itself (autograd's add behind zinc/models.py:66-72): with the addend that sum costs no pass of its own.  Only
 * the long-k kernels (128 < f_in <= 384, the d x GEMM of the reference's 224- and 296-wide nets) carry it: EGC_ERR_UNSUPPORTED
 * elsewhere, and the caller adds; bases_addend == NULL: egc_basis_transform_packed_ex. */
int egc_basis_transform_packed_add(const float* x, const void* packed, const float* bcat, int64_t n_nodes, int32_t f_in,
                                   int32_t f_g, int32_t w_cols, int32_t flags, const float* bases_addend, float* bases, int32_t ldb,
                                   float* weightings, egc_stream_t stream);

/* Scratch bytes egc_aggregate_combine_f32 needs for this layer on this graph.
 * CONTRACT: its first egc_aggregate_workspace_zero_bytes() bytes must be zero before its FIRST use (the long-row
 * arrival counters of the fused kernel: 4 bytes per possible long row); the rest holds chunk records that are written
 * before they are read and may start with any contents -- a per-batch graph costs an allocation and a memset of a
 * few KB, not of the whole capacity-sized buffer.  Every call leaves the workspace ready for the next call on the
 * same stream.  One workspace must not be shared by calls that may run concurrently on different streams, nor
 * between graphs of different sizes (the zero part of one layout overlaps the records of another). */
size_t egc_aggregate_workspace_bytes(const egc_layer* layer, int64_t n_nodes, int64_t n_edges);
size_t egc_aggregate_workspace_zero_bytes(const egc_layer* layer, int64_t n_nodes, int64_t n_edges);
/* The same for one graph: when egc_graph.n_chunks carries the host copy of the plan's chunk count, the records of
 * chunk slots that do not exist are not allocated (ogbn-mag shape: 0.2 GB instead of 1.5 GB); with n_chunks = -1 it
 * equals egc_aggregate_workspace_bytes.  A workspace of this size serves exactly this graph. */
size_t egc_aggregate_workspace_bytes_for(const egc_layer* layer, const egc_graph* graph);

/* Step 2+3 -- fused multi-aggregator neighbourhood reduction + per-node head x basis x aggregator
 * combine (+ weight nonlinearity, + bias).  Replaces, in one pass over the CSR:
 *   gather x_j                      MessagePassing.__collect__ (via propagate, layers.py:191-193)
 *   symnorm message scaling         layers.py:195-199, optimized_layers.py:226-230
 *   scatter / spmm per aggregator   layers.py:201-225, optimized_layers.py:215-278
 *   stack + softmax/sigmoid/hardtanh + weighted sum / bmm + bias
 *                                   layers.py:109-138, optimized_layers.py:183-208
 * out is [n_nodes, out_channels].  arg_max / arg_min must be NULL here: the arg-extremum indices are an
 * output of the training form below (EGC_ERR_UNSUPPORTED otherwise). */
int egc_aggregate_combine_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                              const float* weightings, const float* bias, float* out,
                              int32_t* arg_max, int32_t* arg_min,
                              void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* egc_aggregate_combine_f32 restricted to the rows [row_begin, row_end): the other rows of `out` are not touched.
 * A vertex-partitioned run numbers its interior rows (all sources owned) first and finishes them while the halo
 * rows of `bases` are still in flight, then the boundary rows (egc_amd/partition.py). */
int egc_aggregate_combine_rows_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                                   const float* weightings, const float* bias, float* out, int64_t row_begin,
                                   int64_t row_end, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* egc_aggregate_combine_f32 with the caller's elementwise tail fused into the store: the
 * reference's nets follow every layer with BatchNorm1d -> ReLU -> + identity (zinc/models.py:66-72,
 * mol/pna_style_models.py:71-78, cifar/models.py:67-74); in eval mode the normalisation is a per-channel affine
 * map, so   out = act((z + bias) * scale + shift) + residual   with z the layer's combine result.
 * scale / shift ([out_channels], both or neither), residual ([n_nodes, out_channels]) may be NULL; relu != 0
 * applies max(., 0) before the residual.  residual may be `out` itself: every element is read by the lane that
 * then writes it, so a sum of terms accumulates in place (relational EGC, rmag/models.py:131-144).
 * post == NULL is egc_aggregate_combine_f32. */
typedef struct {
  const float* scale;
  const float* shift;
  const float* residual;
  int32_t relu;
} egc_post;
int egc_aggregate_combine_post_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                                   const float* weightings, const float* bias, const egc_post* post, float* out,
                                   void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* egc_aggregate_combine_post_f32 whose `weightings` rows are ldw floats apart (ldw >= H*B*A, a multiple of 4,
 * weightings 16-byte aligned): the weightings of several terms computed by ONE GEMM share an array and each term
 * reads its column block.  Relational EGC (rmag/models.py:117-144) computes, per node type, the bases, the root
 * weightings and the weightings of every relation that targets the type from the same x -- one
 * egc_basis_transform_packed with w_cols = all of them, then one call of this per term.  post may be NULL. */
int egc_aggregate_combine_strided_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                                      const float* weightings, int32_t ldw, const float* bias, const egc_post* post,
                                      float* out, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* Weight gradient of the layer's two Linear maps in one pass: out[f_in][k_cols] = x^T @ d for x [n_rows][f_in]
 * (row stride ldx) and d [n_rows][k_cols] (row stride ldd; the joint [d_bases | d_weightings] array of
 * egc_aggregate_combine_backward_f32), and, when col_sums != NULL, col_sums[k_cols] = the column sums of d (the
 * gradient of the combination Linear's bias).  Replaces what autograd runs for the reference's
 * `torch.matmul(x, self.bases_weight)` / `self.comb_weights(x)` (experiments/optimized_layers.py:177-178;
 * experiments/layers.py:110-111): split-bf16 products of fp32-level accuracy on the 16-bit matrix cores inside one
 * accumulator tile (below), exact fp32 products on the fp32 matrix-core instruction beyond it and, with EGC_GEMM_EXACT=1,
 * everywhere; fp32 sums, row ranges added in a fixed order (deterministic).  f_in, k_cols, ldx, ldd multiples of 4 and 16-byte
 * aligned pointers, else EGC_ERR_UNSUPPORTED.  workspace: egc_weight_grad_workspace_bytes() bytes, contents irrelevant on entry and exit. */
int64_t egc_weight_grad_workspace_bytes(int64_t n_rows, int32_t f_in, int32_t k_cols);
/* How a call of that shape is laid out (host only, no GPU work; round 6): plan8 = {split-bf16 one-tile kernel (1) or exact-fp32
 * kernel (0), rows of an output tile, columns of an output tile, tiles along f_in, tiles along k_cols, row ranges, rows per range,
 * threads per workgroup}.  The exact-fp32 kernel is compiled for a list of tile shapes (32 .. 224 rows by 64 .. 320 columns) and
 * the host picks shape and row split together by modelled time; tests use this to see that every compiled shape is exercised. */
int egc_weight_grad_plan(int64_t n_rows, int32_t f_in, int32_t k_cols, int32_t* plan8);
/* The same with the column sums of a THIRD array riding along: e [n_rows][e_cols] (row stride lde; e_cols a
 * multiple of 4) -> e_sums[e_cols].  A training step wants three reductions over the nodes -- the weight gradient, the
 * column sums of d weightings (bias of the combination Linear) and the column sums of grad_out (the layer's bias,
 * layers.py:137-138 / optimized_layers.py:207-208) -- and this is all three in one pass.  Only where the weight
 * gradient is one accumulator tile (the limits below, EGC_GEMM_EXACT unset) and col_sums is requested; otherwise
 * EGC_ERR_UNSUPPORTED (use egc_column_sums_f32 for e).  e == NULL or e_sums == NULL: egc_weight_grad_f32. */
#define EGC_WEIGHT_GRAD_TILE_ROWS 128    /* f_in <= this and */
#define EGC_WEIGHT_GRAD_TILE_COLS 192    /* k_cols <= this: the one-tile (split-bf16) kernel */
#define EGC_WEIGHT_GRAD_MAX_SUM_COLS 128 /* e_cols <= this */
int64_t egc_weight_grad_ex_workspace_bytes(int64_t n_rows, int32_t f_in, int32_t k_cols, int32_t e_cols);
int egc_weight_grad_ex_f32(const float* x, int64_t ldx, const float* d, int64_t ldd, int64_t n_rows, int32_t f_in,
                           int32_t k_cols, float* out, float* col_sums, const float* e, int64_t lde, int32_t e_cols,
                           float* e_sums, void* workspace, int64_t workspace_bytes, void* stream);
/* egc_weight_grad_ex_f32 for a layer's OWN parameters (round 3): d = [d bases | d weightings] is the gradient of the GEMM
 * operand egc_weights_pack_f32 builds, and the reduction writes x^T d and the column sums of d straight into the gradients of
 * the basis matrices (one [f_in, B L] or B of [f_in, L]), of the combination Linear's weight and of its bias (d_comb_bias:
 * rows permuted with the weight's; or d_bcat: in the operand's order; either may be NULL) through the pack's index map -- no
 * d wcat array and no unpack launch.  e / e_sums as in egc_weight_grad_ex_f32 (the layer's bias gradient = column sums of
 * grad_out).  Workspace: egc_weight_grad_ex_workspace_bytes(n_rows, f_in, B Ls + H B A, e_cols). */
int egc_weight_grad_params_f32(const float* x, int64_t ldx, const float* d, int64_t ldd, int64_t n_rows, int32_t f_in,
                               int32_t num_heads, int32_t num_aggrs, int32_t num_bases, int32_t basis_len, int32_t basis_stride,
                               int32_t permute_hab, float* const* d_bases_parts, int32_t n_parts, float* d_comb_weight,
                               float* d_comb_bias, float* d_bcat, const float* e, int64_t lde, int32_t e_cols, float* e_sums,
                               void* workspace, int64_t workspace_bytes, void* stream);
int egc_weight_grad_f32(const float* x, int64_t ldx, const float* d, int64_t ldd, int64_t n_rows, int32_t f_in,
                        int32_t k_cols, float* out, float* col_sums, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* The caller-side tail of a layer in TRAINING mode: conv -> BatchNorm1d (batch statistics) -> ReLU -> + input, as the
 * reference's nets run it every step (zinc/models.py:66-72, mol/pna_style_models.py:71-78, cifar/models.py:67-74).
 * Two streaming passes forward and two backward instead of one per PyTorch operator; in eval mode the tail needs no
 * pass at all (egc_post).  h, residual, out, dout, dh are dense [n_rows, cols] float32 arrays, cols a multiple of 4
 * (<= 1024 for the moments), every pointer 16-byte aligned (EGC_ERR_UNSUPPORTED otherwise).
 *
 * The ogbn-arxiv net puts a dropout between the ReLU and the residual add (arxiv/norm_models.py:34-40): `keep`
 * ([n_rows, cols] bytes, 0 = dropped, 4-byte aligned; NULL = no dropout) and keep_scale = 1 / (1 - p) carry it through
 * all three passes -- out = act(.) * keep * keep_scale + residual forward, g = dout * keep * keep_scale * [pre > 0]
 * backward.  The mask itself is the caller's (torch's generator on the Python side).
 *
 * n_valid (device int64, may be NULL): the number of leading rows that are real; rows [*n_valid, n_rows) are the
 * padding of a batch brought to the static shape of a hipGraph recording -- the statistics passes skip them and the
 * per-channel launches divide by *n_valid, so one recording serves batches of any size up to (n_rows, E) with
 * nn.BatchNorm1d's numerics on the real rows.  The elementwise passes write zeros to the padding rows (forward: they
 * stay clean for the next layer; backward: the per-channel constant of the BatchNorm gradient must not reach the
 * layer's bias and weight gradients through them).
 *
 *   egc_column_moments_f64      partials[p][0][c] = sum over the p-th block of rows of g[r][c],
 *                               partials[p][1][c] = sum of g[r][c] * b[r][c], accumulated in float64 (the caller adds
 *                               the n_partials blocks).  b == NULL: g = a, second moment of a itself (forward: batch
 *                               mean and variance of h).  b != NULL: g = a * keep * keep_scale * [b * scale + shift > 0]
 *                               (the last factor only with relu != 0; backward: a =
 *                               dout, b = h; the ReLU mask is recomputed from h, not stored), giving the two sums of
 *                               the BatchNorm backward.  partials: n_partials * 2 * cols doubles, 32-byte aligned.
 *                               count_inc (device int64, may be NULL) is incremented by one: nn.BatchNorm1d's
 *                               num_batches_tracked, bumped one launch before egc_bn_forward_finalize reads it.
 *   egc_bn_forward_finalize     everything per channel between the two forward passes, in one launch: the partials
 *                               added in a fixed order, stats = [mean | biased variance | 1/sqrt(var + eps)] (3 * cols
 *                               doubles), affine = [scale | shift] (2 * cols floats) for the elementwise pass, and --
 *                               running_mean != NULL -- the module's running statistics as nn.BatchNorm1d updates them
 *                               (unbiased variance; momentum >= 0, or momentum < 0: the cumulative average 1 /
 *                               *n_tracked with the count already incremented by the caller).  gamma / beta may be NULL.
 *   egc_bn_backward_finalize    the same between the two backward passes: out5 = [d gamma | d beta | coef_g | coef_h |
 *                               coef_1] (5 * cols floats) from the partial sums of the masked gradient and `stats`.
 *   egc_affine_act_residual_f32 out = act(h * scale + shift) + residual   (scale = gamma * rstd, shift = beta - mean *
 *                               scale; relu != 0: act = max(., 0); residual may be NULL)
 *   egc_affine_act_backward_f32 dh = coef_g * g + coef_h * h + coef_1 per channel, g as above: the BatchNorm backward
 *                               with its two sums folded into the three per-channel coefficient vectors. */
int egc_column_moments_f64(const float* a, const float* b, const float* scale, const float* shift, int32_t relu,
                           const uint8_t* keep, float keep_scale, int64_t n_rows, int32_t cols, double* partials,
                           int32_t n_partials, int64_t* count_inc, const int64_t* n_valid, egc_stream_t stream);
/* Statistics pass + per-channel step as ONE call (round 3): egc_column_moments_f64 followed by egc_bn_forward_finalize /
 * egc_bn_backward_finalize with the same arguments.  With `sync` (a device int32 that is zero on entry; it is zero again
 * on exit, so one word serves a module for ever) and at most 64 partial blocks it is also ONE LAUNCH: the block that
 * finishes last adds the partials (in the finalize kernels' order: same bits) and writes the per-channel results -- the
 * batched nets' training step (zinc/models.py:66-72 at 128 graphs per step) is bound by its launches.  sync == NULL or
 * more partial blocks: the two launches.  MEASURED (ZINC-shaped batch of 128, 4 blocks forward + backward, same box): the one
 * launch is 17-18 us per call against ~6 + ~4.5 for the two kernels (a chain of cross-XCD round trips: write-through
 * partials, the arrival atomic, the last block's reads), 426-429 us per replayed step against 372-373 with two launches;
 * eager 0.98-1.18 ms against 1.03-1.23.  The host side (egc_amd.FusedEGCBlock) therefore passes sync only on request
 * (EGC_BN_ONE_LAUNCH=1). */
int egc_bn_forward_stats_f32(const float* h, int64_t n_rows, int32_t cols, double* partials, int32_t n_partials,
                             int64_t* count_inc, const int64_t* n_valid, const float* gamma, const float* beta, double eps,
                             double* stats, float* affine, float* running_mean, float* running_var, double momentum,
                             const int64_t* n_tracked, int32_t* sync, egc_stream_t stream);
int egc_bn_backward_stats_f32(const float* dout, const float* h, const float* scale, const float* shift, int32_t relu,
                              const uint8_t* keep, float keep_scale, int64_t n_rows, int32_t cols, double* partials,
                              int32_t n_partials, const int64_t* n_valid, const double* stats, const float* gamma, float* out5,
                              int32_t* sync, egc_stream_t stream);
/* egc_bn_backward_stats_f32 that also returns the column sums of the dh egc_affine_act_backward_f32 will write, dh_col_sums[cols]
 * (round 6; NULL: the call above).  In the reference's blocks the conv's bias sits in front of the BatchNorm (zinc/models.py:66-72), so
 * its gradient -- autograd's sum of dh over the rows -- is zero but for rounding; here it is formed per channel from the sums this
 * step holds anyway (coef_g sum g + coef_h sum h + n coef_1 with the float32 coefficients as stored), which spares a training step
 * of the wide nets one pass over [n_rows, cols] per layer. */
int egc_bn_backward_stats_sums_f32(const float* dout, const float* h, const float* scale, const float* shift, int32_t relu,
                                   const uint8_t* keep, float keep_scale, int64_t n_rows, int32_t cols, double* partials,
                                   int32_t n_partials, const int64_t* n_valid, const double* stats, const float* gamma, float* out5,
                                   float* dh_col_sums, int32_t* sync, egc_stream_t stream);
int egc_bn_forward_finalize(const double* partials, int32_t n_partials, int32_t cols, int64_t n_rows, const float* gamma,
                            const float* beta, double eps, double* stats, float* affine, float* running_mean,
                            float* running_var, double momentum, const int64_t* n_tracked, const int64_t* n_valid,
                            egc_stream_t stream);
int egc_bn_backward_finalize(const double* partials, int32_t n_partials, int32_t cols, int64_t n_rows, const double* stats,
                             const float* gamma, float* out5, const int64_t* n_valid, egc_stream_t stream);
int egc_affine_act_residual_f32(const float* h, const float* scale, const float* shift, const float* residual,
                                int32_t relu, const uint8_t* keep, float keep_scale, int64_t n_rows, int32_t cols,
                                float* out, const int64_t* n_valid, egc_stream_t stream);
int egc_affine_act_backward_f32(const float* dout, const float* h, const float* scale, const float* shift, int32_t relu,
                                const uint8_t* keep, float keep_scale, const float* coef_g, const float* coef_h,
                                const float* coef_1, int64_t n_rows, int32_t cols, float* dh, const int64_t* n_valid,
                                egc_stream_t stream);

/* The GEMM operand of a layer from its parameters (grad == 0), or the parameters' gradients from the operand's
 * gradient (grad != 0: the parameter arrays are WRITTEN, wcat / bcat read) -- one launch instead of the cat / pad /
 * permute / transpose chain (and its autograd mirror) around the two weight matrices of layers.py:97-111 /
 * optimized_layers.py:177-182:
 *   wcat [f_in][B * basis_stride + H*B*A] = [the B basis matrices side by side, each padded from basis_len to basis_stride
 *                                           columns | comb_weight^T],        bcat [H*B*A] = comb_bias
 * bases_parts: n_parts = 1 -> one [f_in][B * basis_len] matrix (EGConv.bases_weight); n_parts = B -> B matrices
 * [f_in][basis_len] (EfficientGraphConv.bases_weight.{0..B-1}); a HOST array of device pointers.  permute_hab != 0: the
 * Linear's rows are ordered [h][a][b] (EGConv, optimized_layers.py:195-202) and become columns [h][b][a]; 0: they are
 * [h][b][a] already.  bcat / comb_bias may be NULL together.  All arrays dense float32. */
int egc_weights_pack_f32(const float* const* bases_parts, int32_t n_parts, const float* comb_weight, const float* comb_bias,
                         int32_t f_in, int32_t num_heads, int32_t num_aggrs, int32_t num_bases, int32_t basis_len,
                         int32_t basis_stride, int32_t permute_hab, float* wcat, float* bcat, int32_t grad,
                         egc_stream_t stream);

/* Column sums of a row-major array with row stride ld (floats), as n_partials partial rows:
 * partials[p, c] = sum of x[r, c] over the p-th block of rows, c < cols; the caller adds the few partial rows up.
 * The bias gradients of a training step (grad_out summed over the nodes for `bias`, d_weightings for the
 * combination Linear's bias -- what autograd's sum-to-size does behind layers.py:137-138 /
 * optimized_layers.py:182,207-208).  cols and ld multiples of 4, cols <= 1024, x and partials 16-byte aligned
 * (EGC_ERR_UNSUPPORTED otherwise); deterministic (no atomics). */
int egc_column_sums_f32(const float* x, int64_t n_rows, int32_t ld, int32_t cols, float* partials, int32_t n_partials,
                        egc_stream_t stream);
/* out[c] = sum over p of partials[p][c]: adds the partial rows of egc_column_sums_f32 up in a fixed order (cols a
 * multiple of 4, both pointers 16-byte aligned). */
int egc_sum_partials_f32(const float* partials, int32_t n_partials, int32_t cols, float* out, egc_stream_t stream);

/* Mean of the rows of x [n_rows, width] over consecutive segments: out[g] = mean(x[seg_ptr[g] : seg_ptr[g+1]])
 * (0 for an empty segment; x may be NULL when every segment is empty).  global_mean_pool over a PyG batch
 * vector, whose graphs are contiguous
 * (zinc/models.py:73, mol/pna_style_models.py:79, cifar/models.py:75); seg_ptr is int64 [n_segments + 1]. */
int egc_segment_mean_f32(const float* x, const int64_t* seg_ptr, int64_t n_segments, int32_t width, float* out,
                         egc_stream_t stream);

/* The readout family of the reference's graph-level nets, `x = self.pool(x, batch.batch)` with pool =
 * global_add_pool | global_mean_pool | global_max_pool by the constructor's `readout` (zinc/models.py:45-52,73,
 * mol/pna_style_models.py:52-59,79, cifar/models.py:47-52,75, code/models.py:86-91), over consecutive row segments
 * of x [n_rows, width] (seg_ptr int64 [n_segments + 1], as in egc_segment_mean_f32; clamped to [0, n_rows]).
 * out [n_segments, width].  SUM: ((x[r0] + x[r0+1]) + x[r0+2]) + ..., rows ascending, one float32 add each -- the
 * order of a sequential scatter loop, a pure function of the input.  MEAN: that sum divided by float(max(count, 1)),
 * the bits of egc_segment_mean_f32.  MAX: the first row, then every later row that is strictly greater: the first row in
 * input order wins a tie; arg (int32 [n_segments, width], MAX only, may be NULL) receives the winner's absolute row
 * index, -1 for an empty segment; NaN / Inf follow the strict compare and nothing else.  An empty segment gives 0 for
 * every op.  n_segments == 0 and n_rows == 0 are fine; x may be NULL when there are no rows.  One group of
 * ceil(width / 4) lanes walks a segment: a single very long segment is correct and slow.
 * EGC_ERR_INVALID: unknown op, width <= 0, a missing pointer; EGC_ERR_UNSUPPORTED: MAX with n_rows >= 2^31. */
#define EGC_READOUT_SUM 0
#define EGC_READOUT_MEAN 1
#define EGC_READOUT_MAX 2
int egc_segment_reduce_f32(const float* x, const int64_t* seg_ptr, int64_t n_segments, int64_t n_rows, int32_t width,
                           int32_t op, float* out, int32_t* arg, egc_stream_t stream);

/* Backward of egc_segment_reduce_f32 (what autograd derives from torch_scatter's scatter in the reference's pools):
 * d_x [n_rows, width] from d_out [n_segments, width], every element written exactly once, driven by seg_ptr alone
 * (no batch vector, no zero-fill, no atomics).  SUM: d_x[r] = d_out[g]; MEAN: d_x[r] = d_out[g] / float(max(count, 1));
 * MAX: d_x[r, c] = arg[g, c] == r ? d_out[g, c] : 0 with the forward's arg (required for MAX, ignored otherwise).
 * Rows in no segment (r < seg_ptr[0] or r >= seg_ptr[n_segments]) receive 0. */
int egc_segment_reduce_backward_f32(const float* d_out, const int64_t* seg_ptr, const int32_t* arg, int64_t n_segments,
                                    int64_t n_rows, int32_t width, int32_t op, float* d_x, egc_stream_t stream);

/* The node encoders at the head of the reference's batched nets, `x = self.embedding(batch.x)` followed by
 * `x = self.in_feat_dropout(x)`: nn.Embedding (zinc/models.py:28-30,62-63), ogb's AtomEncoder, nine tables summed
 * (mol/pna_style_models.py:33-34,66-69; table sizes output/pretrained.txt:460-470), ASTNodeEncoder, three tables and
 * `depth[depth > max_depth] = max_depth` (code/models.py:27-45,104-112).  One definition: n_tables tables
 * tables[t] [table_rows[t], width] float32 (device pointers in a HOST array, as are table_rows and clamp: they are read
 * during the call and travel in the kernel arguments), idx int64 [n_rows, n_tables], clamp[t] >= 0: the index of table t
 * is replaced by min(idx, clamp[t]) (-1 or clamp == NULL: none; the caller's idx is never written).
 *   out[n, :] = ((W_0[idx[n,0]] + W_1[idx[n,1]]) + W_2[idx[n,2]]) + ...     tables ascending, one float32 add each
 * -- the order of AtomEncoder.forward (its leading `0 +` is exact) and of ASTNodeEncoder.forward: a pure function of the
 * inputs.  keep (uint8 [n_rows, width], may be NULL) and keep_scale = 1 / (1 - p) are the dropout behind the encoder:
 * out = keep ? sum * keep_scale : 0.  An index outside [0, table_rows[t]) after the clamp is never used as an address:
 * that table contributes a zero row for the node and *host_flag = 1 is stored (may be NULL; the sticky host-visible word
 * of egc_coo_to_csr_checked).  One launch.  n_rows == 0 is fine.
 * EGC_ERR_INVALID: a missing pointer, n_rows < 0, n_tables <= 0, width <= 0, a table without rows;
 * EGC_ERR_UNSUPPORTED: n_tables > EGC_ENCODER_MAX_TABLES, more than EGC_ENCODER_MAX_TABLE_ROWS rows in all tables
 * together, width > EGC_ENCODER_MAX_WIDTH, n_rows >= 2^31 - 256, ceil(n_rows / 256) * total rows >= 2^31.  Any width inside
 * the limit is handled; 16-byte accesses need width % 4 == 0 and 16-byte aligned pointers. */
#define EGC_ENCODER_MAX_TABLES 16
#define EGC_ENCODER_MAX_TABLE_ROWS (1 << 20)
#define EGC_ENCODER_MAX_WIDTH 1024
int egc_encoder_forward_f32(const float* const* tables, const int32_t* table_rows, const int32_t* clamp, int32_t n_tables,
                            const int64_t* idx, int64_t n_rows, int32_t width, const uint8_t* keep, float keep_scale,
                            float* out, int32_t* host_flag, egc_stream_t stream);

/* Backward of egc_encoder_forward_f32 (what autograd derives for the same lines: one embedding_dense_backward per
 * table, each a sort and a segmented sum): d_tables[t] [table_rows[t], width] (device pointers in a host array -- e.g.
 * where the tables' .grad tensors are),
 *   d W_t[v, :] = sum over { n : min(idx[n,t], clamp[t]) == v } of (keep ? d_out[n, :] * keep_scale : 0),
 * rows that nobody indexes receive 0, EVERY element of every d W_t is written exactly once (no zero fill by the caller).
 * No gradient for idx.  Indices outside their table are skipped (the forward reports them).  Two launches, no atomics:
 * nodes are cut into chunks of 256; inside a chunk the rows of one destination are added in ascending n, then a
 * destination's chunk sums are added in ascending chunk order -- the summation order is a function of idx and the shapes
 * alone, the result is bit-reproducible.  workspace: egc_encoder_workspace_bytes(n_rows, n_tables, total rows of all
 * tables, width) bytes, 16-byte aligned, any content (EGC_ERR_WORKSPACE if smaller; 0 bytes for n_rows == 0); the size depends on
 * host-known numbers only.  Errors and limits as the forward. */
size_t egc_encoder_workspace_bytes(int64_t n_rows, int32_t n_tables, int64_t total_table_rows, int32_t width);
int egc_encoder_backward_f32(const float* d_out, const uint8_t* keep, float keep_scale, const int64_t* idx, int64_t n_rows,
                             int32_t width, const int32_t* table_rows, const int32_t* clamp, int32_t n_tables,
                             float* const* d_tables, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* The output head and loss of the reference's classification nets (egc_softmax.hip): `conv(x)[:, :349].log_softmax(-1)`,
 * `out[train_idx]`, `F.nll_loss(out, y[train_idx])` (mag/models.py:68-69 + mag/configs.py:34-35, arxiv/norm_models.py:42-43 +
 * arxiv/configs.py:53-54, rmag/configs.py:35-36) and F.cross_entropy (cifar/configs.py:57).  float32 rows of n_classes columns
 * inside a row stride ld >= n_classes (in floats); columns n_classes .. ld-1 are never read, and the backward forms write
 * them as zeros.  ignore_index and class weights are NOT supported (the reference uses neither).
 * Order of every row sum (sum of exp, sum of grad_out): a group of G lanes owns a row, G the power of two >=
 * ceil(n_classes / 4), at most 64; a lane adds its columns ascending, then the lanes combine over the xor distances
 * G/2, .., 1 -- a function of n_classes alone, so every call gives the same bits.
 * EGC_ERR_INVALID: a missing pointer, n_rows < 0, n_classes <= 0, ld < n_classes; EGC_ERR_UNSUPPORTED: n_classes >
 * EGC_SOFTMAX_MAX_CLASSES (the 5,002-wide token heads of ogbg-code have egc_token_head_forward_f32), n_rows >= 2^38.  n_rows == 0 is
 * fine.  16-byte accesses need the row strides % 4 == 0 and 16-byte aligned pointers; any other shape takes 4-byte ones.
 *
 * egc_log_softmax_forward_f32    out [n_rows, n_classes] dense: out[r, c] = x[r, c] - lse[r], lse[r] = m_r + log(sum_c
 *                                exp(x[r, c] - m_r)), m_r the row maximum.  lse [n_rows] and argmax [n_rows] (int32) may be
 *                                NULL.  argmax: the FIRST maximal column (ties go to the smaller column).  One launch.
 * egc_log_softmax_backward_f32   d_x [n_rows, ld]: d_x[r, c] = grad_out[r, c] - exp(out[r, c]) * sum_c grad_out[r, c] for
 *                                c < n_classes, 0 for the padding; grad_out and out dense [n_rows, n_classes].  Every
 *                                element of d_x is written exactly once.  One launch. */
#define EGC_SOFTMAX_MAX_CLASSES 1024
int egc_log_softmax_forward_f32(const float* x, int64_t n_rows, int32_t n_classes, int32_t ld, float* out, float* lse,
                                int32_t* argmax, egc_stream_t stream);
int egc_log_softmax_backward_f32(const float* grad_out, const float* out, int64_t n_rows, int32_t n_classes, int32_t ld,
                                 float* d_x, egc_stream_t stream);

/* Selection counts of an index vector (the `[train_idx]` of the lines above): cnt[r] = how often r occurs in index
 * [n_index] (int64), *total = the number of indices inside [0, n_rows) -- the M of the mean.  cnt [n_rows] int32 and total
 * (one int64) are device memory, zeroed and filled here (integer atomics: the result does not depend on their order).  An
 * index outside [0, n_rows) is never used as an address: it is not counted and *host_flag = 1 is stored (may be NULL; the
 * sticky host-visible word of egc_coo_to_csr_checked).  EGC_ERR_UNSUPPORTED: n_index >= 2^31. */
int egc_row_selection_count(const int64_t* index, int64_t n_index, int64_t n_rows, int32_t* cnt, int64_t* total,
                            int32_t* host_flag, egc_stream_t stream);

/* Fused selected-row NLL of the row log-softmax, forward: with logp[r, c] = x[r, c] - lse[r],
 *   *loss = -(1 / M) sum_r cnt[r] * logp[r, y[r]]    (mean != 0),    -sum_r cnt[r] * logp[r, y[r]]    (mean == 0)
 * y [n_rows] int64 labels; cnt / total from egc_row_selection_count, or cnt == NULL: every row once, M = n_rows (total is
 * then ignored).  lse [n_rows] is written for the backward (0 on rows with cnt[r] <= 0, which are not read).  A label outside
 * [0, n_classes) on a selected row is never used as an address: the row adds 0 to the loss, receives a zero gradient row,
 * and *host_flag = 1 is stored (may be NULL).  M == 0 with mean gives NaN, as torch does.
 * Summation order (no float atomics, bit-reproducible): rows are cut into chunks of 128; group s of a chunk's 256 / G lane
 * groups adds its rows chunk0 + s, chunk0 + s + 256 / G, ... ascending; the chunk's group sums are added four adjacent ones
 * at a time, ascending, then over the xor distances 32, .., 1; the second launch adds chunk sums t, t + 256, ... ascending in
 * thread t and the 256 thread sums in the same way.  The longest chain of adds is 128 G / 256 + 9 + ceil(chunks / 256) + 9.
 * workspace: egc_nll_log_softmax_workspace_bytes(n_rows, n_classes) bytes (0 outside the limits), 4-byte aligned, any
 * content; EGC_ERR_WORKSPACE if smaller.  Two launches.
 * Backward: d_x [n_rows, ld] from the forward's lse and *grad_loss (device scalar),
 *   d_x[r, c] = w_r * (exp(x[r, c] - lse[r]) - [c == y[r]]),   w_r = (grad_loss * cnt[r]) / M  (mean) or grad_loss * cnt[r],
 * for c < n_classes on selected rows with a label inside the classes, 0 in the padding columns and on every other row.
 * Every element of d_x is written exactly once: no zero fill in front, no atomics.  One launch. */
size_t egc_nll_log_softmax_workspace_bytes(int64_t n_rows, int32_t n_classes);
int egc_nll_log_softmax_forward_f32(const float* x, const int64_t* y, const int32_t* cnt, const int64_t* total, int64_t n_rows,
                                    int32_t n_classes, int32_t ld, int32_t mean, float* loss, float* lse, void* workspace,
                                    size_t workspace_bytes, int32_t* host_flag, egc_stream_t stream);
int egc_nll_log_softmax_backward_f32(const float* x, const int64_t* y, const int32_t* cnt, const int64_t* total,
                                     const float* lse, const float* grad_loss, int64_t n_rows, int32_t n_classes, int32_t ld,
                                     int32_t mean, float* d_x, egc_stream_t stream);

/* The token head of the reference's ogbg-code net fused with its loss (egc_token_head.hip): seq_len Linear maps of the pooled
 * rows onto a vocabulary, the mean cross-entropy over the positions and the arg-max of every position,
 *   preds = [Linear_t(x)];  loss = sum_t F.cross_entropy(preds[t], y[:, t]) / seq_len;  pred = argmax(preds[t], 1)
 * (code/models.py:95-98, 121-125 with code/configs.py:63-66, 94), and what autograd derives from it.  Nothing of size
 * [n_rows, n_classes] is written: with logit[g, t, c] = b_t[c] + sum_k x[g, k] W_t[c, k],
 *   lse[g, t]    = m + log(sum_c exp(logit[g, t, c] - m)), m the maximum over c,
 *   argmax[g, t] = the FIRST maximal column (ties go to the smaller column),
 *   *loss        = (sum over g, t of (lse[g, t] - logit[g, t, y[g, t]])) / float(n_rows * seq_len),
 *   grad         = grad_loss / float(n_rows * seq_len) * (exp(logit - lse) - [c == y[g, t]])       (never stored),
 *   d_W_t = grad_t^T x,   d_b_t[c] = sum_g grad[g, t, c],   d_x = sum over t, c of grad[g, t, c] W_t[c, :].
 * x [n_rows, in_features] float32; weights / biases / d_weights / d_biases: HOST arrays of seq_len device pointers to
 * W_t [n_classes, in_features] and b_t [n_classes] (e.g. the parameters of seq_len nn.Linear and their gradients); y
 * [n_rows, seq_len] int64 row-major; lse [n_rows, seq_len]; argmax [n_rows, seq_len] int32.
 * Forward: y == NULL is the evaluation form (argmax only; loss, lse may be NULL); with y, argmax may be NULL.  A label
 * outside [0, n_classes) is never used as an address: its term adds 0, its gradient is 0 and *host_flag = 1 is stored (may
 * be NULL; the sticky word of egc_coo_to_csr_checked).  n_rows == 0 gives *loss = NaN, as torch's mean does.
 * Backward: from the forward's lse and *grad_loss (device scalar).  d_x, d_weights, d_biases may each be NULL: that product
 * is skipped.  Every element of every gradient is written (no zero fill by the caller).
 * Order.  A logit is ONE float32 fma chain over a fixed permutation of k, the same for every row and column (the four k of
 * MFMA e of step s are 16 s + e + {0, 4, 8, 12}), then one add of the bias: exact products, equal weights give equal bits.
 * The columns of a position are cut into slabs of EGC_TOKEN_HEAD_SLAB; a slab's sum of exp(logit - slab max) adds a lane's four
 * columns 16 apart ascending, then the 16 lanes over the xor distances 1, 2, 4, 8; lse adds the slabs' sums, each scaled by
 * exp(slab max - m), in ascending slab order.  The loss adds term[i = g * seq_len + t]: thread i % 256 takes its terms
 * ascending, the 256 thread sums are added four adjacent ones at a time, ascending, then over the xor distances 32 .. 1: the
 * longest chain is ceil(n_rows seq_len / 256) + 3 + 6 adds.  Rows are walked in blocks of 128.  d_W_t: a block's rows in the
 * order 16 (s / 4) + s % 4 + {0, 4, 8, 12}, s = 0 .. 31, one fma chain; the first block is written, each later block's sum is
 * added to it (n_rows <= 128: every element written exactly once).  d_b_t: a block's rows ascending, blocks as d_W_t.  d_x:
 * inside a workgroup one fma chain over its slabs ascending, a slab's columns in the order 16 (s / 4) + s % 4 + {0, 4, 8, 12},
 * s = 0 .. 15; then the workgroups' partial arrays are added ascending.  No float atomics: two calls give the same bits.
 * workspace: egc_token_head_workspace_bytes(n_rows, in_features, n_classes, seq_len) bytes (one size for both calls; 0
 * outside the limits), 16-byte aligned, any content; EGC_ERR_WORKSPACE if smaller.  Forward: three launches (two without
 * y), backward: two (one without d_x).
 * EGC_ERR_INVALID: a missing pointer, n_rows < 0, in_features, n_classes or seq_len <= 0; EGC_ERR_UNSUPPORTED: in_features % 4
 * != 0 or > EGC_TOKEN_HEAD_MAX_IN, seq_len > EGC_TOKEN_HEAD_MAX_SEQ, n_classes or n_rows > 2^30, x / W_t / d_x / d_W_t not 16-byte aligned. */
#define EGC_TOKEN_HEAD_MAX_SEQ 8
#define EGC_TOKEN_HEAD_SLAB 64
#define EGC_TOKEN_HEAD_MAX_IN 384   /* widest in_features */
size_t egc_token_head_workspace_bytes(int64_t n_rows, int32_t in_features, int32_t n_classes, int32_t seq_len);
int egc_token_head_forward_f32(const float* x, const float* const* weights, const float* const* biases, const int64_t* y,
                               int64_t n_rows, int32_t in_features, int32_t n_classes, int32_t seq_len, float* loss, float* lse,
                               int32_t* argmax, void* workspace, size_t workspace_bytes, int32_t* host_flag,
                               egc_stream_t stream);
int egc_token_head_backward_f32(const float* x, const float* const* weights, const float* const* biases, const int64_t* y,
                                const float* lse, const float* grad_loss, int64_t n_rows, int32_t in_features, int32_t n_classes,
                                int32_t seq_len, float* d_x, float* const* d_weights, float* const* d_biases, void* workspace,
                                size_t workspace_bytes, egc_stream_t stream);

/* The graph-level MLP head of the reference's batched nets fused with its loss (egc_head.hip):
 *   pool -> mlp([K0, K1, .., K_{L-1}, OUT]) -> loss,  mlp = [Linear -> BatchNorm1d -> ReLU -> Dropout(0)] x (L - 1), Linear
 * (experiments/utils.py:30-40; zinc/configs.py:48-50 F.l1_loss, mol/configs.py:64-68 BCE-with-logits over the labelled entries),
 * and what autograd derives from it.  With a_0 = x [n_rows, K0] and, for l = 1 .. L,
 *   z_l = a_{l-1} W_l^T + b_l                              W_l [K_l, K_{l-1}] (nn.Linear.weight), K_L = OUT
 *   stats_l = {mean, biased variance, 1 / sqrt(variance + eps)} of the columns of z_l (training), float64 [3][K_l]
 *   affine_l = {scale = gamma rstd, shift = beta - mean gamma rstd} rounded once from float64, float32 [2][K_l]
 *   a_l = relu(z_l scale + shift), the ReLU decision being the float32 expression fl(fl(z * scale) + shift) > 0 in the forward
 *         and in the backward alike (it is formed again from z_l and affine_l; no mask is stored)
 *   out = z_L [n_rows, OUT]
 *   EGC_HEAD_LOSS_L1          loss = mean |out - y| over all n_rows OUT entries; d out = sign(out - y) grad_loss / (n_rows OUT),
 *                             sign(0) = 0
 *   EGC_HEAD_LOSS_BCE_MASKED  loss = mean over {y == y} of max(o, 0) - o y + log1p(exp(-|o|)); a NaN target adds nothing and
 *                             has a zero gradient; the divisor is the labelled count, taken on the device; no labelled entry:
 *                             loss = NaN; d out = (sigmoid(o) - y) grad_loss / count
 *   EGC_HEAD_LOSS_NONE        out only; the backward takes the caller's d out
 * The loss terms and d out are evaluated in float64 from the float32 out and y and rounded ONCE; loss2 = {loss, count} (float32;
 * count = n_rows OUT for L1).  In evaluation the running statistics take the place of the batch's: scale / shift from
 * running_mean / running_var by the same float64 expressions.
 * Backward of a hidden layer, with g = d a * [pre > 0]: coef_l [5][K_l] = {d gamma = sum g z_hat, d beta = sum g, c_g, c_h, c_1}
 * (float64 sums, rounded once) and dz_l = fl(fl(fl(c_g g) + fl(c_h z)) + c_1) -- egc_bn_backward_finalize's coefficients;
 * d a_{l-1} = dz_l W_l, d W_l = dz_l^T a_{l-1}, d b_l = column sums of dz_l, d x = dz_1 W_1.
 * Envelope: 1 <= L <= EGC_HEAD_MAX_LINEARS; any positive widths K_0 .. K_{L-1} <= EGC_HEAD_MAX_WIDTH (no multiple-of-4
 * requirement), OUT <= EGC_HEAD_MAX_OUT, n_rows <= EGC_HEAD_MAX_ROWS; float32; dense row-major arrays, no alignment beyond
 * their element's (the workspace: 8 bytes).  Training needs n_rows >= 2 when L > 1 (nn.BatchNorm1d raises on one row) and
 * n_rows >= 1 otherwise; evaluation with n_rows == 0 launches nothing.
 * Launches: training forward L (one per Linear; a hidden layer's launch also produces stats_l, affine_l, the running
 * statistics and num_batches_tracked + 1 in its last block -- the arrival counter of egc_bn_forward_stats_f32; the final
 * launch also produces loss2); evaluation forward 1; backward L row passes from the top layer down (the top pass is skipped
 * when it has nothing to form: EGC_HEAD_LOSS_NONE without a layer or d_x below) and 1 launch for every d W_l and d b_l
 * (want_params).  No grid barrier, no spin wait, no cooperative launch, no float atomics; nothing reads back from the device.
 * Order (two calls give the same bits).  Every product element is ONE float32 fma chain over the reduction index ascending
 * (exact products), then one add of the bias (forward).  Column sums are float64: a block of EGC_HEAD_ROW_TILE rows adds its
 * rows ascending; the last block adds the blocks' partials, lane j = 0 .. 7 taking the partials j, j + 8, .. ascending, then the
 * eight lane sums ascending.  Loss (float64): a row block adds, per column, its rows ascending, then its columns ascending; the
 * last block: lane j = 0 .. 63 takes the blocks j, j + 64, .. ascending, then the lane sums ascending; loss = float(sum / count).
 * d W_l and d b_l: one fma chain (one chain of adds) over all rows ascending.  The stand-alone losses: thread j = 0 .. 255 takes
 * the elements j, j + 256, .. ascending, then the thread sums ascending.
 * egc_head: n_linears = L, sizes[0 .. L]; weight / bias [l] of Linear l + 1; gamma / beta (either may be NULL: 1 / 0),
 * running_mean / running_var (both NULL: no running statistics), num_batches_tracked (int64 scalar; may be NULL with a
 * momentum), eps, momentum (< 0: the cumulative average 1 / num_batches_tracked) [l] of the BatchNorm behind Linear l + 1; the
 * per-call arrays z [n_rows, K_{l+1}], stats, affine (written by the training forward, read by the backward), dz
 * [n_rows, K_{l+1}] (dz[L - 1] is unused with EGC_HEAD_LOSS_NONE), g [n_rows, K_{l+1}] (hidden layers) and coef (written by the
 * backward), d_weight / d_bias (written
 * when want_params).  d gamma_l = coef_l[0], d beta_l = coef_l[1].
 * grad: the device scalar grad_loss, or with EGC_HEAD_LOSS_NONE the caller's d out [n_rows, OUT].  d_x may be NULL.
 * workspace: egc_head_workspace_bytes(head, n_rows) bytes (0 outside the envelope), any content; sync: a device int32 that is
 * zero on entry and zero again on exit.
 * EGC_ERR_INVALID: a missing pointer, a width < 1, n_linears < 1, too few rows, an unknown loss, evaluation without running
 * statistics; EGC_ERR_UNSUPPORTED: outside the envelope -- both before any launch.
 * egc_l1_loss_* / egc_bce_masked_*: the two losses alone on n = n_rows OUT elements (n <= EGC_HEAD_MAX_ROWS EGC_HEAD_MAX_OUT),
 * one launch each way; the backward reads the forward's loss2.
 * egc_head_launches: host-only, the number of kernel launches the entry points of this section have issued in this process. */
#define EGC_HEAD_MAX_LINEARS 4
#define EGC_HEAD_MAX_WIDTH 384
#define EGC_HEAD_MAX_OUT 64
#define EGC_HEAD_MAX_ROWS 65536
#define EGC_HEAD_ROW_TILE 16
#define EGC_HEAD_LOSS_NONE 0
#define EGC_HEAD_LOSS_L1 1
#define EGC_HEAD_LOSS_BCE_MASKED 2
typedef struct egc_head {
  int32_t n_linears;
  int32_t sizes[EGC_HEAD_MAX_LINEARS + 1];
  const float* weight[EGC_HEAD_MAX_LINEARS];
  const float* bias[EGC_HEAD_MAX_LINEARS];
  const float* gamma[EGC_HEAD_MAX_LINEARS];
  const float* beta[EGC_HEAD_MAX_LINEARS];
  float* running_mean[EGC_HEAD_MAX_LINEARS];
  float* running_var[EGC_HEAD_MAX_LINEARS];
  int64_t* num_batches_tracked[EGC_HEAD_MAX_LINEARS];
  double eps[EGC_HEAD_MAX_LINEARS];
  double momentum[EGC_HEAD_MAX_LINEARS];
  float* z[EGC_HEAD_MAX_LINEARS];
  double* stats[EGC_HEAD_MAX_LINEARS];
  float* affine[EGC_HEAD_MAX_LINEARS];
  float* dz[EGC_HEAD_MAX_LINEARS];
  float* g[EGC_HEAD_MAX_LINEARS];
  float* coef[EGC_HEAD_MAX_LINEARS];
  float* d_weight[EGC_HEAD_MAX_LINEARS];
  float* d_bias[EGC_HEAD_MAX_LINEARS];
} egc_head;
size_t egc_head_workspace_bytes(const egc_head* head, int64_t n_rows);
int egc_head_forward_train_f32(const egc_head* head, const float* x, int64_t n_rows, int32_t loss_kind, const float* y, float* out,
                               float* loss2, void* workspace, size_t workspace_bytes, int32_t* sync, egc_stream_t stream);
int egc_head_forward_eval_f32(const egc_head* head, const float* x, int64_t n_rows, float* out, egc_stream_t stream);
int egc_head_backward_f32(const egc_head* head, const float* x, int64_t n_rows, int32_t loss_kind, const float* y, const float* out,
                          const float* loss2, const float* grad, float* d_x, int32_t want_params, void* workspace,
                          size_t workspace_bytes, int32_t* sync, egc_stream_t stream);
int egc_l1_loss_forward_f32(const float* out, const float* y, int64_t n, float* loss2, egc_stream_t stream);
int egc_l1_loss_backward_f32(const float* out, const float* y, const float* grad_loss, const float* loss2, int64_t n, float* d_out,
                             egc_stream_t stream);
int egc_bce_masked_forward_f32(const float* out, const float* y, int64_t n, float* loss2, egc_stream_t stream);
int egc_bce_masked_backward_f32(const float* out, const float* y, const float* grad_loss, const float* loss2, int64_t n,
                                float* d_out, egc_stream_t stream);
int64_t egc_head_launches(void);

/* Typed mean aggregation (egc_typed_mean.hip): the sparse part of the reference's R-GCN baseline layer,
 * `self.rel_lins[key](adj_t.matmul(x_dict[src], reduce="mean"))` per relation (rmag/models.py:61-72), and of what autograd
 * derives from it, over a LIST of relations in one call:
 *   out[row, block(r)] (+)= post(row, r) * sum over p in rowptr_r[row] .. rowptr_r[row+1] of pre_r(col_r[p]) * in_r[col_r[p], 0:width]
 * One descriptor per relation (a HOST array: it is read during the call and travels in the kernel arguments):
 *   rowptr / col   int32 CSR whose rows are the rows of `out` (n_rows + 1 offsets, n_edges entries); rowptr == NULL is the
 *                  identity relation: row i has the one entry i (col and n_edges are then ignored)
 *   pre_rowptr     NULL: pre = 1; else int32 [n_in_rows + 1] and pre(j) = 1 / float(max(pre_rowptr[j+1] - pre_rowptr[j], 1)),
 *                  one float32 multiply per entry (the forward graph's rowptr when the CSR is its transpose)
 *   in, ld_in      float32 rows the entries name: n_in_rows rows of stride ld_in floats, `in` pointing at the relation's
 *                  first column (a column block of a wider array is fine)
 *   post_mean      != 0: the row's sum is divided by float(entry count); a row without entries gives 0
 *   out_col        first column of the relation's block of `out` (accumulate == 0)
 * accumulate == 0: every relation writes its own block out[:, out_col : out_col + width] (the forward: one launch per target
 * type fills the operand [x_t | mean_1 | mean_2 ...] of ONE dense product; blocks the descriptors do not name are not
 * touched).  accumulate != 0: the relations' terms are added in table order, ((0 + term_0) + term_1) + ..., into
 * out[:, 0:width] (the backward: one launch per source type over the transposed CSRs); n_rels == 0 then writes zeros.
 * Every element named is written exactly once: no zero fill in front, no atomics.
 * Order of a row's float32 sum: the entries are cut into consecutive chunks of EGC_TYPED_MEAN_CHUNK counted from the row's
 * first entry; a chunk's sum is ((0 + v0) + v1) + ... in entry order; the row's sum is chunk 0's with those of chunks 1, 2, ..
 * added in ascending order -- a function of the CSR and the inputs alone.  Chunks 1.. of long rows are summed by a first
 * launch, one group of lanes per chunk, into `workspace` (egc_typed_mean_workspace_bytes: depends on the descriptors' n_edges
 * and width only; 16-byte aligned, any content; 0 when no relation has more than one chunk's entries; EGC_ERR_WORKSPACE if
 * smaller), which finds them on the device from rowptr; nothing is read back.  Column indices are clamped to the input's
 * rows, offsets to [0, n_edges].  n_rows == 0 is fine.  16-byte accesses need width, ld_in, ld_out, out_col % 4 == 0 and
 * 16-byte aligned pointers; anything else takes 4-byte ones.
 * EGC_ERR_INVALID: a missing pointer, a negative count, ld_in < width, ld_out smaller than the columns named;
 * EGC_ERR_UNSUPPORTED: n_rels > EGC_TYPED_MAX_RELATIONS, n_edges or n_in_rows >= 2^31. */
#define EGC_TYPED_MEAN_CHUNK 256
#define EGC_TYPED_MAX_RELATIONS 8
typedef struct egc_typed_rel {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* pre_rowptr;
  const float* in;
  int64_t n_edges;
  int64_t n_in_rows;
  int32_t ld_in;
  int32_t out_col;
  int32_t post_mean;
  int32_t reserved;
} egc_typed_rel;
int32_t egc_typed_mean_chunk(void);
size_t egc_typed_mean_workspace_bytes(const egc_typed_rel* rels, int32_t n_rels, int32_t width);
int egc_typed_mean_f32(const egc_typed_rel* rels, int32_t n_rels, int64_t n_rows, int32_t width, int32_t accumulate,
                       float* out, int32_t ld_out, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* Message aggregation of the baseline MPNN layer (egc_mpnn.hip): the reference's Mpnn.message + aggregate
 * (experiments/layers.py:251-258 under MessagePassing.propagate) without the [E, 2 d] concatenated endpoint features and the
 * [E, d] messages.  A tower's message Linear acts on [x_i | x_j] and so splits into a target half and a source half: with
 * P = x BD(Ws)^T and Q = x BD(Wd)^T + b_msg, both [N, d], the aggregated message of row i over its entries (no self loops added) is
 *   EGC_MPNN_ADD    m_i = (sum of P[col[p]]) + float(deg_i) * Q_i
 *   EGC_MPNN_MEAN   m_i = (sum of P[col[p]]) / float(deg_i) + Q_i
 *   EGC_MPNN_MAX    m_i = (max of P[col[p]]) + Q_i     per column
 * and 0 for a row without entries.
 *   rowptr / col / edge_id   int32 CSR by destination, stable inside a row (n_rows + 1 offsets, n_edges entries); edge_id[p] is
 *                  the position of entry p in the edge list (read for EGC_MPNN_MAX with `arg` only; NULL: edge_id[p] = p)
 *   P, ld_p        n_src_rows rows of stride ld_p floats; Q, ld_q: n_rows rows of stride ld_q (column blocks of one wider array
 *                  are fine: the pointers name the blocks' first columns)
 *   out, ld_out    m, n_rows rows of stride ld_out, `out` pointing at the first column of the block to write (the left half of
 *                  the [m | x] operand of the layer's second dense product); columns outside the block are not touched
 *   arg            NULL, or (EGC_MPNN_MAX, the training form) int32 [n_rows, width], dense: the edge_id of the FIRST entry of the
 *                  row, in entry order, that attains the column's maximum (duplicate edges are separate entries; a NaN is never
 *                  selected); -1 for a row without entries
 * Every element named is written exactly once: no zero fill in front, no atomics, nothing read back.
 * Order of a row's float32 sum: egc_typed_mean_f32's -- consecutive chunks of EGC_TYPED_MEAN_CHUNK entries counted from the row's
 * first entry, a chunk's sum ((0 + v0) + v1) + ... in entry order, the chunk sums added in ascending order; then the division
 * (mean); the self term last, agg + s * Q, each one IEEE operation.  Chunks 1.. of the rows longer than one chunk are reduced by
 * a first launch into `workspace` (egc_mpnn_message_workspace_bytes: a function of n_edges, width and op only; 16-byte aligned,
 * any content; 0 when n_edges <= one chunk; EGC_ERR_WORKSPACE if smaller).  Column indices are clamped to [0, n_src_rows),
 * offsets to [0, n_edges].  Any width >= 1: 16-byte accesses when width and the strides are multiples of 4 and the pointers
 * 16-byte aligned, 4-byte ones otherwise.
 *
 * egc_mpnn_message_backward_f32: from d m (n_rows rows of stride ld_dm)
 *   d Q_i = s_i * d m_i,  s_i = float(deg_i) (add), 1 (mean, max), and d Q_i = 0 for a row without entries
 *   d P_j = sum over j's entries q of the TRANSPOSED CSR (t_rowptr [n_src_rows + 1], t_col = the destination i, t_edge_id = the
 *           forward CSR position of the entry; stable, so a row's entries ascend in forward position), in the chunked order
 *           above, of   d m_i (add),   d m_i / float(deg_i) (mean, one division per entry),   d m_i[c] where
 *           arg[i, c] == edge_id[t_edge_id[q]] and 0 elsewhere (max: with duplicate edges only the first one receives)
 * rowptr / edge_id are the forward graph's (degrees; NULL edge_id or t_edge_id: the identity).  d P (n_src_rows rows) or d Q
 * (n_rows rows) may be NULL and is then not computed.  Atomic-free, every element written once, bit-reproducible; workspace as
 * above (egc_mpnn_message_backward_workspace_bytes).
 * EGC_ERR_INVALID: width <= 0, an unknown op, a missing pointer, a negative count, a stride smaller than width;
 * EGC_ERR_UNSUPPORTED: n_rows, n_src_rows or n_edges >= 2^31. */
#define EGC_MPNN_ADD 0
#define EGC_MPNN_MEAN 1
#define EGC_MPNN_MAX 2
size_t egc_mpnn_message_workspace_bytes(int64_t n_edges, int32_t width, int32_t op);
int egc_mpnn_message_f32(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, int64_t n_rows, int64_t n_edges,
                         int64_t n_src_rows, const float* P, int32_t ld_p, const float* Q, int32_t ld_q, int32_t width,
                         int32_t op, float* out, int32_t ld_out, int32_t* arg, void* workspace, size_t workspace_bytes,
                         egc_stream_t stream);
size_t egc_mpnn_message_backward_workspace_bytes(int64_t n_edges, int32_t width);
int egc_mpnn_message_backward_f32(const int32_t* rowptr, const int32_t* edge_id, int64_t n_rows, const int32_t* t_rowptr,
                                  const int32_t* t_col, const int32_t* t_edge_id, int64_t n_src_rows, int64_t n_edges,
                                  const float* dm, int32_t ld_dm, const int32_t* arg, int32_t width, int32_t op, float* dP,
                                  int32_t ld_dp, float* dQ, int32_t ld_dq, void* workspace, size_t workspace_bytes,
                                  egc_stream_t stream);

/* Multi-aggregator aggregation of PNAConv (egc_pna.hip): PyG 2.x PNAConv (edge_dim = None, pre_layers = post_layers = 1) without
 * its [E, 2 F] endpoint features, [E, T F] messages, four scatter passes and [N, T, A S F] scaled concatenation.  The pre-transform
 * splits as Mpnn's message Linear does: P = x Ms^T (n_src_rows rows), Q = x Md^T + b_pre (n_rows rows), both `width` = T F_in wide,
 * the message of entry j -> i is P_j + Q_i.  `ops` lists n_ops (1 .. 6) distinct aggregators; block k of the output (columns
 * k * width .. (k + 1) * width of `out`, n_rows rows of stride ld_out >= n_ops * width) receives, for a row of n entries, per column
 *   EGC_PNA_SUM   S0 + float(n) * Q_i         S0 = sum of P[col[p]]
 *   EGC_PNA_MEAN  S0 / float(n) + Q_i
 *   EGC_PNA_MIN   (min of P[col[p]]) + Q_i    EGC_PNA_MAX   (max of P[col[p]]) + Q_i
 *   EGC_PNA_VAR   v = max(S2 / n - (S1 / n)^2, 0),  S1 = sum of (P[col[p]] - s), S2 = sum of (P[col[p]] - s)^2,
 *                 s = P[col[first entry of the row]] (the variance of P alone: Q_i is a row constant)
 *   EGC_PNA_STD   sqrt(v + 1e-5)
 * and 0 (EGC_PNA_STD: sqrt(1e-5)) for a row without entries.  Columns of `out` outside the n_ops blocks are not touched.
 *   rowptr / col / edge_id, P, ld_p, Q, ld_q   as for egc_mpnn_message_f32
 *   arg_min, arg_max   NULL (the inference form), or int32 [n_rows, width], dense: the edge_id of the FIRST entry of the row, in
 *                  entry order, attaining the column's extremum (strict compare; a NaN is never selected); -1 for an empty row.
 *                  Read only when MIN / MAX is listed.
 *   mu, var        NULL, or float [n_rows, width] each, dense (VAR / STD listed): s + S1 / n, the row mean of P, and the clamped
 *                  variance v -- what the backward needs (0 for an empty row)
 * One gather pass over P whatever the list; only what the list needs is carried (no shift and no S2 without VAR / STD, no
 * positions without MIN / MAX).  Order: egc_mpnn_message_f32's chunks of EGC_TYPED_MEAN_CHUNK entries from the row's first entry,
 * every accumulator taking a chunk's entries in order from 0 (+-inf), the chunks merged in ascending order by plain addition (the
 * shift is the row's in every chunk) or a strict compare (the first chunk keeps a tie); then each finishing step one IEEE
 * operation as listed in egc_pna.hip's header.  SUM and MEAN use the unshifted S0, so a block's bits do not depend on the rest of
 * the list.  workspace: egc_pna_aggregate_workspace_bytes(n_edges, width, ops, n_ops), 16-byte aligned, any content, 0 when
 * n_edges <= one chunk.  Indices are clamped as in egc_mpnn_message_f32; any width >= 1 (16-byte accesses when width, strides and
 * pointers allow, 4-byte ones otherwise).
 *
 * egc_pna_aggregate_backward_f32: from dagg (n_rows rows of stride ld_dagg, the blocks in list order), with nf = float(n):
 *   d Q_i = ((nf * g_sum + g_mean) + g_min) + g_max, 0 for an empty row
 *   per-row records  lin = g_sum + g_mean / nf;  c = g_var + g_std / (2 * sqrt(v_i + 1e-5f)), and c = 0 where v_i == 0 (the
 *           derivative 2 (P_j - mu) / n of v is 0 there, as PyG's relu'(0));  b_i = (2 * c) / nf;  a_i = lin - b_i * mu_i
 *   d P_j = ((A + P_j * B) + Mn) + Mx over j's entries of the TRANSPOSED CSR (t_rowptr / t_col / t_edge_id as for
 *           egc_mpnn_message_backward_f32, ascending forward position, chunked as above): A = sum a_i, B = sum b_i,
 *           Mn / Mx = sum of g_min[i] / g_max[i] where arg_min / arg_max [i] names this edge and 0 elsewhere
 * (terms of aggregators not listed are skipped).  mu, var (the forward's), P, ld_p: read when VAR / STD is listed.  d P (n_src_rows rows) or d Q (n_rows rows) may be NULL and is then not computed.
 * The records a and b live in `workspace`, in front of the chunk partials: egc_pna_aggregate_backward_workspace_bytes(n_rows,
 * n_edges, width) bytes, 16-byte aligned, any content.  Atomic-free, every element written once, bit-reproducible.
 *
 * egc_pna_scale_combine_f32: out_i = base_i + sum_k f_k(d_i) * Y_i[k * dim .. (k + 1) * dim], d_i = max(n_i, 1) from rowptr,
 *   IDENTITY 1   AMPLIFICATION log(d + 1) / avg_log   ATTENUATION avg_log / log(d + 1)   LINEAR d / avg_lin   INVERSE_LINEAR avg_lin / d
 * each factor formed in double and rounded once to float; acc = base, then acc = acc + f_k * Y_k in list order.  One read of Y
 * (n_rows rows of stride ld_y >= n_scalers * dim) and base, one write of out (may alias base).  _backward: dY_i[k] = f_k * g_i.
 *
 * EGC_ERR_INVALID: width / dim <= 0, an unknown or duplicate op or scaler, an empty list, a missing pointer, a negative count, a
 * stride smaller than the block; EGC_ERR_WORKSPACE: workspace missing, misaligned or too small; EGC_ERR_UNSUPPORTED: a count >= 2^31. */
#define EGC_PNA_SUM 0
#define EGC_PNA_MEAN 1
#define EGC_PNA_MIN 2
#define EGC_PNA_MAX 3
#define EGC_PNA_VAR 4
#define EGC_PNA_STD 5
#define EGC_PNA_IDENTITY 0
#define EGC_PNA_AMPLIFICATION 1
#define EGC_PNA_ATTENUATION 2
#define EGC_PNA_LINEAR 3
#define EGC_PNA_INVERSE_LINEAR 4
#define EGC_PNA_MAX_SCALERS 5
size_t egc_pna_aggregate_workspace_bytes(int64_t n_edges, int32_t width, const int32_t* ops, int32_t n_ops);
int egc_pna_aggregate_f32(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, int64_t n_rows, int64_t n_edges,
                          int64_t n_src_rows, const float* P, int32_t ld_p, const float* Q, int32_t ld_q, int32_t width,
                          const int32_t* ops, int32_t n_ops, float* out, int32_t ld_out, int32_t* arg_min, int32_t* arg_max,
                          float* mu, float* var, void* workspace, size_t workspace_bytes, egc_stream_t stream);
size_t egc_pna_aggregate_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t width);
int egc_pna_aggregate_backward_f32(const int32_t* rowptr, const int32_t* edge_id, int64_t n_rows, const int32_t* t_rowptr,
                                   const int32_t* t_col, const int32_t* t_edge_id, int64_t n_src_rows, int64_t n_edges,
                                   const float* dagg, int32_t ld_dagg, const int32_t* ops, int32_t n_ops, int32_t width,
                                   const float* P, int32_t ld_p, const int32_t* arg_min, const int32_t* arg_max, const float* mu,
                                   const float* var, float* dP, int32_t ld_dp, float* dQ, int32_t ld_dq,
                                   void* workspace, size_t workspace_bytes, egc_stream_t stream);
int egc_pna_scale_combine_f32(const int32_t* rowptr, int64_t n_rows, const int32_t* scalers, int32_t n_scalers, double avg_lin,
                              double avg_log, int32_t dim, const float* Y, int32_t ld_y, const float* base, int32_t ld_base,
                              float* out, int32_t ld_out, egc_stream_t stream);
int egc_pna_scale_combine_backward_f32(const int32_t* rowptr, int64_t n_rows, const int32_t* scalers, int32_t n_scalers,
                                       double avg_lin, double avg_log, int32_t dim, const float* g, int32_t ld_g, float* dY,
                                       int32_t ld_dy, egc_stream_t stream);

/* Neighbour sum of GCNConv, SAGEConv and GINConv (egc_nbr_sum.hip; PyG 2.x layers, the baselines of experiments/code/models.py):
 * the sparse step all three share, a row-scaled sum of source-scaled neighbour rows plus a multiple of the row's own features.
 * With agg_i the sum over row i's entries p of the term t_p (0 for a row without entries, which is never divided):
 *   EGC_NBR_SUM      t_p = x[col[p]]                                    out_i = agg_i + s * x_self_i
 *   EGC_NBR_MEAN     t_p = x[col[p]]                                    out_i = agg_i / float(deg_i) + s * x_self_i
 *   EGC_NBR_MEAN_T   t_p = x[col[p]] / float(max(deg_of(col[p]), 1))    out_i = agg_i + s * x_self_i
 *   EGC_NBR_SYM      t_p = e_p * x[col[p]]                              out_i = row_scale[i] * (agg_i + row_scale[i] * x_self_i)
 * and without x_self: agg_i, agg_i / float(deg_i), agg_i, row_scale[i] * agg_i.
 *   rowptr / col   int32 CSR (n_rows + 1 offsets, n_edges entries naming rows of x); deg_i is the walked row's entry count
 *   x, ld_x        n_src_rows rows of stride ld_x; x_self, ld_self: n_rows rows of stride ld_self, may be the array x is, NULL: no
 *                  self term; out, ld_out: n_rows rows of stride ld_out.  Column blocks of wider arrays are fine (the pointers
 *                  name the blocks' first columns); only the `width` columns named are written
 *   self_scale, eps   s = self_scale, or 1.f + *eps when the DEVICE pointer eps is not NULL (never read on the host)
 *   deg_rowptr     EGC_NBR_MEAN_T: a second rowptr, n_src_rows + 1 offsets, deg_of(j) = deg_rowptr[j + 1] - deg_rowptr[j] (the
 *                  CSR whose transpose is walked: MEAN_T over the transposed CSR is the transpose of MEAN)
 *   row_scale, src_scale, edge_scale   EGC_NBR_SYM: row_scale [n_rows]; e_p = edge_scale[p] when edge_scale [n_edges] is given,
 *                  else src_scale[col[p]] (src_scale [n_src_rows])
 *   skip_self_entries   != 0: an entry with col[p] == i is not taken; it keeps its place in the chunk layout and contributes
 *                  nothing (the LOOPED edge set above, with the self term standing for the one self loop)
 * The transpose of a form is a form on the transposed CSR -- SUM: SUM; MEAN: MEAN_T with the forward rowptr; SYM: SYM with the
 * same tables, e_p gathered -- and the self term transposes to itself, so this entry point is its own backward.
 * Order of a row's float32 sum: egc_mpnn_message_f32's -- chunks of EGC_TYPED_MEAN_CHUNK entries counted from the row's first
 * entry, a chunk ((0 + t0) + t1) + ... in entry order, the chunk sums added in ascending order; a term's product or division and
 * every step of the finish are one IEEE operation each.  Every element named is written exactly once: no zero fill, no atomics,
 * nothing read back.  Chunks 1.. of the rows longer than one chunk go through a first launch into `workspace`
 * (egc_nbr_sum_workspace_bytes: a function of n_edges and width only; 16-byte aligned, any content; 0 when n_edges <= one chunk).
 * Column indices (and with them the deg_rowptr and src_scale lookups) are clamped to [0, n_src_rows), offsets to [0, n_edges].
 * Any width >= 1: 16-byte accesses when width and the strides are multiples of 4 and the pointers 16-byte aligned, 4-byte ones
 * otherwise.  Compiled: SUM plain, with x_self, and with x_self and skip; MEAN plain; MEAN_T plain and with x_self; SYM plain and
 * with x_self and skip (either source of e_p).  EGC_ERR_UNSUPPORTED: any other combination, a count >= 2^31.
 * EGC_ERR_INVALID: width <= 0, an unknown form, a missing pointer, a negative count, a stride smaller than width, MEAN_T without
 * deg_rowptr, SYM without row_scale or without both edge_scale and src_scale; EGC_ERR_WORKSPACE: workspace missing, misaligned or
 * too small. */
#define EGC_NBR_SUM 0
#define EGC_NBR_MEAN 1
#define EGC_NBR_MEAN_T 2
#define EGC_NBR_SYM 3
size_t egc_nbr_sum_workspace_bytes(int64_t n_edges, int32_t width);
int egc_nbr_sum_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows, const float* x,
                    int32_t ld_x, const float* x_self, int32_t ld_self, int32_t width, int32_t form, int32_t skip_self_entries,
                    float self_scale, const float* eps, const int32_t* deg_rowptr, const float* row_scale, const float* src_scale,
                    const float* edge_scale, float* out, int32_t ld_out, void* workspace, size_t workspace_bytes,
                    egc_stream_t stream);

/* GATv2 attention aggregate (egc_gatv2.hip): PyG 2.x GATv2Conv's propagate without an [E, .] array.  H = heads, C = channels
 * per head, width = H * C <= 512 (any H >= 1, C >= 1).  xl (n_src_rows rows) and xr (n_rows rows) are the lin_l / lin_r
 * projections (column blocks of one wider array are fine); att is [H * C].  For an entry j -> i of the CSR by destination and head h
 *   s_ij = sum_c att[h, c] * leaky_relu(xl[j, h, c] + xr[i, h, c])      alpha_ij = softmax of s over row i's entries
 *   out[i, h, :] = sum_j alpha_ij * xl[j, h, :]                          lse[i, h] = log sum_j exp(s_ij)
 * and out = 0, lse = -inf for a row without entries.  self_loops != 0: the entries whose col equals their row are skipped and
 * one self entry (j = i) is taken last (needs n_src_rows == n_rows).  One gather pass with an online softmax (the maximum is
 * subtracted before every exp); rows longer than EGC_TYPED_MEAN_CHUNK entries are cut into chunks whose partial states a first
 * launch leaves in `workspace` (egc_gatv2_forward_workspace_bytes; 16-byte aligned, any content; 0 when n_edges <= one chunk).
 * out: n_rows rows of stride ld_out; lse: dense [n_rows, H].  Every element is written exactly once, no atomics; the order of
 * every sum is fixed by H, C and the row's entries alone (egc_gatv2.hip's header), so results are bit-reproducible.
 * Column indices are clamped to [0, n_src_rows), offsets to [0, n_edges].
 *
 * egc_gatv2_backward_f32 (a square graph: xl and xr both have n_rows rows): from g = d out, the forward's out and lse, with the
 * scores recomputed.  t_rowptr / t_col: the transposed CSR (rows = sources, entries = destinations), read for d xl only.
 *   d xr[i] = sum_j d z_ij     d xl[j] = sum_i (alpha_ij g_i + d z_ij)     d att = sum_ij d s_ij leaky_relu(z_ij)
 *   d s_ij = alpha_ij (g_i . xl_j - g_i . out_i)  per head,   d z_ij = d s_ij att leaky_relu'(z_ij)
 * Any of d xl, d xr (rows of stride ld_dxl / ld_dxr: the halves of one [N, 2 H C] array are fine), d att ([H * C]) may be NULL.
 * Workspace: egc_gatv2_backward_workspace_bytes (always > 0 for n_rows > 0), 16-byte aligned, any content.
 * EGC_ERR_INVALID: H < 1, C < 1, H * C > 512, a missing pointer, a negative count, a stride smaller than H * C, self_loops with
 * n_src_rows != n_rows; EGC_ERR_UNSUPPORTED: a count >= 2^31; EGC_ERR_WORKSPACE: workspace missing, misaligned or too small. */
size_t egc_gatv2_forward_workspace_bytes(int64_t n_edges, int32_t heads, int32_t channels);
int egc_gatv2_forward_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                          const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att, int32_t heads,
                          int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out, float* lse,
                          void* workspace, size_t workspace_bytes, egc_stream_t stream);
size_t egc_gatv2_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t heads, int32_t channels);
int egc_gatv2_backward_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                           int64_t n_edges, const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att,
                           int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, const float* out,
                           int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* dxr,
                           int32_t ld_dxr, float* datt, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* GAT (v1) attention aggregate (egc_gat.hip): PyG GATConv's propagate without an [E, .] array.  H = heads, C = channels per
 * head, width = H * C <= 512 (any H >= 1, C >= 1).  xl (n_src_rows rows of stride ld_xl) is the lin projection; a_src
 * (n_src_rows rows of stride ld_a_src, H wide) and a_dst (n_rows rows of stride ld_a_dst, H wide) are the per-node halves of
 * the additive score, a_src[j, h] = sum_c xl[j, h, c] * att_src[h, c] and a_dst likewise; the three may be column blocks of one
 * wider array.  For an entry j -> i of the CSR by destination and head h
 *   s_ij = leaky_relu(a_src[j, h] + a_dst[i, h])                alpha_ij = softmax of s over row i's entries
 *   out[i, h, :] = sum_j alpha_ij * xl[j, h, :]                  lse[i, h] = log sum_j exp(s_ij)
 * and out = 0, lse = -inf for a row without entries.  self_loops != 0: the entries whose col equals their row are skipped and
 * one self entry (j = i) is taken last (needs n_src_rows == n_rows).  One gather pass with an online softmax (the maximum is
 * subtracted before every exp) and no cross-lane operation per entry; rows longer than EGC_TYPED_MEAN_CHUNK entries are cut
 * into chunks whose partial states a first launch leaves in `workspace` (egc_gat_forward_workspace_bytes; 16-byte aligned, any
 * content; 0 when n_edges <= one chunk).  out: n_rows rows of stride ld_out; lse: dense [n_rows, H].  Every element is written
 * exactly once, no atomics; the order of every sum is fixed by H, C and the row's entries alone (egc_gat.hip's header), so
 * results are bit-reproducible.  Column indices are clamped to [0, n_src_rows), offsets to [0, n_edges].
 *
 * egc_gat_backward_f32 (a square graph): from g = d out, the forward's out and lse, with the scores recomputed.  t_rowptr /
 * t_col: the transposed CSR (rows = sources, entries = destinations), read for d xl and d a_src.  With D_i = g_i . out_i per
 * head and w_ij = alpha_ij leaky_relu'(a_src[j] + a_dst[i])
 *   d xl[j] = sum_i alpha_ij g_i   (the direct term only: the score's share flows through d a_src and d a_dst)
 *   d a_src[j, h] = sum_i w_ij (g_i . xl_j - D_i)                   d a_dst[i, h] = g_i . (sum_j w_ij xl_j) - D_i sum_j w_ij
 * Any of d xl (rows of stride ld_dxl), d a_src, d a_dst (H wide, strides ld_d_a_src / ld_d_a_dst; column blocks of one array
 * are fine) may be NULL.  Workspace: egc_gat_backward_workspace_bytes (always > 0 for n_rows > 0), 16-byte aligned, any content.
 * EGC_ERR_INVALID: H < 1, C < 1, H * C > 512, a missing pointer, a negative count, a stride smaller than its width (H * C, or
 * H for the per-head arrays), self_loops with n_src_rows != n_rows; EGC_ERR_UNSUPPORTED: a count >= 2^31; EGC_ERR_WORKSPACE:
 * workspace missing, misaligned or too small. */
size_t egc_gat_forward_workspace_bytes(int64_t n_edges, int32_t heads, int32_t channels);
int egc_gat_forward_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                        const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst, int32_t ld_a_dst,
                        int32_t heads, int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out,
                        float* lse, void* workspace, size_t workspace_bytes, egc_stream_t stream);
size_t egc_gat_backward_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t heads, int32_t channels);
int egc_gat_backward_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_rows,
                         int64_t n_edges, const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst,
                         int32_t ld_a_dst, int32_t heads, int32_t channels, float negative_slope, int32_t self_loops,
                         const float* out, int32_t ld_out, const float* lse, const float* g, int32_t ld_g, float* dxl,
                         int32_t ld_dxl, float* d_a_src, int32_t ld_d_a_src, float* d_a_dst, int32_t ld_d_a_dst, void* workspace,
                         size_t workspace_bytes, egc_stream_t stream);

/* Attention dropout in training for the two attention aggregates (PyG's F.dropout on alpha after the softmax: per entry and per
 * head, the self entry included).  The *_dropout_f32 entry points take the arguments of their plain counterparts, compute the
 * same alpha and lse (over ALL of a row's entries, unmasked) and, with m'_ij^h = 0 (dropped) or 1 / (1 - p) (kept),
 *   out[i, h, :] = sum_j m'_ij alpha_ij xl[j, h, :]        d s_ij = alpha_ij (m'_ij g_i . xl_j - g_i . out_i)
 * and m' alpha for alpha in the direct term of d xl.  The mask is a pure function of (seed, entry, head), the same in the forward
 * and in both backward passes: Philox4x32-10 (egc_amd/csrc/egc_philox.h) under the key (low, high 32 bits of *seed), counter
 * (q, h >> 2, 0, 0) for the entry at position q of the FORWARD CSR and (i, h >> 2, 1, 0) for row i's self entry; head h takes
 * output word h & 3 and is dropped iff word < (uint32) floor(p * 2^32).  Entries skipped for self_loops keep their position.
 * `seed` is a DEVICE int64 scalar read by the kernels (no synchronisation); t_edge_id[k] is the forward position of entry k of
 * the transposed CSR (CSRGraph.transposed().edge_id).  Workspaces: those of the plain entry points.  Further EGC_ERR_INVALID
 * (nothing is launched): p not in (0, 1), seed NULL, t_rowptr given without t_edge_id. */
int egc_gat_forward_dropout_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                                const float* xl, int32_t ld_xl, const float* a_src, int32_t ld_a_src, const float* a_dst,
                                int32_t ld_a_dst, int32_t heads, int32_t channels, float negative_slope, int32_t self_loops,
                                float* out, int32_t ld_out, float* lse, void* workspace, size_t workspace_bytes, double p,
                                const int64_t* seed, egc_stream_t stream);
int egc_gat_backward_dropout_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                 const int32_t* t_edge_id, int64_t n_rows, int64_t n_edges, const float* xl, int32_t ld_xl,
                                 const float* a_src, int32_t ld_a_src, const float* a_dst, int32_t ld_a_dst, int32_t heads,
                                 int32_t channels, float negative_slope, int32_t self_loops, const float* out, int32_t ld_out,
                                 const float* lse, const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* d_a_src,
                                 int32_t ld_d_a_src, float* d_a_dst, int32_t ld_d_a_dst, void* workspace, size_t workspace_bytes,
                                 double p, const int64_t* seed, egc_stream_t stream);
int egc_gatv2_forward_dropout_f32(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                                  const float* xl, int32_t ld_xl, const float* xr, int32_t ld_xr, const float* att, int32_t heads,
                                  int32_t channels, float negative_slope, int32_t self_loops, float* out, int32_t ld_out,
                                  float* lse, void* workspace, size_t workspace_bytes, double p, const int64_t* seed,
                                  egc_stream_t stream);
int egc_gatv2_backward_dropout_f32(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                   const int32_t* t_edge_id, int64_t n_rows, int64_t n_edges, const float* xl, int32_t ld_xl,
                                   const float* xr, int32_t ld_xr, const float* att, int32_t heads, int32_t channels,
                                   float negative_slope, int32_t self_loops, const float* out, int32_t ld_out, const float* lse,
                                   const float* g, int32_t ld_g, float* dxl, int32_t ld_dxl, float* dxr, int32_t ld_dxr, float* datt,
                                   void* workspace, size_t workspace_bytes, double p, const int64_t* seed, egc_stream_t stream);

/* Training form of egc_aggregate_combine_f32: same `out`, plus what the backward needs instead of a second
 * gather.  stats (n_nodes * egc_train_stats_floats(layer) floats, opaque to the caller, handed to the backward
 * as it is) receives every row's raw running aggregates after the self-loop term (those of sum / variance -- as the
 * forward forms it, so that the backward's relu mask and std are the forward's -- / max / min / symnorm-weighted sum
 * that the aggregator list uses, [n_nodes][k][ldb]) and, behind them, the arg
 * positions below as one byte each relative to the row's first entry (what the backward gathers per transposed
 * entry: 64 instead of 256 bytes at the north star); cnt [n_nodes] the size of the row's aggregation set.  arg_max / arg_min
 * (each [n_nodes, ldb] int32; NULL allowed when the layer has no max / min aggregator) receive, per basis
 * column, the CSR entry position of the FIRST entry attaining the extremum -- graph.col[pos] is its source,
 * graph.edge_id[pos] its position in the input edge list, i.e. what torch_scatter's scatter_max/min return
 * as `arg` and autograd routes the gradient through -- n_edges for the appended self-loop of a LOOPED set,
 * -1 for an empty row. */
int64_t egc_train_stats_floats(const egc_layer* layer);
int egc_aggregate_combine_train_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                                    const float* weightings, const float* bias, float* out, float* stats,
                                    int32_t* cnt, int32_t* arg_max, int32_t* arg_min, void* workspace,
                                    size_t workspace_bytes, egc_stream_t stream);
/* The same over rows [row_begin, row_end) only, all arrays full-size (the training counterpart of
 * egc_aggregate_combine_rows_f32: on a vertex partition the interior rows are finished while the halo rows of `bases`
 * travel).  The ranges of one forward are issued in ascending order and the last one ends at n_nodes. */
int egc_aggregate_combine_train_rows_f32(const egc_graph* graph, const egc_layer* layer, const float* bases, int32_t ldb,
                                         const float* weightings, const float* bias, float* out, float* stats,
                                         int32_t* cnt, int32_t* arg_max, int32_t* arg_min, int64_t row_begin,
                                         int64_t row_end, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batches of small graphs (BASELINE configs 3 / 4): the aggregate+combine launch on TILES OF WHOLE GRAPHS, with the
 * graph preparation inside it (egc_aggregate_tile.hip).  The reference's batched nets call the layer with a PyG batch
 * (zinc/models.py:60-74, mol/pna_style_models.py:64-79, cifar/models.py:61-75): graphs numbered one after the other
 * (`batch.ptr` = their node offsets), the edges of one graph contiguous in `edge_index` -- a block-diagonal adjacency.
 *   egc_batch_tile_nodes   lds_nodes: how many nodes' basis rows (ldb floats each) fit the LDS of one workgroup (two per
 *                          CU) next to the per-tile CSR areas for (max_tile_nodes, max_tile_edges); 0 = the layer does not
 *                          qualify (envelope of the register-resident kernels: <= 64 slots per row, A <= 4, B a power
 *                          of two, no softmax).  A tile of at most lds_nodes nodes gathers its basis rows from LDS, a
 *                          larger one (up to max_tile_nodes) from memory like the ordinary kernels.
 *   egc_batch_plan         once per batch, one launch: cuts [0, n_nodes) into n_slots = ceil(n_nodes / slot) slots; the
 *                          graphs whose first node lies in slot k form one tile (n0, n1, e0, e1) -- node range and edge
 *                          range; the non-empty tiles are written to tiles[4 i ..] in any order and counted in *n_tiles
 *                          (device).  A tile holds < slot + (largest graph) nodes.  graph_ptr: int64 [n_graphs + 1];
 *                          edge_ptr: the graphs' edge offsets, int64 [n_graphs + 1] (PyG keeps them for a collated batch),
 *                          or NULL: found by searching the destination row of edge_index.
 *   egc_aggregate_combine_batch_f32
 *                          contract of egc_aggregate_combine_post_f32 (same reference call sites; plus those of
 *                          egc_graph_build: no CSR is built beforehand) for the rows of every tile, straight from the
 *                          COO lists src / dst; n_tiles_bound = n_slots (sizes the persistent launch).  ldw = row stride of
 *                          weightings (0 = dense).  max_index: device scalar, needed only by layers with
 *                          loops_all_nodes = 0.  Inference form.
 * Every edge is checked against its tile: an edge that leaves the tile (list not grouped by graph, id out of range) or a
 * tile beyond max_tile_nodes / max_tile_edges raises *status (bit 0 / bit 1; zero it before the call) and the sticky
 * *host_flag (see egc_coo_to_csr_checked); the rows of such a tile are written as zeros.  A row's entries are summed in the order of
 * the edge list (round 6: the tile's CSR is built in input order -- the order the reference's CPU scatter sums a row in): results are
 * bit-reproducible and bit-identical to egc_aggregate_combine_post_f32 on the CSR of the same batch.
 * ------------------------------------------------------------------------------------------ */
int32_t egc_batch_tile_nodes(const egc_layer* layer, int32_t max_tile_nodes, int32_t max_tile_edges, int32_t with_post);
int egc_batch_plan(const int64_t* graph_ptr, const int64_t* edge_ptr, int64_t n_graphs, const int64_t* dst, int64_t n_edges,
                   int64_t n_nodes, int32_t slot, int32_t* tiles, int32_t n_slots, int32_t* n_tiles, egc_stream_t stream);
int egc_aggregate_combine_batch_f32(const int32_t* tiles, const int32_t* n_tiles, int32_t n_tiles_bound, int32_t lds_nodes,
                                    int32_t max_tile_nodes, int32_t max_tile_edges, const int64_t* src, const int64_t* dst,
                                    int64_t n_nodes, const int32_t* max_index, const egc_layer* layer, const float* bases,
                                    int32_t ldb, const float* weightings, int32_t ldw, const float* bias, const egc_post* post,
                                    float* out, int32_t* status, int32_t* host_flag, egc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batches of small graphs, the WHOLE layer in ONE launch (egc_fused_tile.hip): per tile of whole graphs
 *   x rows -> basis transform + weightings Linear on the matrix cores -> LDS -> CSR of the tile's edges in LDS ->
 *   multi-aggregator reduction -> combine (+ bias, egc_post tail) -> out.
 * Neither `bases` nor `weightings` exist in memory and there is no plan launch: every workgroup finds its own tiles from
 * graph_ptr (and edge_ptr, or by searching the destination row of edge_index when it is NULL).
 * Replaces, for such batches, ALL the reference call sites of egc_basis_transform_packed + egc_graph_build +
 * egc_aggregate_combine_post_f32: torch.matmul(x, bases_weight), comb_weight(x) (experiments/layers.py:97-101,110;
 * optimized_layers.py:180-182), gcn_norm / add_remaining_self_loops (optimized_layers.py:127-175; layers.py:172-188),
 * MessagePassing.propagate + scatter per aggregator (optimized_layers.py:186-249; layers.py:191-219), the combine and bias
 * (optimized_layers.py:195-208; layers.py:127-138), and the caller's bn(eval) -> relu -> + identity (zinc/models.py:66-73,
 * cifar/models.py:64-71, mol/pna_style_models.py:70-78).
 *   egc_batch_fused_tile_nodes  rows of a tile whose image (bases + weightings rows, CSR areas for max_tile_edges entries)
 *                               fits the LDS of one CU; 0 = the layer is outside this kernel's envelope.  Two forms share the
 *                               entry points: the register-stationary one (F_in <= 128, ldb + H B A <= 192: the d = 128
 *                               layers) and, since round 5, the WIDE one for the reference's own wider batched nets
 *                               (run_pretrained.sh:7,12,23,24 -- 168 / H8 / B4, 296 / H8 / B4, 224 / H4 / B4): F_in <= 320,
 *                               round32(ldb) + H B A <= 384, weight fragments streamed from L2; both need F_in % 4 == 0 and
 *                               the register-resident aggregate kernels' envelope (ldb <= 256, B a power of two, A <= 4).
 *                               A batch whose largest graph has more nodes than this must take
 *                               egc_aggregate_combine_batch_f32 or the CSR path.  The answer is a tile the launch runs: 0 also
 *                               for a max_tile_edges the launch refuses whatever tile_nodes is (negative, or above 65535).
 *   egc_batch_fused_tile_quantum  rows per matrix-core step of the form that serves the layer (16 / 32; 0 = outside):
 *                               tile_nodes must be a multiple of it.
 *   egc_batch_fused_pack_bytes / egc_batch_fused_pack
 *                               wcat [F_in, F_g + W] (+ bcat [W] or NULL) -> the two fp16 weight planes in MFMA fragment
 *                               order + column scales + comb bias; once per parameter update.
 *   egc_layer_forward_batch_fused_f32
 *                               the launch.  tile_nodes: a multiple of egc_batch_fused_tile_quantum, <= egc_batch_fused_tile_nodes(...); status /
 *                               host_flag as egc_aggregate_combine_batch_f32 (bit 0: an edge leaves its tile or the graph
 *                               offsets do not cover [0, n_nodes); bit 1: a tile beyond tile_nodes / max_tile_edges -- the
 *                               rows of such a tile are written as zeros; bit 2: the workgroup-internal hand-over between
 *                               the wavefronts that build a tile's CSR timed out -- a bounded spin, never a hang; the
 *                               launch's output is then undefined).  Inference form, fp16x2-split GEMM (22-bit operands,
 *                               fp32 accumulate: the arithmetic of egc_basis_transform_packed at the north-star shape).
 *                               A row's entries are summed in the order of the edge list (round 6; the reference's CPU
 *                               scatter order): bit-reproducible; max_tile_edges <= 65535 (16-bit cursors of the CSR build).
 * ------------------------------------------------------------------------------------------ */
int32_t egc_batch_fused_tile_nodes(const egc_layer* layer, int32_t max_tile_edges, int32_t with_post);
int32_t egc_batch_fused_tile_quantum(const egc_layer* layer);
int64_t egc_batch_fused_pack_bytes(const egc_layer* layer);
int egc_batch_fused_pack(const egc_layer* layer, const float* wcat, const float* bcat, void* packed, int64_t packed_bytes,
                         egc_stream_t stream);
int egc_layer_forward_batch_fused_f32(const int64_t* graph_ptr, const int64_t* edge_ptr, int64_t n_graphs, const int64_t* src,
                                      const int64_t* dst, int64_t n_edges, int64_t n_nodes, const int32_t* max_index,
                                      const egc_layer* layer, const float* x, const void* packed, const float* bias,
                                      const egc_post* post, float* out, int32_t tile_nodes, int32_t max_tile_edges,
                                      int32_t* status, int32_t* host_flag, egc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The BACKWARD of egc_layer_forward_batch_fused_f32, tile-local, in ONE launch (round 5; egc_fused_tile.hip, MODE 1): what
 * PyTorch autograd derives through the layer for a PyG batch in the reference's training loops (zinc/configs.py:53-72:
 * loss.backward() through zinc/models.py:60-74 -> layers.py:89-140 / optimized_layers.py:177-210) -- the backward of the two
 * Linears, of propagate's gathers and of the per-aggregator scatters -- without a CSR, a transposed CSR or any saved
 * intermediate: per tile of whole graphs the forward's `bases` / `weightings` and aggregates are formed again in LDS,
 * d weightings = <grad_out, aggregates>, d aggregates = weightings x grad_out travel to the sources' rows of an LDS image kept as
 * 64-bit fixed point (integer LDS atomics: order-independent sums; the scale comes from the tile's largest |grad_out| and |weightings|,
 * 34 bits under the bound -- float LDS atomics run at one lane per clock per CU on gfx950)
 * (sum / mean / symnorm along every entry, max to the FIRST entry in input order attaining it: torch_scatter's arg rule), and
 *   d_x   [n_nodes, in_channels]  = [d bases | d weightings] [bases_weight | comb_weight^T]^T   (split-precision MFMA GEMM)
 *   d_cat [n_nodes, ld_dcat]      = the gradient of [bases (ldb) | pre-activation weightings (H B A, column (h B + b) A + a)]
 * leave the launch (d_cat may be NULL; the caller's weight gradient is x^T d_cat: egc_weight_grad_*).  Two launches on the same inputs
 * agree to the bit (round 6: the tile's CSR is built in input order; a tile whose grad_out or weightings hold an Inf / NaN leaves its
 * d bases rows -- and with them its rows of d_x -- as NaN instead of a fixed-point image of them).  Envelope (egc_batch_fused_bwd_tile_nodes > 0): B = 4 bases of 16 channels, H = 4 or 8
 * (the d = 64 / 128 layers), F_in <= 128, aggregators of sum / mean / max / symnorm, no weight nonlinearity.
 *   egc_batch_fused_bwd_tile_nodes   rows of a tile (its image also holds d bases, 512 B per row: 80 at the north star), 0 = outside,
 *                                    and 0 for a max_tile_edges the launch refuses whatever tile_nodes is (negative, or above 16384:
 *                                    the query used to answer the rows whose image fits, e.g. 48 at H = 4 and 20000 edges)
 *   egc_batch_fused_bwd_pack[_bytes] wcat -> the transposed operand's fp16 planes; once per parameter update
 *   egc_layer_backward_batch_fused_f32   `packed` = egc_batch_fused_pack's buffer (the forward operand, for the recompute);
 *                                    `d_x_add` [n_nodes, in_channels] or NULL: added to d_x in its store -- the gradient that
 *                                    reaches x past the layer (the residual branch of the reference's blocks, zinc/models.py:
 *                                    70-73: x = x + relu(bn(conv(x)))), which autograd otherwise adds in a pass of its own;
 *                                    status / host_flag as the forward launch.
 * ------------------------------------------------------------------------------------------ */
int32_t egc_batch_fused_bwd_tile_nodes(const egc_layer* layer, int32_t max_tile_edges);
int64_t egc_batch_fused_bwd_pack_bytes(const egc_layer* layer);
int egc_batch_fused_bwd_pack(const egc_layer* layer, const float* wcat, void* packed_t, int64_t packed_bytes, egc_stream_t stream);
/* egc_batch_fused_pack + egc_batch_fused_bwd_pack of the same wcat in one launch (a training step packs both once per update) */
int egc_batch_fused_train_pack(const egc_layer* layer, const float* wcat, const float* bcat, void* packed, int64_t packed_bytes,
                               void* packed_t, int64_t packed_t_bytes, egc_stream_t stream);
/* ... straight from the module's parameters through the index map of egc_weights_pack_f32 (bases_parts: ONE [F_in][B L] matrix or B of
 * [F_in][L]; comb_weight [H B A][F_in], its rows [h][a][b] with permute_hab (EGConv) or [h][b][a]; comb_bias in the rows' order, or
 * bcat in the operand's order, or neither): no wcat / bcat arrays and no pack launch in front. */
int egc_batch_fused_train_pack_params(const egc_layer* layer, const float* const* bases_parts, int32_t n_parts, const float* comb_weight,
                                      const float* comb_bias, const float* bcat, int32_t num_heads, int32_t num_aggrs, int32_t num_bases,
                                      int32_t basis_len, int32_t basis_stride, int32_t permute_hab, void* packed, int64_t packed_bytes,
                                      void* packed_t, int64_t packed_t_bytes, egc_stream_t stream);
int egc_layer_backward_batch_fused_f32(const int64_t* graph_ptr, const int64_t* edge_ptr, int64_t n_graphs, const int64_t* src,
                                       const int64_t* dst, int64_t n_edges, int64_t n_nodes, const int32_t* max_index,
                                       const egc_layer* layer, const float* x, const void* packed, const void* packed_t,
                                       const float* grad_out, float* d_x, const float* d_x_add, float* d_cat, int32_t ld_dcat,
                                       int32_t tile_nodes, int32_t max_tile_edges, int32_t* status, int32_t* host_flag,
                                       egc_stream_t stream);

/* Whole layer forward = egc_basis_transform_f32 + egc_aggregate_combine_f32
 * (EfficientGraphConv.forward layers.py:89-140 / EGConv.forward optimized_layers.py:177-210
 * after graph preparation).  bases [N,ldb] and weightings [N,W] are caller-provided intermediates. */
int egc_layer_forward_f32(const egc_graph* graph, const egc_layer* layer, const float* x, const float* wcat,
                          const float* bcat, const float* bias, float* bases, int32_t ldb, float* weightings,
                          float* out, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* Same as egc_layer_forward_f32 with the GEMM in its packed split-precision form (the default production path).
 * Folded weightings: when the layer's four aggregators hold sum and mean once each and symnorm over the same edge set,
 * in HBA order with no weight nonlinearity, and the GEMM is the fp16x2 kernel, mean's weighting is folded into sum's
 * (w_sum + w_mean / max(cnt, 1), cnt = the row's entry count, from the graph's deg^-1/2 table of that edge set) and
 * `weightings` then holds [N, H*B*3]: the (h, b) pairs in HBA order, each with the layer's aggregators minus mean, in
 * their order.  The aggregate forms no mean.  Results agree with the unfolded calls to a few fp32 roundings. */
int egc_layer_forward_packed(const egc_graph* graph, const egc_layer* layer, const float* x, const void* packed,
                             const float* bcat, const float* bias, float* bases, int32_t ldb, float* weightings,
                             float* out, void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* Backward of egc_aggregate_combine_train_f32 (in the reference PyTorch autograd derives
 * it through layers.py:103-138 / optimized_layers.py:186-208).  Inputs: the forward's `bases`, PRE-activation
 * `weightings` (layout HBA), `stats`, `cnt`, `arg_max` / `arg_min`; grad_out = dL/d out [n_nodes, out_channels];
 * and t_graph = the TRANSPOSED graph (rows = sources, entries = destinations: egc_coo_to_csr with src/dst
 * swapped, then egc_csr_prepare for its long-row plan; its dis_* arrays are not used).  With max / min
 * aggregators the transposed graph must be built from the edge list in DESTINATION-CSR ORDER (edge k = CSR
 * entry k: source graph.col[k], destination = k's row), so that t_graph.edge_id maps a transposed entry to the
 * CSR position that arg_max / arg_min name.
 * Outputs: d_bases [n_src_rows, ldb] -- on a square graph (n_src_rows == n_nodes) every row is written and the
 * array may hold anything on entry; on a rectangular one it MUST be zero-filled by the caller (the partial sums
 * of hub rows arrive by float atomics) -- and d_weightings [n_nodes, H*B*A] (gradient w.r.t. the
 * pre-activation weightings).  ld_d_bases / ld_d_weightings are their row strides in floats (0 = dense: ldb
 * and H*B*A; ld_d_bases a multiple of 4, d_bases 16-byte aligned): a caller whose next step is a GEMM with
 * the concatenated weight matrix [bases_weight | comb_weight^T] passes two column blocks of ONE
 * [n_nodes, ldb + H*B*A] array and saves the concatenation.  The dense gradients (x, bases_weight, comb
 * weight/bias, bias) are plain GEMMs / column sums left to the caller.
 * Workspace: egc_backward_workspace_bytes(layer, n_nodes) holds the per-destination tables; with
 * egc_backward_workspace_bytes_for(layer, graph) bytes (64 more per entry and max / min aggregator) the gradients of
 * max / min travel as one 64-byte record per entry instead of arg bytes + pieces of the X rows (round 3: the source
 * kernel then fetches payload, not sectors).  Either size is accepted; the results are the same.  Round 6: the larger size is
 * returned (and records are built) only where an entry receives at most ten columns on average (ldb * n_nodes / n_edges: 4.6 on
 * the ogbn-arxiv graph at 64 basis columns); on batches of small graphs at wide layers (108 at 224 columns on a molecule batch)
 * every 12-item record overflowed, and both sizes are the tables' size there. */
size_t egc_backward_workspace_bytes(const egc_layer* layer, int64_t n_nodes);
size_t egc_backward_workspace_bytes_for(const egc_layer* layer, const egc_graph* graph);
int egc_aggregate_combine_backward_f32(const egc_graph* graph, const egc_graph* t_graph, const egc_layer* layer,
                                       const float* bases, int32_t ldb, const float* weightings,
                                       const float* grad_out, const float* stats, const int32_t* cnt,
                                       const int32_t* arg_max, const int32_t* arg_min, float* d_bases,
                                       int32_t ld_d_bases, float* d_weightings, int32_t ld_d_weightings,
                                       void* workspace, size_t workspace_bytes, egc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mini-batch collation on the device (egc_collate.hip).  The reference's batched nets take their batches from PyG's
 * DataLoader: per-graph collation in Python on the CPU, then `batch.to(device)` (zinc/configs.py:53-67,
 * mol/configs.py:52-70, cifar/configs.py:66-82, code/configs.py:47-69).  Here the dataset lives on the device
 * (egc_collate_store: M graphs back to back, node ids of edge_index LOCAL to their graph, a graph's edges contiguous) and
 * one call writes a batch of up to batch_size = G graphs into static buffers padded to n_pad rows and e_pad edges -- the
 * convention of a recorded step (egc_amd/hipgraph.py): zero feature rows, padding rows in a spare last graph G, padding
 * edges as self-loops on row n_pad - 1.  Slot i of the batch is graph ids[i], i < n_ids (1 <= n_ids <= G, repeats allowed);
 * or, with ids == NULL, graph perm[c G + i] of batch c = *cursor of an epoch of floor(*perm_len / G) full batches -- cursor
 * and perm_len are DEVICE words read by the kernel, a cursor outside the epoch counts as 0, and c + 1 is stored back, so
 * the same recorded launch serves successive batches and wraps.  perm has room for store->n_graphs entries.
 * With g_valid graphs kept, n_valid rows and e_valid edges, EVERY element of every output is written by every call:
 *   node field dst [n_pad, row]   rows of the kept graphs in batch order; rows >= n_valid all-zero bytes
 *   out->edge_index [2, e_pad]    local id + the slot's row offset; columns >= e_valid (n_pad - 1, n_pad - 1)
 *   out->batch [n_pad]            the slot of each row; rows >= n_valid hold G
 *   out->ptr, edge_ptr [G + 2]    row / edge offset of slots 0 .. G (slots >= g_valid repeat n_valid / e_valid); last n_pad / e_pad
 *   out->n_valid, e_valid, g_valid   int64 scalars
 *   out->counts [G + 1] float     rows of the slot; 1 for a slot without rows and for the spare graph
 *   out->graph_mask [G + 1] float 1 for slots < g_valid, else 0;  out->inv_g = (float)(1.0 / max(g_valid, 1))
 *   graph field dst [G + 1, row]  the graph's row; the field's fill element (fill_bits, low elem_bytes bytes) in slots that hold no
 *                                 graph: slots >= g_valid, the spare graph, and a slot whose id is out of range
 * Malformed input never addresses anything and is always reported: an id outside [0, n_graphs) is an empty slot (status bit
 * 1); the first graph with which the rows would exceed n_pad - 1 (bit 2) or the edges e_pad (bit 4), and every graph after
 * it, are dropped.  The bits are OR-ed into *out->status (device, cleared by the caller) and *host_flag = 1 is stored (may
 * be NULL; the sticky host-visible word of egc_coo_to_csr_checked).
 * Fields: at most EGC_COLLATE_MAX_FIELDS of each kind, elements of 4 or 8 bytes, contiguous rows of at most
 * EGC_COLLATE_MAX_ROW_BYTES bytes, pointers aligned to the element; 16- and 8-byte accesses where the row size and both
 * base addresses are multiples of 16 / 8.  The structs are read during the call and travel in the kernel arguments.
 * workspace: egc_collate_workspace_bytes(batch_size) bytes (0 outside 1 .. EGC_COLLATE_MAX_GRAPHS), 8-byte aligned, any
 * content.  Two launches whatever the fields; launch sizes depend on batch_size, n_pad, e_pad alone.
 * EGC_ERR_INVALID: a missing pointer, n_ids outside 1 .. batch_size, n_pad or e_pad < 1, a row size that is no multiple of
 * its element, a misaligned field; EGC_ERR_UNSUPPORTED: batch_size > EGC_COLLATE_MAX_GRAPHS, n_pad or e_pad >= 2^31, too
 * many fields, an element size other than 4 / 8, a row over the limit; EGC_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------ */
#define EGC_COLLATE_MAX_FIELDS 8
#define EGC_COLLATE_MAX_GRAPHS 4096
#define EGC_COLLATE_MAX_ROW_BYTES 4096
typedef struct {
  const void* src;     /* [rows of the store, row_bytes] */
  void* dst;           /* [n_pad or G + 1, row_bytes] */
  int32_t row_bytes;
  int32_t elem_bytes;  /* 4 or 8 */
  uint64_t fill_bits;  /* graph fields: bit pattern of the fill element (low 32 bits for 4-byte elements); node fields: unused */
} egc_collate_field;
typedef struct {
  int32_t n_node, n_graph;
  egc_collate_field node[EGC_COLLATE_MAX_FIELDS];
  egc_collate_field graph[EGC_COLLATE_MAX_FIELDS];
} egc_collate_fields;
typedef struct {
  const int64_t* node_ptr;    /* [n_graphs + 1] non-decreasing */
  const int64_t* edge_ptr;    /* [n_graphs + 1] non-decreasing */
  const int64_t* edge_index;  /* [2, n_edges_all] node ids local to their graph */
  int64_t n_graphs;
  int64_t n_edges_all;
} egc_collate_store;
typedef struct {
  int64_t* edge_index;
  int64_t* batch;
  int64_t* ptr;
  int64_t* edge_ptr;
  int64_t* n_valid;
  int64_t* e_valid;
  int64_t* g_valid;
  float* counts;
  float* graph_mask;
  float* inv_g;
  int32_t* status;
} egc_collate_out;
size_t egc_collate_workspace_bytes(int32_t batch_size);
int egc_collate(const egc_collate_store* store, const egc_collate_fields* fields, const egc_collate_out* out,
                const int64_t* ids, int64_t n_ids, const int64_t* perm, const int64_t* perm_len, int64_t* cursor,
                int32_t batch_size, int64_t n_pad, int64_t e_pad, void* workspace, size_t workspace_bytes,
                int32_t* host_flag, egc_stream_t stream);

/* Human-readable text of the last HIP failure seen on the calling thread ("" if none). */
const char* egc_last_error(void);

/* Library build tag: "egc_hip <version> gfx950". */
const char* egc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EGC_HIP_H */
