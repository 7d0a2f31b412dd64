"""ctypes binding of libegc_hip.so (the C ABI declared in include/egc_hip.h).

There is NO CPU fallback: if the shared library is missing or cannot be loaded, every entry point
raises RuntimeError.  Build it with ``egc_amd/csrc/build.sh`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

_LIB_PATH = os.environ.get("EGC_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                         "libegc_hip.so")
_lib = None

EGC_MAX_AGGRS = 8
LONG_ROW_THRESHOLD = 64
LONG_ROW_CHUNK = 256

# enum egc_aggr
AGGR_SUM, AGGR_MEAN, AGGR_MAX, AGGR_MIN, AGGR_VAR, AGGR_STD, AGGR_SYMNORM = range(7)
# enum egc_edge_set
SET_RAW, SET_LOOPED = 0, 1
# enum egc_weight_layout
LAYOUT_HBA, LAYOUT_HAB = 0, 1
# enum egc_weight_act
ACT_NONE, ACT_SOFTMAX, ACT_SIGMOID, ACT_HARDTANH = range(4)
# EGC_READOUT_*
READOUT_SUM, READOUT_MEAN, READOUT_MAX = range(3)
SOFTMAX_MAX_CLASSES = 1024   # EGC_SOFTMAX_MAX_CLASSES
TYPED_MAX_RELATIONS = 8      # EGC_TYPED_MAX_RELATIONS
TOKEN_HEAD_MAX_SEQ = 8       # EGC_TOKEN_HEAD_MAX_SEQ
TOKEN_HEAD_SLAB = 64         # EGC_TOKEN_HEAD_SLAB: vocabulary columns of one workgroup step
TOKEN_HEAD_MAX_IN = 384      # widest in_features of the token head's kernels
# EGC_HEAD_*: the envelope of the graph-level MLP head's kernels, its row tile and its fused losses
HEAD_MAX_LINEARS = 4
HEAD_MAX_WIDTH = 384
HEAD_MAX_OUT = 64
HEAD_MAX_ROWS = 65536
HEAD_ROW_TILE = 16
HEAD_LOSS_NONE, HEAD_LOSS_L1, HEAD_LOSS_BCE_MASKED = range(3)
# EGC_COLLATE_*: fields of each kind, graphs per batch, bytes per field row of the device-side collation
COLLATE_MAX_FIELDS = 8
COLLATE_MAX_GRAPHS = 4096
COLLATE_MAX_ROW_BYTES = 4096
# EGC_MPNN_*
MPNN_ADD, MPNN_MEAN, MPNN_MAX = range(3)
# EGC_PNA_* aggregators and scalers
PNA_SUM, PNA_MEAN, PNA_MIN, PNA_MAX, PNA_VAR, PNA_STD = range(6)
PNA_IDENTITY, PNA_AMPLIFICATION, PNA_ATTENUATION, PNA_LINEAR, PNA_INVERSE_LINEAR = range(5)
# EGC_NBR_*
NBR_SUM, NBR_MEAN, NBR_MEAN_T, NBR_SYM = range(4)
# EGC_GP_*: header words of a gather plan, its forms
GP_HEADER_INTS = 16
GP_FORM, GP_COL_BITS, GP_TABLE_SIZE = range(3)
GP_PACKED, GP_UNFIT = 1, 2

_STATUS = {1: "EGC_ERR_INVALID", 2: "EGC_ERR_WORKSPACE", 3: "EGC_ERR_HIP", 4: "EGC_ERR_UNSUPPORTED"}


class EgcGraph(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64), ("n_edges", C.c_int64),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("edge_id", C.c_void_p),
        ("dis_raw", C.c_void_p), ("dis_looped", C.c_void_p),
        ("max_index", C.c_void_p), ("plan", C.c_void_p), ("n_chunks", C.c_int64),
        ("n_src_rows", C.c_int64), ("edge_dis_raw", C.c_void_p), ("edge_dis_looped", C.c_void_p),
        ("gather_plan_raw", C.c_void_p), ("gather_plan_looped", C.c_void_p),
        ("gather_plan_form_raw", C.c_int32), ("gather_plan_form_looped", C.c_int32),
    ]


class EgcLayer(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_heads", C.c_int32),
        ("num_bases", C.c_int32), ("num_aggrs", C.c_int32), ("aggrs", C.c_int32 * EGC_MAX_AGGRS),
        ("agg_set", C.c_int32), ("sym_set", C.c_int32), ("loops_all_nodes", C.c_int32),
        ("weight_layout", C.c_int32), ("weight_act", C.c_int32), ("basis_stride", C.c_int32),
    ]


_ENV_DATA = getattr(os.environ, "_data", None)     # CPython on POSIX: the bytes dict behind os.environ


def env_flag(name: str) -> bool:
    """True when the environment variable is set to something other than "" / "0" -- read on every call (tests and
    notebooks flip these), but through the bytes dict behind os.environ where CPython has one: os.environ.get costs
    1.5 us per lookup (key encoding + value decoding), four of them were a quarter of an eval-mode layer call."""
    if _ENV_DATA is not None:
        v = _ENV_DATA.get(name.encode())
        return v is not None and v not in (b"", b"0")
    return os.environ.get(name, "0") not in ("", "0")


class EgcPost(C.Structure):
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("residual", C.c_void_p), ("relu", C.c_int32)]


class EgcTypedRel(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("pre_rowptr", C.c_void_p), ("in_", C.c_void_p),
                ("n_edges", C.c_int64), ("n_in_rows", C.c_int64), ("ld_in", C.c_int32), ("out_col", C.c_int32),
                ("post_mean", C.c_int32), ("reserved", C.c_int32)]


class EgcHead(C.Structure):
    _fields_ = ([("n_linears", C.c_int32), ("sizes", C.c_int32 * (HEAD_MAX_LINEARS + 1))]
                + [(name, C.c_void_p * HEAD_MAX_LINEARS)
                   for name in ("weight", "bias", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked")]
                + [("eps", C.c_double * HEAD_MAX_LINEARS), ("momentum", C.c_double * HEAD_MAX_LINEARS)]
                + [(name, C.c_void_p * HEAD_MAX_LINEARS) for name in ("z", "stats", "affine", "dz", "g", "coef", "d_weight", "d_bias")])


class EgcCollateField(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int32), ("elem_bytes", C.c_int32),
                ("fill_bits", C.c_uint64)]


class EgcCollateFields(C.Structure):
    _fields_ = [("n_node", C.c_int32), ("n_graph", C.c_int32), ("node", EgcCollateField * COLLATE_MAX_FIELDS),
                ("graph", EgcCollateField * COLLATE_MAX_FIELDS)]


class EgcCollateStore(C.Structure):
    _fields_ = [("node_ptr", C.c_void_p), ("edge_ptr", C.c_void_p), ("edge_index", C.c_void_p), ("n_graphs", C.c_int64),
                ("n_edges_all", C.c_int64)]


class EgcCollateOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("edge_index", "batch", "ptr", "edge_ptr", "n_valid", "e_valid", "g_valid",
                                                "counts", "graph_mask", "inv_g", "status")]


# name -> (restype, argtypes): exactly the symbols include/egc_hip.h declares
SYMBOLS = {
    "egc_plan_ints": (C.c_int64, [C.c_int64, C.c_int64]),
    "egc_coo_to_csr_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "egc_coo_to_csr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_coo_to_csr_checked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_graph_build_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "egc_graph_build_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "egc_graph_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_csr_edge_dis": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_gather_plan_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "egc_gather_plan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "egc_gather_plan_offset": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "egc_gather_plan_form": (C.c_int32, [C.c_int64, C.c_int64, C.c_int32]),
    "egc_gather_plan_build": (C.c_int, [C.POINTER(EgcGraph), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "egc_gather_plan_launches": (C.c_int64, []),
    "egc_csr_prepare": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "egc_bases_ld": (C.c_int32, [C.POINTER(EgcLayer)]),
    "egc_basis_transform_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_basis_pack_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "egc_basis_pack": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_layer_gemm_flags": (C.c_int32, [C.POINTER(EgcLayer)]),
    "egc_basis_pack_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_basis_transform_packed_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_basis_transform_packed_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_basis_pack_transposed": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    "egc_basis_transform_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_layer_forward_packed": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_aggregate_workspace_bytes": (C.c_size_t, [C.POINTER(EgcLayer), C.c_int64, C.c_int64]),
    "egc_aggregate_workspace_zero_bytes": (C.c_size_t, [C.POINTER(EgcLayer), C.c_int64, C.c_int64]),
    "egc_aggregate_workspace_bytes_for": (C.c_size_t, [C.POINTER(EgcLayer), C.POINTER(EgcGraph)]),
    "egc_aggregate_combine_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_layer_forward_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_backward_workspace_bytes": (C.c_size_t, [C.POINTER(EgcLayer), C.c_int64]),
    "egc_backward_workspace_bytes_for": (C.c_size_t, [C.POINTER(EgcLayer), C.POINTER(EgcGraph)]),
    "egc_aggregate_combine_rows_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_aggregate_combine_post_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.POINTER(EgcPost), C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_aggregate_combine_strided_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(EgcPost), C.c_void_p,
                                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_weight_grad_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "egc_weight_grad_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "egc_weight_grad_ex_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "egc_weight_grad_ex_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    "egc_weight_grad_params_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p]),
    "egc_weight_grad_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egc_csr_transposed_coo": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_column_moments_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float,
                                         C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_bn_forward_stats_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_bn_backward_stats_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int64,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "egc_bn_backward_stats_sums_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int64,
                                                 C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_bn_forward_finalize": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_double,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "egc_bn_backward_finalize": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "egc_affine_act_residual_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float,
                                              C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_affine_act_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "egc_weights_pack_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    "egc_sum_partials_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_column_sums_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "egc_segment_mean_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_segment_reduce_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "egc_segment_reduce_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_encoder_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_encoder_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "egc_encoder_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_log_softmax_forward_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "egc_log_softmax_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_row_selection_count": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_nll_log_softmax_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "egc_nll_log_softmax_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                  C.c_void_p]),
    "egc_nll_log_softmax_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_token_head_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "egc_token_head_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p]),
    "egc_token_head_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]),
    "egc_head_workspace_bytes": (C.c_size_t, [C.POINTER(EgcHead), C.c_int64]),
    "egc_head_forward_train_f32": (C.c_int, [C.POINTER(EgcHead), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "egc_head_forward_eval_f32": (C.c_int, [C.POINTER(EgcHead), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egc_head_backward_f32": (C.c_int, [C.POINTER(EgcHead), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "egc_l1_loss_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egc_l1_loss_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egc_bce_masked_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egc_bce_masked_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egc_head_launches": (C.c_int64, []),
    "egc_typed_mean_chunk": (C.c_int32, []),
    "egc_typed_mean_workspace_bytes": (C.c_size_t, [C.POINTER(EgcTypedRel), C.c_int32, C.c_int32]),
    "egc_typed_mean_f32": (C.c_int, [C.POINTER(EgcTypedRel), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_mpnn_message_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "egc_mpnn_message_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "egc_mpnn_message_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "egc_mpnn_message_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_pna_aggregate_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_void_p, C.c_int32]),
    "egc_pna_aggregate_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_pna_aggregate_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "egc_pna_aggregate_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_pna_scale_combine_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                            C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "egc_pna_scale_combine_backward_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "egc_nbr_sum_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "egc_nbr_sum_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_gatv2_forward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "egc_gatv2_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_gatv2_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "egc_gatv2_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_gat_forward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "egc_gat_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_gat_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "egc_gat_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    # attention dropout: the arguments of the plain entry points, t_edge_id after t_col (backward), p and the device seed before the stream
    "egc_gat_forward_dropout_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]),
    "egc_gat_backward_dropout_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_float, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                               C.c_double, C.c_void_p, C.c_void_p]),
    "egc_gatv2_forward_dropout_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                                C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]),
    "egc_gatv2_backward_dropout_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                                 C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p,
                                                 C.c_void_p]),
    "egc_train_stats_floats": (C.c_int64, [C.POINTER(EgcLayer)]),
    "egc_aggregate_combine_train_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_aggregate_combine_train_rows_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                                       C.c_void_p]),
    "egc_batch_tile_nodes": (C.c_int32, [C.POINTER(EgcLayer), C.c_int32, C.c_int32, C.c_int32]),
    "egc_batch_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_aggregate_combine_batch_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(EgcLayer), C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(EgcPost), C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "egc_batch_fused_tile_nodes": (C.c_int32, [C.POINTER(EgcLayer), C.c_int32, C.c_int32]),
    "egc_batch_fused_tile_quantum": (C.c_int32, [C.POINTER(EgcLayer)]),
    "egc_batch_fused_pack_bytes": (C.c_int64, [C.POINTER(EgcLayer)]),
    "egc_batch_fused_pack": (C.c_int, [C.POINTER(EgcLayer), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egc_layer_forward_batch_fused_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                    C.c_int64, C.c_void_p, C.POINTER(EgcLayer), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.POINTER(EgcPost), C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "egc_batch_fused_bwd_tile_nodes": (C.c_int32, [C.POINTER(EgcLayer), C.c_int32]),
    "egc_batch_fused_bwd_pack_bytes": (C.c_int64, [C.POINTER(EgcLayer)]),
    "egc_batch_fused_bwd_pack": (C.c_int, [C.POINTER(EgcLayer), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egc_batch_fused_train_pack": (C.c_int, [C.POINTER(EgcLayer), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
    "egc_batch_fused_train_pack_params": (C.c_int, [C.POINTER(EgcLayer), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                    C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "egc_layer_backward_batch_fused_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                     C.c_void_p, C.POINTER(EgcLayer), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]),
    "egc_gather_rows_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "egc_aggregate_combine_backward_f32": (C.c_int, [C.POINTER(EgcGraph), C.POINTER(EgcGraph), C.POINTER(EgcLayer),
                                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egc_collate_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "egc_collate": (C.c_int, [C.POINTER(EgcCollateStore), C.POINTER(EgcCollateFields), C.POINTER(EgcCollateOut), C.c_void_p,
                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                              C.c_size_t, C.c_void_p, C.c_void_p]),
    "egc_last_error": (C.c_char_p, []),
    "egc_version": (C.c_char_p, []),
}


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libegc_hip.so once; raise RuntimeError (never fall back) if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"egc_amd: HIP library not built: {_LIB_PATH} is missing. Run egc_amd/csrc/build.sh "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise RuntimeError(f"egc_amd: cannot load {_LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status: int, what: str):
    if status != 0:
        detail = load().egc_last_error().decode() if status == 3 else ""
        raise RuntimeError(f"egc_amd: {what} failed with {_STATUS.get(status, status)} {detail}".rstrip())


def make_layer(in_channels, out_channels, num_heads, num_bases, aggr_codes, agg_set, sym_set, loops_all_nodes,
               weight_layout, weight_act, basis_stride=0) -> EgcLayer:
    if len(aggr_codes) > EGC_MAX_AGGRS:
        raise RuntimeError(f"egc_amd: at most {EGC_MAX_AGGRS} aggregators are supported")
    arr = (C.c_int32 * EGC_MAX_AGGRS)(*(list(aggr_codes) + [0] * (EGC_MAX_AGGRS - len(aggr_codes))))
    return EgcLayer(in_channels, out_channels, num_heads, num_bases, len(aggr_codes), arr, agg_set, sym_set,
                    int(loops_all_nodes), weight_layout, weight_act, int(basis_stride))
