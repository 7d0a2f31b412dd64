"""What the entry points of several modules share when they marshal a C call: argument checks, optional pointers and the
row-block count of the column reductions."""
from __future__ import annotations

import torch

from .graph import CSRGraph, GraphBatch, _require_cuda, graph_from_input


def _check_f32(t, name, shape=None):
    _require_cuda(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"egc_amd: {name} must be float32 (got {t.dtype})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"egc_amd: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _ptr(t):
    """Device address of an optional tensor: NULL for None."""
    return t.data_ptr() if t is not None else None


def _check_keep(keep, n, width, dev, what="the output"):
    """A dropout mask (or None) for an [n, width] result on `dev`: one dense byte per element."""
    if keep is not None and (keep.dtype != torch.uint8 or tuple(keep.shape) != (n, width) or keep.device != dev
                             or not keep.is_contiguous()):
        raise RuntimeError(f"egc_amd: the dropout mask must be a dense uint8 tensor of the shape of {what}")


def _rows2d(t, name, n, width, dev):
    """A float32 [n, width] device tensor with unit column stride (a column block of a wider array is fine)."""
    _check_f32(t, name)
    if t.dim() != 2 or tuple(t.shape) != (n, width) or t.device != dev or (t.numel() > 0 and t.stride(1) != 1):
        raise RuntimeError(f"egc_amd: {name} must be [{n}, {width}] with unit column stride on {dev} "
                           f"(got {tuple(t.shape)} on {t.device})")
    return t.stride(0) if n > 1 else max(t.stride(0), width)


def _as_csr(graph, n: int) -> CSRGraph:
    g = graph_from_input(graph, n)
    return g.csr() if isinstance(g, GraphBatch) else g


def _layer_graph(x, edge_index, in_channels, who):
    """The CSR of a layer's ``forward(x, edge_index)``: x is float32 [rows, in_channels] and the graph [rows, rows]."""
    if x.dim() != 2 or x.size(1) != in_channels:
        raise RuntimeError(f"egc_amd.{who}: x has shape {tuple(x.shape)}, expected (rows, {in_channels})")
    _check_f32(x, "x")
    g = _as_csr(edge_index, x.size(0))
    if g.n_nodes != x.size(0) or g.n_src_rows != x.size(0):
        raise RuntimeError(f"egc_amd.{who}: the graph is [{g.n_nodes}, {g.n_src_rows}], x has {x.size(0)} rows")
    return g


def _out_block(out, out_col, width, who, grads):
    """The ``out=`` inference form: columns out_col .. out_col + width of ``out``, the block the kernel writes.  It cannot
    carry a gradient, so none of ``grads`` (the differentiable operands; None entries skipped) may require one."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in grads):
        raise RuntimeError(f"egc_amd.{who}: out= is the inference form; call it under no_grad or without out")
    if out.dim() != 2 or out_col < 0 or out_col + width > out.size(1):
        raise RuntimeError(f"egc_amd: out must be [N, >= {out_col + width}] (got {tuple(out.shape)})")
    return out[:, out_col:out_col + width]


def _unit_columns(t):
    """``t`` [rows, columns] with unit column stride: itself when it has one (or is empty), else a dense copy."""
    return t.contiguous() if t.stride(1) != 1 and t.numel() > 0 else t


def _workspace(nbytes, dev, what=None):
    """(workspace, nbytes) for a size the library gave: no tensor when it asks for none.  ``what``: zero is the library's
    "not this shape" (the heads' size queries), raised with that message."""
    nbytes = int(nbytes)
    if what is not None and nbytes == 0:
        raise RuntimeError(what)
    return (torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None), nbytes


def _row_parts(n: int) -> int:
    """Partial rows of a column reduction over n rows: one workgroup per 128 rows, 1024 at the most.  The C side is
    handed this count and splits the rows by it (egc_column_sums_f32, egc_column_moments_f64, egc_bn_*_stats_f32)."""
    return max(1, min(1024, (n + 127) // 128))
