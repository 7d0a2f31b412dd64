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


def _unit_columns(t):
    """``t`` [rows, columns] with unit column stride: itself when it has one (or is empty), else a dense copy."""
    return t.contiguous() if t.stride(1) != 1 and t.numel() > 0 else t


def _workspace(nbytes, dev):
    """(workspace, nbytes) for a size the library gave: no tensor when it asks for none."""
    nbytes = int(nbytes)
    return (torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None), nbytes


def _row_parts(n: int) -> int:
    """Partial rows of a column reduction over n rows: one workgroup per 128 rows, 1024 at the most.  The C side is
    handed this count and splits the rows by it (egc_column_sums_f32, egc_column_moments_f64, egc_bn_*_stats_f32)."""
    return max(1, min(1024, (n + 127) // 128))
