"""Entry points of the node encoders: the embedding-sum forward and its table gradients (egc_encoder.hip through the
C ABI).  The modules that use them are in ``encoders.py``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _C
from ._args import _check_f32, _check_keep, _ptr
from .graph import _IndexFlag, _device_guard, _require_cuda, _stream_ptr


def _encoder_args(tables, idx, clamp):
    """Validated (idx [N, T] contiguous, host arrays of table rows and clamps, width) of an encoder call."""
    tables = list(tables)
    if not tables:
        raise RuntimeError("egc_amd: an encoder needs at least one table")
    width = tables[0].size(1) if tables[0].dim() == 2 else -1
    for k, w in enumerate(tables):
        _check_f32(w, f"tables[{k}]")
        if w.dim() != 2 or w.size(1) != width or not w.is_contiguous() or w.device != tables[0].device:
            raise RuntimeError("egc_amd: encoder tables must be dense [rows, width] tensors of one width on one device")
    _require_cuda(idx, "idx")
    if idx.dim() == 1:
        idx = idx[:, None]
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.size(1) != len(tables) or idx.device != tables[0].device:
        raise RuntimeError(f"egc_amd: idx must be an int64 tensor of shape [N, {len(tables)}] on the tables' device "
                           f"(got {idx.dtype} {tuple(idx.shape)})")
    clamp = [-1] * len(tables) if clamp is None else [-1 if c is None else int(c) for c in clamp]
    if len(clamp) != len(tables):
        raise RuntimeError("egc_amd: one clamp (or None) per table")
    rows = (C.c_int32 * len(tables))(*[w.size(0) for w in tables])
    return idx.contiguous(), rows, (C.c_int32 * len(tables))(*clamp), width


def encoder_forward(tables, idx: torch.Tensor, clamp=None, keep: torch.Tensor | None = None,
                    keep_scale: float = 1.0) -> torch.Tensor:
    """Sum of embedding rows (egc_encoder_forward_f32): out[n] = ((W_0[idx[n,0]] + W_1[idx[n,1]]) + ...), float32 adds in
    table order, one launch.  ``tables``: float32 [R_t, F] device tensors; ``idx`` int64 [N, T] ([N] for one table);
    ``clamp[t]`` (or None): the index of table t is min(idx, clamp[t]) -- ``idx`` itself is not written; ``keep`` uint8
    [N, F] with ``keep_scale``: out = keep ? sum * keep_scale : 0.  An index outside its table contributes a zero row
    and raises the deferred index flag (reported at the next call into the package, graph._IndexFlag)."""
    lib = _C.load()
    _IndexFlag.poll()
    idx, rows, clamps, width = _encoder_args(tables, idx, clamp)
    dev = idx.device
    _check_keep(keep, idx.size(0), width, dev)
    ptrs = (C.c_void_p * len(rows))(*[w.data_ptr() for w in tables])
    with _device_guard(dev):
        out = torch.empty((idx.size(0), width), dtype=torch.float32, device=dev)
        _C.check(lib.egc_encoder_forward_f32(ptrs, rows, clamps, len(rows), idx.data_ptr(), idx.size(0), width, _ptr(keep),
                                             float(keep_scale), out.data_ptr(), _IndexFlag.ptr(), _stream_ptr(dev)),
                 "egc_encoder_forward_f32")
    return out


def encoder_backward(d_out: torch.Tensor, idx: torch.Tensor, table_rows, clamp=None, keep: torch.Tensor | None = None,
                     keep_scale: float = 1.0, out=None) -> list:
    """Gradients of encoder_forward's tables (egc_encoder_backward_f32): d W_t[v] = sum of the (masked, scaled) rows of
    ``d_out`` whose index into table t is v; rows nobody indexes receive 0; every element is written exactly once, in two
    launches without atomics and with a summation order that depends on ``idx`` and the shapes alone (bit-reproducible).
    Returns one [R_t, F] tensor per table: ``out`` when given (dense float32 tensors that are overwritten), else row
    ranges of ONE new [sum R_t, F] buffer."""
    lib = _C.load()
    _check_f32(d_out, "d_out")
    table_rows = [int(r) for r in table_rows]
    dev, width = d_out.device, d_out.size(1) if d_out.dim() == 2 else -1
    d_out = d_out.contiguous()
    with _device_guard(dev):
        if out is None:
            packed = torch.empty((sum(table_rows), width), dtype=torch.float32, device=dev)
            out = list(packed.split(table_rows))
        idx, rows, clamps, _ = _encoder_args(out, idx, clamp)
        if [w.size(0) for w in out] != table_rows or width != out[0].size(1) or d_out.size(0) != idx.size(0):
            raise RuntimeError("egc_amd: d_out / idx / table shapes of the encoder backward do not agree")
        _check_keep(keep, idx.size(0), width, dev)
        ptrs = (C.c_void_p * len(rows))(*[w.data_ptr() for w in out])
        nbytes = int(lib.egc_encoder_workspace_bytes(idx.size(0), len(rows), sum(table_rows), width))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _C.check(lib.egc_encoder_backward_f32(d_out.data_ptr(), _ptr(keep), float(keep_scale), idx.data_ptr(), idx.size(0),
                                              width, rows, clamps, len(rows), ptrs, ws.data_ptr(), nbytes, _stream_ptr(dev)),
                 "egc_encoder_backward_f32")
    return list(out)


def encoder_supported(tables, idx: torch.Tensor) -> bool:
    """Whether encoder_forward / encoder_backward take these tensors: float32 tables of one width on one ROCm device,
    int64 indices there, and a shape inside the library's limits -- asked of the library itself
    (egc_encoder_workspace_bytes is 0 outside them), so the limits are written once.  Host-side checks only."""
    tables = list(tables)
    if not tables or not all(w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() for w in tables):
        return False
    dev, width = tables[0].device, tables[0].size(1)
    if not (all(w.device == dev and w.size(1) == width for w in tables) and idx.device == dev and idx.dtype == torch.int64
            and idx.dim() >= 1):
        return False
    # (at least one row: the query also answers 0 for an empty batch, which needs no workspace)
    return _C.load().egc_encoder_workspace_bytes(max(idx.size(0), 1), len(tables), sum(w.size(0) for w in tables), width) > 0
