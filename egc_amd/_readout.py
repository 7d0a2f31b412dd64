"""Segmented graph readouts on the device: mean, sum and max of consecutive row segments and their backward
(egc_readout.hip through the C ABI).  ``fusion.py`` wraps them in autograd as the global pools."""
from __future__ import annotations

import torch

from . import _C
from ._args import _check_f32
from .graph import _device_guard, _require_cuda, _stream_ptr


def segment_mean(x: torch.Tensor, seg_ptr: torch.Tensor) -> torch.Tensor:
    """Mean of consecutive row segments of x [N, C]: out[g] = mean(x[seg_ptr[g]:seg_ptr[g+1]]) (egc_segment_mean_f32)."""
    lib = _C.load()
    _check_f32(x, "x")
    x = x.contiguous()
    seg_ptr = seg_ptr.to(device=x.device, dtype=torch.int64).contiguous()
    n_seg = int(seg_ptr.numel()) - 1
    with _device_guard(x.device):
        out = torch.empty((n_seg, x.size(1)), dtype=torch.float32, device=x.device)
        _C.check(lib.egc_segment_mean_f32(x.data_ptr(), seg_ptr.data_ptr(), n_seg, x.size(1), out.data_ptr(),
                                          _stream_ptr(x.device)), "egc_segment_mean_f32")
    return out


READOUT_OPS = {"sum": _C.READOUT_SUM, "mean": _C.READOUT_MEAN, "max": _C.READOUT_MAX}


def _readout_code(op) -> int:
    if op not in READOUT_OPS:
        raise ValueError(f"egc_amd: unknown readout {op!r} (expected one of {sorted(READOUT_OPS)})")
    return READOUT_OPS[op]


def segment_reduce(x: torch.Tensor, seg_ptr: torch.Tensor, op: str, want_arg: bool = False):
    """Sum / mean / max of consecutive row segments of x [N, C] (egc_segment_reduce_f32): out[g] reduces
    x[seg_ptr[g]:seg_ptr[g+1]] in input order (float32 adds rows ascending; the first row wins a tie of max); an empty
    segment gives 0.  ``want_arg`` (max only): also the int32 [G, C] row index of each winner, -1 for an empty segment."""
    code = _readout_code(op)
    if want_arg and op != "max":
        raise ValueError("egc_amd: want_arg is for the max readout only")
    lib = _C.load()
    _check_f32(x, "x")
    if x.dim() != 2:
        raise RuntimeError(f"egc_amd: x must be [rows, width] (got {tuple(x.shape)})")
    x = x.contiguous()
    seg_ptr = seg_ptr.to(device=x.device, dtype=torch.int64).contiguous()
    n_seg = int(seg_ptr.numel()) - 1
    with _device_guard(x.device):
        out = torch.empty((n_seg, x.size(1)), dtype=torch.float32, device=x.device)
        arg = torch.empty((n_seg, x.size(1)), dtype=torch.int32, device=x.device) if want_arg else None
        _C.check(lib.egc_segment_reduce_f32(x.data_ptr(), seg_ptr.data_ptr(), n_seg, x.size(0), x.size(1), code,
                                            out.data_ptr(), arg.data_ptr() if want_arg else None,
                                            _stream_ptr(x.device)), "egc_segment_reduce_f32")
    return (out, arg) if want_arg else out


def segment_reduce_backward(d_out: torch.Tensor, seg_ptr: torch.Tensor, op: str, n_rows: int,
                            arg: torch.Tensor | None = None) -> torch.Tensor:
    """d x [n_rows, C] of segment_reduce from d out [G, C] (egc_segment_reduce_backward_f32): every row of a segment
    receives d out[g] (sum), d out[g] / count (mean) or, per column, d out[g] on the forward's ``arg`` row and 0
    elsewhere (max); rows in no segment receive 0."""
    code = _readout_code(op)
    lib = _C.load()
    _check_f32(d_out, "d_out")
    d_out = d_out.contiguous()
    seg_ptr = seg_ptr.to(device=d_out.device, dtype=torch.int64).contiguous()
    n_seg = int(seg_ptr.numel()) - 1
    if d_out.dim() != 2 or d_out.size(0) != n_seg:
        raise RuntimeError(f"egc_amd: d_out has shape {tuple(d_out.shape)}, expected ({n_seg}, width)")
    if op == "max":
        if arg is None:
            raise RuntimeError("egc_amd: the max readout's backward needs the forward's arg")
        _require_cuda(arg, "arg")
        if arg.dtype != torch.int32 or arg.shape != d_out.shape or arg.device != d_out.device:
            raise RuntimeError("egc_amd: arg must be the int32 [segments, width] tensor of the forward, on d_out's device")
        arg = arg.contiguous()
    with _device_guard(d_out.device):
        d_x = torch.empty((int(n_rows), d_out.size(1)), dtype=torch.float32, device=d_out.device)
        _C.check(lib.egc_segment_reduce_backward_f32(d_out.data_ptr(), seg_ptr.data_ptr(),
                                                     arg.data_ptr() if op == "max" else None, n_seg, int(n_rows),
                                                     d_out.size(1), code, d_x.data_ptr(), _stream_ptr(d_out.device)),
                 "egc_segment_reduce_backward_f32")
    return d_x
