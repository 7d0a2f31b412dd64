"""GATv2Conv (PyG 2.x formulas) on the fused edge-softmax aggregate kernels of egc_gatv2.hip.

H = heads, C = out_channels per head.  xl = lin_l(x) and xr = lin_r(x) are the halves of ONE [N, 2 H C] dense product (one
[N, H C] product when the weights are shared).  Over the edge set (``add_self_loops``: the given edges without their j == i
entries plus exactly one (i, i) per node, taken last; duplicates count each time), per edge j -> i and head h

    s_ij = sum_c att[h, c] leaky_relu(xl_j[h, c] + xr_i[h, c])     alpha_ij = softmax over i's in-edges     out_i[h] = sum_j alpha_ij xl_j[h]

PyG evaluates this through several [E, H, C] and [E, H] arrays that autograd keeps.  The kernel makes one gather pass over xl
with an online softmax and keeps only lse [N, H]; the backward recomputes the scores (d xr and d att over the CSR, d xl over
the transposed CSR) and writes d xl and d xr into the two halves of one [N, 2 H C] array.  No [E, .] array, no atomics, every
element written once, bit-reproducible.  Head mean (``concat=False``) and the bias are torch."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _as_csr, _check_f32, _ptr, _rows2d, _unit_columns, _workspace
from .graph import CSRGraph, _device_guard, _stream_ptr


def _heads_channels(att):
    if att.dim() == 3 and att.size(0) == 1:
        att = att[0]
    if att.dim() != 2 or att.numel() == 0 or att.numel() > 512:
        raise RuntimeError(f"egc_amd: att must be [H, C] or [1, H, C] with 1 <= H C <= 512 (got {tuple(att.shape)})")
    _check_f32(att, "att")
    return att.contiguous(), att.size(0), att.size(1)


def _launch_forward(xl, xr, att, g: CSRGraph, heads, channels, slope, loops, out, lse):
    lib = _C.load()
    width, dev = heads * channels, xr.device
    ld_xl, ld_xr = _rows2d(xl, "xl", g.n_src_rows, width, dev), _rows2d(xr, "xr", g.n_nodes, width, dev)
    ld_out = _rows2d(out, "out", g.n_nodes, width, dev)
    if g.device != dev or att.device != dev:
        raise RuntimeError(f"egc_amd: the graph is on {g.device}, att on {att.device}, xl and xr on {dev}")
    if loops and g.n_src_rows != g.n_nodes:
        raise RuntimeError(f"egc_amd: add_self_loops needs a square graph, got [{g.n_nodes}, {g.n_src_rows}]")
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_gatv2_forward_workspace_bytes(g.n_edges, heads, channels), dev)
        _C.check(lib.egc_gatv2_forward_f32(g.rowptr.data_ptr(), g.col.data_ptr(), g.n_nodes, g.n_edges, g.n_src_rows, xl.data_ptr(),
                                           ld_xl, xr.data_ptr(), ld_xr, att.data_ptr(), heads, channels, float(slope), int(loops),
                                           out.data_ptr(), ld_out, lse.data_ptr(), _ptr(ws), nbytes, _stream_ptr(dev)),
                 "egc_gatv2_forward_f32")


def _launch_backward(xl, xr, att, g: CSRGraph, heads, channels, slope, loops, out, lse, gout, dxl, dxr, datt):
    """egc_gatv2_backward_f32: d xl, d xr [N, H C] (column blocks are fine) and d att [H C]; any may be None."""
    lib = _C.load()
    width, dev, n = heads * channels, xr.device, g.n_nodes
    if g.n_src_rows != n:
        raise RuntimeError(f"egc_amd: the GATv2 backward needs a square graph, got [{n}, {g.n_src_rows}]")
    ld_xl, ld_xr = _rows2d(xl, "xl", n, width, dev), _rows2d(xr, "xr", n, width, dev)
    ld_out, ld_g = _rows2d(out, "out", n, width, dev), _rows2d(gout, "d out", n, width, dev)
    ld_dxl = _rows2d(dxl, "d xl", n, width, dev) if dxl is not None else 0
    ld_dxr = _rows2d(dxr, "d xr", n, width, dev) if dxr is not None else 0
    t = g.transposed() if dxl is not None else None
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_gatv2_backward_workspace_bytes(n, g.n_edges, heads, channels), dev)
        _C.check(lib.egc_gatv2_backward_f32(
            g.rowptr.data_ptr(), g.col.data_ptr(), _ptr(t.rowptr if t else None), _ptr(t.col if t else None), n, g.n_edges,
            xl.data_ptr(), ld_xl, xr.data_ptr(), ld_xr, att.data_ptr(), heads, channels, float(slope), int(loops), out.data_ptr(),
            ld_out, lse.data_ptr(), gout.data_ptr(), ld_g, _ptr(dxl), ld_dxl, _ptr(dxr), ld_dxr, _ptr(datt), _ptr(ws), nbytes,
            _stream_ptr(dev)), "egc_gatv2_backward_f32")


def _forward(xl, xr, att, g, slope, loops):
    att2, heads, channels = _heads_channels(att)
    _check_f32(xr, "xr")
    n, dev = g.n_nodes, xr.device
    out = torch.empty((n, heads * channels), dtype=torch.float32, device=dev)
    lse = torch.empty((n, heads), dtype=torch.float32, device=dev)
    _launch_forward(xl, xr, att2, g, heads, channels, slope, loops, out, lse)
    return out, lse, att2, heads, channels


def _backward(saved, needs, gout):
    """(d xl, d xr, d att) for one saved forward; d xl and d xr are the halves of one [N, 2 H C] array when both are wanted."""
    xl, xr, att2, g, heads, channels, slope, loops, out, lse, att_shape = saved
    width, n, dev = heads * channels, g.n_nodes, gout.device
    gout = _unit_columns(gout)
    both = torch.empty((n, 2 * width), dtype=torch.float32, device=dev) if needs[0] and needs[1] else None
    dxl = both[:, :width] if both is not None else (torch.empty((n, width), dtype=torch.float32, device=dev) if needs[0] else None)
    dxr = both[:, width:] if both is not None else (torch.empty((n, width), dtype=torch.float32, device=dev) if needs[1] else None)
    datt = torch.empty(width, dtype=torch.float32, device=dev) if needs[2] else None
    if n == 0:
        datt = torch.zeros(width, dtype=torch.float32, device=dev) if needs[2] else None
    else:
        _launch_backward(xl, xr, att2, g, heads, channels, slope, loops, out, lse, gout, dxl, dxr, datt)
    return dxl, dxr, (datt.view(att_shape) if datt is not None else None), both


class _GatV2Aggregate(torch.autograd.Function):
    """out [N, H C] from xl, xr (separate arrays or column blocks) and att."""

    @staticmethod
    def forward(ctx, xl, xr, att, g, slope, loops):
        xl, xr, att = xl.detach(), xr.detach(), att.detach()
        out, lse, att2, heads, channels = _forward(xl, xr, att, g, slope, loops)
        ctx.saved = (xl, xr, att2, g, heads, channels, slope, loops, out, lse, att.shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        dxl, dxr, datt, _ = _backward(ctx.saved, ctx.needs_input_grad[:3], gout)
        return dxl, dxr, datt, None, None, None


class _GatV2Fused(torch.autograd.Function):
    """out [N, H C] from lr = [xl | xr] ([N, 2 H C], one dense product): the backward writes both halves of ONE d lr."""

    @staticmethod
    def forward(ctx, lr, att, g, slope, loops):
        lr, att = lr.detach(), att.detach()
        width = lr.size(1) // 2
        out, lse, att2, heads, channels = _forward(lr[:, :width], lr[:, width:], att, g, slope, loops)
        ctx.saved = (lr[:, :width], lr[:, width:], att2, g, heads, channels, slope, loops, out, lse, att.shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        need = ctx.needs_input_grad[0]
        _, _, datt, both = _backward(ctx.saved, (need, need, ctx.needs_input_grad[1]), gout)
        return both, datt, None, None, None


def gatv2_aggregate(xl, xr, att, graph, negative_slope=0.2, add_self_loops=True):
    """out [N, H C] of the GATv2 attention aggregate (module docstring) from xl [rows the edges' sources name, H C], xr [N, H C]
    (separate arrays or column blocks of one wider array) and att ([H, C] or [1, H, C]) over ``graph`` (a CSRGraph, SparseTensor,
    GraphBatch or [2, E] int64 edge_index).  Differentiable with respect to xl, xr and att (the backward needs a square graph)."""
    if xr.dim() != 2:
        raise RuntimeError(f"egc_amd: xr must be [N, H C] (got {tuple(xr.shape)})")
    _heads_channels(att)
    _check_f32(xr, "xr")
    return _GatV2Aggregate.apply(xl, xr, att, _as_csr(graph, xr.size(0)), float(negative_slope), bool(add_self_loops))


def gatv2_aggregate_lse(xl, xr, att, graph, negative_slope=0.2, add_self_loops=True):
    """(out [N, H C], lse [N, H]) of the forward kernel: lse is the log-sum-exp of every row's scores, -inf for an empty row.
    Not differentiable."""
    if xr.dim() != 2:
        raise RuntimeError(f"egc_amd: xr must be [N, H C] (got {tuple(xr.shape)})")
    _heads_channels(att)
    _check_f32(xr, "xr")
    out, lse, _, _, _ = _forward(xl.detach(), xr.detach(), att.detach(), _as_csr(graph, xr.size(0)), float(negative_slope),
                                 bool(add_self_loops))
    return out, lse


def gatv2_aggregate_backward(xl, xr, att, graph, out, lse, gout, negative_slope=0.2, add_self_loops=True):
    """(d xl, d xr, d att) from d out: the backward kernels on their own (d xl and d xr are the halves of one array)."""
    att2, heads, channels = _heads_channels(att)
    saved = (xl, xr, att2, _as_csr(graph, xr.size(0)), heads, channels, float(negative_slope), bool(add_self_loops), out, lse,
             att.shape)
    return _backward(saved, (True, True, True), gout)[:3]


def _glorot_(t):
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-bound, bound)


class GATv2Conv(nn.Module):
    """PyG 2.x ``GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
    add_self_loops=True, bias=True, share_weights=False)``; ``forward(x, edge_index)`` with edge_index a [2, E] int64 tensor, an
    ``egc_amd.SparseTensor``, a ``CSRGraph`` or a ``GraphBatch``.  Parameters ``lin_l.{weight,bias}``, ``lin_r.{weight,bias}``,
    ``att`` [1, H, C] and ``bias`` ([H C], or [C] for concat=False) as in PyG, so its state dicts load with strict=True (with
    ``share_weights`` lin_r IS lin_l).  Glorot weights and att, zero biases.  Attention dropout is not implemented: dropout > 0
    raises in training mode and is ignored in eval mode."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, share_weights=False):
        super().__init__()
        if heads < 1 or out_channels < 1 or heads * out_channels > 512:
            raise ValueError(f"egc_amd.GATv2Conv: heads * out_channels must be in 1..512, got {heads} * {out_channels}")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops, self.share_weights = negative_slope, dropout, add_self_loops, share_weights
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=True)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r):
            _glorot_(lin.weight)
            nn.init.zeros_(lin.bias)
        _glorot_(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index):
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise RuntimeError(f"egc_amd.GATv2Conv: x has shape {tuple(x.shape)}, expected (rows, {self.in_channels})")
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError(f"egc_amd.GATv2Conv: attention dropout ({self.dropout}) is not implemented for training; "
                                      "construct the layer with dropout=0.0 (the reference's gat_dropout) or call .eval()")
        _check_f32(x, "x")
        g = _as_csr(edge_index, x.size(0))
        if g.n_nodes != x.size(0) or g.n_src_rows != x.size(0):
            raise RuntimeError(f"egc_amd.GATv2Conv: the graph is [{g.n_nodes}, {g.n_src_rows}], x has {x.size(0)} rows")
        slope, loops = float(self.negative_slope), bool(self.add_self_loops)
        if self.share_weights:
            xl = F.linear(x, self.lin_l.weight, self.lin_l.bias)
            out = _GatV2Aggregate.apply(xl, xl, self.att, g, slope, loops)
        else:
            lr = F.linear(x, torch.cat([self.lin_l.weight, self.lin_r.weight]), torch.cat([self.lin_l.bias, self.lin_r.bias]))
            out = _GatV2Fused.apply(lr, self.att, g, slope, loops)
        if not self.concat:
            out = out.view(-1, self.heads, self.out_channels).mean(dim=1)
        return out if self.bias is None else out + self.bias

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}, concat={self.concat}"
