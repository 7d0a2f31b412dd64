"""GATv2Conv (PyG 2.x formulas) on the fused edge-softmax aggregate kernels of egc_gatv2.hip, and, in the second half of
this file, GATConv (GAT v1) on the additive-score kernels of egc_gat.hip.

H = heads, C = out_channels per head.  xl = lin_l(x) and xr = lin_r(x) are the halves of ONE [N, 2 H C] dense product (one
[N, H C] product when the weights are shared).  Over the edge set (``add_self_loops``: the given edges without their j == i
entries plus exactly one (i, i) per node, taken last; duplicates count each time), per edge j -> i and head h

    s_ij = sum_c att[h, c] leaky_relu(xl_j[h, c] + xr_i[h, c])     alpha_ij = softmax over i's in-edges     out_i[h] = sum_j alpha_ij xl_j[h]

PyG evaluates this through several [E, H, C] and [E, H] arrays that autograd keeps.  The kernel makes one gather pass over xl
with an online softmax and keeps only lse [N, H]; the backward recomputes the scores (d xr and d att over the CSR, d xl over
the transposed CSR) and writes d xl and d xr into the two halves of one [N, 2 H C] array.  No [E, .] array, no atomics, every
element written once, bit-reproducible.  Head mean (``concat=False``) and the bias are torch.

Attention dropout (PyG's ``F.dropout`` on alpha in training: per edge and head, the self loops included) keeps no [E, H] mask
either: the kernels' DROP instances regenerate it in the forward and in both backward passes from a counter-based generator
(Philox4x32-10, keyed by one int64 seed on the device, counted by the entry's position in the destination-keyed CSR and the
head; egc_amd/csrc/egc_gat_dev.h).  ``dropout=p, seed=t`` on the functions below (t: an int64 device tensor of one element);
the modules draw a seed per training forward with a torch device op, so ``torch.manual_seed`` governs it and nothing
synchronises."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _as_csr, _check_f32, _layer_graph, _ptr, _rows2d, _unit_columns, _workspace
from .graph import CSRGraph, _device_guard, _stream_ptr


def _heads_channels(att):
    if att.dim() == 3 and att.size(0) == 1:
        att = att[0]
    if att.dim() != 2 or att.numel() == 0 or att.numel() > 512:
        raise RuntimeError(f"egc_amd: att must be [H, C] or [1, H, C] with 1 <= H C <= 512 (got {tuple(att.shape)})")
    _check_f32(att, "att")
    return att.contiguous(), att.size(0), att.size(1)


def _drop_args(dropout, seed, dev):
    """None for dropout == 0 (the plain kernels); else (p, seed): p in (0, 1) and an int64 tensor of one element on ``dev``."""
    p = float(dropout)
    if p == 0.0:
        return None
    if not 0.0 < p < 1.0:
        raise RuntimeError(f"egc_amd: dropout must be in [0, 1) here (got {dropout}); the modules handle dropout >= 1")
    if seed is None:
        raise RuntimeError("egc_amd: dropout > 0 needs seed=, an int64 tensor of one element on the inputs' device")
    if not torch.is_tensor(seed) or seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != dev:
        raise RuntimeError(f"egc_amd: seed must be an int64 tensor of one element on {dev}")
    return p, seed


def _new_seed(dev):
    """A fresh seed from torch's generator of ``dev``, by a device op: no synchronisation, fresh in every replay of a captured step."""
    return torch.empty(1, dtype=torch.int64, device=dev).random_()


@functools.lru_cache(maxsize=None)
def _entry(lib, name, dropout):
    """(launch entry, its name, workspace query) of egc_<name>[_dropout]_f32 in ``lib``, looked up once."""
    entry = f"egc_{name}_dropout_f32" if dropout else f"egc_{name}_f32"
    return getattr(lib, entry), entry, getattr(lib, f"egc_{name}_workspace_bytes")


def _lib_call(name, dev, g, heads, channels, args, drop, src_pass=None):
    """egc_<name>_f32(CSR pointers, *args, workspace, bytes, stream) under the device guard, the workspace sized by
    egc_<name>_workspace_bytes.  A forward (``src_pass`` None) names rowptr and col; a backward also the transposed graph's, NULL
    unless a gradient of the source pass is wanted (``src_pass``).  With ``drop`` = (p, seed): egc_<name>_dropout_f32, which takes
    (p, seed pointer) after the workspace and, in a backward, the transposed entries' forward positions after the CSR pointers."""
    launch, entry, ws_bytes = _entry(_C.load(), name, drop is not None)
    csr, query = (g.rowptr.data_ptr(), g.col.data_ptr()), (g.n_edges, heads, channels)
    if src_pass is not None:
        t = g.transposed() if src_pass else None
        csr += (_ptr(t.rowptr if t else None), _ptr(t.col if t else None)) + (() if drop is None else (_ptr(t.edge_id if t else None),))
        query = (g.n_nodes,) + query
    with _device_guard(dev):
        ws, nbytes = _workspace(ws_bytes(*query), dev)
        tail = () if drop is None else (drop[0], drop[1].data_ptr())
        _C.check(launch(*csr, *args, _ptr(ws), nbytes, *tail, _stream_ptr(dev)), entry)


def _check_graph(g, dev, loops=False, operands=None, att=None, backward=None):
    """A launch's graph checks.  A forward (``operands``: the message's words for them): the graph, and ``att``, on the
    operands' device, square under add_self_loops.  A backward (``backward``: the flavour's name): a square graph."""
    if backward is not None and g.n_src_rows != g.n_nodes:
        raise RuntimeError(f"egc_amd: the {backward} backward needs a square graph, got [{g.n_nodes}, {g.n_src_rows}]")
    if operands is not None and (g.device != dev or (att is not None and att.device != dev)):
        where = operands if att is None else f"att on {att.device}, {operands}"
        raise RuntimeError(f"egc_amd: the graph is on {g.device}, {where} on {dev}")
    if loops and g.n_src_rows != g.n_nodes:
        raise RuntimeError(f"egc_amd: add_self_loops needs a square graph, got [{g.n_nodes}, {g.n_src_rows}]")


def _launch_forward(xl, xr, att, g: CSRGraph, heads, channels, slope, loops, out, lse, drop=None):
    width, dev = heads * channels, xr.device
    ld_xl, ld_xr = _rows2d(xl, "xl", g.n_src_rows, width, dev), _rows2d(xr, "xr", g.n_nodes, width, dev)
    ld_out = _rows2d(out, "out", g.n_nodes, width, dev)
    _check_graph(g, dev, loops, "xl and xr", att)
    _lib_call("gatv2_forward", dev, g, heads, channels,
              (g.n_nodes, g.n_edges, g.n_src_rows, xl.data_ptr(), ld_xl, xr.data_ptr(), ld_xr, att.data_ptr(), heads, channels,
               float(slope), int(loops), out.data_ptr(), ld_out, lse.data_ptr()), drop)


def _launch_backward(xl, xr, att, g: CSRGraph, heads, channels, slope, loops, out, lse, gout, dxl, dxr, datt, drop=None):
    """egc_gatv2_backward_f32: d xl, d xr [N, H C] (column blocks are fine) and d att [H C]; any may be None."""
    width, dev, n = heads * channels, xr.device, g.n_nodes
    _check_graph(g, dev, backward="GATv2")
    ld_xl, ld_xr = _rows2d(xl, "xl", n, width, dev), _rows2d(xr, "xr", n, width, dev)
    ld_out, ld_g = _rows2d(out, "out", n, width, dev), _rows2d(gout, "d out", n, width, dev)
    ld_dxl = _rows2d(dxl, "d xl", n, width, dev) if dxl is not None else 0
    ld_dxr = _rows2d(dxr, "d xr", n, width, dev) if dxr is not None else 0
    _lib_call("gatv2_backward", dev, g, heads, channels,
              (n, g.n_edges, xl.data_ptr(), ld_xl, xr.data_ptr(), ld_xr, att.data_ptr(), heads, channels, float(slope), int(loops),
               out.data_ptr(), ld_out, lse.data_ptr(), gout.data_ptr(), ld_g, _ptr(dxl), ld_dxl, _ptr(dxr), ld_dxr, _ptr(datt)),
              drop, src_pass=dxl is not None)


def _forward(xl, xr, att, g, slope, loops, drop=None):
    att2, heads, channels = _heads_channels(att)
    _check_f32(xr, "xr")
    n, dev = g.n_nodes, xr.device
    out = torch.empty((n, heads * channels), dtype=torch.float32, device=dev)
    lse = torch.empty((n, heads), dtype=torch.float32, device=dev)
    _launch_forward(xl, xr, att2, g, heads, channels, slope, loops, out, lse, drop)
    return out, lse, att2, heads, channels


def _backward(saved, needs, gout):
    """(d xl, d xr, d att) for one saved forward; d xl and d xr are the halves of one [N, 2 H C] array when both are wanted."""
    xl, xr, att2, g, heads, channels, slope, loops, out, lse, att_shape, drop = saved
    width, n, dev = heads * channels, g.n_nodes, gout.device
    gout = _unit_columns(gout)
    both = torch.empty((n, 2 * width), dtype=torch.float32, device=dev) if needs[0] and needs[1] else None
    dxl = both[:, :width] if both is not None else (torch.empty((n, width), dtype=torch.float32, device=dev) if needs[0] else None)
    dxr = both[:, width:] if both is not None else (torch.empty((n, width), dtype=torch.float32, device=dev) if needs[1] else None)
    datt = torch.empty(width, dtype=torch.float32, device=dev) if needs[2] else None
    if n == 0:
        datt = torch.zeros(width, dtype=torch.float32, device=dev) if needs[2] else None
    else:
        _launch_backward(xl, xr, att2, g, heads, channels, slope, loops, out, lse, gout, dxl, dxr, datt, drop)
    return dxl, dxr, (datt.view(att_shape) if datt is not None else None), both


class _GatV2Aggregate(torch.autograd.Function):
    """out [N, H C] from xl, xr (separate arrays or column blocks) and att."""

    @staticmethod
    def forward(ctx, xl, xr, att, g, slope, loops, drop=None):
        xl, xr, att = xl.detach(), xr.detach(), att.detach()
        out, lse, att2, heads, channels = _forward(xl, xr, att, g, slope, loops, drop)
        ctx.saved = (xl, xr, att2, g, heads, channels, slope, loops, out, lse, att.shape, drop)
        return out

    @staticmethod
    def backward(ctx, gout):
        dxl, dxr, datt, _ = _backward(ctx.saved, ctx.needs_input_grad[:3], gout)
        return dxl, dxr, datt, None, None, None, None


class _GatV2Fused(torch.autograd.Function):
    """out [N, H C] from lr = [xl | xr] ([N, 2 H C], one dense product): the backward writes both halves of ONE d lr."""

    @staticmethod
    def forward(ctx, lr, att, g, slope, loops, drop=None):
        lr, att = lr.detach(), att.detach()
        width = lr.size(1) // 2
        out, lse, att2, heads, channels = _forward(lr[:, :width], lr[:, width:], att, g, slope, loops, drop)
        ctx.saved = (lr[:, :width], lr[:, width:], att2, g, heads, channels, slope, loops, out, lse, att.shape, drop)
        return out

    @staticmethod
    def backward(ctx, gout):
        need = ctx.needs_input_grad[0]
        _, _, datt, both = _backward(ctx.saved, (need, need, ctx.needs_input_grad[1]), gout)
        return both, datt, None, None, None, None


def gatv2_aggregate(xl, xr, att, graph, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """out [N, H C] of the GATv2 attention aggregate (module docstring) from xl [rows the edges' sources name, H C], xr [N, H C]
    (separate arrays or column blocks of one wider array) and att ([H, C] or [1, H, C]) over ``graph`` (a CSRGraph, SparseTensor,
    GraphBatch or [2, E] int64 edge_index).  Differentiable with respect to xl, xr and att (the backward needs a square graph).
    ``dropout`` in (0, 1) with ``seed`` (an int64 device tensor of one element): attention dropout under that seed's mask."""
    drop = _drop_args(dropout, seed, xr.device)
    if xr.dim() != 2:
        raise RuntimeError(f"egc_amd: xr must be [N, H C] (got {tuple(xr.shape)})")
    _heads_channels(att)
    _check_f32(xr, "xr")
    return _GatV2Aggregate.apply(xl, xr, att, _as_csr(graph, xr.size(0)), float(negative_slope), bool(add_self_loops), drop)


def gatv2_aggregate_lse(xl, xr, att, graph, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """(out [N, H C], lse [N, H]) of the forward kernel: lse is the log-sum-exp of every row's scores (dropout does not touch
    it), -inf for an empty row.  Not differentiable."""
    drop = _drop_args(dropout, seed, xr.device)
    if xr.dim() != 2:
        raise RuntimeError(f"egc_amd: xr must be [N, H C] (got {tuple(xr.shape)})")
    _heads_channels(att)
    _check_f32(xr, "xr")
    out, lse, _, _, _ = _forward(xl.detach(), xr.detach(), att.detach(), _as_csr(graph, xr.size(0)), float(negative_slope),
                                 bool(add_self_loops), drop)
    return out, lse


def gatv2_aggregate_backward(xl, xr, att, graph, out, lse, gout, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """(d xl, d xr, d att) from d out: the backward kernels on their own (d xl and d xr are the halves of one array).  ``dropout``
    and ``seed``: those of the forward that produced ``out``."""
    att2, heads, channels = _heads_channels(att)
    saved = (xl, xr, att2, _as_csr(graph, xr.size(0)), heads, channels, float(negative_slope), bool(add_self_loops), out, lse,
             att.shape, _drop_args(dropout, seed, xr.device))
    return _backward(saved, (True, True, True), gout)[:3]


def _module_dropout(layer, x):
    """(drop, all_dropped) of one module forward: (None, False) in eval mode or at dropout == 0; a fresh seed, kept as
    ``layer.last_dropout_seed``, for 0 < dropout < 1 in training; all_dropped for dropout >= 1 in training.  The layer's dropout
    is its constructor's: a ``.dropout`` assigned afterwards raises in training as it did before there was a dropout path (a
    layer built with dropout = 0 keeps exactly its earlier behaviour), and so does a tensor that is not on the device, where the
    mask would have to be drawn."""
    if not layer.training:
        return None, False
    p, name = float(layer.dropout), type(layer).__name__
    if p != layer._dropout_built:
        raise NotImplementedError(f"egc_amd.{name}: attention dropout changed after construction ({layer._dropout_built} -> {p}) is "
                                  f"not implemented for training; construct the layer with dropout={p} or call .eval()")
    if p <= 0.0:
        return None, False
    if not x.is_cuda:
        raise NotImplementedError(f"egc_amd.{name}: attention dropout ({p}) is not implemented for tensors on {x.device}: the mask "
                                  "is generated in the HIP kernels (no CPU fallback)")
    if p >= 1.0:
        return None, True
    layer.last_dropout_seed = _new_seed(x.device)
    return (p, layer.last_dropout_seed), False


def _all_dropped(rows, *params):
    """The aggregate at dropout >= 1: zeros [N, H C] (F.dropout's result), connected to ``rows`` [N, H C] and to ``params`` so
    that their gradients are zeros and not None.  No launch."""
    out = rows * 0.0
    for q in params:
        out = out + (q * 0.0).sum()
    return out


def _glorot_(t):
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-bound, bound)


class _AttentionConv(nn.Module):
    """What GATv2Conv and GATConv share: the width check and the attributes, the bias (registered last, after the flavour's own
    parameters: ``_finish``), the dropout bookkeeping, and of ``forward`` the input, dropout and graph checks, the head mean and
    the bias.  A flavour builds its parameters, resets them and turns x into the aggregate [N, H C] (``_aggregate``)."""

    def __init__(self, in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops):
        super().__init__()
        if heads < 1 or out_channels < 1 or heads * out_channels > 512:
            raise ValueError(f"egc_amd.{type(self).__name__}: heads * out_channels must be in 1..512, got {heads} * {out_channels}")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = negative_slope, dropout, add_self_loops
        self.last_dropout_seed, self._dropout_built = None, float(dropout)

    def _finish(self, bias):
        if bias:
            self.bias = nn.Parameter(torch.empty(self.heads * self.out_channels if self.concat else self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def forward(self, x, edge_index):
        drop, all_dropped = _module_dropout(self, x)   # (ahead of the device check: its message names the dropout)
        g = _layer_graph(x, edge_index, self.in_channels, type(self).__name__)
        out = self._aggregate(x, g, float(self.negative_slope), bool(self.add_self_loops), drop, all_dropped)
        if not self.concat:
            out = out.view(-1, self.heads, self.out_channels).mean(dim=1)
        return out if self.bias is None else out + self.bias

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}, concat={self.concat}"


class GATv2Conv(_AttentionConv):
    """PyG 2.x ``GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
    add_self_loops=True, bias=True, share_weights=False)``; ``forward(x, edge_index)`` with edge_index a [2, E] int64 tensor, an
    ``egc_amd.SparseTensor``, a ``CSRGraph`` or a ``GraphBatch``.  Parameters ``lin_l.{weight,bias}``, ``lin_r.{weight,bias}``,
    ``att`` [1, H, C] and ``bias`` ([H C], or [C] for concat=False) as in PyG, so its state dicts load with strict=True (with
    ``share_weights`` lin_r IS lin_l).  Glorot weights and att, zero biases.  ``dropout``: attention dropout in training mode
    (per edge and head, self loops included, as PyG's; the mask is regenerated in the kernels from ``last_dropout_seed``, the
    int64 device tensor drawn for the last training forward; module docstring), ignored in eval mode.  The value is the
    constructor's: a ``.dropout`` assigned afterwards, or a training forward with dropout on a tensor off the device, raises
    NotImplementedError as before."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, share_weights=False):
        super().__init__(in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops)
        self.share_weights = share_weights
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=True)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self._finish(bias)

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r):
            _glorot_(lin.weight)
            nn.init.zeros_(lin.bias)
        _glorot_(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _aggregate(self, x, g, slope, loops, drop, all_dropped):
        if self.share_weights:
            xl = F.linear(x, self.lin_l.weight, self.lin_l.bias)
            return _all_dropped(xl, self.att) if all_dropped else _GatV2Aggregate.apply(xl, xl, self.att, g, slope, loops, drop)
        lr = F.linear(x, torch.cat([self.lin_l.weight, self.lin_r.weight]), torch.cat([self.lin_l.bias, self.lin_r.bias]))
        if all_dropped:
            return _all_dropped(lr[:, :lr.size(1) // 2] + lr[:, lr.size(1) // 2:], self.att)
        return _GatV2Fused.apply(lr, self.att, g, slope, loops, drop)


# ------------------------------------------------------------------------------------------------------------------ GAT v1
#
# GATConv (PyG's first GAT layer) on the kernels of egc_gat.hip.  The score leaky_relu(a_src[j, h] + a_dst[i, h]) separates
# into two per-node scalars per head, a_src[j, h] = sum_c xl[j, h, c] att_src[h, c] and a_dst likewise, so xl, a_src and a_dst
# are the column blocks of ONE dense product x W_ext^T with W_ext = [W ; A_src ; A_dst ; 0], A_src[h, :] =
# sum_c att_src[h, c] W[h C + c, :].  The forward kernel reads the two scalars per entry and needs no per-entry head sum; the
# backward needs one head sum per row (egc_gat.hip's header).

def _ext_width(heads, channels):
    """Columns of [xl | a_src | a_dst | pad]: H C + 2 H rounded up to a multiple of four, so that xl keeps 16-byte rows."""
    return (heads * channels + 2 * heads + 3) // 4 * 4


def _gat1_shape(xl, a_src, a_dst):
    for t, name in ((xl, "xl"), (a_src, "a_src"), (a_dst, "a_dst")):
        if t.dim() != 2:
            raise RuntimeError(f"egc_amd: {name} must be two-dimensional (got {tuple(t.shape)})")
    for t, name in ((xl, "xl"), (a_src, "a_src"), (a_dst, "a_dst")):
        _check_f32(t, name)
    heads = a_dst.size(1)
    if heads < 1 or a_src.size(1) != heads or xl.size(1) < heads or xl.size(1) % heads != 0 or xl.size(1) > 512:
        raise RuntimeError(f"egc_amd: xl must be [rows, H C] with 1 <= H C <= 512, a_src and a_dst [rows, H] "
                           f"(got {tuple(xl.shape)}, {tuple(a_src.shape)}, {tuple(a_dst.shape)})")
    return heads, xl.size(1) // heads


def _gat1_launch_forward(xl, a_src, a_dst, g: CSRGraph, heads, channels, slope, loops, out, lse, drop=None):
    width, dev = heads * channels, a_dst.device
    ld_xl, ld_as = _rows2d(xl, "xl", g.n_src_rows, width, dev), _rows2d(a_src, "a_src", g.n_src_rows, heads, dev)
    ld_ad, ld_out = _rows2d(a_dst, "a_dst", g.n_nodes, heads, dev), _rows2d(out, "out", g.n_nodes, width, dev)
    _check_graph(g, dev, loops, "xl, a_src and a_dst")
    _lib_call("gat_forward", dev, g, heads, channels,
              (g.n_nodes, g.n_edges, g.n_src_rows, xl.data_ptr(), ld_xl, a_src.data_ptr(), ld_as, a_dst.data_ptr(), ld_ad, heads,
               channels, float(slope), int(loops), out.data_ptr(), ld_out, lse.data_ptr()), drop)


def _gat1_launch_backward(xl, a_src, a_dst, g: CSRGraph, heads, channels, slope, loops, out, lse, gout, dxl, das, dad, drop=None):
    """egc_gat_backward_f32: d xl [N, H C], d a_src and d a_dst [N, H] (column blocks are fine); any may be None."""
    width, dev, n = heads * channels, a_dst.device, g.n_nodes
    _check_graph(g, dev, backward="GAT")
    ld_xl, ld_as, ld_ad = _rows2d(xl, "xl", n, width, dev), _rows2d(a_src, "a_src", n, heads, dev), _rows2d(a_dst, "a_dst", n, heads, dev)
    ld_out, ld_g = _rows2d(out, "out", n, width, dev), _rows2d(gout, "d out", n, width, dev)
    _check_f32(lse, "lse", (n, heads))
    if not lse.is_contiguous() or lse.device != dev:
        raise RuntimeError(f"egc_amd: lse must be a dense [{n}, {heads}] tensor on {dev}")
    ld_dxl = _rows2d(dxl, "d xl", n, width, dev) if dxl is not None else 0
    ld_das = _rows2d(das, "d a_src", n, heads, dev) if das is not None else 0
    ld_dad = _rows2d(dad, "d a_dst", n, heads, dev) if dad is not None else 0
    _lib_call("gat_backward", dev, g, heads, channels,
              (n, g.n_edges, xl.data_ptr(), ld_xl, a_src.data_ptr(), ld_as, a_dst.data_ptr(), ld_ad, heads, channels, float(slope),
               int(loops), out.data_ptr(), ld_out, lse.data_ptr(), gout.data_ptr(), ld_g, _ptr(dxl), ld_dxl, _ptr(das), ld_das,
               _ptr(dad), ld_dad), drop, src_pass=dxl is not None or das is not None)


def _gat1_forward(xl, a_src, a_dst, g, slope, loops, drop=None):
    heads, channels = _gat1_shape(xl, a_src, a_dst)
    n, dev = g.n_nodes, a_dst.device
    out = torch.empty((n, heads * channels), dtype=torch.float32, device=dev)
    lse = torch.empty((n, heads), dtype=torch.float32, device=dev)
    _gat1_launch_forward(xl, a_src, a_dst, g, heads, channels, slope, loops, out, lse, drop)
    return out, lse, heads, channels


def _gat1_backward(saved, needs, gout):
    """(d xl, d a_src, d a_dst, ext) for one saved forward: the wanted gradients are the blocks of ONE array ``ext`` in the layout
    [d xl | d a_src | d a_dst | pad]; the blocks nobody wants and the pad columns are zero."""
    xl, a_src, a_dst, g, heads, channels, slope, loops, out, lse, drop = saved
    width, n, dev = heads * channels, g.n_nodes, gout.device
    gout = _unit_columns(gout)
    ext = torch.empty((n, _ext_width(heads, channels)), dtype=torch.float32, device=dev)
    blocks = [ext[:, :width], ext[:, width:width + heads], ext[:, width + heads:width + 2 * heads]]
    for b, need in zip(blocks + [ext[:, width + 2 * heads:]], tuple(needs) + (False,)):
        if not need and b.numel() > 0:
            b.zero_()
    wanted = [b if need else None for b, need in zip(blocks, needs)]
    if n > 0 and any(needs):
        _gat1_launch_backward(xl, a_src, a_dst, g, heads, channels, slope, loops, out, lse, gout, *wanted, drop=drop)
    return wanted[0], wanted[1], wanted[2], ext


class _GatAggregate(torch.autograd.Function):
    """out [N, H C] from xl, a_src and a_dst (separate arrays or column blocks)."""

    @staticmethod
    def forward(ctx, xl, a_src, a_dst, g, slope, loops, drop=None):
        xl, a_src, a_dst = xl.detach(), a_src.detach(), a_dst.detach()
        out, lse, heads, channels = _gat1_forward(xl, a_src, a_dst, g, slope, loops, drop)
        ctx.saved = (xl, a_src, a_dst, g, heads, channels, slope, loops, out, lse, drop)
        return out

    @staticmethod
    def backward(ctx, gout):
        dxl, das, dad, _ = _gat1_backward(ctx.saved, ctx.needs_input_grad[:3], gout)
        return dxl, das, dad, None, None, None, None


class _GatFused(torch.autograd.Function):
    """out [N, H C] from ext = [xl | a_src | a_dst | pad] (one dense product): the backward writes the three gradients into the
    blocks of ONE d ext of the same layout, the pad columns zero."""

    @staticmethod
    def forward(ctx, ext, heads, channels, g, slope, loops, drop=None):
        ext = ext.detach()
        w = heads * channels
        if ext.dim() != 2 or ext.size(1) != _ext_width(heads, channels):
            raise RuntimeError(f"egc_amd: [xl | a_src | a_dst | pad] must be [N, {_ext_width(heads, channels)}] (got {tuple(ext.shape)})")
        xl, a_src, a_dst = ext[:, :w], ext[:, w:w + heads], ext[:, w + heads:w + 2 * heads]
        out, lse, _, _ = _gat1_forward(xl, a_src, a_dst, g, slope, loops, drop)
        ctx.saved = (xl, a_src, a_dst, g, heads, channels, slope, loops, out, lse, drop)
        return out

    @staticmethod
    def backward(ctx, gout):
        return _gat1_backward(ctx.saved, (True, True, True), gout)[3], None, None, None, None, None, None


def gat_aggregate(xl, a_src, a_dst, graph, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """out [N, H C] of the GAT attention aggregate from xl [rows the edges' sources name, H C], a_src [the same rows, H] and
    a_dst [N, H] (separate arrays or column blocks of one wider array) over ``graph`` (a CSRGraph, SparseTensor, GraphBatch or
    [2, E] int64 edge_index): s_ij = leaky_relu(a_src[j] + a_dst[i]), alpha = softmax over i's in-edges, out_i = sum_j alpha_ij
    xl_j per head.  Differentiable with respect to xl, a_src and a_dst (the backward needs a square graph).  ``dropout`` in (0, 1)
    with ``seed`` (an int64 device tensor of one element): attention dropout under that seed's mask."""
    drop = _drop_args(dropout, seed, a_dst.device)
    _gat1_shape(xl, a_src, a_dst)
    return _GatAggregate.apply(xl, a_src, a_dst, _as_csr(graph, a_dst.size(0)), float(negative_slope), bool(add_self_loops), drop)


def gat_aggregate_lse(xl, a_src, a_dst, graph, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """(out [N, H C], lse [N, H]) of the forward kernel: lse is the log-sum-exp of every row's scores (dropout does not touch
    it), -inf for an empty row.  Not differentiable."""
    drop = _drop_args(dropout, seed, a_dst.device)
    _gat1_shape(xl, a_src, a_dst)
    out, lse, _, _ = _gat1_forward(xl.detach(), a_src.detach(), a_dst.detach(), _as_csr(graph, a_dst.size(0)), float(negative_slope),
                                   bool(add_self_loops), drop)
    return out, lse


def gat_aggregate_backward(xl, a_src, a_dst, graph, out, lse, gout, negative_slope=0.2, add_self_loops=True, dropout=0.0, seed=None):
    """(d xl, d a_src, d a_dst) from d out: the backward kernels on their own (the three are the column blocks of one array in
    the layout [d xl | d a_src | d a_dst | pad]).  ``dropout`` and ``seed``: those of the forward that produced ``out``."""
    heads, channels = _gat1_shape(xl, a_src, a_dst)
    saved = (xl, a_src, a_dst, _as_csr(graph, a_dst.size(0)), heads, channels, float(negative_slope), bool(add_self_loops), out, lse,
             _drop_args(dropout, seed, a_dst.device))
    return _gat1_backward(saved, (True, True, True), gout)[:3]


class GATConv(_AttentionConv):
    """PyG ``GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
    bias=True)``, non-bipartite (``in_channels`` an int); ``forward(x, edge_index)`` with edge_index a [2, E] int64 tensor, an
    ``egc_amd.SparseTensor``, a ``CSRGraph`` or a ``GraphBatch``.  State dict in the PyG 2.0 - 2.2 layout, so such state dicts
    load with strict=True: ``lin_src.weight`` [H C, F_in] and ``lin_dst.weight`` (lin_dst IS lin_src), ``att_src`` and
    ``att_dst`` [1, H, C], ``bias`` ([H C], or [C] for concat=False); the later layout with a single ``lin.weight`` loads too.
    Glorot weights and att, zero bias.  [xl | a_src | a_dst] is one dense product with the att vectors folded into 2 H extra
    weight rows; autograd takes d W, d att_src and d att_dst from the one dense gradient.  ``dropout``: attention dropout in
    training mode (per edge and head, self loops included, as PyG's; the mask is regenerated in the kernels from
    ``last_dropout_seed``, the int64 device tensor drawn for the last training forward), ignored in eval mode; the value is the
    constructor's (a ``.dropout`` assigned afterwards, or a tensor off the device, raises NotImplementedError in training as
    before).  Not implemented:
    ``edge_dim`` (edge features), bipartite ``in_channels`` (a pair), ``fill_value`` and ``residual``."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True):
        if not isinstance(in_channels, int):
            raise ValueError(f"egc_amd.GATConv: in_channels must be an int (bipartite inputs are not implemented), got {in_channels!r}")
        super().__init__(in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops)
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self._finish(bias)

    def reset_parameters(self):
        _glorot_(self.lin_src.weight)
        _glorot_(self.att_src)
        _glorot_(self.att_dst)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # the later PyG layout: one lin.weight for both ends
        if prefix + "lin_src.weight" not in state_dict and prefix + "lin.weight" in state_dict:
            state_dict[prefix + "lin_src.weight"] = state_dict[prefix + "lin_dst.weight"] = state_dict.pop(prefix + "lin.weight")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extended_weight(self):
        """W_ext = [W ; A_src ; A_dst ; 0], [H C + 2 H rounded up to a multiple of 4, F_in]: x W_ext^T = [xl | a_src | a_dst | pad]."""
        h, c, w = self.heads, self.out_channels, self.lin_src.weight
        w3 = w.view(h, c, self.in_channels)
        rows = [w, (self.att_src.view(h, c, 1) * w3).sum(dim=1), (self.att_dst.view(h, c, 1) * w3).sum(dim=1)]
        pad = _ext_width(h, c) - h * c - 2 * h
        if pad:
            rows.append(w.new_zeros((pad, self.in_channels)))
        return torch.cat(rows)

    def _aggregate(self, x, g, slope, loops, drop, all_dropped):
        ext = F.linear(x, self.extended_weight())
        if all_dropped:
            return _all_dropped(ext[:, :self.heads * self.out_channels])
        return _GatFused.apply(ext, self.heads, self.out_channels, g, slope, loops, drop)
