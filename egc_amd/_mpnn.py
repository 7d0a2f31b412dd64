"""The baseline MPNN layer (reference experiments/layers.py:231-267) on the message-aggregate kernels of egc_mpnn.hip.

The reference's ``message()`` concatenates both endpoints' features per edge ([E, 2 d]) and runs a per-tower Linear on them
([E, d]); autograd keeps both.  A tower's weight is [Wd_t | Ws_t] (target half, source half), so with
P = x BD(Ws)^T and Q = x BD(Wd)^T + b_msg (BD: the block diagonal of the tower blocks) the aggregated message is

    add   m_i = sum_j P_j + deg_i Q_i        mean   m_i = sum_j P_j / deg_i + Q_i        max   m_i = max_j P_j + Q_i

over the row's in-edges in edge-list order (no self loops added), 0 for a row without edges: O(N d) memory and one gather
pass over a [N, d] array.  ``update`` and ``lin`` are both linear with nothing in between and fold into one [d, 2 d] product.
``Mpnn.forward`` is: one dense product x -> [P | Q], the message kernel writing m into the left half of [m | x], one dense
product with the folded weights.  The dense products are torch's (rocBLAS); the folds are torch on the small weight matrices
inside autograd, so the parameter gradients fall out of them."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _as_csr, _check_f32, _layer_graph, _out_block, _ptr, _rows2d, _unit_columns, _workspace
from .graph import CSRGraph, _device_guard, _stream_ptr

_OP = {"add": _C.MPNN_ADD, "mean": _C.MPNN_MEAN, "max": _C.MPNN_MAX}


def _op_code(aggr) -> int:
    if aggr not in _OP:
        raise ValueError(f"egc_amd.Mpnn: aggr must be one of {sorted(_OP)}, got {aggr!r}")
    return _OP[aggr]


def _launch_forward(P, Q, g: CSRGraph, op: int, out, arg):
    """egc_mpnn_message_f32: ``out`` [n_nodes, width] (a column block of the caller's operand) = the aggregated messages."""
    lib = _C.load()
    width, dev = Q.size(1), Q.device
    ld_q, ld_p, ld_out = _rows2d(Q, "Q", g.n_nodes, width, dev), _rows2d(P, "P", g.n_src_rows, width, dev), \
        _rows2d(out, "out", g.n_nodes, width, dev)
    if g.device != dev:
        raise RuntimeError(f"egc_amd: the graph is on {g.device}, P and Q on {dev}")
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_mpnn_message_workspace_bytes(g.n_edges, width, op), dev)
        _C.check(lib.egc_mpnn_message_f32(g.rowptr.data_ptr(), g.col.data_ptr(), g.edge_id.data_ptr(), g.n_nodes, g.n_edges,
                                          g.n_src_rows, P.data_ptr(), ld_p, Q.data_ptr(), ld_q, width, op, out.data_ptr(), ld_out,
                                          _ptr(arg), _ptr(ws), nbytes, _stream_ptr(dev)), "egc_mpnn_message_f32")


def _launch_backward(dm, g: CSRGraph, op: int, arg, dP, dQ):
    """egc_mpnn_message_backward_f32: dP [n_src_rows, width] and dQ [n_nodes, width] (either may be None) from dm."""
    lib = _C.load()
    width, dev = dm.size(1), dm.device
    ld_dm = _rows2d(dm, "d m", g.n_nodes, width, dev)
    ld_dp = _rows2d(dP, "d P", g.n_src_rows, width, dev) if dP is not None else 0
    ld_dq = _rows2d(dQ, "d Q", g.n_nodes, width, dev) if dQ is not None else 0
    t = g.transposed() if dP is not None else None
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_mpnn_message_backward_workspace_bytes(g.n_edges, width) if dP is not None else 0, dev)
        _C.check(lib.egc_mpnn_message_backward_f32(
            g.rowptr.data_ptr(), g.edge_id.data_ptr(), g.n_nodes, _ptr(t.rowptr if t else None), _ptr(t.col if t else None),
            _ptr(t.edge_id if t else None), g.n_src_rows, g.n_edges, dm.data_ptr(), ld_dm, _ptr(arg), width, op, _ptr(dP), ld_dp,
            _ptr(dQ), ld_dq, _ptr(ws), nbytes, _stream_ptr(dev)), "egc_mpnn_message_backward_f32")


def _new_arg(op, n, width, dev, training):
    return torch.empty((n, width), dtype=torch.int32, device=dev) if (op == _C.MPNN_MAX and training) else None


class _MpnnMessage(torch.autograd.Function):
    """m [N, d] from P and Q: the message kernel forward, the backward kernel over the transposed CSR."""

    @staticmethod
    def forward(ctx, P, Q, g, op):
        P, Q = P.detach(), Q.detach()
        arg = _new_arg(op, g.n_nodes, Q.size(1), Q.device, any(ctx.needs_input_grad[:2]))
        m = torch.empty((g.n_nodes, Q.size(1)), dtype=torch.float32, device=Q.device)
        _launch_forward(P, Q, g, op, m, arg)
        ctx.g, ctx.op, ctx.arg = g, op, arg
        return m

    @staticmethod
    def backward(ctx, dm):
        g, width = ctx.g, dm.size(1)
        dm = _unit_columns(dm)
        dP = torch.empty((g.n_src_rows, width), dtype=torch.float32, device=dm.device) if ctx.needs_input_grad[0] else None
        dQ = torch.empty((g.n_nodes, width), dtype=torch.float32, device=dm.device) if ctx.needs_input_grad[1] else None
        _launch_backward(dm, g, ctx.op, ctx.arg, dP, dQ)
        return dP, dQ, None, None


class _MpnnOperand(torch.autograd.Function):
    """A = [m | x] from pq = [P | Q] and x: the message kernel writes the left half of A, x is copied into the right one.
    Backward: the kernel writes d P and d Q into the two halves of ONE d pq; d x is the right half of d A."""

    @staticmethod
    def forward(ctx, pq, x, g, op):
        pq, x = pq.detach(), x.detach()
        n, d = x.shape
        arg = _new_arg(op, n, d, x.device, ctx.needs_input_grad[0])
        a = torch.empty((n, 2 * d), dtype=torch.float32, device=x.device)
        _launch_forward(pq[:, :d], pq[:, d:], g, op, a[:, :d], arg)
        a[:, d:].copy_(x)
        ctx.g, ctx.op, ctx.arg, ctx.d = g, op, arg, d
        return a

    @staticmethod
    def backward(ctx, da):
        g, d = ctx.g, ctx.d
        da = _unit_columns(da)
        dpq = None
        if ctx.needs_input_grad[0]:
            dpq = torch.empty((g.n_nodes, 2 * d), dtype=torch.float32, device=da.device)
            _launch_backward(da[:, :d], g, ctx.op, ctx.arg, dpq[:, :d], dpq[:, d:])
        return dpq, (da[:, d:] if ctx.needs_input_grad[1] else None), None, None


def mpnn_message(P, Q, graph, aggr, out=None, out_col=0):
    """The aggregated messages m [N, d] of the baseline MPNN layer from P [rows the edges' sources name, d] and Q [N, d] (module
    docstring) over ``graph`` (a CSRGraph, SparseTensor or [2, E] int64 edge_index): add / mean / max over every row's
    in-edges in edge-list order, the self term fused in, in the summation order of include/egc_hip.h (tests/mpnn_ref.py
    restates it bit for bit).  Differentiable with respect to P and Q.  ``out`` [N, >= out_col + d]: the inference form --
    m is written into its columns out_col .. out_col + d (the other columns are not touched) and that block is returned;
    it cannot carry a gradient, so with ``out`` neither P nor Q may require one."""
    op = _op_code(aggr)
    _check_f32(Q, "Q")
    if Q.dim() != 2:
        raise RuntimeError(f"egc_amd: Q must be [N, d] (got {tuple(Q.shape)})")
    g = _as_csr(graph, Q.size(0))
    if out is None:
        return _MpnnMessage.apply(P, Q, g, op)
    block = _out_block(out, out_col, Q.size(1), "mpnn_message", (P, Q))
    _launch_forward(P.detach(), Q.detach(), g, op, block, None)
    return block


def mpnn_message_arg(P, Q, graph):
    """(m, arg) of the max form: arg [N, d] int32 is the position in the edge list of the first in-edge of the row, in edge-list
    order, that attains the column's maximum (-1 for a row without edges) -- what the backward routes d m through."""
    _check_f32(Q, "Q")
    g = _as_csr(graph, Q.size(0))
    m = torch.empty((g.n_nodes, Q.size(1)), dtype=torch.float32, device=Q.device)
    arg = torch.empty((g.n_nodes, Q.size(1)), dtype=torch.int32, device=Q.device)
    _launch_forward(P.detach(), Q.detach(), g, _C.MPNN_MAX, m, arg)
    return m, arg


def mpnn_message_backward(dm, graph, aggr, arg=None):
    """(d P, d Q) of ``mpnn_message`` from d m [N, d] (and the forward's ``arg`` for max): the backward kernel on its own."""
    op = _op_code(aggr)
    _check_f32(dm, "d m")
    g = _as_csr(graph, dm.size(0))
    if op == _C.MPNN_MAX and arg is None:
        raise RuntimeError("egc_amd.mpnn_message_backward: max needs the forward's arg")
    dP = torch.empty((g.n_src_rows, dm.size(1)), dtype=torch.float32, device=dm.device)
    dQ = torch.empty((g.n_nodes, dm.size(1)), dtype=torch.float32, device=dm.device)
    _launch_backward(dm, g, op, arg, dP, dQ)
    return dP, dQ


class Mpnn(nn.Module):
    """Baseline MPNN (reference experiments/layers.py:231): ``Mpnn(aggr, in_dim, out_dim, towers=4)``, ``forward(x, edge_index)``
    with edge_index a [2, E] int64 tensor, an ``egc_amd.SparseTensor`` or a ``CSRGraph``.  Submodules ``message_layer.{t}``,
    ``update_layer.{t}``, ``lin`` as in the reference (state dicts interchange with strict=True; the Linears are built in the
    reference's order, so a seed gives the reference's initial parameters).  Like the reference's ``update()``, the layer
    only works with in_dim == out_dim; ``forward`` raises otherwise."""

    def __init__(self, aggr, in_dim, out_dim, towers=4):
        super().__init__()
        _op_code(aggr)
        assert out_dim % towers == 0 and in_dim % towers == 0
        self.aggr = aggr
        self.message_layer = nn.ModuleList([nn.Linear(2 * in_dim // towers, out_dim // towers) for _ in range(towers)])
        self.update_layer = nn.ModuleList([nn.Linear(2 * out_dim // towers, out_dim // towers) for _ in range(towers)])
        self.lin = nn.Linear(out_dim, out_dim)
        self.towers = towers
        self.in_dim = in_dim
        self.out_dim = out_dim
        self._fold_key, self._fold = None, None

    def _folded(self):
        """([2 d, d] weight and [2 d] bias of x -> [P | Q]; [d, 2 d] weight and [d] bias of [m | x] -> out): the tower blocks
        laid on block diagonals, update and lin folded.  Differentiable; kept between calls that need no gradient."""
        c = self.in_dim // self.towers
        msg, upd = list(self.message_layer), list(self.update_layer)
        w_pq = torch.cat([torch.block_diag(*[l.weight[:, c:] for l in msg]),          # P: the source halves
                          torch.block_diag(*[l.weight[:, :c] for l in msg])], dim=0)  # Q: the target halves
        b_msg = torch.cat([l.bias for l in msg])
        b_pq = torch.cat([torch.zeros_like(b_msg), b_msg])
        w_upd = torch.cat([torch.block_diag(*[l.weight[:, :c] for l in upd]),         # acts on m
                           torch.block_diag(*[l.weight[:, c:] for l in upd])], dim=1)  # acts on x
        w_out = self.lin.weight @ w_upd
        b_out = self.lin.weight @ torch.cat([l.bias for l in upd]) + self.lin.bias
        return w_pq, b_pq, w_out, b_out

    def _weights(self):
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return self._folded()
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self._fold_key:
            with torch.no_grad():
                self._fold = tuple(t.contiguous() for t in self._folded())
            self._fold_key = key
        return self._fold

    def forward(self, x, edge_index):
        if self.in_dim != self.out_dim:
            raise RuntimeError(f"egc_amd.Mpnn: in_dim ({self.in_dim}) != out_dim ({self.out_dim}): the reference's update() "
                               "reshapes the aggregated messages by in_dim // towers and only works when they are equal")
        g = _layer_graph(x, edge_index, self.in_dim, "Mpnn")
        w_pq, b_pq, w_out, b_out = self._weights()
        pq = F.linear(x, w_pq, b_pq)                                         # layers.py:251-258, both halves of every tower
        a = _MpnnOperand.apply(pq, x, g, _OP[self.aggr])                     # aggregate + the [inputs | x_init] of update()
        return F.linear(a, w_out, b_out)                                     # layers.py:260-267 and :249

    def extra_repr(self):
        return f"aggr={self.aggr}, in_dim={self.in_dim}, out_dim={self.out_dim}, towers={self.towers}"
