"""Drop-in ``EGConv`` backed by the fused gfx950 kernels.

Mirrors the constructor signature, attributes, parameter names/shapes, ``__repr__`` and error
behaviour of the reference class (experiments/optimized_layers.py:19-286, the version upstreamed to
PyG); ``forward`` hands (x, graph, parameters) to ``libegc_hip.so``.

Semantics carried over from the reference (SURVEY.md 8a notes):
  * weightings column order is h*A*B + a*B + b (optimized_layers.py:195-202);
  * with ``symnorm`` among the aggregators the gcn_norm edge set (self-loops replaced by exactly one
    per node when ``add_self_loops``) is used by EVERY aggregator (optimized_layers.py:127-156);
  * without ``symnorm`` but with ``add_self_loops`` the loops come from
    ``add_remaining_self_loops(edge_index)``, which infers the node count from the largest index
    present, so trailing isolated nodes get none (optimized_layers.py:158-166) -- a SparseTensor
    input goes through ``fill_diag`` instead and every node gets one (168-175);
  * ``cached=True`` pins the first graph seen (optimized_layers.py:138-139, 153-154).
"""
from __future__ import annotations

from typing import Iterable

import torch
import torch.nn as nn

from . import _C
from . import ops
from .functional import (TrainCall, egc_layer_apply, egc_layer_apply_params, gemm_exact, make_spec, pack_layer_weights,
                         pack_weights, pad_bases_columns, padded_basis_stride)
from .graph import GraphBatch, graph_from_input
from .layers import glorot_

_AGGR_CODE = {"sum": _C.AGGR_SUM, "mean": _C.AGGR_MEAN, "symnorm": _C.AGGR_SYMNORM, "min": _C.AGGR_MIN,
              "max": _C.AGGR_MAX, "var": _C.AGGR_VAR, "std": _C.AGGR_STD}


class EGConv(nn.Module):
    """Efficient Graph Convolution (reference: experiments/optimized_layers.py:19)."""

    def __init__(self, in_channels: int, out_channels: int, aggrs: Iterable[str] = ("symnorm",),
                 num_heads: int = 8, num_bases: int = 4, cached: bool = False, add_self_loops: bool = True,
                 bias: bool = True, sigmoid: bool = False, **kwargs):
        super().__init__()
        if out_channels % num_heads != 0:
            raise ValueError("out_channels must be divisible by the number of heads")
        for a in aggrs:
            if a not in _AGGR_CODE:
                raise ValueError("Unsupported aggregator: {}".format(a))

        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_heads, self.num_bases = num_heads, num_bases
        self.cached, self.add_self_loops = cached, add_self_loops
        self.aggregators = list(aggrs)
        self.sigmoid = sigmoid
        self.node_dim = 0

        self.bases_weight = nn.Parameter(torch.empty(in_channels, (out_channels // num_heads) * num_bases))
        self.comb_weight = nn.Linear(in_channels, num_heads * num_bases * len(self.aggregators))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)

        codes = [_AGGR_CODE[a] for a in self.aggregators]
        act = _C.ACT_SIGMOID if sigmoid else _C.ACT_NONE
        has_sym = "symnorm" in self.aggregators
        edge_set = _C.SET_LOOPED if add_self_loops else _C.SET_RAW
        # The weightings tensor is an internal intermediate, so its column order is ours to choose: the
        # comb_weight rows are permuted from the reference's h*A*B + a*B + b (optimized_layers.py:195-202)
        # to h*B*A + b*A + a when packed, which lets the kernel fetch w[h][b][0..A) with one 16-byte load.
        common = dict(weight_layout=_C.LAYOUT_HBA, weight_act=act,
                      basis_stride=padded_basis_stride(out_channels, num_heads, num_bases))
        # COO input: loops for every node only when gcn_norm (which knows num_nodes) adds them
        self._spec_coo = make_spec(in_channels, out_channels, num_heads, num_bases, codes, agg_set=edge_set,
                                   sym_set=edge_set, loops_all_nodes=has_sym, **common)
        # adj_t input: gcn_norm(SparseTensor) / fill_diag put a loop on every node
        self._spec_adj = make_spec(in_channels, out_channels, num_heads, num_bases, codes, agg_set=edge_set,
                                   sym_set=edge_set, loops_all_nodes=True, **common)
        self._cached_graph = None
        self._wcat_key, self._wcat, self._planes = None, None, None
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.bases_weight)
        self.comb_weight.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)
        self._cached_graph = None
        self._wcat_key, self._wcat, self._planes = None, None, None

    def _pack(self):
        H, A, B, F = self.num_heads, len(self.aggregators), self.num_bases, self.in_channels
        sp = self._spec_coo
        if (torch.is_grad_enabled() and self.bases_weight.is_cuda and self.bases_weight.dtype == torch.float32
                and self.comb_weight.bias is not None):
            # training: one launch each way instead of the differentiable torch chain below
            # (comb rows [h][a][b] permuted to [h][b][a]: optimized_layers.py:195-202)
            return pack_layer_weights([self.bases_weight], self.comb_weight.weight, self.comb_weight.bias, F, H, A, B,
                                      sp.basis_len, sp.basis_stride, True)
        w = self.comb_weight.weight.view(H, A, B, F).permute(0, 2, 1, 3).reshape(H * B * A, F)
        b = self.comb_weight.bias.view(H, A, B).permute(0, 2, 1).reshape(H * B * A)
        sp = self._spec_coo
        bases = pad_bases_columns(self.bases_weight, B, sp.basis_len, sp.basis_stride)
        return torch.cat([bases, w.t()], dim=1).contiguous(), b.contiguous()

    def _packed_weights(self):
        """([bases_weight | permuted comb_weight.weight^T], permuted comb_weight.bias), cached until a
        parameter changes in place."""
        params = [self.bases_weight, self.comb_weight.weight, self.comb_weight.bias]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return self._pack()
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self._wcat_key:
            with torch.no_grad():
                self._wcat = self._pack()
            self._wcat_key = key
            self._planes = None
        return self._wcat

    def _weight_planes(self, spec, wcat):
        """split-precision planes of wcat for the matrix-core GEMM, rebuilt with the packed weights."""
        if not wcat.is_cuda or gemm_exact() or wcat.requires_grad:
            return None
        if self._planes is None or self._planes.device != wcat.device:
            self._planes = pack_weights(spec, wcat)
        return self._planes

    def _train_record(self, graph, spec, x):
        """The layer's training call on `graph` (functional.TrainCall): the parameters as they are, comb rows to be permuted."""
        return TrainCall(graph, spec, x, self.bias, self.comb_weight.weight, self.comb_weight.bias, None, [self.bases_weight],
                         self.in_channels, self.num_heads, len(self.aggregators), self.num_bases, spec.basis_len,
                         spec.basis_stride, True)

    def _train_call(self, x, edge_index):
        """The TrainCall of functional.egc_layer_apply_params for a training call, or None (what forward() below passes on its
        training path; egc_amd.FusedEGCBlock hands it to the compiled binding's block nodes)."""
        bw, cb = self.bases_weight, self.comb_weight.bias
        if not (bw.is_cuda and bw.dtype == torch.float32 and cb is not None and x.is_cuda) or ops.use_torch_op():
            return None
        if self.cached and self._cached_graph is not None:
            graph, spec = self._cached_graph
        elif isinstance(edge_index, GraphBatch):
            graph, spec = edge_index, self._spec_coo
        else:
            if self.cached:
                return None          # (forward() builds and caches the graph first)
            graph = graph_from_input(edge_index, x.size(self.node_dim))
            spec = self._spec_coo if (isinstance(edge_index, torch.Tensor) and edge_index.layout == torch.strided) else self._spec_adj
        return self._train_record(graph, spec, x)

    def forward(self, x, edge_index):
        if self.cached and self._cached_graph is not None:
            graph, spec = self._cached_graph
        else:
            graph = graph_from_input(edge_index, x.size(self.node_dim), static=bool(self.cached))
            is_coo = (isinstance(edge_index, torch.Tensor) and edge_index.layout == torch.strided) or isinstance(edge_index, GraphBatch)
            spec = self._spec_coo if is_coo else self._spec_adj
            if self.cached:
                self._cached_graph = (graph.trim_launches(), spec)
        bw, cw, cb = self.bases_weight, self.comb_weight.weight, self.comb_weight.bias
        if (torch.is_grad_enabled() and bw.is_cuda and bw.dtype == torch.float32 and cb is not None and x.is_cuda
                and (bw.requires_grad or cw.requires_grad or cb.requires_grad) and not ops.use_torch_op()):
            # training: parameters in, parameter gradients out, one autograd node (pack + layer + unpack)
            return egc_layer_apply_params(self._train_record(graph, spec, x))
        wcat, bcat = self._packed_weights()
        return egc_layer_apply(graph, spec, x, wcat, bcat, self.bias, packed=self._weight_planes(spec, wcat))

    def __repr__(self):
        return "{}({}, {}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels,
                                       self.aggregators)
