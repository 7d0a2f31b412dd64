"""Node encoders: the first stage of the reference's batched nets, ``x = self.embedding(batch.x)`` followed by
``x = self.in_feat_dropout(x)`` (zinc/models.py:28-30,62-63; mol/pna_style_models.py:33-34,66-69;
code/models.py:27-45,62-70,104-112).

All three encoders of the reference are one operation -- a sum of rows of T embedding tables, tables in ascending
order -- and run here as one forward launch and two backward launches (``egc_amd/csrc/egc_encoder.hip``) instead of a
gather and an add per table forward and a sort plus a segmented sum per table backward.  The forward's bits are those
of the reference's expression; the backward sums in an order that depends on the indices and the shapes alone, so it is
reproducible from run to run.

``Embedding``, ``AtomEncoder`` and ``ASTNodeEncoder`` keep the constructor arguments, the initialisation and the
state-dict keys of what they replace: the tables ARE ``nn.Embedding`` modules, the reference's checkpoints load with
``strict=True``, and the gradients land in their ``weight.grad`` (row ranges of one buffer, no copy per table).
CPU tensors, tables that are not float32, and shapes beyond the limits of ``include/egc_hip.h`` take torch's own
operators.  Nothing here reads back from the device: the encoders work inside ``GraphedStep``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

from .functional import encoder_backward, encoder_forward, encoder_supported

# rows of the nine tables of ogb's AtomEncoder (ogb.utils.features.get_atom_feature_dims(); as printed with the
# reference's pretrained molhiv nets, output/pretrained.txt:460-470)
ATOM_FEATURE_DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)


class _EncoderFunction(torch.autograd.Function):
    """out = (dropout of) the sum of the tables' rows; the tables' gradients from the two backward launches."""

    @staticmethod
    def forward(ctx, idx, clamp, keep, keep_scale, *tables):
        ctx.clamp, ctx.keep_scale, ctx.rows = clamp, keep_scale, [w.size(0) for w in tables]
        ctx.save_for_backward(idx, keep) if keep is not None else ctx.save_for_backward(idx)
        return encoder_forward([w.detach() for w in tables], idx, clamp, keep, keep_scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        idx, *keep = ctx.saved_tensors
        grads = encoder_backward(d_out, idx, ctx.rows, ctx.clamp, keep[0] if keep else None, ctx.keep_scale)
        return (None, None, None, None, *grads)


class _EncoderBase(nn.Module):
    """Shared forward of the encoders; a subclass owns the ``nn.Embedding`` tables and names them as its original does."""

    def _init_encoder(self, clamp, dropout: float):
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout probability has to be in [0, 1), got {dropout}")
        self.clamp = None if clamp is None else tuple(None if c is None else int(c) for c in clamp)
        self.dropout = float(dropout)
        self.last_keep_mask = None

    def _tables(self) -> list:
        raise NotImplementedError

    def _encode(self, idx: torch.Tensor) -> torch.Tensor:
        tables = [m.weight for m in self._tables()]
        if idx.dim() == 1:
            idx = idx[:, None]
        if idx.dim() != 2 or idx.size(1) != len(tables):
            raise ValueError(f"egc_amd: expected an index tensor of shape [N, {len(tables)}]"
                             f"{' or [N]' if len(tables) == 1 else ''}, got {tuple(idx.shape)}")
        if idx.dtype != torch.int64:
            raise ValueError(f"egc_amd: encoder indices must be int64 (got {idx.dtype})")
        dropping = self.dropout > 0.0 and self.training
        if not encoder_supported(tables, idx):
            return self._encode_torch(idx, dropping)
        keep, scale = None, 1.0
        if dropping:
            keep = torch.empty((idx.size(0), tables[0].size(1)), dtype=torch.uint8, device=idx.device)
            keep.bernoulli_(1.0 - self.dropout)
            self.last_keep_mask = keep
            scale = 1.0 / (1.0 - self.dropout)
        if torch.is_grad_enabled() and any(w.requires_grad for w in tables):
            return _EncoderFunction.apply(idx, self.clamp, keep, scale, *tables)
        return encoder_forward(tables, idx, self.clamp, keep, scale)

    def _encode_torch(self, idx: torch.Tensor, dropping: bool) -> torch.Tensor:
        """torch's operators, composed as the reference composes them (CPU tensors, other dtypes, beyond the limits)."""
        out = None
        for t, m in enumerate(self._tables()):
            col = idx[:, t]
            if self.clamp is not None and self.clamp[t] is not None:
                col = col.clamp(max=self.clamp[t])     # (a new tensor: the caller's indices stay as they are)
            out = m(col) if out is None else out + m(col)
        return nn.functional.dropout(out, self.dropout, True) if dropping else out


class NodeEncoder(_EncoderBase):
    """``out[n] = ((W_0[idx[n,0]] + W_1[idx[n,1]]) + ...)``, then an optional dropout: the general form of the three
    encoders below.  ``table_rows``: rows of each table; ``clamp[t]`` (or None): indices of table t above it are read as
    ``clamp[t]``; ``dropout``: the net's ``in_feat_dropout`` folded into the store (one uint8 mask per element drawn from
    torch's generator on the device, kept in ``last_keep_mask``; nothing is drawn in eval mode or at 0).
    Tables are ``nn.Embedding`` modules under ``tables`` (N(0, 1) initialisation)."""

    def __init__(self, table_rows: Sequence[int], emb_dim: int, clamp: Optional[Sequence[Optional[int]]] = None,
                 dropout: float = 0.0):
        super().__init__()
        table_rows = [int(r) for r in table_rows]
        if not table_rows or min(table_rows) <= 0 or int(emb_dim) <= 0:
            raise ValueError("egc_amd: NodeEncoder needs at least one table, every table with rows, and emb_dim > 0")
        if clamp is not None and len(clamp) != len(table_rows):
            raise ValueError("egc_amd: clamp must name one value (or None) per table")
        self._init_encoder(clamp, dropout)
        self.tables = nn.ModuleList([nn.Embedding(r, emb_dim) for r in table_rows])

    def _tables(self):
        return list(self.tables)

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        return self._encode(idx)


class Embedding(_EncoderBase):
    """Drop-in for the ``nn.Embedding(num_embeddings, embedding_dim)`` at the head of the ZINC nets
    (zinc/models.py:28-29,62): state-dict key ``weight``, N(0, 1) initialisation, input ``[N]`` int64.  ``padding_idx``,
    ``max_norm``, ``scale_grad_by_freq`` and sparse gradients are not offered (the reference uses none of them)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, dropout: float = 0.0):
        super().__init__()
        if int(num_embeddings) <= 0 or int(embedding_dim) <= 0:
            raise ValueError("egc_amd: Embedding needs num_embeddings > 0 and embedding_dim > 0")
        self._init_encoder(None, dropout)
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self.weight = nn.Parameter(torch.empty(self.num_embeddings, self.embedding_dim))
        nn.init.normal_(self.weight)

    def _tables(self):
        return [self]

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        return self._encode(idx.reshape(-1)).view(*idx.shape, self.embedding_dim)

    def _encode_torch(self, idx, dropping):
        out = nn.functional.embedding(idx[:, 0], self.weight)
        return nn.functional.dropout(out, self.dropout, True) if dropping else out


class AtomEncoder(_EncoderBase):
    """Drop-in for ``ogb.graphproppred.mol_encoder.AtomEncoder(emb_dim)`` (mol/pna_style_models.py:5,33,66): nine tables
    of 119, 4, 12, 12, 10, 6, 6, 2, 2 rows under ``atom_embedding_list.{0..8}.weight``, ``xavier_uniform_``
    initialisation, input ``[N, 9]`` int64, output ``0 + sum_t table_t[x[:, t]]`` in table order."""

    def __init__(self, emb_dim: int, dropout: float = 0.0):
        super().__init__()
        if int(emb_dim) <= 0:
            raise ValueError("egc_amd: AtomEncoder needs emb_dim > 0")
        self._init_encoder(None, dropout)
        self.atom_embedding_list = nn.ModuleList()
        for rows in ATOM_FEATURE_DIMS:
            emb = nn.Embedding(rows, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)

    def _tables(self):
        return list(self.atom_embedding_list)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._encode(x)


class ASTNodeEncoder(_EncoderBase):
    """Drop-in for the reference's ``ASTNodeEncoder(emb_dim, num_nodetypes, num_nodeattributes, max_depth)``
    (code/models.py:27-45): ``type_encoder.weight``, ``attribute_encoder.weight``, ``depth_encoder.weight`` (the last with
    ``max_depth + 1`` rows), ``forward(x, depth) = (type[x[:, 0]] + attribute[x[:, 1]]) + depth_table[min(depth, max_depth)]``.
    The reference clamps ``depth`` IN PLACE (code/models.py:40); here the clamp happens where the index is read and the
    caller's ``depth`` tensor is left untouched.  The two inputs are joined into one ``[N, 3]`` index matrix first (one
    small concatenation in front of the encoder's launch)."""

    def __init__(self, emb_dim: int, num_nodetypes: int, num_nodeattributes: int, max_depth: int, dropout: float = 0.0):
        super().__init__()
        if min(int(emb_dim), int(num_nodetypes), int(num_nodeattributes)) <= 0 or int(max_depth) < 0:
            raise ValueError("egc_amd: ASTNodeEncoder needs positive sizes and max_depth >= 0")
        self.max_depth = int(max_depth)
        self._init_encoder((None, None, self.max_depth), dropout)
        self.type_encoder = nn.Embedding(num_nodetypes, emb_dim)
        self.attribute_encoder = nn.Embedding(num_nodeattributes, emb_dim)
        self.depth_encoder = nn.Embedding(self.max_depth + 1, emb_dim)

    def _tables(self):
        return [self.type_encoder, self.attribute_encoder, self.depth_encoder]

    def forward(self, x: torch.Tensor, depth: torch.Tensor) -> torch.Tensor:
        if x.dim() != 2 or x.size(1) < 2 or depth.numel() != x.size(0):
            raise ValueError(f"egc_amd: ASTNodeEncoder takes x [N, 2] and depth [N] (got {tuple(x.shape)}, {tuple(depth.shape)})")
        return self._encode(torch.cat([x[:, :2], depth.reshape(-1, 1)], dim=1))
