"""Mini-batches collated on the device into the static buffers of a recording (egc_collate.hip through the C ABI).

The reference takes its batches from PyG's ``DataLoader``: per-graph collation in Python on the CPU, then
``batch.to(device)`` (zinc/configs.py:53-67, mol/configs.py:52-70, cifar/configs.py:66-82, code/configs.py:47-69).  The
datasets of its batched nets fit in a fraction of device memory, so here the dataset lives there (``GraphStore``) and one
call (``BatchCollator.collate`` / ``next``: two launches, no allocation, no read-back, no synchronisation) writes a batch
into buffers padded to one static shape, following the padding convention of a recorded step (hipgraph.py): zero feature
rows, padding rows in a spare last graph, padding edges as self-loops on the last row.  Recorded inside a ``GraphedStep``,
``next()`` makes one replay the entire iteration.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _C
from .graph import _IndexFlag, _device_guard, _require_cuda, _stream_ptr

EGC_COLLATE_MAX_FIELDS = _C.COLLATE_MAX_FIELDS
EGC_COLLATE_MAX_GRAPHS = _C.COLLATE_MAX_GRAPHS
EGC_COLLATE_MAX_ROW_BYTES = _C.COLLATE_MAX_ROW_BYTES

_FIELD_DTYPES = (torch.float32, torch.int32, torch.int64, torch.float64)
_BITS_DTYPE = {4: torch.int32, 8: torch.int64}


def _check_ptr(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1:
        raise RuntimeError(f"egc_amd: {what} must be an int64 tensor of shape [M + 1]")


def _check_fields(fields, kind, rows):
    fields = dict(fields or {})
    if len(fields) > EGC_COLLATE_MAX_FIELDS:
        raise RuntimeError(f"egc_amd: at most EGC_COLLATE_MAX_FIELDS = {EGC_COLLATE_MAX_FIELDS} {kind} fields "
                           f"(got {len(fields)})")
    for name, t in fields.items():
        if not isinstance(t, torch.Tensor) or t.dtype not in _FIELD_DTYPES:
            raise RuntimeError(f"egc_amd: {kind} field '{name}' must be a float32, int32, int64 or float64 tensor "
                               f"(got {getattr(t, 'dtype', type(t))})")
        if t.dim() < 1 or t.size(0) != rows or not t.is_contiguous():
            raise RuntimeError(f"egc_amd: {kind} field '{name}' must be a contiguous tensor of shape [{rows}, ...] "
                               f"(got {tuple(t.shape)})")
        row_bytes = _row_bytes(t)
        if row_bytes == 0 or row_bytes > EGC_COLLATE_MAX_ROW_BYTES:
            raise RuntimeError(f"egc_amd: a row of {kind} field '{name}' has {row_bytes} bytes; 1 to "
                               f"EGC_COLLATE_MAX_ROW_BYTES = {EGC_COLLATE_MAX_ROW_BYTES} are supported")
    return fields


def _row_bytes(t: torch.Tensor) -> int:
    n = t.element_size()
    for s in t.shape[1:]:
        n *= int(s)
    return n


class GraphStore:
    """M graphs back to back on one device; none of the tensors is copied.

    ``node_ptr`` / ``edge_ptr``: int64 [M + 1] offsets of each graph's nodes and edges; ``edge_index``: int64
    [2, E_all] with node ids LOCAL to their graph (as PyG stores a dataset), a graph's edges contiguous and in their
    stored order; ``node_fields``: name -> [N_all, ...]; ``graph_fields``: name -> [M, ...].  Fields are float32, int32,
    int64 or float64 with contiguous rows of at most EGC_COLLATE_MAX_ROW_BYTES bytes, at most EGC_COLLATE_MAX_FIELDS of
    each kind, names unique over both kinds.  The constructor validates shapes, dtypes and the pointers (it
    synchronises: this is set-up)."""

    def __init__(self, node_ptr, edge_ptr, edge_index, node_fields=None, graph_fields=None):
        _check_ptr(node_ptr, "node_ptr")
        _check_ptr(edge_ptr, "edge_ptr")
        if edge_ptr.numel() != node_ptr.numel():
            raise RuntimeError("egc_amd: node_ptr and edge_ptr must both have M + 1 entries")
        if (not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() != 2
                or edge_index.size(0) != 2):
            raise RuntimeError("egc_amd: edge_index must be an int64 tensor of shape [2, E]")
        self.n_graphs = node_ptr.numel() - 1
        self.n_edges_all = int(edge_index.size(1))
        self.n_nodes_all = int(node_ptr[-1].item())
        self.node_fields = _check_fields(node_fields, "node", self.n_nodes_all)
        self.graph_fields = _check_fields(graph_fields, "graph", self.n_graphs)
        if set(self.node_fields) & set(self.graph_fields):
            raise RuntimeError("egc_amd: a node field and a graph field share a name")
        if not node_ptr.is_contiguous() or not edge_ptr.is_contiguous() or not edge_index.is_contiguous():
            raise RuntimeError("egc_amd: node_ptr, edge_ptr and edge_index must be contiguous")
        for what, p, end in (("node_ptr", node_ptr, self.n_nodes_all), ("edge_ptr", edge_ptr, self.n_edges_all)):
            if int(p[0].item()) != 0 or int(p[-1].item()) != end or bool((p[1:] < p[:-1]).any().item()):
                raise RuntimeError(f"egc_amd: {what} must be non-decreasing, start at 0 and end at {end}")
        tensors = [node_ptr, edge_ptr, edge_index, *self.node_fields.values(), *self.graph_fields.values()]
        for t in tensors:
            _require_cuda(t, "every tensor of a GraphStore")
        if any(t.device != node_ptr.device for t in tensors):
            raise RuntimeError("egc_amd: every tensor of a GraphStore must live on one device")
        self.node_ptr, self.edge_ptr, self.edge_index = node_ptr, edge_ptr, edge_index
        self.device = node_ptr.device
        self._capacity = {}

    def capacity(self, batch_size: int):
        """(n_pad, e_pad) that hold ANY batch of ``batch_size`` graphs of this store: the sum of the ``batch_size`` largest
        node counts plus 1 (the last row always belongs to the spare graph), the sum of the ``batch_size`` largest edge
        counts and at least 1.  Computed once per batch size with torch (synchronises)."""
        g = int(batch_size)
        hit = self._capacity.get(g)
        if hit is None:
            k = min(max(g, 0), self.n_graphs)
            n_top = torch.topk(self.node_ptr[1:] - self.node_ptr[:-1], k).values.sum() if k else 0
            e_top = torch.topk(self.edge_ptr[1:] - self.edge_ptr[:-1], k).values.sum() if k else 0
            hit = self._capacity[g] = (int(n_top) + 1, max(int(e_top), 1))
        return hit


class BatchCollator:
    """The static, padded buffers of one batch of up to ``batch_size`` = G graphs of a ``GraphStore``, and the launch that
    fills them.  The buffers are allocated once and stay the same objects, so a recording can hold them:

      fields[name] (node)   [n_pad, ...]   real rows in batch order; rows >= n_valid are all-zero bytes
      edge_index            int64 [2, e_pad]   local id + the graph's row offset; columns >= e_valid are (n_pad - 1, n_pad - 1)
      batch                 int64 [n_pad]   the slot of each row; rows >= n_valid hold G, the spare graph of the padding
      ptr, edge_ptr         int64 [G + 2]   offsets of slots 0 .. G (slots >= g_valid repeat n_valid / e_valid); last: n_pad / e_pad
      n_valid, e_valid, g_valid   int64 []
      counts                float32 [G + 1, 1]   rows per slot; 1.0 for slots without rows and for the spare graph
      graph_mask            float32 [G + 1, 1]   1.0 for slots < g_valid, else 0.0
      inv_g                 float32 []   1 / max(g_valid, 1)
      fields[name] (graph)  [G + 1, ...]   gathered rows; ``graph_fill[name]`` (default 0; NaN allowed for float fields) in
                            slots that hold no graph: slots >= g_valid, the spare graph, a slot whose id is out of range

    Every element of every buffer is written by every collate.  ``n_pad`` / ``e_pad`` default to ``store.capacity(G)``; at
    most n_pad - 1 rows are real.  The encoders (and a Linear embedding) take the node fields as they are,
    ``FusedEGCBlock(..., n_valid=)`` -- around an EGC layer or ``egc_amd.Mpnn`` -- the activations, ``edge_index`` and
    ``n_valid``, ``global_*_pool(x, batch, size=G + 1)`` the batch vector; the loss heads (``GraphHead``, ``TokenHead``,
    ``cross_entropy``) take the first G pooled rows and the first G rows of the label field (a full batch; NaN-filled labels
    of empty slots drop out of the masked BCE).  Every row of every intermediate array stays finite, padding included
    (tests/test_batched_nets_golden.py runs the reference's molhiv, CIFAR and ogbg-code nets this way).

    Malformed input never writes out of bounds and never goes unreported: a graph id outside [0, M) is an empty slot
    (status bit 1); the first graph with which the rows would exceed n_pad - 1 (bit 2) or the edges e_pad (bit 4), and
    every graph after it, are dropped.  The bits collect in the device word ``status`` and raise the package's sticky host
    word, so the error surfaces at the next call into the package at the latest; ``check()`` names the cause."""

    def __init__(self, store: GraphStore, batch_size: int, n_pad=None, e_pad=None, graph_fill=None):
        if not isinstance(store, GraphStore):
            raise RuntimeError("egc_amd: BatchCollator needs a GraphStore")
        g = int(batch_size)
        if not 1 <= g <= EGC_COLLATE_MAX_GRAPHS:
            raise RuntimeError(f"egc_amd: batch_size must be in 1 .. EGC_COLLATE_MAX_GRAPHS = {EGC_COLLATE_MAX_GRAPHS} (got {g})")
        graph_fill = dict(graph_fill or {})
        unknown = set(graph_fill) - set(store.graph_fields)
        if unknown:
            raise RuntimeError(f"egc_amd: graph_fill names no graph field of the store: {sorted(unknown)}")
        if n_pad is None or e_pad is None:
            cap = store.capacity(g)
            n_pad, e_pad = cap[0] if n_pad is None else n_pad, cap[1] if e_pad is None else e_pad
        n_pad, e_pad = int(n_pad), int(e_pad)
        if not (1 <= n_pad < 2 ** 31 and 1 <= e_pad < 2 ** 31):
            raise RuntimeError(f"egc_amd: n_pad and e_pad must be in 1 .. 2^31 - 1 (got {n_pad}, {e_pad})")
        lib = _C.load()
        self.store, self.batch_size, self.n_pad, self.e_pad = store, g, n_pad, e_pad
        dev = self.device = store.device
        with _device_guard(dev):
            i64 = dict(dtype=torch.int64, device=dev)
            self.edge_index = torch.zeros((2, e_pad), **i64)
            self.batch = torch.zeros(n_pad, **i64)
            self.ptr, self.edge_ptr = torch.zeros(g + 2, **i64), torch.zeros(g + 2, **i64)
            self.n_valid, self.e_valid, self.g_valid = (torch.zeros((), **i64) for _ in range(3))
            self.counts = torch.ones((g + 1, 1), dtype=torch.float32, device=dev)
            self.graph_mask = torch.zeros((g + 1, 1), dtype=torch.float32, device=dev)
            self.inv_g = torch.ones((), dtype=torch.float32, device=dev)
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.fields = {}
            self._c_fields = _C.EgcCollateFields()
            self._c_fields.n_node, self._c_fields.n_graph = len(store.node_fields), len(store.graph_fields)
            for k, (name, src) in enumerate(store.node_fields.items()):
                dst = self.fields[name] = torch.zeros((n_pad,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
                self._c_fields.node[k] = _C.EgcCollateField(src.data_ptr(), dst.data_ptr(), _row_bytes(src), src.element_size(), 0)
            for k, (name, src) in enumerate(store.graph_fields.items()):
                dst = self.fields[name] = torch.zeros((g + 1,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
                fill = graph_fill.get(name, 0)
                bits = int(torch.tensor([fill], dtype=src.dtype).view(_BITS_DTYPE[src.element_size()]).item())
                self._c_fields.graph[k] = _C.EgcCollateField(src.data_ptr(), dst.data_ptr(), _row_bytes(src), src.element_size(),
                                                             bits & (2 ** 64 - 1))
            # cursor mode: a permutation of up to M graph ids, its length and the batch cursor, all read on the device
            self._perm = torch.arange(max(store.n_graphs, 1), **i64)
            self._perm_len = torch.full((), store.n_graphs, **i64)
            self._cursor = torch.zeros((), **i64)
            self._epoch_len = store.n_graphs
            self._ws_bytes = int(lib.egc_collate_workspace_bytes(g))
            self._ws = torch.zeros(self._ws_bytes // 8, **i64)
        self._c_store = _C.EgcCollateStore(store.node_ptr.data_ptr(), store.edge_ptr.data_ptr(), store.edge_index.data_ptr(),
                                           store.n_graphs, store.n_edges_all)
        self._c_out = _C.EgcCollateOut(self.edge_index.data_ptr(), self.batch.data_ptr(), self.ptr.data_ptr(),
                                       self.edge_ptr.data_ptr(), self.n_valid.data_ptr(), self.e_valid.data_ptr(),
                                       self.g_valid.data_ptr(), self.counts.data_ptr(), self.graph_mask.data_ptr(),
                                       self.inv_g.data_ptr(), self.status.data_ptr())
        self._call = lib.egc_collate
        self._store_ref, self._fields_ref, self._out_ref = C.byref(self._c_store), C.byref(self._c_fields), C.byref(self._c_out)

    def _launch(self, ids_ptr, n_ids):
        _IndexFlag.poll()
        dev = self.device
        with _device_guard(dev):
            _C.check(self._call(self._store_ref, self._fields_ref, self._out_ref, ids_ptr, n_ids, self._perm.data_ptr(),
                                self._perm_len.data_ptr(), self._cursor.data_ptr(), self.batch_size, self.n_pad, self.e_pad,
                                self._ws.data_ptr(), self._ws_bytes, _IndexFlag.ptr(), _stream_ptr(dev)), "egc_collate")

    def collate(self, ids: torch.Tensor) -> "BatchCollator":
        """Write the batch of graphs ``ids`` (device int64 [k], 1 <= k <= G, repeats allowed) into the buffers: two launches
        on the current stream, no allocation, no read-back, no synchronisation; records inside a ``GraphedStep`` (``ids``
        is then a static buffer)."""
        _require_cuda(ids, "ids")
        if ids.dtype != torch.int64 or ids.dim() != 1 or not 1 <= ids.numel() <= self.batch_size or not ids.is_contiguous() \
                or ids.device != self.device:
            raise RuntimeError(f"egc_amd: ids must be a contiguous int64 tensor of shape [k], 1 <= k <= {self.batch_size}, on "
                               f"the store's device (got {ids.dtype} {tuple(ids.shape)} on {ids.device})")
        self._launch(ids.data_ptr(), ids.numel())
        return self

    def set_epoch(self, perm: torch.Tensor) -> "BatchCollator":
        """Start an epoch over ``perm`` (device int64 [M'], G <= M' <= M: any subset / order of graph ids): the ids are copied
        into the collator's fixed buffer and the cursor is zeroed, so a recording that holds ``next()`` stays valid.  The
        epoch is floor(M' / G) full batches (drop-last)."""
        _require_cuda(perm, "perm")
        if perm.dtype != torch.int64 or perm.dim() != 1 or perm.device != self.device:
            raise RuntimeError("egc_amd: perm must be an int64 tensor of shape [M'] on the store's device")
        if not self.batch_size <= perm.numel() <= self.store.n_graphs:
            raise ValueError(f"egc_amd: an epoch needs between batch_size = {self.batch_size} and M = {self.store.n_graphs} "
                             f"graph ids (got {perm.numel()})")
        with _device_guard(self.device):
            self._perm[:perm.numel()].copy_(perm)
            self._perm_len.fill_(perm.numel())
            self._cursor.zero_()
        self._epoch_len = perm.numel()
        return self

    def next(self) -> "BatchCollator":
        """Collate batch perm[cursor * G : (cursor + 1) * G] of the epoch and advance the cursor, all on the device: the same
        (recorded) launch serves successive batches; past the last full batch the cursor wraps to 0.  Without a
        ``set_epoch`` the epoch is the store in its stored order."""
        if self._epoch_len < self.batch_size:
            raise ValueError(f"egc_amd: the store holds fewer than batch_size = {self.batch_size} graphs: no full batch")
        self._launch(None, 0)
        return self

    def batches_per_epoch(self) -> int:
        return self._epoch_len // self.batch_size

    def check(self) -> "BatchCollator":
        """Raise if a collate since the last check met malformed input, naming the cause (synchronises; clears the status)."""
        code = int(self.status.item())
        if code != 0:
            self.status.zero_()
            if _IndexFlag._view is not None:
                _IndexFlag._view.value = 0      # reported here
            causes = [text for bit, text in ((1, "a graph id outside [0, M) (an empty slot)"),
                                             (2, f"a batch of more than n_pad - 1 = {self.n_pad - 1} rows (cut short)"),
                                             (4, f"a batch of more than e_pad = {self.e_pad} edges (cut short)")) if code & bit]
            raise RuntimeError(f"egc_amd.BatchCollator: status {code}: " + "; ".join(causes))
        return self
