"""CPU tests of the device-side collation: the numpy oracle (tests/collate_ref.py) against a hand-written example and its
own cut / fill rules, the argument validation of GraphStore / BatchCollator, and the host-only entry point of the library."""

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
import collate_ref as ref

# three graphs: A = 2 nodes, 2 edges; B = 1 node, no edge; C = 3 nodes, 3 edges (node ids local to their graph)
NODE_PTR = [0, 2, 3, 6]
EDGE_PTR = [0, 2, 2, 5]
EDGE_INDEX = [[0, 1, 0, 1, 2],
              [1, 0, 1, 2, 0]]
X = np.array([[10, 11], [20, 21], [30, 31], [40, 41], [50, 51], [60, 61]], dtype=np.int64)
Y = np.array([1.5, 2.5, 3.5], dtype=np.float32)


def _example(ids, g_pad, n_pad, e_pad, fill=None):
    return ref.collate(NODE_PTR, EDGE_PTR, EDGE_INDEX, {"x": X}, {"y": Y}, ids, g_pad, n_pad, e_pad, fill)


def test_oracle_against_a_hand_written_three_graph_batch():
    """Batch (C, A) in four slots, padded to 8 rows and 7 edges: every buffer spelled out."""
    out = _example([2, 0], 4, 8, 7, {"y": float("nan")})
    assert out["status"] == 0
    assert (int(out["n_valid"]), int(out["e_valid"]), int(out["g_valid"])) == (5, 5, 2)
    assert out["ptr"].tolist() == [0, 3, 5, 5, 5, 8]             # slots 0 .. 4 (4 = the spare graph), then n_pad
    assert out["edge_ptr"].tolist() == [0, 3, 5, 5, 5, 7]
    assert out["batch"].tolist() == [0, 0, 0, 1, 1, 4, 4, 4]
    assert out["edge_index"].tolist() == [[0, 1, 2, 3, 4, 7, 7], [1, 2, 0, 4, 3, 7, 7]]
    assert out["fields"]["x"].tolist() == [[40, 41], [50, 51], [60, 61], [10, 11], [20, 21], [0, 0], [0, 0], [0, 0]]
    assert out["counts"][:, 0].tolist() == [3.0, 2.0, 1.0, 1.0, 1.0]
    assert out["graph_mask"][:, 0].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert float(out["inv_g"]) == 0.5
    y = out["fields"]["y"]
    assert y[:2].tolist() == [3.5, 1.5] and np.isnan(y[2:]).all() and y.dtype == np.float32
    assert all(out[k].dtype == np.int64 for k in ("ptr", "edge_ptr", "batch", "edge_index", "n_valid"))


def test_oracle_capacity_cut_and_fill_rules():
    # exactly n_pad - 1 rows and e_pad edges: nothing is cut
    out = _example([0, 1, 2], 3, 7, 5)
    assert out["status"] == 0 and int(out["g_valid"]) == 3 and int(out["n_valid"]) == 6 and int(out["e_valid"]) == 5
    assert out["ptr"].tolist() == [0, 2, 3, 6, 7] and out["batch"].tolist() == [0, 0, 1, 2, 2, 2, 3]
    # one row too many: the first graph that does not fit and EVERY graph after it go (B would still fit)
    out = _example([0, 2, 1], 3, 5, 9)
    assert out["status"] == ref.STATUS_NODE_CAP and int(out["g_valid"]) == 1 and int(out["n_valid"]) == 2
    assert out["ptr"].tolist() == [0, 2, 2, 2, 5] and out["fields"]["y"].tolist() == [1.5, 0.0, 0.0, 0.0]
    assert out["edge_index"][:, 2:].tolist() == [[4] * 7, [4] * 7] and out["graph_mask"][:, 0].tolist() == [1, 0, 0, 0]
    # one edge too many
    out = _example([0, 2], 2, 9, 4)
    assert out["status"] == ref.STATUS_EDGE_CAP and int(out["g_valid"]) == 1 and int(out["e_valid"]) == 2
    # both at once are both named
    assert _example([0, 2], 2, 5, 4)["status"] == ref.STATUS_NODE_CAP | ref.STATUS_EDGE_CAP
    # ids outside the store: empty slots that stay in the batch, with the fill in their graph fields
    out = _example([3, 1, -1], 3, 4, 1, {"y": -7.0})
    assert out["status"] == ref.STATUS_BAD_ID and int(out["g_valid"]) == 3 and int(out["n_valid"]) == 1
    assert out["ptr"].tolist() == [0, 0, 1, 1, 4] and out["counts"][:, 0].tolist() == [1, 1, 1, 1]
    assert out["fields"]["y"].tolist() == [-7.0, 2.5, -7.0, -7.0] and out["graph_mask"][:, 0].tolist() == [1, 1, 1, 0]
    assert float(out["inv_g"]) == float(np.float32(1.0 / 3))
    # repeats are separate slots
    out = _example([1, 1, 1], 3, 4, 1)
    assert out["batch"].tolist() == [0, 1, 2, 3] and out["fields"]["x"][:3].tolist() == [[30, 31]] * 3
    assert ref.capacity(NODE_PTR, EDGE_PTR, 2) == (6, 5) and ref.capacity(NODE_PTR, [0, 0, 0, 0], 5) == (7, 1)
    nan = np.array([np.nan], dtype=np.float32)
    assert ref.same_bits(nan, nan) and not ref.same_bits(nan, -nan) and not ref.same_bits(nan, nan.astype(np.float64))


def _store_args():
    return (torch.tensor(NODE_PTR), torch.tensor(EDGE_PTR), torch.tensor(EDGE_INDEX)), {"x": torch.from_numpy(X)}, \
        {"y": torch.from_numpy(Y)}


def test_graph_store_validates_its_arguments():
    (nptr, eptr, ei), nf, gf = _store_args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # everything in order, but on the CPU
        egc_amd.GraphStore(nptr, eptr, ei, nf, gf)
    with pytest.raises(RuntimeError, match="int64"):
        egc_amd.GraphStore(nptr.int(), eptr, ei, nf, gf)
    with pytest.raises(RuntimeError, match="M \\+ 1"):
        egc_amd.GraphStore(nptr, eptr[:-1], ei, nf, gf)
    with pytest.raises(RuntimeError, match="edge_index"):
        egc_amd.GraphStore(nptr, eptr, ei.int(), nf, gf)
    with pytest.raises(RuntimeError, match="edge_index"):
        egc_amd.GraphStore(nptr, eptr, ei.t().contiguous(), nf, gf)
    with pytest.raises(RuntimeError, match="non-decreasing"):
        egc_amd.GraphStore(torch.tensor([0, 3, 2, 6]), eptr, ei, nf, gf)
    with pytest.raises(RuntimeError, match="non-decreasing"):              # does not end at E_all
        egc_amd.GraphStore(nptr, torch.tensor([0, 2, 2, 4]), ei, nf, gf)
    with pytest.raises(RuntimeError, match="non-decreasing"):              # does not start at 0
        egc_amd.GraphStore(nptr, torch.tensor([1, 2, 2, 5]), ei, nf, gf)
    with pytest.raises(RuntimeError, match="float32, int32, int64 or float64"):
        egc_amd.GraphStore(nptr, eptr, ei, {"x": torch.zeros(6, 2, dtype=torch.float16)}, gf)
    with pytest.raises(RuntimeError, match="float32, int32, int64 or float64"):
        egc_amd.GraphStore(nptr, eptr, ei, nf, {"y": torch.zeros(3, dtype=torch.uint8)})
    with pytest.raises(RuntimeError, match=r"\[6, \.\.\.\]"):
        egc_amd.GraphStore(nptr, eptr, ei, {"x": torch.zeros(5, 2)}, gf)
    with pytest.raises(RuntimeError, match=r"\[3, \.\.\.\]"):
        egc_amd.GraphStore(nptr, eptr, ei, nf, {"y": torch.zeros(4)})
    with pytest.raises(RuntimeError, match="contiguous"):
        egc_amd.GraphStore(nptr, eptr, ei, {"x": torch.zeros(2, 6).t()}, gf)
    with pytest.raises(RuntimeError, match="EGC_COLLATE_MAX_FIELDS"):
        egc_amd.GraphStore(nptr, eptr, ei, {f"f{k}": torch.zeros(6) for k in range(egc_amd.EGC_COLLATE_MAX_FIELDS + 1)}, gf)
    with pytest.raises(RuntimeError, match="EGC_COLLATE_MAX_FIELDS"):
        egc_amd.GraphStore(nptr, eptr, ei, nf, {f"f{k}": torch.zeros(3) for k in range(9)})
    with pytest.raises(RuntimeError, match="4104 bytes"):                  # 1,026 float32: one element over the row limit
        egc_amd.GraphStore(nptr, eptr, ei, {"x": torch.zeros(6, 1026)}, gf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # exactly the limits: accepted as far as the device
        egc_amd.GraphStore(nptr, eptr, ei, {f"f{k}": torch.zeros(6, 512, dtype=torch.float64) for k in range(8)}, gf)
    with pytest.raises(RuntimeError, match="share a name"):
        egc_amd.GraphStore(nptr, eptr, ei, nf, {"x": torch.zeros(3)})
    assert egc_amd.EGC_COLLATE_MAX_FIELDS == 8 == _C.COLLATE_MAX_FIELDS


def test_batch_collator_validates_its_arguments():
    """Without a device no store can be built, so the collator's own checks run against a stand-in with a store's attributes."""
    (nptr, eptr, ei), nf, gf = _store_args()
    with pytest.raises(RuntimeError, match="GraphStore"):
        egc_amd.BatchCollator(object(), 4)
    store = object.__new__(egc_amd.GraphStore)
    store.node_ptr, store.edge_ptr, store.edge_index, store.node_fields, store.graph_fields = nptr, eptr, ei, nf, gf
    store.n_graphs, store.n_nodes_all, store.n_edges_all, store.device, store._capacity = 3, 6, 5, nptr.device, {}
    assert store.capacity(2) == ref.capacity(NODE_PTR, EDGE_PTR, 2) == (6, 5)
    assert store.capacity(64) == ref.capacity(NODE_PTR, EDGE_PTR, 64) == (7, 5)
    for g in (0, -1, 4097):
        with pytest.raises(RuntimeError, match="batch_size"):
            egc_amd.BatchCollator(store, g)
    with pytest.raises(RuntimeError, match="graph_fill"):
        egc_amd.BatchCollator(store, 2, graph_fill={"x": 0.0})
    for n_pad, e_pad in ((0, 4), (4, 0), (2 ** 31, 4), (4, 2 ** 31)):
        with pytest.raises(RuntimeError, match="n_pad and e_pad"):
            egc_amd.BatchCollator(store, 2, n_pad=n_pad, e_pad=e_pad)


def test_library_exports_the_collate_entry_points_and_sizes_its_workspace():
    lib = _C.load()
    assert hasattr(lib, "egc_collate") and hasattr(lib, "egc_collate_workspace_bytes")
    # three int64 words per slot (source node offset, source edge offset, source graph); 0 outside 1 .. 4096 graphs
    assert [lib.egc_collate_workspace_bytes(g) for g in (1, 3, 128, 2048, 4096)] == [24, 72, 3072, 49152, 98304]
    assert [lib.egc_collate_workspace_bytes(g) for g in (0, -5, 4097)] == [0, 0, 0]
    assert (_C.COLLATE_MAX_FIELDS, _C.COLLATE_MAX_GRAPHS, _C.COLLATE_MAX_ROW_BYTES) == (8, 4096, 4096)
    # a call that fails its host-side checks launches nothing (no device is touched)
    import ctypes as C
    st, fl, out = _C.EgcCollateStore(), _C.EgcCollateFields(), _C.EgcCollateOut()
    assert lib.egc_collate(C.byref(st), C.byref(fl), C.byref(out), None, 0, None, None, None, 4, 8, 8, None, 0, None, None) == 1
    assert lib.egc_collate(None, None, None, None, 0, None, None, None, 4, 8, 8, None, 0, None, None) == 1
