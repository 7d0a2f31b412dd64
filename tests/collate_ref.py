"""numpy restatement of the padded-batch layout that egc_amd.BatchCollator writes: concatenate the
selected graphs, add their row offsets, pad, apply the capacity cut.  The oracle of tests/test_collate_*.py; every
comparison against it is exact.  Written from the layout table alone, one graph at a time -- no scan, no bisection."""
import numpy as np

STATUS_BAD_ID, STATUS_NODE_CAP, STATUS_EDGE_CAP = 1, 2, 4


def capacity(node_ptr, edge_ptr, batch_size):
    """(n_pad, e_pad) of GraphStore.capacity: the batch_size largest node counts + 1; the largest edge counts, at least 1."""
    n = np.sort(np.diff(np.asarray(node_ptr)))[::-1][:batch_size].sum()
    e = np.sort(np.diff(np.asarray(edge_ptr)))[::-1][:batch_size].sum()
    return int(n) + 1, max(int(e), 1)


def fill_element(value, dtype):
    return np.array([value]).astype(dtype)


def collate(node_ptr, edge_ptr, edge_index, node_fields, graph_fields, ids, batch_size, n_pad, e_pad, graph_fill=None):
    """All buffers of a collate of graphs `ids` (a list) as a dict of numpy arrays, plus 'status' (the bits this call raises)."""
    node_ptr, edge_ptr, edge_index = np.asarray(node_ptr), np.asarray(edge_ptr), np.asarray(edge_index)
    g_pad, m = batch_size, len(node_ptr) - 1
    graph_fill = graph_fill or {}
    status = 0
    kept = []                      # (graph id or None) per kept slot
    n_valid = e_valid = 0
    ptr, eptr = [], []
    cut = False
    for gid in ids:
        gid = int(gid)
        if not 0 <= gid < m:
            status |= STATUS_BAD_ID          # reported wherever it stands, even behind a cut
            gid, n, e = None, 0, 0
        else:
            n, e = int(node_ptr[gid + 1] - node_ptr[gid]), int(edge_ptr[gid + 1] - edge_ptr[gid])
        if cut:
            continue
        if n_valid + n > n_pad - 1 or e_valid + e > e_pad:
            status |= (STATUS_NODE_CAP if n_valid + n > n_pad - 1 else 0) | (STATUS_EDGE_CAP if e_valid + e > e_pad else 0)
            cut = True
            continue
        kept.append(gid)
        ptr.append(n_valid)
        eptr.append(e_valid)
        n_valid += n
        e_valid += e
    g_valid = len(kept)
    out = {"status": status}
    out["n_valid"], out["e_valid"], out["g_valid"] = (np.array(v, dtype=np.int64) for v in (n_valid, e_valid, g_valid))
    out["ptr"] = np.array(ptr + [n_valid] * (g_pad + 1 - g_valid) + [n_pad], dtype=np.int64)
    out["edge_ptr"] = np.array(eptr + [e_valid] * (g_pad + 1 - g_valid) + [e_pad], dtype=np.int64)
    batch = np.full(n_pad, g_pad, dtype=np.int64)
    ei = np.full((2, e_pad), n_pad - 1, dtype=np.int64)
    counts = np.ones((g_pad + 1, 1), dtype=np.float32)
    mask = np.zeros((g_pad + 1, 1), dtype=np.float32)
    mask[:g_valid] = 1.0
    fields = {}
    for name, src in node_fields.items():
        src = np.asarray(src)
        fields[name] = np.zeros((n_pad,) + src.shape[1:], dtype=src.dtype)
    for name, src in graph_fields.items():
        src = np.asarray(src)
        fields[name] = np.empty((g_pad + 1,) + src.shape[1:], dtype=src.dtype)
        fields[name][...] = fill_element(graph_fill.get(name, 0), src.dtype)
    for slot, gid in enumerate(kept):
        if gid is None:
            continue
        n0, n1, e0, e1 = int(node_ptr[gid]), int(node_ptr[gid + 1]), int(edge_ptr[gid]), int(edge_ptr[gid + 1])
        o, eo = ptr[slot], eptr[slot]
        batch[o:o + n1 - n0] = slot
        ei[:, eo:eo + e1 - e0] = edge_index[:, e0:e1] + o
        if n1 > n0:
            counts[slot, 0] = n1 - n0
        for name, src in node_fields.items():
            fields[name][o:o + n1 - n0] = np.asarray(src)[n0:n1]
        for name, src in graph_fields.items():
            fields[name][slot] = np.asarray(src)[gid]
    out.update(batch=batch, edge_index=ei, counts=counts, graph_mask=mask, fields=fields,
               inv_g=np.array(np.float32(1.0 / max(g_valid, 1)), dtype=np.float32))
    return out


def same_bits(a, b):
    """Exact equality of two arrays of one dtype and shape, NaNs compared by bit pattern."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
