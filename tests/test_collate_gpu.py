"""egc_amd.GraphStore / BatchCollator on the device against the numpy oracle (tests/collate_ref.py), exactly: every buffer is
filled with a sentinel byte pattern before each call and compared whole, NaN fills by bit pattern."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import collate_ref as ref

pytestmark = pytest.mark.gpu

SCALARS = ("edge_index", "batch", "ptr", "edge_ptr", "n_valid", "e_valid", "g_valid", "counts", "graph_mask", "inv_g")


def _dev():
    return torch.device("cuda:0")


def _random_store(seed, node_counts, edge_counts):
    """numpy arrays of a store with the given per-graph sizes: every field kind and row size the copy dispatches on."""
    rng = np.random.default_rng(seed)
    node_counts, edge_counts = np.asarray(node_counts, dtype=np.int64), np.asarray(edge_counts, dtype=np.int64)
    m, n_all = len(node_counts), int(node_counts.sum())
    node_ptr = np.concatenate([[0], np.cumsum(node_counts)]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(edge_counts)]).astype(np.int64)
    ei = np.concatenate([rng.integers(0, n, size=(2, e)) for n, e in zip(node_counts, edge_counts)], axis=1).astype(np.int64)
    node_fields = {
        "a_i64": rng.integers(-2 ** 40, 2 ** 40, size=n_all).astype(np.int64),                  # 8-byte rows
        "x9_i64": rng.integers(0, 120, size=(n_all, 9)).astype(np.int64),                       # 72-byte rows: 8-byte units
        "pos3_f32": rng.standard_normal((n_all, 3)).astype(np.float32),                         # 12-byte rows: 4-byte units
        "f5_f32": rng.standard_normal((n_all, 5)).astype(np.float32),                           # 20-byte rows
        "d2_f64": rng.standard_normal((n_all, 2)),                                              # 16-byte rows: 16-byte units
        "depth_i32": rng.integers(0, 50, size=n_all).astype(np.int32),                          # 4-byte rows
        "q4_f32": rng.standard_normal((n_all, 4)).astype(np.float32),                           # 16-byte rows of 4-byte elements
        "off8_f64": rng.standard_normal((n_all, 2)),                                            # 16-byte rows at an 8 mod 16 address
    }
    graph_fields = {
        "y": rng.standard_normal(m).astype(np.float32),
        "tok_i64": rng.integers(0, 5002, size=(m, 5)).astype(np.int64),
        "w_f64": rng.standard_normal(m),
        "c_i32": rng.integers(0, 9, size=(m, 3)).astype(np.int32),
    }
    return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, edge_index=ei, node_fields=node_fields, graph_fields=graph_fields)


FILL = {"y": float("nan"), "tok_i64": -1, "w_f64": float("nan"), "c_i32": 7}


def _device_store(s):
    import egc_amd
    dev = _dev()
    nf = {k: torch.from_numpy(v).to(dev) for k, v in s["node_fields"].items()}
    # the same rows one element into a buffer: source rows of 16 bytes whose addresses are 8 mod 16 (the 8-byte path)
    raw = torch.zeros(nf["off8_f64"].numel() + 1, dtype=torch.float64, device=dev)
    raw[1:] = nf["off8_f64"].reshape(-1)
    nf["off8_f64"] = raw[1:].view(-1, 2)
    assert nf["off8_f64"].data_ptr() % 16 == 8 and nf["d2_f64"].data_ptr() % 16 == 0
    gf = {k: torch.from_numpy(v).to(dev) for k, v in s["graph_fields"].items()}
    return egc_amd.GraphStore(torch.from_numpy(s["node_ptr"]).to(dev), torch.from_numpy(s["edge_ptr"]).to(dev),
                              torch.from_numpy(s["edge_index"]).to(dev), nf, gf)


def _sentinel(col):
    for t in [getattr(col, k) for k in SCALARS] + list(col.fields.values()):
        t.view(-1).view(torch.uint8).fill_(0xA5)


def _want(s, col, ids):
    return ref.collate(s["node_ptr"], s["edge_ptr"], s["edge_index"], s["node_fields"], s["graph_fields"], list(ids),
                       col.batch_size, col.n_pad, col.e_pad, FILL)


def _assert_equals_oracle(col, want, what):
    torch.cuda.synchronize()
    for k in SCALARS:
        assert ref.same_bits(getattr(col, k).cpu().numpy(), want[k]), (what, k)
    assert set(col.fields) == set(want["fields"])
    for k, v in want["fields"].items():
        assert ref.same_bits(col.fields[k].cpu().numpy(), v), (what, k)
    assert int(col.status.item()) == want["status"], what


@pytest.fixture(scope="module")
def sweep_store():
    rng = np.random.default_rng(11)
    m = 300
    nodes = rng.integers(1, 13, size=m)
    nodes[rng.choice(m, 40, replace=False)] = 1                   # graphs of one node
    nodes[rng.choice(m, 30, replace=False)] = rng.integers(36, 45, size=30)   # graphs of about 40 nodes
    edges = rng.integers(0, 3 * nodes + 1)
    edges[rng.choice(m, 60, replace=False)] = 0                   # graphs without edges
    assert nodes.sum() <= 4000
    s = _random_store(5, nodes, edges)
    return s, _device_store(s)


@pytest.mark.parametrize("g", [1, 3, 64, 257, 1025])
def test_geometry_sweep_equals_the_oracle(sweep_store, g):
    """One pass of the header's scan (G <= 1024), two with a partial last one (1025); k < G, k = G, repeated ids; every row size
    and alignment branch of the copy; selections that start at odd rows of the store; padding of 0, 3 and many rows."""
    import egc_amd
    s, store = sweep_store
    m = len(s["node_ptr"]) - 1
    rng = np.random.default_rng(100 + g)
    selections = [rng.integers(0, m, size=g),                                   # k = G, repeats as they fall
                  rng.integers(0, m, size=max(1, g // 2)),                      # k < G
                  np.repeat(rng.integers(0, m, size=max(1, g // 3)), 3)[:g],    # every id three times in a row
                  np.array([m - 1]), np.arange(1, 1 + min(g, m - 1))]           # one graph; a run that starts at graph 1
    need_n = [int(np.diff(s["node_ptr"])[ids].sum()) for ids in selections]
    need_e = [int(np.diff(s["edge_ptr"])[ids].sum()) for ids in selections]
    for slack in (0, 3, 301):
        col = egc_amd.BatchCollator(store, g, n_pad=max(need_n) + 1 + slack, e_pad=max(max(need_e), 1) + slack, graph_fill=FILL)
        for j, ids in enumerate(selections):
            _sentinel(col)
            col.collate(torch.from_numpy(ids.astype(np.int64)).to(_dev()))
            _assert_equals_oracle(col, _want(s, col, ids), (g, slack, j))
        col.check()
    if g <= m:                     # the default capacity holds any batch of distinct graphs, the largest ones included
        col = egc_amd.BatchCollator(store, g, graph_fill=FILL)
        assert (col.n_pad, col.e_pad) == store.capacity(g) == ref.capacity(s["node_ptr"], s["edge_ptr"], g)
        ids = np.argsort(-np.diff(s["node_ptr"]), kind="stable")[:g]
        _sentinel(col)
        col.collate(torch.from_numpy(ids.astype(np.int64)).to(_dev())).check()
        _assert_equals_oracle(col, _want(s, col, ids), (g, "capacity"))
        assert int(col.n_valid.item()) == col.n_pad - 1


def test_capacity_edges_are_clamped_flagged_and_named():
    """Exactly full: no flag.  One row / one edge too many: the tail is dropped as the oracle says, bit 2 / 4.  Ids M and -1:
    empty slots, bit 1.  After each flagged call the buffers equal the oracle's, check() raises, names the cause and clears,
    and a following good call is clean.  Nothing here may write outside a buffer."""
    import egc_amd
    # graph 0: 1 node, no edge; graph 1: 2 nodes, 1 edge; then graphs of 3 .. 9 nodes
    nodes = np.array([1, 2, 5, 9, 3, 7, 4, 6])
    edges = np.array([0, 1, 7, 12, 2, 9, 0, 5])
    s = _random_store(7, nodes, edges)
    store = _device_store(s)
    dev = _dev()
    m = len(nodes)

    def run(col, ids, what):
        _sentinel(col)
        col.collate(torch.tensor(ids, dtype=torch.int64, device=dev))
        want = _want(s, col, ids)
        _assert_equals_oracle(col, want, what)
        return want

    first = [3, 2, 5]                                       # 21 rows, 28 edges
    col = egc_amd.BatchCollator(store, 6, n_pad=22, e_pad=28, graph_fill=FILL)
    want = run(col, first, "exactly full")
    assert want["status"] == 0 and int(col.n_valid.item()) == 21 and int(col.e_valid.item()) == 28
    col.check()
    # one row too many: the one-node graph does not fit; the graph behind it (which has room in e_pad) goes with it
    want = run(col, first + [0, 6], "one row too many")
    assert want["status"] == ref.STATUS_NODE_CAP and int(col.g_valid.item()) == 3 and int(col.n_valid.item()) == 21
    with pytest.raises(RuntimeError, match="n_pad - 1 = 21 rows"):
        col.check()
    col.check()                                             # cleared
    want = run(col, first, "good call after the row cut")
    assert want["status"] == 0
    col.check()
    # one edge too many
    col = egc_amd.BatchCollator(store, 6, n_pad=40, e_pad=28, graph_fill=FILL)
    want = run(col, first + [1, 0], "one edge too many")
    assert want["status"] == ref.STATUS_EDGE_CAP and int(col.g_valid.item()) == 3 and int(col.e_valid.item()) == 28
    with pytest.raises(RuntimeError, match="e_pad = 28 edges"):
        col.check()
    run(col, first + [0, 6, 0], "good call after the edge cut")     # 27 rows, 28 edges
    col.check()
    # both capacities at the same graph: both named
    col = egc_amd.BatchCollator(store, 6, n_pad=22, e_pad=28, graph_fill=FILL)
    want = run(col, first + [1], "row and edge too many")
    assert want["status"] == ref.STATUS_NODE_CAP | ref.STATUS_EDGE_CAP
    with pytest.raises(RuntimeError, match="rows.*edges"):
        col.check()
    # ids outside the store
    want = run(col, [m, 4, -1, 1], "ids M and -1")
    assert want["status"] == ref.STATUS_BAD_ID and int(col.g_valid.item()) == 4 and int(col.n_valid.item()) == 5
    # not checked: the sticky host word reports it at the next call into the package, check() still names it
    with pytest.raises(RuntimeError, match="BatchCollator"):
        col.collate(torch.tensor(first, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="outside \\[0, M\\)"):
        col.check()
    run(col, first, "good call after the bad ids")
    col.check()
    # argument checks of the calls themselves
    with pytest.raises(RuntimeError, match="ids must be"):
        col.collate(torch.arange(7, device=dev))
    with pytest.raises(RuntimeError, match="ids must be"):
        col.collate(torch.arange(2, device=dev, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        col.collate(torch.arange(2))
    with pytest.raises(ValueError, match="epoch"):
        col.set_epoch(torch.arange(5, device=dev))
    with pytest.raises(ValueError, match="epoch"):
        col.set_epoch(torch.arange(m + 1, device=dev))


def _snapshot(col):
    return {k: getattr(col, k).clone() for k in SCALARS} | {"field:" + k: v.clone() for k, v in col.fields.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(-1).view(torch.uint8), b[k].view(-1).view(torch.uint8)) for k in a)


def test_next_recorded_once_serves_successive_batches_and_epochs(sweep_store):
    """next() reads cursor and permutation on the device: ONE recording of it, replayed floor(len / G) + 2 times, writes the
    batches perm[i G : (i + 1) G] in turn and wraps to 0; a second set_epoch goes through the same recording."""
    import egc_amd
    s, store = sweep_store
    m, g, dev = len(s["node_ptr"]) - 1, 7, _dev()
    col = egc_amd.BatchCollator(store, g, graph_fill=FILL)
    other = egc_amd.BatchCollator(store, g, graph_fill=FILL)
    graphed = egc_amd.GraphedStep(lambda: col.next(), warmup=2)       # (recording it at all: no synchronisation, no allocation)
    gen = torch.Generator().manual_seed(3)
    for length in (31, 23, m):
        perm = torch.randperm(m, generator=gen)[:length].to(dev)
        col.set_epoch(perm)
        batches = length // g
        assert col.batches_per_epoch() == batches and length % g != 0
        for i in list(range(batches + 2)) if length < m else (0, 1):
            _sentinel(col)
            graphed()
            got = _snapshot(col)
            ids = perm[(i % batches) * g:(i % batches + 1) * g]
            other.collate(ids)
            assert _same(got, _snapshot(other)), (length, i)
            if i == 0:
                _assert_equals_oracle(col, _want(s, col, ids.cpu().numpy()), (length, i))
    col.check()
    other.check()
    # eager next() continues where the replays stopped: the cursor lives on the device
    col.next()
    other.collate(perm[2 * g:3 * g])
    assert _same(_snapshot(col), _snapshot(other))


def test_training_through_next_in_the_recording_equals_training_fed_by_torch():
    """The small net of test_hipgraph_gpu.py::test_small_net_trained_on_padded_batches_through_one_recording behind an
    egc_amd.Embedding, trained for six steps twice from one start state: once with col.next() recorded inside the step
    (one replay = the whole iteration), once with the batch written into static buffers by torch operators.  Identical
    buffers feed a bit-reproducible step: all parameters and BatchNorm buffers are equal bit for bit."""
    import egc_amd
    from egc_amd import workloads as wl
    from egc_amd.fusion import FusedEGCBlock
    dev = _dev()
    hidden, n_types, g, m = 64, 28, 32, 200
    atom, ei, n_all, batch = wl.zinc_like_batch(m, seed=1)
    node_counts = torch.bincount(batch, minlength=m)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), node_counts.cumsum(0)])
    edge_counts = torch.bincount(batch[ei[0]], minlength=m)           # a graph's edges are contiguous, in graph order
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), edge_counts.cumsum(0)])
    assert bool((batch[ei[0]][1:] >= batch[ei[0]][:-1]).all())
    ei_local = ei - node_ptr[batch[ei[0]]]
    y = torch.randn(m, 1, generator=torch.Generator().manual_seed(2))
    store = egc_amd.GraphStore(node_ptr.to(dev), edge_ptr.to(dev), ei_local.to(dev), {"atom": atom.to(dev)}, {"y": y.to(dev)})
    col = egc_amd.BatchCollator(store, g)
    n_pad, e_pad, g_pad = col.n_pad, col.e_pad, g + 1
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(4))[:6 * g + 5]

    torch.manual_seed(0)
    emb = egc_amd.Embedding(n_types, hidden)
    blocks = nn.ModuleList([FusedEGCBlock(egc_amd.EGConv(hidden, hidden, aggrs=["sum", "max", "symnorm"], num_heads=4, num_bases=4),
                                          nn.BatchNorm1d(hidden)) for _ in range(2)])
    net_a = nn.ModuleList([emb, blocks, nn.Linear(hidden, 1)]).to(dev).train()
    net_b = copy.deepcopy(net_a)
    start = copy.deepcopy(net_a.state_dict())

    def make_step(net, opt, atom_, ei_, batch_, target, gmask, inv_g, n_valid, before=None):
        def step():
            if before is not None:
                before()
            h = net[0](atom_)
            for b in net[1]:
                h = b(h, ei_, n_valid=n_valid)
            out = net[2](egc_amd.global_mean_pool(h, batch_, size=g_pad))
            (((out - target) ** 2 * gmask).sum() * inv_g).backward()     # mean over the real graphs
            opt.step()
            opt.zero_grad(set_to_none=False)
        return step

    def record(net, step):
        params = list(net.parameters())
        graphed = egc_amd.GraphedStep(step, params=params, warmup=2)
        net.load_state_dict(start)                              # (the warm-up runs were real steps)
        for p in params:
            p.grad.zero_()
        return graphed

    # A: the collator's buffers, next() inside the recording
    opt_a = torch.optim.SGD(list(net_a.parameters()), lr=0.05, foreach=True)
    graphed_a = record(net_a, make_step(net_a, opt_a, col.fields["atom"], col.edge_index, col.batch, col.fields["y"],
                                        col.graph_mask, col.inv_g, col.n_valid, before=col.next))
    # B: static buffers written by torch, the load() of the test named above
    s_atom = torch.zeros(n_pad, dtype=torch.int64, device=dev)
    s_ei = torch.full((2, e_pad), n_pad - 1, dtype=torch.int64, device=dev)
    s_batch = torch.full((n_pad,), g_pad - 1, dtype=torch.int64, device=dev)
    s_target = torch.zeros(g_pad, 1, device=dev)
    s_gmask = torch.zeros(g_pad, 1, device=dev)
    s_inv_g = torch.ones((), device=dev)
    s_nvalid = torch.zeros((), dtype=torch.int64, device=dev)

    def load(ids):
        rows = torch.cat([torch.arange(int(node_ptr[i]), int(node_ptr[i + 1])) for i in ids.tolist()])
        offs = torch.cumsum(node_counts[ids], 0) - node_counts[ids]
        cols = [ei_local[:, int(edge_ptr[i]):int(edge_ptr[i + 1])] + int(o) for i, o in zip(ids.tolist(), offs.tolist())]
        b_atom, b_ei, n, k = atom[rows].to(dev), torch.cat(cols, dim=1).to(dev), rows.numel(), ids.numel()
        b_batch = torch.repeat_interleave(torch.arange(k), node_counts[ids]).to(dev)
        s_atom.zero_(); s_atom[:n] = b_atom
        s_ei.fill_(n_pad - 1); s_ei[:, :b_ei.size(1)] = b_ei
        s_batch.fill_(g_pad - 1); s_batch[:n] = b_batch
        s_target.zero_(); s_target[:k] = y[ids].to(dev)
        s_gmask.zero_(); s_gmask[:k] = 1.0
        s_inv_g.fill_(1.0 / k)
        s_nvalid.fill_(n)

    load(perm[:g])
    opt_b = torch.optim.SGD(list(net_b.parameters()), lr=0.05, foreach=True)
    graphed_b = record(net_b, make_step(net_b, opt_b, s_atom, s_ei, s_batch, s_target, s_gmask, s_inv_g, s_nvalid))

    col.set_epoch(perm.to(dev))                                 # (the warm-up ran next() too: start the epoch here)
    for i in range(6):
        graphed_a()
        load(perm[i * g:(i + 1) * g])
        graphed_b()
        for a, b in ((col.fields["atom"], s_atom), (col.edge_index, s_ei), (col.batch, s_batch), (col.n_valid, s_nvalid),
                     (col.fields["y"], s_target), (col.graph_mask, s_gmask), (col.inv_g, s_inv_g)):
            assert torch.equal(a, b), i                         # identical inputs ...
    torch.cuda.synchronize()
    col.check()
    moved = False
    for (name, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), name                          # ... identical nets
        moved = moved or not torch.equal(a, start[name].to(a.device))
    assert moved
