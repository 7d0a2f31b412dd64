#!/usr/bin/env python3
"""Time of the device-side collation (egc_collate under egc_amd.BatchCollator) against the torch composition that does the
same job from the same device-resident store, on the batch shapes of the reference's nets:

  zinc b128     128 ZINC-like molecules      node field atom int64 [N],                    graph field y float32 [M, 1]
  molhiv b2048  2,048 molhiv-like molecules  node field x int64 [N, 9],                    graph field y float32 [M, 1] (NaN fill)
  cifar b64     64 superpixel k-NN graphs    node fields x float32 [N, 3], pos float32 [N, 2],  graph field y int64 [M]

(a) ``col.collate(ids)``: two launches that write EVERY buffer of the padded batch, ptr / edge_ptr included.
(b) torch operators: one index_select per field for the selected graphs' rows, one for their edge columns plus the offset
    add, repeat_interleave for the batch vector, then the ``load()`` of tests/test_hipgraph_gpu.py (zero_ / fill_ / slice
    copies) into static padded buffers.  The row and column index lists of the batch and its sizes are built BEFORE the
    timed region -- (b) is charged for the device work alone, not for the host's per-graph bookkeeping, and does not
    write ptr / edge_ptr: the baseline is the generous one.
Both are timed eager (host launch cost included) and as a replay of their capture into a hipGraph.

HIP events, warmed up, median of the repetitions; the contenders alternate repetition by repetition in ONE process, in
the order B1, A, B2: B is timed as two series and |B1 - B2| is the spread this run shows for identical work.  A passes a
shape when it is not slower than the mean of B1 and B2 by more than that spread.

--step: the ZINC b128 training iteration (Embedding -> 4 x FusedEGCBlock -> mean pool -> Linear -> loss -> SGD) as ONE
recording with ``col.next()`` inside, against the same recording without it fed by (b) before every replay -- both go
through the same epoch of eight batches in the same order (the step's own time depends on how much of the padded shape a
batch fills); ``step_alone`` is the second recording replayed on whatever batch was loaded last.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402


def series(fns, reps, min_window_us=2000.0):
    """Interleaved timing: per repetition every fn in turn, a fixed number of calls between two events -- per fn as many
    as make the window at least `min_window_us` long (from a first window of 20 calls).  Median microseconds per call."""
    def window(fn, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e3
    iters = [max(20, int(min_window_us / max(window(fn, 20), 1e-3)) + 1) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(window(fn, iters[k]))
    return [sorted(t)[len(t) // 2] for t in ts]


def build_store(kind, n_graphs, seed, dev):
    """(GraphStore, graph_fill) of `n_graphs` graphs of a workload: the batch generators' graphs, ids made local."""
    g = torch.Generator().manual_seed(seed + 17)
    if kind == "zinc":
        atom, ei, n, batch = wl.zinc_like_batch(n_graphs, seed=seed)
        node_fields, y, fill = {"atom": atom}, torch.randn(n_graphs, 1, generator=g), {}
    elif kind == "molhiv":
        ei, n, batch = wl.molecule_batch(n_graphs, seed=seed)
        node_fields = {"x": torch.randint(0, 100, (n, 9), generator=g)}
        y, fill = torch.randint(0, 2, (n_graphs, 1), generator=g).float(), {"y": float("nan")}
    else:
        ei, n, batch = wl.knn_superpixel_batch(n_graphs, seed=seed)
        node_fields = {"x": torch.rand(n, 3, generator=g), "pos": torch.rand(n, 2, generator=g)}
        y, fill = torch.randint(0, 10, (n_graphs,), generator=g), {}
    counts = torch.bincount(batch, minlength=n_graphs)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    owner = batch[ei[1]]
    assert bool((owner[1:] >= owner[:-1]).all()), "a graph's edges must be contiguous"
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(owner, minlength=n_graphs).cumsum(0)])
    store = egc_amd.GraphStore(node_ptr.to(dev), edge_ptr.to(dev), (ei - node_ptr[owner]).to(dev),
                               {k: v.to(dev) for k, v in node_fields.items()}, {"y": y.to(dev)})
    return store, fill


class TorchCollate:
    """(b): the torch composition into static padded buffers of the collator's shapes, for ONE batch whose index lists are
    built here, outside the timed call."""

    def __init__(self, store, col, ids, fill, share=None):
        dev, g = store.device, col.batch_size
        self.store, self.ids, self.k, self.g = store, ids, ids.numel(), g
        self.n_pad, self.e_pad = col.n_pad, col.e_pad
        node_ptr, edge_ptr, ids_h = store.node_ptr.cpu(), store.edge_ptr.cpu(), ids.cpu()
        self.node_cnt_all = store.node_ptr[1:] - store.node_ptr[:-1]
        cnt = (node_ptr[1:] - node_ptr[:-1])[ids_h]
        offs = cnt.cumsum(0) - cnt
        self.rows = torch.cat([torch.arange(int(node_ptr[i]), int(node_ptr[i + 1])) for i in ids_h.tolist()]).to(dev)
        self.cols = torch.cat([torch.arange(int(edge_ptr[i]), int(edge_ptr[i + 1])) for i in ids_h.tolist()]).to(dev)
        self.edge_off = torch.repeat_interleave(offs, (edge_ptr[1:] - edge_ptr[:-1])[ids_h]).to(dev)
        self.n, self.e = self.rows.numel(), self.cols.numel()
        self.slots = torch.arange(self.k, device=dev)
        self.fill = fill.get("y", 0)
        if share is not None:                               # another batch into the SAME static buffers
            for k in ("fields", "edge_index", "batch", "counts", "graph_mask", "inv_g", "n_valid"):
                setattr(self, k, getattr(share, k))
            return
        self.fields = {name: torch.zeros_like(t) for name, t in col.fields.items()}
        self.edge_index, self.batch = torch.zeros_like(col.edge_index), torch.zeros_like(col.batch)
        self.counts, self.graph_mask = torch.zeros_like(col.counts), torch.zeros_like(col.graph_mask)
        self.inv_g, self.n_valid = torch.zeros_like(col.inv_g), torch.zeros_like(col.n_valid)

    def __call__(self):
        st, n, e, k = self.store, self.n, self.e, self.k
        for name, src in st.node_fields.items():
            dst = self.fields[name]
            dst.zero_(); dst[:n] = src.index_select(0, self.rows)
        self.edge_index.fill_(self.n_pad - 1)
        self.edge_index[:, :e] = st.edge_index.index_select(1, self.cols) + self.edge_off
        cnt = self.node_cnt_all.index_select(0, self.ids)
        self.batch.fill_(self.g); self.batch[:n] = torch.repeat_interleave(self.slots, cnt, output_size=n)
        self.counts.fill_(1.0); self.counts[:k, 0] = cnt.float()
        y = self.fields["y"]
        y.fill_(self.fill); y[:k] = st.graph_fields["y"].index_select(0, self.ids)
        self.graph_mask.zero_(); self.graph_mask[:k] = 1.0
        self.inv_g.fill_(1.0 / k)
        self.n_valid.fill_(n)

    def equals(self, col):
        pairs = [(self.fields[k], col.fields[k]) for k in self.fields] + [
            (self.edge_index, col.edge_index), (self.batch, col.batch), (self.counts, col.counts),
            (self.graph_mask, col.graph_mask), (self.inv_g, col.inv_g), (self.n_valid, col.n_valid)]
        return all(torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8)) for a, b in pairs)


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def collate_shapes(args, dev):
    records = []
    for name, kind, g in (("zinc b128", "zinc", 128), ("molhiv b2048", "molhiv", 2048), ("cifar b64", "cifar", 64)):
        if not name.startswith(args.only):
            continue
        m = 2 * g                                           # the batch is a random half of the store: scattered source graphs
        store, fill = build_store(kind, m, 0, dev)
        col = egc_amd.BatchCollator(store, g, graph_fill=fill)
        ids = torch.randperm(m, generator=torch.Generator().manual_seed(1))[:g].to(dev)
        b = TorchCollate(store, col, ids, fill)
        col.collate(ids).check()
        b()
        assert b.equals(col), "the torch composition and the collator disagree"
        moved = sum(t.numel() * t.element_size() for t in list(col.fields.values()) + [col.edge_index, col.batch])
        for mode, fa, fb in (("eager", lambda: col.collate(ids), b), ("captured", captured(lambda: col.collate(ids)), captured(b))):
            for fn in (fa, fb):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            b1, us_a, b2 = series([fb, fa, fb], args.reps)
            spread = abs(b1 - b2)
            rec = dict(workload=name, graphs=g, n_pad=col.n_pad, e_pad=col.e_pad, mode=mode, written_bytes=moved,
                       a_us=round(us_a, 2), b_us=[round(b1, 2), round(b2, 2)], spread_us=round(spread, 2),
                       b_over_a=round((b1 + b2) / 2 / us_a, 2), not_slower=bool(us_a <= (b1 + b2) / 2 + spread))
            records.append(rec)
            print(json.dumps(rec), flush=True)
        col.check()
    return records


def training_step(args, dev):
    """The ZINC b128 iteration as one recording: next() inside it, against the same net's recording fed by (b)."""
    g, m, hidden = 128, 1024, 128
    store, fill = build_store("zinc", m, 0, dev)
    col = egc_amd.BatchCollator(store, g)
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(1)).to(dev)
    col.set_epoch(perm)

    def net_and_step(atom, ei, batch, target, gmask, inv_g, n_valid, before=None):
        torch.manual_seed(0)
        blocks = nn.ModuleList([egc_amd.FusedEGCBlock(egc_amd.EGConv(hidden, hidden, aggrs=["sum", "mean", "max", "symnorm"],
                                                                     num_heads=8, num_bases=4), nn.BatchNorm1d(hidden))
                                for _ in range(4)])
        net = nn.ModuleList([egc_amd.Embedding(28, hidden), blocks, nn.Linear(hidden, 1)]).to(dev).train()
        params = list(net.parameters())
        opt = torch.optim.SGD(params, lr=0.01, foreach=True)

        def step():
            if before is not None:
                before()
            h = net[0](atom)
            for blk in net[1]:
                h = blk(h, ei, n_valid=n_valid)
            out = net[2](egc_amd.global_mean_pool(h, batch, size=g + 1))
            (((out - target) ** 2 * gmask).sum() * inv_g).backward()
            opt.step()
            opt.zero_grad(set_to_none=False)
        return egc_amd.GraphedStep(step, params=params)

    b = TorchCollate(store, col, perm[:g].contiguous(), fill)
    feeds = [b] + [TorchCollate(store, col, perm[i * g:(i + 1) * g].contiguous(), fill, share=b) for i in range(1, m // g)]
    graphed_a = net_and_step(col.fields["atom"], col.edge_index, col.batch, col.fields["y"], col.graph_mask, col.inv_g,
                             col.n_valid, before=col.next)
    b()
    graphed_b = net_and_step(b.fields["atom"], b.edge_index, b.batch, b.fields["y"], b.graph_mask, b.inv_g, b.n_valid)

    turn = [0]

    def iter_b():                                           # the same batches in the same order as next() takes them
        feeds[turn[0] % len(feeds)]()
        turn[0] += 1
        graphed_b()

    if args.profile:                                        # no timing: replays for rocprofv3 --kernel-trace
        torch.cuda.synchronize()
        for _ in range(20):
            (graphed_a if args.profile == "next" else iter_b)()
        torch.cuda.synchronize()
        print(json.dumps(dict(profile=args.profile, replays=20)), flush=True)
        return None

    def wall(fn, it=200):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(it):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / it * 1e6

    # every contender twice, alternating: the two figures of one contender show the spread of identical work
    b1, a1, only1, b2, a2, only2 = (wall(fn) for fn in (iter_b, graphed_a, graphed_b) * 2)
    col.check()
    rec = dict(workload="zinc b128 4-block training iteration, one recording", width=hidden,
               next_inside_us=[round(a1, 1), round(a2, 1)], fed_by_torch_us=[round(b1, 1), round(b2, 1)],
               step_alone_us=[round(only1, 1), round(only2, 1)])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="", help="workload name prefix")
    ap.add_argument("--step", action="store_true", help="also the ZINC b128 training iteration with next() in the recording")
    ap.add_argument("--profile", default="", choices=("", "next", "torch"),
                    help="no timing: twenty replays of the training iteration (next() inside | fed by torch) for rocprofv3")
    ap.add_argument("--json", default=None, help="write every record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("collate_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    if args.profile:
        training_step(args, dev)
        return
    records = collate_shapes(args, dev)
    step = training_step(args, dev) if args.step else None
    print(f"\n{'workload':<14}{'mode':<10}{'A us':>9}{'B1 us':>9}{'B2 us':>9}{'spread':>8}{'B / A':>8}{'MB':>8}  verdict")
    for r in records:
        print(f"{r['workload']:<14}{r['mode']:<10}{r['a_us']:>9.2f}{r['b_us'][0]:>9.2f}{r['b_us'][1]:>9.2f}{r['spread_us']:>8.2f}"
              f"{r['b_over_a']:>8.2f}{r['written_bytes'] / 1e6:>8.2f}  {'ok' if r['not_slower'] else 'SLOWER'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(collate=records, training_step=step), f, indent=1)


if __name__ == "__main__":
    main()
