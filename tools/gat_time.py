#!/usr/bin/env python3
"""Time and peak memory of egc_amd.GATv2Conv against the plain per-edge torch composition of the same formulas (index_select both
ends, leaky_relu, per-head dot, scatter softmax, index_add: what tests/golden/make_golden_gat.py runs on the CPU), run
alternately in the same process, on the shapes the reference trains GATv2 at:

  the arxiv-shaped graph (workloads.arxiv_like)             H C = 112: H = 8, C = 14 and (the last layer) H = 1, C = 112
  a ZINC batch of 128 graphs (workloads.zinc_like_batch)    H C = 104: H = 8, C = 13

Per shape: the forward launch and the backward launches alone, by HIP events, with a byte model of their compulsory traffic
(every gathered row, index and offset read once, every output written once) and its share of 8 TB/s; then GATv2Conv forward
(no_grad) and forward + backward through autograd against the composition.  Per record: microseconds (median of the
repetitions) of two series of each side, taken in the order torch 1, new 1, torch 2, new 2 inside every repetition:
|series 1 - series 2| is the spread this run shows between two runs of the same thing.  Peak memory: the rise of
torch.cuda.max_memory_allocated over one training step, graph structures built before.  Nothing here is a target; the figures are
reported as measured.

``--layer gat`` times egc_amd.GATConv (GAT v1, egc_gat.hip) the same way instead, on the shapes the reference trains it at:

  the arxiv-shaped graph                                    H C = 152: H = 8, C = 19 and (the last layer) H = 1, C = 152
  a molhiv-shaped batch (workloads.molecule_batch)          H C = 240: H = 8, C = 30

and, in the same run, GATv2's forward and backward launches at the same width and graph: that kernel is the yardstick.  Byte
model of the v1 launches (d = H C, E' = entries with the self loops, N = nodes; what the kernels touch, each once):
  forward                        E' (4 d + 4 H + 4) + N (4 d + 8 H + 4)     xl_j, a_src[j], index | a_dst, out, lse, offset
  backward, destination pass     E' (4 d + 4 H + 4) + N (8 d + 16 H + 4)    the same | g, out, a_dst, lse, D, d a_dst, offset
  backward, source pass          E' (4 d + 12 H + 4) + N (8 d + 8 H + 4)    g_i, a_dst[i], lse_i, D_i, index | xl, d xl, a_src,
                                                                            d a_src, offset

``--dropout P`` (with either ``--layer``) times attention dropout in training instead, on the same shapes: the DROP launches
(forward; backward) against the same run's p = 0 launches on the same operands, in the order p = 0, P, p = 0, P inside every
repetition; then the layer's training forward (no_grad) and forward + backward against the per-edge composition with F.dropout
on alpha, with peak memory.  The byte model of the DROP launches is that of the plain ones plus 4 E' in the source pass (the
forward position of every transposed entry); the mask itself costs integer work, no bytes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402
from egc_amd._gat import gatv2_aggregate_backward, gatv2_aggregate_lse  # noqa: E402

PEAK = 8e12


def series(fns, iters, reps):
    """Interleaved timing: per repetition every fn in turn, `iters` calls between two events.  Median microseconds per call."""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) / iters * 1e3)
    return [sorted(t)[len(t) // 2] for t in ts]


def compare(what, new, ref, iters, reps):
    for fn in (ref, new):
        fn()
    torch.cuda.synchronize()
    t1, n1, t2, n2 = series([ref, new, ref, new], iters, reps)
    spread = max(abs(t1 - t2), abs(n1 - n2))
    rec = dict(what=what, new_us=[round(n1, 1), round(n2, 1)], torch_us=[round(t1, 1), round(t2, 1)], spread_us=round(spread, 1),
               speedup=round((t1 + t2) / (n1 + n2), 2))
    print(json.dumps(rec), flush=True)
    return rec


def versus(what, new, base, iters, reps):
    """`new` against `base` (the p = 0 launches), two series of each."""
    for fn in (base, new):
        fn()
    torch.cuda.synchronize()
    b1, n1, b2, n2 = series([base, new, base, new], iters, reps)
    rec = dict(what=what, new_us=[round(n1, 1), round(n2, 1)], p0_us=[round(b1, 1), round(b2, 1)],
               spread_us=round(max(abs(b1 - b2), abs(n1 - n2)), 1), ratio_to_p0=round((n1 + n2) / (b1 + b2), 3))
    print(json.dumps(rec), flush=True)
    return rec


def kernel(what, fn, nbytes, iters, reps):
    fn()
    torch.cuda.synchronize()
    a, b = series([fn, fn], iters, reps)
    rec = dict(what=what, new_us=[round(a, 1), round(b, 1)], bytes=int(nbytes), floor_us=round(nbytes / PEAK * 1e6, 1),
               share_of_8TBps=round(nbytes / (0.5 * (a + b) * 1e-6) / PEAK, 4))
    print(json.dumps(rec), flush=True)
    return rec


class TorchGATv2(torch.nn.Module):
    """The per-edge composition (parameters shared with `layer`)."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, ei):
        la = self.layer
        h, c, n = la.heads, la.out_channels, x.size(0)
        xl, xr = la.lin_l(x), la.lin_r(x)
        src, dst = ei[0], ei[1]
        if la.add_self_loops:
            keep = src != dst
            loops = torch.arange(n, device=x.device)
            src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
        xj = xl.index_select(0, src).view(-1, h, c)
        z = xj + xr.index_select(0, dst).view(-1, h, c)
        s = (torch.nn.functional.leaky_relu(z, la.negative_slope) * la.att).sum(dim=-1)
        idx = dst.view(-1, 1).expand_as(s)
        top = torch.full((n, h), -float("inf"), device=x.device).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
        ex = torch.exp(s - top.index_select(0, dst))
        den = torch.zeros((n, h), device=x.device).index_add(0, dst, ex)
        alpha = torch.nn.functional.dropout(ex / den.index_select(0, dst), la.dropout, la.training)
        out = torch.zeros((n, h, c), device=x.device).index_add(0, dst, alpha.unsqueeze(-1) * xj)
        out = out.reshape(n, h * c) if la.concat else out.mean(dim=1)
        return out + la.bias


class TorchGAT(torch.nn.Module):
    """The per-edge composition of GAT v1 (parameters shared with `layer`)."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, ei):
        la = self.layer
        h, c, n = la.heads, la.out_channels, x.size(0)
        xl = la.lin_src(x).view(n, h, c)
        a_src, a_dst = (xl * la.att_src).sum(dim=-1), (xl * la.att_dst).sum(dim=-1)
        src, dst = ei[0], ei[1]
        if la.add_self_loops:
            keep = src != dst
            loops = torch.arange(n, device=x.device)
            src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
        s = torch.nn.functional.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, dst), la.negative_slope)
        idx = dst.view(-1, 1).expand_as(s)
        top = torch.full((n, h), -float("inf"), device=x.device).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
        ex = torch.exp(s - top.index_select(0, dst))
        den = torch.zeros((n, h), device=x.device).index_add(0, dst, ex)
        alpha = torch.nn.functional.dropout(ex / den.index_select(0, dst), la.dropout, la.training)
        out = torch.zeros((n, h, c), device=x.device).index_add(0, dst, alpha.unsqueeze(-1) * xl.index_select(0, src))
        out = out.reshape(n, h * c) if la.concat else out.mean(dim=1)
        return out + la.bias


def main_gat(args, dev):
    """--layer gat: GATConv's launches and layer, and GATv2's launches at the same width and graph (module docstring)."""
    from egc_amd._gat import gat_aggregate_backward, gat_aggregate_lse
    shapes = [("arxiv_h8", lambda: wl.arxiv_like(seed=0), 8, 19), ("arxiv_h1", lambda: wl.arxiv_like(seed=0), 1, 152),
              ("molhiv_h8", lambda: wl.molecule_batch(seed=0)[:2], 8, 30)]
    records = []
    for name, make, h, c in shapes:
        if args.only and name not in args.only:
            continue
        ei, n = make()
        ei = ei.to(dev)
        e, d = int(ei.size(1)), h * c
        graph = egc_amd.CSRGraph.from_edge_index(ei, n)
        graph.transposed()
        deg = torch.bincount(ei[1], minlength=n)
        e_eff = int((ei[0] != ei[1]).sum()) + n
        print(json.dumps(dict(shape=name, layer="gat", nodes=n, edges=e, entries_with_self_loops=e_eff, heads=h, channels=c,
                              longest_row=int(deg.max()), rows_over_chunk=int((deg > 256).sum()))), flush=True)
        torch.manual_seed(0)
        layer = egc_amd.GATConv(d, c, heads=h).to(dev)
        comp = TorchGAT(layer)
        x = torch.randn(n, d, device=dev)
        tag = f"{name} H={h} C={c}"
        with torch.no_grad():
            a, b = layer(x, graph), comp(x, ei)
            print(json.dumps(dict(what=f"{tag}: layer against the composition, max abs / max |out|",
                                  value=float((a - b).abs().max() / b.abs().max()))), flush=True)
            ext = 0.3 * torch.randn(n, (d + 2 * h + 3) // 4 * 4, device=dev)
            xl, a_src, a_dst, gout = ext[:, :d], ext[:, d:d + h], ext[:, d + h:d + 2 * h], torch.randn(n, d, device=dev)
            out, lse = gat_aggregate_lse(xl, a_src, a_dst, graph)
            fwd_bytes = e_eff * (4 * d + 4 * h + 4) + n * (4 * d + 8 * h + 4)
            dst_bytes = e_eff * (4 * d + 4 * h + 4) + n * (8 * d + 16 * h + 4)
            src_bytes = e_eff * (4 * d + 12 * h + 4) + n * (8 * d + 8 * h + 4)
            records.append(kernel(f"{tag}: GAT forward launch", lambda: gat_aggregate_lse(xl, a_src, a_dst, graph), fwd_bytes,
                                  args.iters, args.reps))
            records.append(kernel(f"{tag}: GAT backward launches", lambda: gat_aggregate_backward(xl, a_src, a_dst, graph, out, lse, gout),
                                  dst_bytes + src_bytes, args.iters, args.reps))
            # the yardstick: GATv2's launches at the same width and graph, with their own byte model (main)
            lr = 0.3 * torch.randn(n, 2 * d, device=dev)
            xl2, xr2, att2 = lr[:, :d], lr[:, d:], 0.3 * torch.randn(h, c, device=dev)
            out2, lse2 = gatv2_aggregate_lse(xl2, xr2, att2, graph)
            v2_fwd = e_eff * (4 * d + 4) + n * (8 * d + 4 * h + 4)
            v2_bwd = e_eff * (4 * d + 4) + n * (16 * d + 8 * h + 4) + e_eff * (8 * d + 8 * h + 4) + n * (8 * d + 4)
            records.append(kernel(f"{tag}: GATv2 forward launch", lambda: gatv2_aggregate_lse(xl2, xr2, att2, graph), v2_fwd,
                                  args.iters, args.reps))
            records.append(kernel(f"{tag}: GATv2 backward launches",
                                  lambda: gatv2_aggregate_backward(xl2, xr2, att2, graph, out2, lse2, gout), v2_bwd, args.iters, args.reps))
            del ext, xl, a_src, a_dst, gout, out, lse, lr, xl2, xr2, out2, lse2

        def fwd(f, g):
            def run():
                with torch.no_grad():
                    f(x, g)
            return run
        records.append(compare(f"{tag}: GATConv forward", fwd(layer, graph), fwd(comp, ei), args.iters, args.reps))
        xg = x.clone().requires_grad_(True)

        def step(f, g):
            def run():
                layer.zero_grad(set_to_none=True)
                xg.grad = None
                f(xg, g).sum().backward()
            return run
        rec = compare(f"{tag}: GATConv forward + backward", step(layer, graph), step(comp, ei), args.iters, args.reps)
        rec.update(new_peak_bytes=peak_of(step(layer, graph)), torch_peak_bytes=peak_of(step(comp, ei)), one_edge_array_bytes=4 * e_eff * d)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del layer, comp, xg, x, graph
        torch.cuda.empty_cache()
    return records


def main_dropout(args, dev):
    """--dropout P: the DROP launches against the p = 0 launches, and the training layer against the composition with F.dropout
    on alpha (module docstring)."""
    from egc_amd._gat import gat_aggregate_backward, gat_aggregate_lse
    v1 = args.layer == "gat"
    if v1:
        shapes = [("arxiv_h8", lambda: wl.arxiv_like(seed=0)[:2], 8, 19), ("arxiv_h1", lambda: wl.arxiv_like(seed=0)[:2], 1, 152),
                  ("molhiv_h8", lambda: wl.molecule_batch(seed=0)[:2], 8, 30)]
    else:
        shapes = [("arxiv_h8", lambda: wl.arxiv_like(seed=0)[:2], 8, 14), ("arxiv_h1", lambda: wl.arxiv_like(seed=0)[:2], 1, 112),
                  ("zinc_h8", lambda: wl.zinc_like_batch(seed=0)[1:3], 8, 13)]
    p, records = args.dropout, []
    for name, make, h, c in shapes:
        if args.only and name not in args.only:
            continue
        ei, n = make()
        ei = ei.to(dev)
        e, d = int(ei.size(1)), h * c
        graph = egc_amd.CSRGraph.from_edge_index(ei, n)
        graph.transposed()
        e_eff = int((ei[0] != ei[1]).sum()) + n
        print(json.dumps(dict(shape=name, layer=args.layer, dropout=p, nodes=n, edges=e, entries_with_self_loops=e_eff, heads=h,
                              channels=c)), flush=True)
        torch.manual_seed(0)
        layer = (egc_amd.GATConv if v1 else egc_amd.GATv2Conv)(d, c, heads=h, dropout=p).to(dev)
        comp = (TorchGAT if v1 else TorchGATv2)(layer)
        x = torch.randn(n, d, device=dev)
        seed = torch.empty(1, dtype=torch.int64, device=dev).random_()
        kw = dict(dropout=p, seed=seed)
        tag = f"{name} H={h} C={c} p={p}"
        with torch.no_grad():
            gout = torch.randn(n, d, device=dev)
            if v1:
                ext = 0.3 * torch.randn(n, (d + 2 * h + 3) // 4 * 4, device=dev)
                ops = (ext[:, :d], ext[:, d:d + h], ext[:, d + h:d + 2 * h])
                fwd_fn, bwd_fn = gat_aggregate_lse, gat_aggregate_backward
            else:
                lr = 0.3 * torch.randn(n, 2 * d, device=dev)
                ops = (lr[:, :d], lr[:, d:], layer.att.detach()[0].contiguous())
                fwd_fn, bwd_fn = gatv2_aggregate_lse, gatv2_aggregate_backward
            out0, lse0 = fwd_fn(*ops, graph)
            out1, lse1 = fwd_fn(*ops, graph, **kw)
            print(json.dumps(dict(what=f"{tag}: lse of the DROP forward is the plain forward's, bit for bit",
                                  value=bool(torch.equal(lse0, lse1)))), flush=True)
            records.append(versus(f"{tag}: forward launch", lambda: fwd_fn(*ops, graph, **kw), lambda: fwd_fn(*ops, graph),
                                  args.iters, args.reps))
            records.append(versus(f"{tag}: backward launches", lambda: bwd_fn(*ops, graph, out1, lse1, gout, **kw),
                                  lambda: bwd_fn(*ops, graph, out0, lse0, gout), args.iters, args.reps))
            del ops, gout, out0, lse0, out1, lse1

        def fwd(f, g):
            def run():
                with torch.no_grad():
                    f(x, g)
            return run
        layer.train()
        records.append(compare(f"{tag}: training forward", fwd(layer, graph), fwd(comp, ei), args.iters, args.reps))
        xg = x.clone().requires_grad_(True)

        def step(f, g):
            def run():
                layer.zero_grad(set_to_none=True)
                xg.grad = None
                f(xg, g).sum().backward()
            return run
        rec = compare(f"{tag}: training forward + backward", step(layer, graph), step(comp, ei), args.iters, args.reps)
        rec.update(new_peak_bytes=peak_of(step(layer, graph)), torch_peak_bytes=peak_of(step(comp, ei)), one_edge_array_bytes=4 * e_eff * d)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del layer, comp, xg, x, graph
        torch.cuda.empty_cache()
    return records


def table(records):
    print(f"\n{'what':<58}{'new us':>20}{'torch | p = 0 us':>22}{'x':>7}{'floor us':>10}{'of 8 TB/s':>11}{'peak MB new / torch':>24}")
    for r in records:
        share = f"{100 * r['share_of_8TBps']:.1f}%" if "share_of_8TBps" in r else ""
        peak = f"{r['new_peak_bytes'] / 1e6:.0f} / {r['torch_peak_bytes'] / 1e6:.0f}" if "new_peak_bytes" in r else ""
        print(f"{r['what']:<58}{str(r['new_us']):>20}{str(r.get('torch_us', r.get('p0_us', ''))):>22}{str(r.get('speedup', r.get('ratio_to_p0', ''))):>7}"
              f"{str(r.get('floor_us', '')):>10}{share:>11}{peak:>24}")


def peak_of(step):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None, help="shape names to run (arxiv_h8 arxiv_h1 zinc_h8; molhiv_h8 with --layer gat)")
    ap.add_argument("--layer", choices=("gatv2", "gat"), default="gatv2", help="gatv2: GATv2Conv (the default); gat: GATConv, with "
                    "GATv2's launches at the same width and graph next to it")
    ap.add_argument("--dropout", type=float, default=0.0, help="P in (0, 1): time attention dropout in training instead (the DROP "
                    "launches against the p = 0 launches, the training layer against the composition with F.dropout on alpha)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gat_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    if args.dropout != 0.0:
        if not 0.0 < args.dropout < 1.0:
            sys.exit("--dropout wants P in (0, 1)")
        table(main_dropout(args, dev))
        return
    if args.layer == "gat":
        table(main_gat(args, dev))
        return
    shapes = [("arxiv_h8", lambda: wl.arxiv_like(seed=0)[:2], 8, 14), ("arxiv_h1", lambda: wl.arxiv_like(seed=0)[:2], 1, 112),
              ("zinc_h8", lambda: wl.zinc_like_batch(seed=0)[1:3], 8, 13)]
    records = []
    for name, make, h, c in shapes:
        if args.only and name not in args.only:
            continue
        ei, n = make()
        ei = ei.to(dev)
        e, d = int(ei.size(1)), h * c
        graph = egc_amd.CSRGraph.from_edge_index(ei, n)
        graph.transposed()
        deg = torch.bincount(ei[1], minlength=n)
        e_eff = int((ei[0] != ei[1]).sum()) + n
        print(json.dumps(dict(shape=name, nodes=n, edges=e, entries_with_self_loops=e_eff, heads=h, channels=c,
                              longest_row=int(deg.max()), rows_over_chunk=int((deg > 256).sum()))), flush=True)
        torch.manual_seed(0)
        layer = egc_amd.GATv2Conv(d, c, heads=h).to(dev)
        comp = TorchGATv2(layer)
        x = torch.randn(n, d, device=dev)
        tag = f"{name} H={h} C={c}"
        with torch.no_grad():
            a, b = layer(x, graph), comp(x, ei)
            print(json.dumps(dict(what=f"{tag}: layer against the composition, max abs / max |out|",
                                  value=float((a - b).abs().max() / b.abs().max()))), flush=True)
            lr = 0.3 * torch.randn(n, 2 * d, device=dev)
            xl, xr, att, gout = lr[:, :d], lr[:, d:], layer.att.detach()[0].contiguous(), torch.randn(n, d, device=dev)
            out, lse = gatv2_aggregate_lse(xl, xr, att, graph)
            # forward: a row of xl and an index per entry; xr, out, lse, offsets per node
            fwd_bytes = e_eff * (4 * d + 4) + n * (8 * d + 4 * h + 4)
            records.append(kernel(f"{tag}: forward launch", lambda: gatv2_aggregate_lse(xl, xr, att, graph), fwd_bytes, args.iters, args.reps))
            # backward: destination pass (xl row + index per entry; xr, g, out, lse read, d xr and D written per node) and source
            # pass (xr and g rows, lse, D, index per entry; xl read and d xl written per node)
            bwd_bytes = e_eff * (4 * d + 4) + n * (16 * d + 8 * h + 4) + e_eff * (8 * d + 8 * h + 4) + n * (8 * d + 4)
            records.append(kernel(f"{tag}: backward launches", lambda: gatv2_aggregate_backward(xl, xr, att, graph, out, lse, gout),
                                  bwd_bytes, args.iters, args.reps))
            del lr, xl, xr, gout, out, lse

        def fwd(f, g):
            def run():
                with torch.no_grad():
                    f(x, g)
            return run
        records.append(compare(f"{tag}: GATv2Conv forward", fwd(layer, graph), fwd(comp, ei), args.iters, args.reps))
        xg = x.clone().requires_grad_(True)

        def step(f, g):
            def run():
                layer.zero_grad(set_to_none=True)
                xg.grad = None
                f(xg, g).sum().backward()
            return run
        rec = compare(f"{tag}: GATv2Conv forward + backward", step(layer, graph), step(comp, ei), args.iters, args.reps)
        rec.update(new_peak_bytes=peak_of(step(layer, graph)), torch_peak_bytes=peak_of(step(comp, ei)), one_edge_array_bytes=4 * e_eff * d)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del layer, comp, xg, x, graph
        torch.cuda.empty_cache()
    table(records)


if __name__ == "__main__":
    main()
