#!/usr/bin/env python3
"""Time of egc_amd.GCNConv, SAGEConv and GINConv against the plain torch composition of each layer (index_select of the source
rows, index_add_ into the destinations, the normalisation / division / self term as elementwise operations, the same Linears),
run alternately in the same process, at the widths the reference's configs run these baselines at:

  the arxiv-shaped graph (workloads.arxiv_like)         GCN 156, SAGE 115, GIN 156
  a code-like batch (workloads.code_like_batch)         GCN 304, SAGE 293, GIN 304

forward (no_grad) and forward + backward through autograd, by HIP events, and of the neighbour-sum kernel alone in the forms the
layers launch, with its algorithmic bytes (every gathered row, index, per-entry factor and offset read once, the self row read once,
every output written once) and their share of 8 TB/s.  Per record: microseconds (median of the repetitions) of two series of
each side, taken in the order torch 1, new 1, torch 2, new 2 inside every repetition: |series 1 - series 2| is the spread this
run shows between two runs of the same thing.  Nothing here is a target; the figures are reported as measured."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402

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
               torch_over_new=round((t1 + t2) / (n1 + n2), 2))
    print(json.dumps(rec), flush=True)
    return rec


def kernel(what, fn, nbytes, iters, reps):
    fn()
    torch.cuda.synchronize()
    a, b = series([fn, fn], iters, reps)
    rec = dict(what=what, new_us=[round(a, 1), round(b, 1)], bytes=int(nbytes), bytes_per_s=round(nbytes / (0.5 * (a + b) * 1e-6)),
               share_of_8TBps=round(nbytes / (0.5 * (a + b) * 1e-6) / PEAK, 4))
    print(json.dumps(rec), flush=True)
    return rec


def scatter_sum(v, dst, n):
    return torch.zeros((n, v.size(1)), dtype=v.dtype, device=v.device).index_add_(0, dst, v)


class TorchGCN(torch.nn.Module):
    """GCNConv(normalize=True, add_self_loops=True) spelled out in torch (parameters shared with `layer`); the looped edge list
    and its weights are built once, as a cached PyG layer keeps them."""

    def __init__(self, layer, ei, n):
        super().__init__()
        self.layer = layer
        keep = ei[0] != ei[1]
        loops = torch.arange(n, device=ei.device)
        self.src, self.dst = torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])
        deg = torch.zeros(n, device=ei.device).index_add_(0, self.dst, torch.ones(self.dst.numel(), device=ei.device))
        dis = deg.pow(-0.5)
        self.w = (dis[self.src] * dis[self.dst]).view(-1, 1)

    def forward(self, x, ei):
        h = self.layer.lin(x)
        return scatter_sum(self.w * h.index_select(0, self.src), self.dst, x.size(0)) + self.layer.bias


class TorchSAGE(torch.nn.Module):
    def __init__(self, layer, ei, n):
        super().__init__()
        self.layer = layer
        self.cnt = torch.bincount(ei[1], minlength=n).clamp(min=1).float().view(-1, 1)

    def forward(self, x, ei):
        agg = scatter_sum(x.index_select(0, ei[0]), ei[1], x.size(0)) / self.cnt
        return self.layer.lin_l(agg) + self.layer.lin_r(x)


class TorchGIN(torch.nn.Module):
    def __init__(self, layer, ei, n):
        super().__init__()
        self.layer = layer

    def forward(self, x, ei):
        return self.layer.nn((1 + self.layer.eps) * x + scatter_sum(x.index_select(0, ei[0]), ei[1], x.size(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None, help="shape names to run (arxiv code)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nbr_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    shapes = [("arxiv", lambda: wl.arxiv_like(seed=0)[:2], dict(gcn=156, sage=115, gin=156)),
              ("code", lambda: wl.code_like_batch(seed=0)[:2], dict(gcn=304, sage=293, gin=304))]
    records = []
    for name, make, widths in shapes:
        if args.only and name not in args.only:
            continue
        ei, n = make()
        ei = ei.to(dev)
        e = int(ei.size(1))
        graph = egc_amd.CSRGraph.from_edge_index(ei, n)
        graph.transposed()
        deg = torch.bincount(ei[1], minlength=n)
        print(json.dumps(dict(shape=name, nodes=n, edges=e, widths=widths, longest_row=int(deg.max()),
                              rows_over_chunk=int((deg > 256).sum()))), flush=True)
        for kind, d in widths.items():
            torch.manual_seed(0)
            if kind == "gcn":
                layer, comp_cls = egc_amd.GCNConv(d, d), TorchGCN
            elif kind == "sage":
                layer, comp_cls = egc_amd.SAGEConv(d, d), TorchSAGE
            else:
                layer, comp_cls = egc_amd.GINConv(torch.nn.Linear(d, d), train_eps=True), TorchGIN
            layer = layer.to(dev)
            comp = comp_cls(layer, ei, n)
            x = torch.randn(n, d, device=dev)
            tag = f"{name} {kind} d={d}"
            with torch.no_grad():
                a, b = layer(x, graph), comp(x, ei)
                print(json.dumps(dict(what=f"{tag}: layer against the composition, max abs / max |out|",
                                      value=float((a - b).abs().max() / b.abs().max()))), flush=True)
                out = torch.empty(n, d, device=dev)
                rows, idx = 4 * d * e, 4 * e + 4 * n         # the gathered rows; the column indices and the offsets
                if kind == "gcn":       # + the per-entry factor, the row factor, the self row, the output
                    fn = lambda: egc_amd.neighbor_sum(x, graph, "sym", x_self=x, skip_self_entries=True, scale=graph.dis_looped,  # noqa: E731
                                                      edge_scale=graph.edge_dis_looped, out=out)
                    nbytes = rows + idx + 4 * e + 4 * n + 8 * n * d
                elif kind == "sage":    # + the output
                    fn = lambda: egc_amd.neighbor_sum(x, graph, "mean", out=out)  # noqa: E731
                    nbytes = rows + idx + 4 * n * d
                else:                   # + the self row, the output
                    fn = lambda: egc_amd.neighbor_sum(x, graph, "sum", x_self=x, eps=layer.eps, out=out)  # noqa: E731
                    nbytes = rows + idx + 8 * n * d
                records.append(kernel(f"{tag}: neighbour-sum kernel", fn, nbytes, args.iters, args.reps))
                del out

            def fwd(f, g):
                def run():
                    with torch.no_grad():
                        f(x, g)
                return run
            records.append(compare(f"{tag}: forward", fwd(layer, graph), fwd(comp, ei), args.iters, args.reps))
            xg = x.clone().requires_grad_(True)

            def step(f, g):
                def run():
                    layer.zero_grad(set_to_none=True)
                    xg.grad = None
                    f(xg, g).sum().backward()
                return run
            records.append(compare(f"{tag}: forward + backward", step(layer, graph), step(comp, ei), args.iters, args.reps))
            del layer, comp, x, xg
            torch.cuda.empty_cache()
        del graph
        torch.cuda.empty_cache()
    print(f"\n{'what':<44}{'new us':>20}{'torch us':>22}{'torch / new':>13}{'of 8 TB/s':>11}")
    for r in records:
        share = f"{100 * r['share_of_8TBps']:.1f}%" if "share_of_8TBps" in r else ""
        print(f"{r['what']:<44}{str(r['new_us']):>20}{str(r.get('torch_us', '')):>22}{str(r.get('torch_over_new', '')):>13}{share:>11}")


if __name__ == "__main__":
    main()
