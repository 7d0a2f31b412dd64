#!/usr/bin/env python3
"""Time of the typed mean aggregation (egc_typed_mean_f32) and of egc_amd.RGCNConv on the ogbn-mag-shaped typed graph
(workloads.rmag_like at full size: 1.94 M nodes, seven relations) at F_in = 64 and 128, each against the torch composition of
the same thing, run alternately in the same process:

  typed-mean forward, per target type     one launch over [identity | every relation into the type] -> A_t
      against, per relation,              index_select + index_add_ into zeros + a divide   (no copy of x_t, no concatenation)
  typed-mean backward, per source type    one launch over [identity | transposed CSR of every relation out of the type] -> d x_s
      against, per relation,              a divide + index_select + index_add_ into one d x_s (what autograd derives)
  RGCNConv forward and forward + backward against a module of the same Linears over that composition, through autograd

Per record: microseconds (HIP events, median of the repetitions) of two series of each side, taken in the order
torch 1, new 1, torch 2, new 2 inside every repetition: |series 1 - series 2| is the spread this run shows between two
runs of the same thing.  For the kernels also the algorithmic bytes (every gathered row, index and offset read once, the
output written once) and their share of 8 TB/s.  Nothing here is a target; the figures are reported as measured."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402
from egc_amd._typed import TypedRel, typed_mean  # noqa: E402
from egc_amd.relational import EDGE_TYPES, NODE_TYPES  # noqa: E402

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


def compare(what, width, new, ref, iters, reps, nbytes=None):
    for fn in (ref, new):
        fn()
    torch.cuda.synchronize()
    t1, n1, t2, n2 = series([ref, new, ref, new], iters, reps)
    spread = max(abs(t1 - t2), abs(n1 - n2))
    rec = dict(what=what, width=width, new_us=[round(n1, 1), round(n2, 1)], torch_us=[round(t1, 1), round(t2, 1)],
               spread_us=round(spread, 1), faster_beyond_spread=bool(max(n1, n2) + spread < min(t1, t2)),
               speedup=round((t1 + t2) / (n1 + n2), 2))
    if nbytes is not None:
        rec.update(bytes=int(nbytes), share_of_8TBps=round(nbytes / (0.5 * (n1 + n2) * 1e-6) / PEAK, 4))
    print(json.dumps(rec), flush=True)
    return rec


class TorchRGCN(torch.nn.Module):
    """The composition per relation: index_select + index_add_ + a divide, then Linear (parameters shared with `conv`)."""

    def __init__(self, conv, edges, deg):
        super().__init__()
        self.conv, self.edges, self.deg = conv, edges, deg

    def forward(self, x_dict):
        out = {t: self.conv.root_lins[t](x) for t, x in x_dict.items()}
        for k, (src, dst) in self.edges.items():
            s = torch.zeros((x_dict[k[2]].size(0), x_dict[k[0]].size(1)), device=src.device).index_add_(0, dst, x_dict[k[0]].index_select(0, src))
            out[k[2]] = out[k[2]] + self.conv.rel_lins[f"{k[0]}_{k[1]}_{k[2]}"](s / self.deg[k][:, None])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out-channels", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rgcn_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    nodes, rel = wl.rmag_like(seed=0, scale=args.scale)
    keys = [k for k in EDGE_TYPES if k in rel]
    edges = {k: (rel[k][0].to(dev), rel[k][1].to(dev)) for k in keys}
    adj = {k: egc_amd.SparseTensor(row=edges[k][1], col=edges[k][0], sparse_sizes=(nodes[k[2]], nodes[k[0]])) for k in keys}
    deg = {k: torch.bincount(edges[k][1], minlength=nodes[k[2]]).clamp_(min=1).float() for k in keys}
    for k in keys:
        d = torch.bincount(edges[k][1], minlength=nodes[k[2]])
        print(json.dumps(dict(relation="_".join(k), edges=int(edges[k][0].numel()), rows=nodes[k[2]], longest_row=int(d.max()),
                              rows_over_chunk=int((d > 256).sum()))), flush=True)
    records = []
    for width in args.widths:
        x = {t: torch.randn(nodes[t], width, device=dev) for t in NODE_TYPES}
        into = {t: [k for k in keys if k[2] == t] for t in NODE_TYPES}
        out_of = {t: [k for k in keys if k[0] == t] for t in NODE_TYPES}
        ops = {t: torch.empty(nodes[t], (1 + len(into[t])) * width, device=dev) for t in NODE_TYPES}
        for t in NODE_TYPES:               # forward, per target type
            rels = [TypedRel(None, x[t])] + [TypedRel(adj[k].graph, x[k[0]], post_mean=True, out_col=(1 + j) * width)
                                            for j, k in enumerate(into[t])]

            def new(t=t, rels=rels):
                typed_mean(rels, nodes[t], width, ops[t])

            def ref(t=t):
                for k in into[t]:
                    s = torch.zeros(nodes[t], width, device=dev).index_add_(0, edges[k][1], x[k[0]].index_select(0, edges[k][0]))
                    s.div_(deg[k][:, None])
            e = sum(edges[k][0].numel() for k in into[t])
            nbytes = e * (4 * width + 4) + nodes[t] * (4 * width * (2 + len(into[t])) + 4 * len(into[t]))
            records.append(compare(f"typed-mean fwd into {t} ({len(into[t])} relations, {e} entries)", width, new, ref,
                                   args.iters, args.reps, nbytes))
        d_ops = {t: torch.randn_like(ops[t]) for t in NODE_TYPES}
        d_x = {t: torch.empty(nodes[t], width, device=dev) for t in NODE_TYPES}
        for s in NODE_TYPES:               # backward, per source type
            rels = [TypedRel(None, d_ops[s])]
            for k in out_of[s]:
                j = into[k[2]].index(k)
                rels.append(TypedRel(adj[k].graph.transposed(), d_ops[k[2]], in_col=(1 + j) * width, pre_rowptr=adj[k].graph.rowptr))

            def new(s=s, rels=rels):
                typed_mean(rels, nodes[s], width, d_x[s], accumulate=True)

            def ref(s=s):
                g = d_ops[s][:, :width].clone()
                for k in out_of[s]:
                    j = into[k[2]].index(k)
                    d_mean = d_ops[k[2]][:, (1 + j) * width:(2 + j) * width] / deg[k][:, None]
                    g.index_add_(0, edges[k][0], d_mean.index_select(0, edges[k][1]))
            e = sum(edges[k][0].numel() for k in out_of[s])
            nbytes = e * (4 * width + 12) + nodes[s] * (8 * width + 4 * len(out_of[s]))
            records.append(compare(f"typed-mean bwd out of {s} ({len(out_of[s])} relations, {e} entries)", width, new, ref,
                                   args.iters, args.reps, nbytes))
        del ops, d_ops, d_x
        conv = egc_amd.RGCNConv(width, args.out_channels).to(dev)
        comp = TorchRGCN(conv, {k: edges[k] for k in keys}, deg)
        with torch.no_grad():
            a, b = conv(x, adj), comp(x)
            worst = max(float((a[t] - b[t]).abs().max()) for t in NODE_TYPES)
        print(json.dumps(dict(width=width, layer_vs_composition_max_abs=worst)), flush=True)

        def fwd_new():
            with torch.no_grad():
                conv(x, adj)

        def fwd_ref():
            with torch.no_grad():
                comp(x)
        records.append(compare(f"RGCNConv({width}, {args.out_channels}) forward", width, fwd_new, fwd_ref, args.iters, args.reps))
        xg = {t: v.clone().requires_grad_(True) for t, v in x.items()}

        def step(f):
            def run():
                conv.zero_grad(set_to_none=True)
                for v in xg.values():
                    v.grad = None
                out = f()
                sum(o.sum() for o in out.values()).backward()
            return run
        records.append(compare(f"RGCNConv({width}, {args.out_channels}) forward + backward", width, step(lambda: conv(xg, adj)),
                               step(lambda: comp(xg)), args.iters, args.reps))
        del conv, comp, xg, x
        torch.cuda.empty_cache()
    print(f"\n{'what':<72}{'width':>6}{'new us':>20}{'torch us':>22}{'x':>7}{'of 8 TB/s':>11}")
    for r in records:
        share = f"{100 * r['share_of_8TBps']:.1f}%" if "share_of_8TBps" in r else ""
        print(f"{r['what']:<72}{r['width']:>6}{str(r['new_us']):>20}{str(r['torch_us']):>22}{r['speedup']:>7.2f}{share:>11}")
    print("\nfaster than the torch composition by more than the spread, every record:",
          all(r["faster_beyond_spread"] for r in records))


if __name__ == "__main__":
    main()
