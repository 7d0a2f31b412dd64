#!/usr/bin/env python3
"""Time and peak memory of egc_amd.PNAConv against the literal per-edge torch composition of PyG's layer (index_select both ends,
concatenate, per-tower pre Linear, one scatter_reduce per aggregator -- one of them over the squares --, the degree scalers on
the [N, T, S A F] concatenation, per-tower post Linear, lin), run alternately in the same process, on the arxiv-shaped graph
(workloads.arxiv_like) at d = 128 with the reference's PNA configuration: aggregators mean / min / max / std, scalers identity /
amplification / attenuation, towers 4, divide_input.

Forward (no_grad) and forward + backward through autograd, by HIP events, and the aggregate launch alone (inference form,
training form, backward) with its algorithmic bytes and their share of 8 TB/s.  The forward's bytes: one gather of a P row and one
index per entry, Q in and A W out per row, the offsets.  Per record: microseconds (median of the repetitions) of two series of
each side, taken in the order torch 1, new 1, torch 2, new 2 inside every repetition: |series 1 - series 2| is the spread this run
shows between two runs of the same thing.  For scale the same P and Q go through egc_mpnn_message_f32 once per aggregator family
(mean, max, max again for min, mean again for std's second moment): what four single-aggregator passes cost.  Nothing here is a
target; the figures are reported as measured."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402
from egc_amd._mpnn import mpnn_message  # noqa: E402
from egc_amd._pna import pna_aggregate_saved  # noqa: E402
from mpnn_time import compare, kernel, peak_of  # noqa: E402

AGGREGATORS = ["mean", "min", "max", "std"]
SCALERS = ["identity", "amplification", "attenuation"]


class TorchPNA(torch.nn.Module):
    """PyG's layer spelled out in torch (parameters shared with `layer`)."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, ei):
        la = self.layer
        t, n = la.towers, x.size(0)
        src, dst = ei[0], ei[1]
        xi, xj = x.index_select(0, dst), x.index_select(0, src)
        if la.divide_input:
            xi, xj = xi.view(-1, t, la.F_in), xj.view(-1, t, la.F_in)
        else:
            xi, xj = xi.unsqueeze(1).expand(-1, t, -1), xj.unsqueeze(1).expand(-1, t, -1)
        h = torch.cat([xi, xj], dim=-1)
        msg = torch.stack([nn(h[:, i]) for i, nn in enumerate(la.pre_nns)], dim=1)                  # [E, T, F]
        idx = dst.view(-1, 1, 1).expand_as(msg)

        def red(v, how):
            return torch.zeros((n, t, la.F_in), device=x.device).scatter_reduce(0, idx, v, how, include_self=False)
        outs = []
        for a in la.aggregators:
            if a in ("sum", "mean"):
                outs.append(red(msg, a))
            elif a in ("min", "max"):
                outs.append(red(msg, "a" + a))
            else:
                mean = red(msg, "mean")
                var = torch.relu(red(msg * msg, "mean") - mean * mean)
                outs.append(var if a == "var" else torch.sqrt(var + 1e-5))
        out = torch.cat(outs, dim=-1)
        deg = torch.bincount(dst, minlength=n).clamp_(min=1).to(x.dtype).view(-1, 1, 1)
        lin, log = la.avg_deg["lin"], la.avg_deg["log"]
        fac = dict(identity=lambda: 1.0, amplification=lambda: torch.log(deg + 1) / log, attenuation=lambda: log / torch.log(deg + 1),
                   linear=lambda: deg / lin, inverse_linear=lambda: lin / deg)
        out = torch.cat([out * fac[s]() for s in la.scalers], dim=-1)
        xt = x.view(n, t, -1) if la.divide_input else x.unsqueeze(1).expand(-1, t, -1)
        out = torch.cat([xt, out], dim=-1)
        return la.lin(torch.cat([nn(out[:, i]) for i, nn in enumerate(la.post_nns)], dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--d", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pna_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    d, towers = args.d, 4
    ei, n = wl.arxiv_like(seed=0)[:2]
    ei = ei.to(dev)
    e = int(ei.size(1))
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    graph.transposed()
    indeg = torch.bincount(ei[1], minlength=n)
    print(json.dumps(dict(shape="arxiv", nodes=n, edges=e, d=d, longest_row=int(indeg.max()), rows_over_chunk=int((indeg > 256).sum()))),
          flush=True)
    torch.manual_seed(0)
    layer = egc_amd.PNAConv(d, d, AGGREGATORS, SCALERS, egc_amd.degree_histogram(graph), towers=towers, divide_input=True).to(dev)
    comp = TorchPNA(layer)
    x = torch.randn(n, d, device=dev)
    tag = f"arxiv d={d} PNA"
    records = []
    a = len(AGGREGATORS)
    with torch.no_grad():
        o1, o2 = layer(x, graph), comp(x, ei)
        print(json.dumps(dict(what=f"{tag}: layer against the composition, max abs / max |out|",
                              value=float((o1 - o2).abs().max() / o2.abs().max()))), flush=True)
        pq = torch.randn(n, 2 * d, device=dev)
        P, Q, dagg = pq[:, :d], pq[:, d:], torch.randn(n, a * d, device=dev)
        out = torch.empty(n, a * d, device=dev)
        fwd_bytes = e * (4 * d + 4) + n * (4 * d + 4 * a * d + 4)
        records.append(kernel(f"{tag}: aggregate forward (4 aggregators, one pass)",
                              lambda: egc_amd.pna_aggregate(P, Q, graph, AGGREGATORS, out=out), fwd_bytes, args.iters, args.reps))
        records.append(kernel(f"{tag}: aggregate forward, training form", lambda: pna_aggregate_saved(P, Q, graph, AGGREGATORS),
                              fwd_bytes + n * 16 * d, args.iters, args.reps))
        _, arg_min, arg_max, mu, var = pna_aggregate_saved(P, Q, graph, AGGREGATORS)
        # destination pass: d agg, mu, v in, d Q, a, b out; source pass per entry: a, b, two gradients, two args, three indices
        bwd_bytes = n * (4 * a * d + 8 * d + 12 * d + 4) + e * (24 * d + 12) + n * (8 * d + 4)
        records.append(kernel(f"{tag}: aggregate backward", lambda: egc_amd.pna_aggregate_backward(
            dagg, graph, AGGREGATORS, P=P, arg_min=arg_min, arg_max=arg_max, mu=mu, var=var), bwd_bytes, args.iters, args.reps))
        one = torch.empty(n, d, device=dev)

        def four_passes():
            for op in ("mean", "max", "max", "mean"):
                mpnn_message(P, Q, graph, op, out=one)
        records.append(kernel(f"{tag}: four egc_mpnn_message_f32 passes", four_passes, 4 * (e * (4 * d + 4) + n * (8 * d + 4)),
                              args.iters, args.reps))
        del pq, P, Q, dagg, out, arg_min, arg_max, mu, var, one

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
    rec = compare(f"{tag}: forward + backward", step(layer, graph), step(comp, ei), args.iters, args.reps)
    rec.update(new_peak_bytes=peak_of(step(layer, graph)), torch_peak_bytes=peak_of(step(comp, ei)), one_message_tensor_bytes=4 * e * d)
    print(json.dumps(rec), flush=True)
    records.append(rec)
    print(f"\n{'what':<62}{'new us':>20}{'torch us':>22}{'x':>7}{'of 8 TB/s':>11}{'peak MB new / torch':>24}")
    for r in records:
        share = f"{100 * r['share_of_8TBps']:.1f}%" if "share_of_8TBps" in r else ""
        peak = f"{r['new_peak_bytes'] / 1e6:.0f} / {r['torch_peak_bytes'] / 1e6:.0f}" if "new_peak_bytes" in r else ""
        print(f"{r['what']:<62}{str(r['new_us']):>20}{str(r.get('torch_us', '')):>22}{str(r.get('speedup', '')):>7}{share:>11}{peak:>24}")


if __name__ == "__main__":
    main()
