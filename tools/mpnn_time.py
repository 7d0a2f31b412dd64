#!/usr/bin/env python3
"""Time and peak memory of egc_amd.Mpnn against the literal torch composition of the reference's layer (index_select both ends,
concatenate, per-tower Linear, scatter_reduce, update, lin: experiments/layers.py:248-267 under PyG's propagate), run
alternately in the same process, on the shapes the reference's configs run the baseline at:

  the arxiv-shaped graph (workloads.arxiv_like)         d = 116
  a molhiv-shaped batch (workloads.molecule_batch)      d = 180
  a code-like batch (workloads.code_like_batch)         d = 292

each with aggr add and max: forward (no_grad) and forward + backward through autograd, by HIP events, and of each message kernel
alone with its algorithmic bytes (every gathered row, index and offset read once, every output written once) and their share
of 8 TB/s.  Per record: microseconds (median of the repetitions) of two series of each side, taken in the order torch 1, new 1,
torch 2, new 2 inside every repetition: |series 1 - series 2| is the spread this run shows between two runs of the same thing.
Peak memory: the rise of torch.cuda.max_memory_allocated over one training step, graph structures built before.  Nothing here
is a target; the figures are reported as measured."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402
from egc_amd._mpnn import mpnn_message, mpnn_message_arg, mpnn_message_backward  # noqa: E402

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


def kernel(what, fn, nbytes, iters, reps):
    fn()
    torch.cuda.synchronize()
    a, b = series([fn, fn], iters, reps)
    rec = dict(what=what, new_us=[round(a, 1), round(b, 1)], bytes=int(nbytes), bytes_per_s=round(nbytes / (0.5 * (a + b) * 1e-6)),
               share_of_8TBps=round(nbytes / (0.5 * (a + b) * 1e-6) / PEAK, 4))
    print(json.dumps(rec), flush=True)
    return rec


class TorchMpnn(torch.nn.Module):
    """The reference's layer spelled out in torch (parameters shared with `layer`)."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, ei):
        la = self.layer
        t, c, n = la.towers, la.in_dim // la.towers, x.size(0)
        src, dst = ei[0], ei[1]
        h = torch.cat([x.index_select(0, dst).view(-1, t, c), x.index_select(0, src).view(-1, t, c)], dim=-1)
        msg = torch.cat([lin(h[:, i]) for i, lin in enumerate(la.message_layer)], dim=-1)
        red = {"add": "sum", "mean": "mean", "max": "amax"}[la.aggr]
        m = torch.zeros((n, msg.size(1)), device=x.device).scatter_reduce(0, dst.view(-1, 1).expand_as(msg), msg, red,
                                                                        include_self=False)
        h = torch.cat([m.view(-1, t, c), x.view(-1, t, c)], dim=-1)
        return la.lin(torch.cat([lin(h[:, i]) for i, lin in enumerate(la.update_layer)], dim=-1))


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
    ap.add_argument("--only", nargs="*", default=None, help="shape names to run (arxiv molhiv code)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mpnn_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    shapes = [("arxiv", lambda: wl.arxiv_like(seed=0)[:2], 116, 4), ("molhiv", lambda: wl.molecule_batch(seed=0)[:2], 180, 4),
              ("code", lambda: wl.code_like_batch(seed=0)[:2], 292, 4)]
    records = []
    for name, make, d, towers in shapes:
        if args.only and name not in args.only:
            continue
        ei, n = make()
        ei = ei.to(dev)
        e = int(ei.size(1))
        graph = egc_amd.CSRGraph.from_edge_index(ei, n)
        graph.transposed()
        deg = torch.bincount(ei[1], minlength=n)
        print(json.dumps(dict(shape=name, nodes=n, edges=e, d=d, longest_row=int(deg.max()), rows_over_chunk=int((deg > 256).sum()))),
              flush=True)
        x = torch.randn(n, d, device=dev)
        for aggr in ("add", "max"):
            torch.manual_seed(0)
            layer = egc_amd.Mpnn(aggr, d, d, towers=towers).to(dev)
            comp = TorchMpnn(layer)
            tag = f"{name} d={d} {aggr}"
            with torch.no_grad():
                a, b = layer(x, graph), comp(x, ei)
                print(json.dumps(dict(what=f"{tag}: layer against the composition, max abs / max |out|",
                                      value=float((a - b).abs().max() / b.abs().max()))), flush=True)
                pq = torch.randn(n, 2 * d, device=dev)
                P, Q, dm = pq[:, :d], pq[:, d:], torch.randn(n, d, device=dev)
                op = torch.empty(n, 2 * d, device=dev)
                arg = mpnn_message_arg(P, Q, graph)[1] if aggr == "max" else None
                fwd_bytes = e * (4 * d + 4) + n * (12 * d + 4)
                records.append(kernel(f"{tag}: message kernel forward", lambda: mpnn_message(P, Q, graph, aggr, out=op), fwd_bytes,
                                      args.iters, args.reps))
                if aggr == "max":
                    records.append(kernel(f"{tag}: message kernel forward with arg", lambda: mpnn_message_arg(P, Q, graph),
                                          fwd_bytes + 4 * n * d, args.iters, args.reps))
                bwd_bytes = e * (4 * d + 4 + ((4 * d + 8) if aggr == "max" else 0)) + n * (12 * d + 8)
                records.append(kernel(f"{tag}: message kernel backward", lambda: mpnn_message_backward(dm, graph, aggr, arg),
                                      bwd_bytes, args.iters, args.reps))
                del pq, P, Q, dm, op, arg

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
            rec.update(new_peak_bytes=peak_of(step(layer, graph)), torch_peak_bytes=peak_of(step(comp, ei)),
                       one_message_tensor_bytes=4 * e * d)
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del layer, comp, xg
            torch.cuda.empty_cache()
        del x, graph
        torch.cuda.empty_cache()
    print(f"\n{'what':<52}{'new us':>20}{'torch us':>22}{'x':>7}{'of 8 TB/s':>11}{'peak MB new / torch':>24}")
    for r in records:
        share = f"{100 * r['share_of_8TBps']:.1f}%" if "share_of_8TBps" in r else ""
        peak = f"{r['new_peak_bytes'] / 1e6:.0f} / {r['torch_peak_bytes'] / 1e6:.0f}" if "new_peak_bytes" in r else ""
        print(f"{r['what']:<52}{str(r['new_us']):>20}{str(r.get('torch_us', '')):>22}{str(r.get('speedup', '')):>7}{share:>11}{peak:>24}")


if __name__ == "__main__":
    main()
