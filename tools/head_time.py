#!/usr/bin/env python3
"""Time of the graph-level MLP head (egc_head.hip) against the reference's torch composition on the same device, forward +
backward (the gradients of x and of every parameter), at the heads of the reference's batched nets:

    ZINC    128 rows,  h in {128, 168}, out 1,  F.l1_loss
    molhiv  2048 rows, h in {224, 296}, out 1,  BCE-with-logits over the labelled entries (30 % NaN targets)
    CIFAR   64 rows,   h = 168,         out 10, F.cross_entropy (A: egc_amd.cross_entropy on the head's output)

A = egc_amd.GraphHead with its fused loss; B = tests/callers.head_mlp with torch's loss and autograd.  Both run in one process,
eager (host-bound: what a loop without hipGraph sees) and as ONE captured graph each (what GraphedStep replays; torch's masked
BCE is captured as the equal weighted sum, its own selection cannot be).  B is timed as two series B1 / B2 around A in every repetition: |B1 - B2| is the spread this run shows between two runs of the same code,
and A beats B where it lies below both.  HIP events, `iters` calls per window, the median of `reps` windows, three warm-up
calls first.  The launch counts are egc_head_launches' for A.  Raw records go to --out (profiles/head_time.json)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import egc_amd  # noqa: E402
from egc_amd import _C  # noqa: E402
import callers  # noqa: E402

SHAPES = (("zinc", 128, 128, 1, "l1"), ("zinc", 128, 168, 1, "l1"), ("molhiv", 2048, 224, 1, "bce"),
          ("molhiv", 2048, 296, 1, "bce"), ("cifar", 64, 168, 10, "ce"))


def series(fns, iters, reps):
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
    return ts, [sorted(t)[len(t) // 2] for t in ts]


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nets", default="zinc,molhiv,cifar", help="which of the nets' shapes to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib = _C.load()
    records = []
    for net, g, h, out, loss in SHAPES:
        if net not in args.nets.split(","):
            continue
        torch.manual_seed(0)
        sizes = [h, h // 2, h // 4, out]
        ours = egc_amd.GraphHead(sizes).to(dev)
        theirs = callers.head_mlp(sizes).to(dev)
        theirs.load_state_dict(ours.state_dict(), strict=True)
        x = torch.randn(g, h, device=dev).requires_grad_(True)
        if loss == "ce":
            y = torch.randint(0, out, (g,), device=dev)
        else:
            y = torch.randn(g, out, device=dev) if loss == "l1" else torch.randint(0, 2, (g, out), device=dev).float()
            if loss == "bce":
                y[torch.rand(g, out, device=dev) < 0.3] = float("nan")

        def a_step():
            if loss == "l1":
                val = ours.l1_loss(x, y)
            elif loss == "bce":
                val = ours.bce_with_logits_loss(x, y)
            else:
                val = egc_amd.cross_entropy(ours(x), y)
            return torch.autograd.grad(val, [x] + list(ours.parameters()))

        def b_step(capturable=False):
            o = theirs(x)
            if loss == "l1":
                val = F.l1_loss(o, y.view_as(o))
            elif loss == "bce" and capturable:
                # (the reference's o[ok] has a data-dependent shape and cannot be captured: the same mean as a weighted sum)
                ok = y == y
                val = F.binary_cross_entropy_with_logits(o, torch.where(ok, y, torch.zeros_like(y)), weight=ok.float(),
                                                         reduction="sum") / ok.sum()
            elif loss == "bce":
                ok = y == y
                val = F.binary_cross_entropy_with_logits(o[ok], y[ok])
            else:
                val = F.cross_entropy(o, y)
            return torch.autograd.grad(val, [x] + list(theirs.parameters()))

        for fn in (b_step, a_step, b_step):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        n0 = lib.egc_head_launches()
        a_step()
        a_launches = lib.egc_head_launches() - n0
        eager_w, eager = series([b_step, a_step, b_step], args.iters, args.reps)
        rec = dict(net=net, rows=g, hidden=h, out=out, loss=loss, iters=args.iters, reps=args.reps, A_head_launches=a_launches,
                   eager=dict(B1_us=round(eager[0], 2), A_us=round(eager[1], 2), B2_us=round(eager[2], 2)))
        try:
            ga, gb = graphed(a_step), graphed(lambda: b_step(capturable=True))
            graph_w, gr = series([gb.replay, ga.replay, gb.replay], args.iters, args.reps)
            rec["graph"] = dict(B1_us=round(gr[0], 2), A_us=round(gr[1], 2), B2_us=round(gr[2], 2),
                                A_not_slower=bool(gr[1] <= max(gr[0], gr[2])), A_beats_both=bool(gr[1] < min(gr[0], gr[2])),
                                speedup=round(min(gr[0], gr[2]) / gr[1], 2),
                                windows_us=dict(B1=[round(u, 2) for u in graph_w[0]], A=[round(u, 2) for u in graph_w[1]],
                                                B2=[round(u, 2) for u in graph_w[2]]))
        except RuntimeError as exc:
            rec["graph"] = dict(error=str(exc).splitlines()[0][:200])
            torch.cuda.synchronize()
        records.append(rec)
        print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "windows_us"} if isinstance(v, dict) else v)
                          for k, v in rec.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), records=records), f, indent=1)


if __name__ == "__main__":
    main()
