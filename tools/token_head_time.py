#!/usr/bin/env python3
"""Time of the ogbg-code token head (egc_token_head.hip) against the reference's torch composition on the same device, at
the reference's training shape: G = 128 pooled rows, in_features 300 and 304, V = 5002 classes, T = 5 positions.

A = egc_amd.token_head_loss / token_head_argmax; B = `sum(F.cross_entropy(F.linear(x, W_i, b_i), y[:, i])) / T` (and
`argmax(F.linear(..), 1)` per position) with autograd's backward.  Two measurements per shape: loss forward + backward (the
gradients of x and of every weight and bias) and prediction only.  B is timed as two series B1 / B2 around A in every
repetition of one process: |B1 - B2| is the spread this run shows between two runs of the same code, and A beats B where it
lies below both.  HIP events, `iters` calls per window, the median of `reps` windows; the parameters rotate over enough
copies (9 x 30.4 MB) to exceed the 256 MiB Infinity Cache.  A's algorithmic bytes: forward reads W once; backward reads W
once, writes d W once and writes and reads the dx partials.  Raw records go to --out (profiles/token_head_time.json)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import _C  # noqa: E402

PEAK = 8e12
SHAPES = ((128, 300, 5002, 5), (128, 304, 5002, 5))


def series(fns, iters, reps):
    """Interleaved timing: per repetition every fn in turn, `iters` calls between two events.  Microseconds per call of
    every window, and their median."""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(i)
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) / iters * 1e3)
    return ts, [sorted(t)[len(t) // 2] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "token_head_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("token_head_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    records = []
    for g, k, v, t in SHAPES:
        torch.manual_seed(0)
        w_bytes = t * v * k * 4
        copies = -(-280 * 2 ** 20 // w_bytes)
        heads = [egc_amd.TokenHead(k, v, t).to(dev) for _ in range(copies)]
        params = [([p.weight for p in h], [p.bias for p in h]) for h in heads]
        x = torch.randn(g, k, device=dev).requires_grad_(True)
        y = torch.randint(0, v, (g, t), device=dev)
        workspace = int(_C.load().egc_token_head_workspace_bytes(g, k, v, t))

        def a_loss(i):
            ws, bs = params[i % copies]
            torch.autograd.grad(egc_amd.token_head_loss(x, ws, bs, y), [x] + ws + bs)

        def b_loss(i):
            ws, bs = params[i % copies]
            loss = sum(F.cross_entropy(F.linear(x, w, b), y[:, j]) for j, (w, b) in enumerate(zip(ws, bs))) / t
            torch.autograd.grad(loss, [x] + ws + bs)

        def a_pred(i):
            egc_amd.token_head_argmax(x.detach(), *params[i % copies])

        def b_pred(i):
            with torch.no_grad():
                ws, bs = params[i % copies]
                torch.stack([torch.argmax(F.linear(x, w, b), dim=1) for w, b in zip(ws, bs)], dim=1)

        for what, a, b, by in (("loss forward + backward", a_loss, b_loss, 3 * w_bytes + 2 * workspace),
                               ("prediction only", a_pred, b_pred, w_bytes)):
            fns = [b, a, b]                       # the order inside a repetition: B1, A, B2
            for fn in fns:
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            windows, (b1, med_a, b2) = series(fns, args.iters, args.reps)
            rec = dict(rows=g, in_features=k, classes=v, positions=t, measurement=what, copies=copies, iters=args.iters,
                       reps=args.reps, A_us=round(med_a, 2), B1_us=round(b1, 2), B2_us=round(b2, 2), A_bytes=by,
                       A_share_of_8TBps=round(by / (med_a * 1e-6) / PEAK, 4), A_beats_both=bool(med_a < min(b1, b2)),
                       speedup=round(min(b1, b2) / med_a, 2),
                       windows_us=dict(B1=[round(u, 2) for u in windows[0]], A=[round(u, 2) for u in windows[1]],
                                       B2=[round(u, 2) for u in windows[2]]))
            records.append(rec)
            print(json.dumps({key: val for key, val in rec.items() if key != "windows_us"}), flush=True)
        del heads, params
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), records=records), f, indent=1)
    print(f"\n{'K':<6}{'measurement':<28}{'A us':>10}{'B1 us':>10}{'B2 us':>10}{'A MB':>9}{'of 8 TB/s':>11}")
    for r in records:
        print(f"{r['in_features']:<6}{r['measurement']:<28}{r['A_us']:>10.2f}{r['B1_us']:>10.2f}{r['B2_us']:>10.2f}"
              f"{r['A_bytes'] / 1e6:>9.1f}{100 * r['A_share_of_8TBps']:>10.1f}%")


if __name__ == "__main__":
    main()
