#!/usr/bin/env python3
"""Time of the output head and loss (egc_softmax.hip) against the reference's torch composition, at the shapes of the
reference's classification nets: ogbn-mag (N = 736,389 rows of 349 classes in a 352-wide row, about 630 k training rows),
ogbn-arxiv (N = 169,343, 40 classes, 90,941 training rows) and a CIFAR batch (128 x 10, every row).

A = egc_amd.log_softmax / nll_log_softmax; B = `x[:, :C].log_softmax(-1)` (+ `.argmax(-1)`), `[idx]`, `F.nll_loss(.., y[idx])`
and autograd's backward through them.  Two measurements per shape: forward only (no_grad log-softmax + arg-max, the
reference's test()) and loss forward + backward (the gradient with respect to the full-width logits).  B is timed as two
series B1 / B2 around A in every repetition of one process: |B1 - B2| is the spread this run shows between two runs of the
same code, and A beats B where it lies below both.  HIP events, `iters` calls per window, the median of `reps` windows; the
inputs rotate over enough copies to exceed the 256 MiB Infinity Cache.  A's algorithmic bytes: forward only reads the class
columns and writes the log-probabilities and the arg-max; the loss reads the selected rows once per pass and writes the
gradient once.  Raw records go to --out (profiles/softmax_time.json)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402

PEAK = 8e12
SHAPES = (("mag", 736_389, 352, 349, 629_571), ("arxiv", 169_343, 40, 40, 90_941), ("cifar b128", 128, 10, 10, None))


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
    ap.add_argument("--only", default="", help="shape name prefix")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "softmax_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmax_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    records = []
    for name, n, ld, c, m in SHAPES:
        if not name.startswith(args.only):
            continue
        torch.manual_seed(0)
        copies = max(1, min(64, -(-600 * 2 ** 20 // (n * ld * 4))))
        xs = [torch.randn(n, ld, device=dev).requires_grad_(True) for _ in range(copies)]
        y = torch.randint(0, c, (n,), device=dev)
        idx = torch.randperm(n, device=dev)[:m] if m is not None else None
        sel = egc_amd.RowSelection(idx, n) if idx is not None else None
        sel_rows = m if m is not None else n

        def a_fwd(i):
            with torch.no_grad():
                egc_amd.log_softmax(xs[i % copies], num_classes=c, return_argmax=True)

        def b_fwd(i):
            with torch.no_grad():
                xs[i % copies][:, :c].log_softmax(-1).argmax(-1)

        def a_loss(i):
            x = xs[i % copies]
            torch.autograd.grad(egc_amd.nll_log_softmax(x, y, sel, num_classes=c), x)

        def b_loss(i):
            x = xs[i % copies]
            out = x[:, :c].log_softmax(-1)
            loss = F.nll_loss(out[idx], y[idx]) if idx is not None else F.nll_loss(out, y)
            torch.autograd.grad(loss, x)

        for what, a, b, by in (("forward only (log-softmax + arg-max)", a_fwd, b_fwd, n * c * 4 * 2 + n * 4),
                               ("loss forward + backward", a_loss, b_loss, 2 * sel_rows * c * 4 + n * ld * 4)):
            fns = [b, a, b]                       # the order inside a repetition: B1, A, B2
            for fn in fns:
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            windows, (b1, med_a, b2) = series(fns, args.iters, args.reps)
            rec = dict(shape=name, rows=n, ld=ld, classes=c, selected=sel_rows, measurement=what, copies=copies,
                       iters=args.iters, reps=args.reps, A_us=round(med_a, 2), B1_us=round(b1, 2), B2_us=round(b2, 2),
                       A_bytes=by, A_share_of_8TBps=round(by / (med_a * 1e-6) / PEAK, 4),
                       A_beats_both=bool(med_a < min(b1, b2)), speedup=round(min(b1, b2) / med_a, 2),
                       windows_us=dict(B1=[round(t, 2) for t in windows[0]], A=[round(t, 2) for t in windows[1]],
                                       B2=[round(t, 2) for t in windows[2]]))
            records.append(rec)
            print(json.dumps({k: v for k, v in rec.items() if k != "windows_us"}), flush=True)
        del xs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), records=records), f, indent=1)
    print(f"\n{'shape':<12}{'measurement':<40}{'A us':>10}{'B1 us':>10}{'B2 us':>10}{'A MB':>9}{'of 8 TB/s':>11}")
    for r in records:
        print(f"{r['shape']:<12}{r['measurement']:<40}{r['A_us']:>10.2f}{r['B1_us']:>10.2f}{r['B2_us']:>10.2f}"
              f"{r['A_bytes'] / 1e6:>9.1f}{100 * r['A_share_of_8TBps']:>10.1f}%")


if __name__ == "__main__":
    main()
