"""Float64 reference of the output head and loss (egc_amd/csrc/egc_softmax.hip): the four formulas of include/egc_hip.h in
plain torch on the CPU, and the float32 error bounds the GPU tests hold the kernels to.  Everything takes and returns
CPU tensors; float32 inputs are widened exactly."""
import math

import torch

U = 2.0 ** -24          # unit roundoff of float32
TINY = 2.0 ** -126      # smallest normal float32: a product or an exp below it may be flushed to zero or lose its last bits, an
                        # ABSOLUTE error of at most TINY that no relative bound covers (exp(-100) times a weight of 1e-3)


def log_softmax(x, n_classes):
    """(logp [N, C], lse [N]) of the first n_classes columns of x [N, ld]; the padding columns are not touched."""
    v = x[:, :n_classes].double()
    m = v.max(dim=1, keepdim=True).values if v.size(0) else v.new_zeros((0, 1))
    lse = (m + (v - m).exp().sum(dim=1, keepdim=True).log()).squeeze(1)
    return v - lse[:, None], lse


def first_argmax(x, n_classes):
    """The first maximal column of every row."""
    v = x[:, :n_classes]
    cols = torch.arange(n_classes).expand_as(v)
    return torch.where(v == v.max(dim=1, keepdim=True).values, cols, n_classes).min(dim=1).values


def log_softmax_backward(g, out, ld):
    """d x [N, ld] = g - exp(out) * sum_c g on the class columns, 0 in the padding; g, out [N, C]."""
    g, out = g.double(), out.double()
    dx = torch.zeros((g.size(0), ld), dtype=torch.float64)
    dx[:, :g.size(1)] = g - out.exp() * g.sum(dim=1, keepdim=True)
    return dx


def counts(index, n_rows):
    """cnt [n_rows] of an index vector (None: every row once); indices outside [0, n_rows) are not counted."""
    if index is None:
        return torch.ones(n_rows, dtype=torch.int64)
    index = index[(index >= 0) & (index < n_rows)]
    return torch.bincount(index, minlength=n_rows)


def nll_forward(x, y, cnt, n_classes, mean):
    """loss = -(1 / M) sum_r cnt[r] logp[r, y[r]] (or the sum); a label outside the classes contributes 0 (and still
    counts in M).  Also the per-row picked log-probabilities (0 where nothing is picked)."""
    logp, lse = log_softmax(x, n_classes)
    ok = (y >= 0) & (y < n_classes) & (cnt > 0)
    picked = torch.zeros(x.size(0), dtype=torch.float64)
    picked[ok] = logp[ok, y[ok]]
    total = -(cnt.double() * picked).sum()
    return (total / float(cnt.sum()) if mean else total), picked


def nll_backward(g, x, y, cnt, n_classes, mean):
    """d x [N, ld] = g cnt[r] / M (softmax - onehot) on selected rows with a valid label, 0 elsewhere and in the padding."""
    logp, _ = log_softmax(x, n_classes)
    ok = (y >= 0) & (y < n_classes) & (cnt > 0)
    w = float(g) * cnt.double() / (float(cnt.sum()) if mean else 1.0)
    d = logp.exp()
    d[ok, y[ok]] -= 1.0
    d = d * torch.where(ok, w, torch.zeros_like(w))[:, None]
    d[~ok] = 0.0            # (also clears NaN * 0 of rows that were never meant to be read)
    dx = torch.zeros(x.shape, dtype=torch.float64)
    dx[:, :n_classes] = d
    return dx


# ---------------------------------------------------------------------------------------------------------------------
# Bounds.  u = 2^-24, C = n_classes.  The kernel forms m = max (exact), s = sum_c exp(x_c - m), lse = m + log s,
# logp = x - lse, every operation float32 with one rounding, expf / logf within 3 ulp (the OpenCL full-profile limit).
# ---------------------------------------------------------------------------------------------------------------------
def lse_bound(lse, n_classes):
    """|lse_f32 - lse|.  x_c - m rounds with relative error u, which exp turns into a relative error u |x_c - m| of the
    term; weighted by the term's share of s that is the softmax-weighted mean of |x - m| <= ln C.  expf adds 3u per term,
    the sum gamma_{C-1} = (C - 1) u in any order (positive terms): s has relative error <= u (ln C + 3) + (C - 1) u, which
    log s inherits as an ABSOLUTE error; logf adds 3u |log s| <= 3u ln C, and m + log s rounds once: u |lse|."""
    ln_c = math.log(n_classes)
    return U * (lse.abs() + 4.0 * ln_c + 3.0) + (n_classes - 1) * U


def logp_bound(logp, lse, n_classes):
    """|logp_f32 - logp| <= u (|logp| + |lse| + 4 ln C + 3) + (C - 1) u: lse_bound plus the rounding of x - lse."""
    return U * logp.abs() + lse_bound(lse, n_classes)[:, None]


def loss_chain(n_rows, n_classes):
    """The longest chain of float32 adds behind the loss (include/egc_hip.h): 128 G / 256 rows in a lane group, 3 + 6 adds
    for the chunk, ceil(chunks / 256) chunk sums in a thread, 3 + 6 for the rest."""
    g = 1
    while g < (n_classes + 3) // 4 and g < 64:
        g *= 2
    chunks = (n_rows + 127) // 128
    return max(128 * g // 256, 1) + 9 + (chunks + 255) // 256 + 9


def loss_bound(picked, lse, cnt, n_rows, n_classes, mean):
    """|loss_f32 - loss|.  Every term cnt[r] (x[r, y] - lse[r]) carries logp's bound times cnt plus one rounding of the
    product; the sum adds gamma_k of sum |term| with k = loss_chain (NOT gamma_{M-1}: no term passes through more adds);
    the negated quotient by M rounds once more.  1.01 covers the second-order terms."""
    c = cnt.double()
    term = U * picked.abs() + lse_bound(lse, n_classes)
    k = loss_chain(n_rows, n_classes)
    m = float(cnt.sum()) if mean else 1.0
    loss = float((c * picked).sum()) / m if m else 0.0
    return 1.01 * (float((c * term).sum()) + (k + 1) * U * float((c * picked.abs()).sum())) / max(m, 1.0) + U * abs(loss)


def nll_grad_bound(dx_ref, x, y, cnt, g, n_classes, mean):
    """|dx_f32 - dx| per element.  p = exp(x - lse): the argument carries lse's error and its own rounding u |logp|, both
    become relative errors of p, expf adds 3u; p - [c == y] rounds once; w = (g cnt) / M rounds twice and the product
    once: |err| <= |w| (p (lse_bound + u |logp| + 3u) + 4u |p - onehot|), times 1.01 for the second-order terms, plus
    TINY (1 + |w|) for the subnormal range: either p itself (then scaled by w) or the product may be flushed."""
    logp, lse = log_softmax(x, n_classes)
    w = (abs(float(g)) * cnt.double() / (float(cnt.sum()) if mean else 1.0))[:, None]
    p = logp.exp()
    b = torch.zeros(x.shape, dtype=torch.float64)
    with torch.no_grad():
        wp = torch.where(w > 0, w * p * (lse_bound(lse, n_classes)[:, None] + U * logp.abs() + 3.0 * U), torch.zeros_like(p))
    b[:, :n_classes] = 1.01 * (wp + 4.0 * U * dx_ref[:, :n_classes].abs()) + TINY * (1.0 + w)
    return b


def log_softmax_grad_bound(g, out, n_classes):
    """|dx_f32 - dx| per class column for dx = g - exp(out) S, S = sum_c g (the float32 g and out are the inputs of both
    sides).  S: every term passes through at most C - 1 adds in any order, |dS| <= (C - 1) u sum |g|; expf 3u, the product
    and the difference one rounding each: |err| <= e (C - 1) u sum|g| + 4u |e S| + u |dx|, times 1.01, plus
    TINY (1 + |S|) for the subnormal range: either exp(out) itself (then scaled by S) or the product may be flushed."""
    g, e = g.double(), out.double().exp()
    s_abs = g.abs().sum(dim=1, keepdim=True)
    s = g.sum(dim=1, keepdim=True)
    dx = g - e * s
    return 1.01 * (e * (n_classes - 1) * U * s_abs + 4.0 * U * (e * s).abs() + U * dx.abs()) + TINY * (1.0 + s.abs())


# ---------------------------------------------------------------------------------------------------------------------
# Inputs, and the geometry table of tests/test_softmax_shapes_gpu.py (guarded without a GPU by test_softmax_shapes_cpu.py).
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ["randn1", "randn10", "randn50", "dominant", "equal"]


def logits(n, c, ld, kind, seed):
    """CPU float32 logits [n, ld]: the class columns by `kind` ("mixed": the five kinds row after row), NaN in the padding."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ld, generator=g)
    kinds = [kind] * n if kind != "mixed" else [KINDS[r % len(KINDS)] for r in range(n)]
    for k in set(kinds):
        rows = torch.tensor([r for r in range(n) if kinds[r] == k], dtype=torch.int64)
        if k.startswith("randn"):
            x[rows] *= float(k[5:])
        elif k == "dominant":
            x[rows, torch.randint(0, c, (rows.numel(),), generator=g)] += 100.0
        else:
            x[rows] = x[rows, :1].expand(-1, ld).clone()
    x[:, c:] = float("nan")
    return x


def ties_logits(n, c, ld, seed):
    """Integer-valued rows drawn from {0, 1, 2}: the maximum occurs several times in most rows.  NaN in the padding."""
    x = torch.randint(0, 3, (n, ld), generator=torch.Generator().manual_seed(seed)).float()
    x[:, c:] = float("nan")
    return x


def tied_share(x, n_classes):
    """The share of rows whose maximum occurs twice or more."""
    v = x[:, :n_classes]
    return float(((v == v.max(dim=1, keepdim=True).values).sum(dim=1) >= 2).float().mean())


def sample_index(n, share, seed):
    """A permutation sample of round(share n) of the n rows, unsorted."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:int(round(n * share))]


SM_CHUNK = 128          # rows of a workgroup (include/egc_hip.h)
SM_BLOCK = 256          # threads of a workgroup = chunk sums a finalize trip takes in
# The ten (lanes G = 2^gl, pieces K per lane) cells of the launcher as (first, last) class count: gl 0..5 with K = 1, then
# gl = 6 with K = 1..4.
CELLS = [(1, 4), (5, 8), (9, 16), (17, 32), (33, 64), (65, 128), (129, 256), (257, 512), (513, 768), (769, 1024)]


def roundup4(c):
    return (c + 3) // 4 * 4


def cell_geometries(c_lo, c_hi):
    """(n_classes, ld) x 3 of a cell: the vector form in all four kernels; a scalar log-softmax with vector NLL kernels whose
    last piece straddles n_classes; an odd stride, scalar everywhere."""
    return [(c_hi, c_hi), (c_lo, roundup4(c_lo)), (c_lo, c_lo)]


# ld far beyond 4 K G: the zero-fill loop behind the registers' columns runs several trips (both forms)
WIDE_PADDING = [(10, 64), (10, 63), (40, 128), (349, 1024)]
GEOMETRIES = [g for cell in CELLS for g in cell_geometries(*cell)] + WIDE_PADDING
SWEEP_ROWS = 300        # two full chunks and a part
# rows on, one before and one after a chunk edge, at G = 1 (256 groups for 128 rows: half of them idle), G = 16 and G = 64
LADDER_ROWS = [1, 127, 128, 129, 255, 256, 257]
LADDER_GEOMETRIES = [(4, 4), (61, 64), (349, 352)]
# one, two and three trips of the finalize kernel's loop over the chunk sums
FINALIZE_ROWS = [SM_CHUNK * SM_BLOCK, SM_CHUNK * SM_BLOCK + 1, SM_CHUNK * 2 * SM_BLOCK + 1]
FINALIZE_GEOMETRY = (4, 4)
UNALIGNED_GEOMETRIES = [(40, 40), (349, 352), (768, 768)]
