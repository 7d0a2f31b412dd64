"""The training-mode BatchNorm -> ReLU (-> dropout) -> residual tail (egc_tail.hip) through the C ABI, against float64.

Every training step of the batched nets runs these kernels; the block-level tests elsewhere hold them against torch's
fp32 BatchNorm1d on one small batch.  Here each export is held against a float64 evaluation of the same operation, from
the same float32 inputs, at the shapes where the kernels' own logic branches:

* the partial-block layout, n_parts = min(1024, ceil(n / 128)): 8,192 / 8,193 rows (the one-launch limit of 64
  partials), 131,072 / 131,073 (the first layout with empty trailing blocks), 169,343 (the arxiv graph, 166 rows per
  block) and 10^6 rows;
* the column geometry, cg = cols / 4 thread groups x 256 / cg row lanes: widths whose cg does not divide 256 (12, 124,
  168, 224, 296, 300, 304), one row lane at 1,024 columns, a single column group at 4;
* the folded elementwise forms (out = h scale + shift, dh = c_g g + c_h h + c_1) on columns where |mean| / std is large
  (nearly constant, offset, zero, 1e30, denormal) against torch's fp32 BatchNorm, and the
  ReLU mask the backward recomputes, on pre-activations planted at and next to 0.

Budgets are componentwise, in units of the terms each kernel actually adds (see each check); the worst ratios seen are
printed (pytest -s).  The float64 block tests at the end run FusedEGCBlock in training on each of its routes against
the conv of oracle/egc_torch_ref.py, F.batch_norm, the block's own ReLU decision and dropout mask and the residual, all in
float64.

Open finding (test_adversarial_columns_no_less_accurate_than_torch, a strict xfail): the folded forms lose to torch's fp32 on
columns of large |mean| / std.  Centring h on the batch mean carried in two floats -- t = (h - c_hi) - c_lo, out = t scale
+ beta, dh = c_g g + c_h t + c_1 -- was measured to pass that yardstick and every test in this file, but it moves the tail's
values by an ulp and with them two existing results past their bounds: the molhiv 4-block step on the GraphBatch path
(test_determinism_gpu.py, bases gradient of block 2: 2.6e-3 against 1.8e-3), a max-sensitive gradient of the one-launch
backward that also shows in the widening block below when max is among the aggregators, and the zero-by-analysis conv bias
gradient of test_callers.py at its noise level (1.14e-4 against 1e-4).  The centred tail waits for the first of these."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import elementwise_excess

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OK, INVALID, UNSUPPORTED = 0, 1, 4
U = 2.0 ** -24          # unit roundoff of float32 (half an ulp, relative)
U64 = 2.0 ** -53        # ... of float64
EPS = 1e-5
TINY = 1e-300


def _lib():
    from egc_amd import _C
    return _C.load()


def _check(st, what):
    from egc_amd import _C
    _C.check(st, what)


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _n_parts(n):
    return max(1, min(1024, (n + 127) // 128))


def _ratio(err, budget):
    return float((err / (budget + TINY)).max()) if err.numel() else 0.0


def _columns(n, c, seed):
    """[n, c] float32: every column its own spread (0.1 .. 10) and offset (-3 .. 3, so |mean| / std up to 30)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    h = torch.randn(n, c, device=DEV, generator=g)
    h.mul_(torch.logspace(-1, 1, c, device=DEV)).add_(torch.linspace(-3, 3, c, device=DEV))
    return h


def _params(c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    gamma = torch.rand(c, device=DEV, generator=g) + 0.5
    beta = torch.randn(c, device=DEV, generator=g)
    return gamma, beta


def _stats64(h, n_valid=None):
    """Two-pass float64 mean, biased variance, 1 / sqrt(var + eps) over the first n_valid rows."""
    hv = (h if n_valid is None else h[:n_valid]).double()
    mean = hv.mean(0)
    var = ((hv - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + EPS), (hv * hv).mean(0), hv.abs().mean(0)


# ----------------------------------------------------------------------------------------------------------------------
# statistics: egc_bn_forward_stats_f32 (one launch with a sync word at <= 64 partials, else two), egc_column_moments_f64
# followed by egc_bn_forward_finalize

def _forward_stats(h, gamma, beta, mode, n_parts=None, running=None, momentum=0.1, n_tracked=None, n_valid=None, sync=None):
    lib = _lib()
    n, c = h.shape
    n_parts = n_parts or _n_parts(n)
    parts = torch.full((n_parts, 2, c), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((3, c), float("nan"), dtype=torch.float64, device=DEV)
    affine = torch.full((2, c), float("nan"), device=DEV)   # scale | shift
    rm, rv = running if running is not None else (None, None)
    mom = -1.0 if momentum is None else momentum
    count = n_tracked if rm is not None else None
    if mode == "split":
        _check(lib.egc_column_moments_f64(h.data_ptr(), None, None, None, 0, None, 1.0, n, c, parts.data_ptr(), n_parts, _p(count),
                                          _p(n_valid), _stream()), "egc_column_moments_f64")
        _check(lib.egc_bn_forward_finalize(parts.data_ptr(), n_parts, c, n, _p(gamma), _p(beta), EPS, stats.data_ptr(),
                                           affine.data_ptr(), _p(rm), _p(rv), mom, _p(n_tracked), _p(n_valid), _stream()),
               "egc_bn_forward_finalize")
    else:
        _check(lib.egc_bn_forward_stats_f32(h.data_ptr(), n, c, parts.data_ptr(), n_parts, _p(count), _p(n_valid), _p(gamma), _p(beta),
                                            EPS, stats.data_ptr(), affine.data_ptr(), _p(rm), _p(rv), mom, _p(n_tracked), _p(sync),
                                            _stream()), "egc_bn_forward_stats_f32")
    return stats, affine


def _chain(n, c, n_parts=None):
    """The longest chain of float64 adds behind a column sum: rows per lane (rows per block / row lanes), the row lanes of a
    block, then the partials -- per finalize lane (n_parts / 64), eight lanes, eight runs."""
    n_parts = n_parts or _n_parts(n)
    rl = 256 // (c // 4)
    return -(-(-(-n // n_parts)) // rl) + rl + -(-n_parts // 64) + 16


def _check_stats(stats, affine, h, gamma, beta, n_valid=None, worst=None):
    """stats against the two-pass float64 values.  The kernel forms mean = sum h / n and var = sum h^2 / n - mean^2 with float64
    sums over float32 inputs (exact products).  Each sum is a chain of L float64 adds (_chain: rows per lane + lanes +
    partials); its rounding error grows as sqrt(L) units of 2^-53 of the sum of |terms| (independent roundings; L of them is the
    worst case, never approached), so the budget is 2 sqrt(L) units of 2^-52 of E|h| (mean) and of E[h^2] (variance: s2 / n
    and mean^2 each bring one such error; the cancellation of the kernel's form is what this budget admits, not a relative
    error on a variance that cancels), and at least 4 units.  rstd
    inherits the variance's budget through d rstd = -rstd^3 / 2 d var.  scale: at most 1 float32 ulp from the float64 gamma rstd
    (one rounding of a float64 value: half an ulp; the other half covers the stats) plus gamma times the rstd budget; shift:
    1 ulp from the float64 beta - mean gamma rstd plus what the mean and rstd budgets propagate into it."""
    mean, var, rstd, e2, eabs = _stats64(h, n_valid)
    k = max(4.0, 2.0 * math.sqrt(_chain(h.size(0), h.size(1))))
    b_mean = k * 2 * U64 * eabs
    b_var = k * 2 * U64 * e2
    b_rstd = 0.5 * rstd ** 3 * b_var + 4 * U64 * rstd
    r = [_ratio((stats[0] - mean).abs(), b_mean), _ratio((stats[1] - var).abs(), b_var), _ratio((stats[2] - rstd).abs(), b_rstd)]
    g64 = gamma.double() if gamma is not None else torch.ones_like(mean)
    b64 = beta.double() if beta is not None else torch.zeros_like(mean)
    scale = g64 * rstd
    ulp = lambda v: torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    # (scale: its own rounding, and gamma times the rstd budget -- more than an ulp only where the variance cancels)
    r.append(_ratio((affine[0].double() - scale).abs(), ulp(scale) + g64.abs() * b_rstd))
    # (shift: its own rounding, and the one of a float64 mean gamma rstd whose error is the mean's budget times gamma rstd)
    shift = b64 - mean * g64 * rstd
    r.append(_ratio((affine[1].double() - shift).abs(), ulp(shift) + b_mean * (g64 * rstd).abs() + b_rstd * (mean * g64).abs()))
    names = ("mean", "var", "rstd", "scale", "shift")
    if worst is not None:
        for k, v in zip(names, r):
            worst[k] = max(worst.get(k, 0.0), v)
    assert max(r) <= 1.0, dict(zip(names, r))
    return mean, var


# every row count meets a column group count that does not divide 256; 1,024 columns meet the largest row counts
STAT_SHAPES = [(2, 300), (2, 4), (3, 12), (3, 1024), (127, 168), (127, 304), (128, 224), (128, 124), (129, 296), (129, 4),
               (8192, 300), (8192, 1024), (8193, 168), (8193, 128), (131072, 224), (131072, 1024), (131073, 300),
               (131073, 1024), (169343, 168), (169343, 1024), (10 ** 6, 128), (10 ** 6, 12)]


@pytest.mark.parametrize("mode", ["sync", "nosync", "split"])
@pytest.mark.parametrize("n,c", STAT_SHAPES)
def test_forward_statistics_and_running_statistics_against_float64(n, c, mode):
    torch.manual_seed(n + c)
    gamma, beta = _params(c, n + c)
    momentum = None if mode == "split" else 0.1            # the cumulative average through the two-launch form
    rm = torch.zeros(c, device=DEV)
    rv = torch.ones(c, device=DEV)
    nt = torch.zeros((), dtype=torch.int64, device=DEV)
    sync = torch.zeros(1, dtype=torch.int32, device=DEV) if mode == "sync" else None
    base = _columns(n, c, n * 7 + c)
    worst = {}
    calls = 3 if n >= 2 else 1
    for k in range(calls):
        h = base * (1.0 + 0.25 * k) + 0.5 * k                 # three different batches
        rm_prev, rv_prev = rm.double(), rv.double()
        stats, affine = _forward_stats(h, gamma, beta, mode, running=(rm, rv), momentum=momentum, n_tracked=nt, sync=sync)
        torch.cuda.synchronize()
        mean, var = _check_stats(stats, affine, h, gamma, beta, worst=worst)
        assert int(nt) == k + 1                                # num_batches_tracked bumped once per call
        if sync is not None:
            assert int(sync) == 0                              # the arrival counter is back at zero
        m = 0.1 if momentum is not None else 1.0 / (k + 1)
        rm_ref = (1 - m) * rm_prev + m * mean
        rv_ref = (1 - m) * rv_prev + m * var * (n / (n - 1))       # the unbiased factor
        # one float32 rounding each (half an ulp), and as much again for m times the stats budget (<< 1 ulp)
        for got, ref in ((rm, rm_ref), (rv, rv_ref)):
            err = (got.double() - ref).abs()
            assert bool((err <= 2 * U * ref.abs() + 1e-30).all()), (k, float((err / (ref.abs() + 1e-30)).max()))
    print(f"stats n={n} c={c} {mode}: worst ratio to budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("n,c", [(300, 168), (8193, 224)])
@pytest.mark.parametrize("mode", ["sync", "split"])
def test_padding_rows_past_n_valid(n, c, mode):
    """n_valid (device int64): only the leading rows count.  0 rows: mean 0, variance 0 (the kernels divide by max(n, 1));
    1 row: the row itself, variance 0; n_valid >= n: every row.  The elementwise passes write exact zeros from row n_valid on,
    forward and backward, and the backward sums skip the padding."""
    lib = _lib()
    h = _columns(n, c, 5)
    gamma, beta = _params(c, 5)
    dout = torch.randn(n, c, device=DEV)
    for nv in (0, 1, n // 3, n, n + 7):
        n_valid = torch.tensor(nv, dtype=torch.int64, device=DEV)
        sync = torch.zeros(1, dtype=torch.int32, device=DEV) if mode == "sync" else None
        stats, affine = _forward_stats(h, gamma, beta, mode, n_valid=n_valid, sync=sync)
        out = torch.full_like(h, float("nan"))
        _check(lib.egc_affine_act_residual_f32(h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), h.data_ptr(), 1, None, 1.0, n, c,
                                               out.data_ptr(), n_valid.data_ptr(), _stream()), "egc_affine_act_residual_f32")
        parts = torch.empty((_n_parts(n), 2, c), dtype=torch.float64, device=DEV)
        out5 = torch.full((5, c), float("nan"), device=DEV)
        _check(lib.egc_bn_backward_stats_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), 1, None, 1.0, n, c,
                                             parts.data_ptr(), parts.size(0), n_valid.data_ptr(), stats.data_ptr(), gamma.data_ptr(),
                                             out5.data_ptr(), _p(sync), _stream()), "egc_bn_backward_stats_f32")
        dh = torch.full_like(h, float("nan"))
        _check(lib.egc_affine_act_backward_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), 1, None, 1.0,
                                               out5[2].data_ptr(), out5[3].data_ptr(), out5[4].data_ptr(), n, c, dh.data_ptr(),
                                               n_valid.data_ptr(), _stream()), "egc_affine_act_backward_f32")
        torch.cuda.synchronize()
        v = min(nv, n)
        if v == 0:
            assert bool((stats[0] == 0).all() and (stats[1] == 0).all()), nv
            assert torch.allclose(stats[2], torch.full_like(stats[2], 1.0 / math.sqrt(EPS)), rtol=1e-15, atol=0), nv
        else:
            _check_stats(stats, affine, h, gamma, beta, n_valid=v)
        assert bool((out[v:] == 0).all()) and bool((dh[v:] == 0).all()), nv
        assert bool(torch.isfinite(out[:v]).all()) and bool(torch.isfinite(dh[:v]).all()), nv
        if v:
            _check_out(out[:v], h[:v], affine[0], affine[1], h[:v], True, None, 1.0)
            g = dout[:v].double() * ((h[:v] * affine[0] + affine[1]) > 0).double()
            assert bool(((out5[1].double() - g.sum(0)).abs() <= 2 * U * g.abs().sum(0) + 1e-30).all()), nv


# ----------------------------------------------------------------------------------------------------------------------
# elementwise forward: egc_affine_act_residual_f32

K_OUT = 4


def _affine_act(h, scale, shift, residual, relu, keep, keep_scale, n_valid=None):
    n, c = h.shape
    out = torch.full_like(h, float("nan"))
    _check(_lib().egc_affine_act_residual_f32(h.data_ptr(), scale.data_ptr(), shift.data_ptr(), _p(residual), int(relu), _p(keep),
                                              float(keep_scale), n, c, out.data_ptr(), _p(n_valid), _stream()),
           "egc_affine_act_residual_f32")
    return out


def _check_out(out, h, scale, shift, residual, relu, keep, keep_scale):
    """|out - ref| <= K_OUT 2^-24 (ks (|h scale| + |shift|) + |residual| + |out|), ref and terms in float64 from the same float32
    operands.  K_OUT = 4 roundings of at most half an ulp each: the product h scale and the add of shift (2, each within
    |h scale| + |shift|; 1 if contracted), the dropout scaling (1, within ks (|h scale| + |shift|)), the residual add (1, within
    |out|)."""
    h64, s64, b64 = h.double(), scale.double(), shift.double()
    ks = torch.ones_like(h64) if keep is None else keep.double() * float(np.float32(keep_scale))
    pre = h64 * s64 + b64
    ref = (torch.relu(pre) if relu else pre) * ks
    res = residual.double() if residual is not None else torch.zeros_like(h64)
    ref = ref + res
    budget = K_OUT * U * (ks * ((h64 * s64).abs() + b64.abs()) + res.abs() + out.double().abs())
    r = _ratio((out.double() - ref).abs(), budget)
    assert r <= 1.0, r
    return r


ELEM_SHAPES = [(2, 4), (3, 12), (127, 300), (129, 168), (8193, 224), (131073, 12), (169343, 1024), (10 ** 6, 128)]


@pytest.mark.parametrize("n,c", ELEM_SHAPES)
def test_affine_act_residual_against_float64(n, c):
    h = _columns(n, c, n + 3 * c)
    gamma, beta = _params(c, c)
    mean, var, rstd = _stats64(h)[:3]
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - mean * gamma.double() * rstd).float()
    res = torch.randn(n, c, device=DEV) * 4
    keep = (torch.rand(n, c, device=DEV) > 0.2).to(torch.uint8)
    worst = 0.0
    for relu, residual, kp, ks in ((True, res, None, 1.0), (False, res, None, 1.0), (True, None, None, 1.0), (False, None, None, 1.0),
                                   (True, res, keep, 1.25), (False, None, keep, 1.0 / 0.7)):
        out = _affine_act(h, scale, shift, residual, relu, kp, ks)
        torch.cuda.synchronize()
        worst = max(worst, _check_out(out, h, scale, shift, residual, relu, kp, ks))
    # padding rows: exact zeros from n_valid on, the rows before as without it
    nv = torch.tensor(n // 2, dtype=torch.int64, device=DEV)
    out = _affine_act(h, scale, shift, res, True, keep, 1.25, n_valid=nv)
    full = _affine_act(h, scale, shift, res, True, keep, 1.25)
    torch.cuda.synchronize()
    assert bool((out[n // 2:] == 0).all()) and torch.equal(out[:n // 2], full[:n // 2])
    print(f"out n={n} c={c}: worst ratio to budget {worst:.3g}")


# ----------------------------------------------------------------------------------------------------------------------
# backward: egc_bn_backward_stats_sums_f32 / egc_bn_backward_stats_f32 / egc_column_moments_f64 + egc_bn_backward_finalize,
# then egc_affine_act_backward_f32

K_DH = 5


def _backward(dout, h, affine, stats, gamma, keep, keep_scale, mode, relu=True, sums=True):
    lib = _lib()
    n, c = h.shape
    n_parts = _n_parts(n)
    parts = torch.full((n_parts, 2, c), float("nan"), dtype=torch.float64, device=DEV)
    out5 = torch.full((5, c), float("nan"), device=DEV)
    dh_sums = torch.full((c,), float("nan"), device=DEV) if sums else None
    sync = torch.zeros(1, dtype=torch.int32, device=DEV) if mode == "sync" else None
    if mode == "split":
        _check(lib.egc_column_moments_f64(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), int(relu), _p(keep),
                                          float(keep_scale), n, c, parts.data_ptr(), n_parts, None, None, _stream()), "egc_column_moments_f64")
        _check(lib.egc_bn_backward_finalize(parts.data_ptr(), n_parts, c, n, stats.data_ptr(), _p(gamma), out5.data_ptr(), None, _stream()),
               "egc_bn_backward_finalize")
    elif sums:
        _check(lib.egc_bn_backward_stats_sums_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), int(relu),
                                                  _p(keep), float(keep_scale), n, c, parts.data_ptr(), n_parts, None, stats.data_ptr(),
                                                  _p(gamma), out5.data_ptr(), _p(dh_sums), _p(sync), _stream()),
               "egc_bn_backward_stats_sums_f32")
    else:
        _check(lib.egc_bn_backward_stats_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), int(relu), _p(keep),
                                             float(keep_scale), n, c, parts.data_ptr(), n_parts, None, stats.data_ptr(), _p(gamma),
                                             out5.data_ptr(), _p(sync), _stream()), "egc_bn_backward_stats_f32")
    dh = torch.full_like(h, float("nan"))
    _check(lib.egc_affine_act_backward_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), int(relu), _p(keep),
                                           float(keep_scale), out5[2].data_ptr(), out5[3].data_ptr(), out5[4].data_ptr(), n, c,
                                           dh.data_ptr(), None, _stream()), "egc_affine_act_backward_f32")
    torch.cuda.synchronize()
    if sync is not None:
        assert int(sync) == 0
    return out5, dh, (dh_sums if (sums and mode != "split") else None)


def _backward_ref(dout, h, gamma, keep, keep_scale, mask):
    """The textbook BatchNorm backward in float64 on g = dout * keep * keep_scale * mask (mask: the kernel forward's own ReLU
    decision): dgamma = sum g h^, dbeta = sum g, dh = a (g - (sum g + h^ sum g h^) / n), a = gamma rstd."""
    n = h.size(0)
    mean, var, rstd = _stats64(h)[:3]
    g = dout.double() * mask.double()
    if keep is not None:
        g = g * keep.double() * float(np.float32(keep_scale))      # (keep_scale reaches the kernels as a float32)
    hhat = (h.double() - mean) * rstd
    s1, s2 = g.sum(0), (g * hhat).sum(0)
    a = gamma.double() * rstd
    dh = a * (g - (s1 + hhat * s2) / n)
    # the three coefficients of dh = c_g g + c_h h + c_1, in float64 (the budget's terms)
    cg, ch, c1 = a, -(a / n) * rstd * s2, -(a / n) * (s1 - mean * rstd * s2)
    terms = (cg * g).abs() + (ch * h.double()).abs() + c1.abs()
    return g, hhat, s1, s2, dh, terms, mean, rstd


def _check_backward(out5, dh, dh_sums, dout, h, gamma, keep, keep_scale, mask, worst=None, affine=None, stats=None):
    """d gamma / d beta: 2^-23 |ref| + 2^-40 sum |terms| (the terms the kernel adds in float64: g h rstd and mean g rstd for
    d gamma, g for d beta).  dh: componentwise K_DH 2^-24 (|c_g g| + |c_h h| + |c_1|), K_DH = 5 roundings of at most half an
    ulp, each within the terms: the three float32 coefficients (1 in all), the product c_h h, the product c_g g and two adds
    (at most 3 when not contracted), the dropout scaling of g (1); with dropout, also the float32 rounding of g inside the two
    sums, through c_h and c_1.  dh_col_sums: (a) the float64 sum of the kernel's own dh, within the rounding of
    those dh elements (each off its exact value by up to ~2 ulp of its terms) -- 2^-24 n max |terms| per column; (b) the value
    the stored coefficients give from the step's own sums, c_g sum g + c_h n mean + n c_1, to its float32 rounding:
    it is rounding noise around 0, so only (b) tells a working kernel from one that writes zeros."""
    g, hhat, s1, s2, dh_ref, terms, mean, rstd = _backward_ref(dout, h, gamma, keep, keep_scale, mask)
    t_dg = ((g * h.double()).abs().sum(0) + mean.abs() * g.abs().sum(0)) * rstd
    # with dropout every g = dout keep_scale is a float32 product, rounded before the float64 sums: 2^-24 of each term
    ut = 2.0 ** -40 + (U if keep is not None else 0.0)
    r_dg = _ratio((out5[0].double() - s2).abs(), 2 * U * s2.abs() + ut * t_dg)
    r_db = _ratio((out5[1].double() - s1).abs(), 2 * U * s1.abs() + ut * g.abs().sum(0))
    # ... which reaches c_h and c_1 through the two sums: (a / n) (ut sum |g| + |h^| ut sum |g h^|)
    a_n = (gamma.double() * rstd) / h.size(0)
    coef = a_n * (ut * g.abs().sum(0) + hhat.abs() * ut * (g * hhat).abs().sum(0))
    r_dh = _ratio((dh.double() - dh_ref).abs(), K_DH * U * terms + 2 * coef)
    r = {"dgamma": r_dg, "dbeta": r_db, "dh": r_dh}
    if dh_sums is not None:
        n = h.size(0)
        ref = dh.double().sum(0)
        kt = (out5[2].double().abs() * g.abs() + out5[3].double().abs() * h.double().abs() + out5[4].double().abs())
        r["dh_sums"] = _ratio((dh_sums.double() - ref).abs(), U * n * kt.max(0).values + 1e-30)
        # (b): the kernel's g as float32 products, its own mean; the float64 sums differ in order only
        g32 = dout * mask.float()
        if keep is not None:
            g32 = g32 * (keep.float() * float(np.float32(keep_scale)))
        cg, ch, c1 = (out5[i].double() for i in (2, 3, 4))
        exact = cg * g32.double().sum(0) + ch * (n * stats[0]) + n * c1
        size = (cg * g32.double().abs().sum(0)).abs() + (ch * n * stats[0]).abs() + (n * c1).abs()
        r["dh_sums_exact"] = _ratio((dh_sums.double() - exact).abs(), U * exact.abs() + 2.0 ** -40 * size + 1e-300)
    if worst is not None:
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert max(r.values()) <= 1.0, r


BWD_SHAPES = [(2, 300), (3, 12), (127, 168), (128, 4), (129, 224), (8192, 296), (8193, 300), (8193, 1024), (131072, 168),
              (131073, 224), (169343, 1024), (10 ** 6, 128)]


@pytest.mark.parametrize("mode", ["sync", "nosync", "split"])
@pytest.mark.parametrize("n,c", BWD_SHAPES)
def test_backward_against_float64(n, c, mode):
    h = _columns(n, c, 11 * n + c)
    gamma, beta = _params(c, 3 * c)
    dout = torch.randn(n, c, device=DEV)
    stats, affine = _forward_stats(h, gamma, beta, "nosync")
    # the ReLU mask the forward applies: its own decision, read back from an output without residual
    mask = _affine_act(h, affine[0], affine[1], None, True, None, 1.0) > 0
    worst = {}
    out5, dh, sums = _backward(dout, h, affine, stats, gamma, None, 1.0, mode, sums=(mode != "nosync"))
    _check_backward(out5, dh, sums, dout, h, gamma, None, 1.0, mask, worst, affine=affine, stats=stats)
    if n >= 8192 or mode == "sync":           # the arxiv net's dropout rides along
        keep = (torch.rand(n, c, device=DEV) > 0.3).to(torch.uint8)
        ks = 1.0 / 0.7
        out5, dh, sums = _backward(dout, h, affine, stats, gamma, keep, ks, mode, sums=(mode != "nosync"))
        _check_backward(out5, dh, sums, dout, h, gamma, keep, ks, mask, worst, affine=affine, stats=stats)
    print(f"backward n={n} c={c} {mode}: worst ratio to budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ----------------------------------------------------------------------------------------------------------------------
# adversarial columns

def _adversarial(n):
    """[n, 128] float32: an exactly constant column, |mean| / std ~ 1e3 and ~ 1e5, an all-zero column, a column of magnitude
    ~1e30 (h^2 overflows float32, not the float64 sums), a column of denormals, then ordinary columns."""
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, 128, generator=g, dtype=torch.float64)
    h = z * torch.logspace(-1, 1, 128, dtype=torch.float64) + torch.linspace(-3, 3, 128, dtype=torch.float64)
    h[:, 0] = 3.0
    h[:, 1] = 1e3 + z[:, 1]
    h[:, 2] = 1e5 + z[:, 2]
    h[:, 3] = -2e2 + 2e-3 * z[:, 3]
    h[:, 4] = 0.0
    h[:, 5] = 1e30 * z[:, 5]
    h[:, 6] = 1e-40 * z[:, 6]
    h[:, 7] = 7e4 + 0.7 * z[:, 7]
    return h.float().to(DEV)       # (rounded on the host: denormals survive)


ADV_COLS = {0: "constant", 1: "mean/std 1e3", 2: "mean/std 1e5", 3: "mean/std 1e5 (2)", 4: "zero", 5: "1e30", 6: "denormal",
            7: "mean/std 1e5 (3)"}


def test_adversarial_columns_statistics():
    for n in (4099, 8192, 131073):
        h = _adversarial(n)
        gamma, beta = _params(128, 17)
        for mode in ("sync", "split"):
            sync = torch.zeros(1, dtype=torch.int32, device=DEV) if mode == "sync" else None
            stats, affine = _forward_stats(h, gamma, beta, mode, sync=sync)
            torch.cuda.synchronize()
            _check_stats(stats, affine, h, gamma, beta)
            assert float(stats[1, 0]) == 0.0 and abs(float(stats[2, 0]) * math.sqrt(EPS) - 1.0) <= 1e-15   # exactly constant
            assert float(stats[0, 4]) == 0.0 and float(stats[1, 4]) == 0.0                       # all zero
            assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(affine).all())


def _torch_fp32_bn(h, gamma, beta, dout):
    hh = h.clone().requires_grad_(True)
    out = F.batch_norm(hh, None, None, gamma, beta, True, 0.1, EPS)
    out.backward(dout)
    return out.detach(), hh.grad


def _adversarial_case(n=8192):
    h = _adversarial(n)
    gamma, beta = _params(128, 23)
    dout = torch.randn(n, 128, device=DEV)
    stats, affine = _forward_stats(h, gamma, beta, "nosync")
    out = _affine_act(h, affine[0], affine[1], None, False, None, 1.0)
    out5, dh, _ = _backward(dout, h, affine, stats, gamma, None, 1.0, "nosync", relu=False, sums=False)
    return h, gamma, beta, dout, affine, out, out5, dh


def test_adversarial_columns_within_the_elementwise_bounds():
    """On the adversarial columns the elementwise passes keep the componentwise bounds of their folded forms (the K_OUT
    roundings above; for dh two products and two adds), and nothing overflows (h^2 of the 1e30 column exists only in
    float64)."""
    h, gamma, beta, dout, affine, out, out5, dh = _adversarial_case()
    r_out = _check_out(out, h, affine[0], affine[1], None, False, None, 1.0)
    # dh against the float64 value of the kernel's own float32 coefficients (their accuracy is that of the statistics, whose
    # variance cancels on these columns: held above)
    cg, ch, c1 = (out5[i].double() for i in (2, 3, 4))
    g64 = dout.double()
    h64 = h.double()
    terms = (cg * g64).abs() + (ch * h64).abs() + c1.abs()
    r_dh = _ratio((dh.double() - (cg * g64 + ch * h64 + c1)).abs(), 4 * U * terms)
    s1 = g64.sum(0)
    r_db = _ratio((out5[1].double() - s1).abs(), 2 * U * s1.abs() + 2.0 ** -40 * g64.abs().sum(0))
    assert r_dh <= 1.0 and r_db <= 1.0, (r_dh, r_db)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dh).all()) and bool(torch.isfinite(out5).all())
    print(f"adversarial: out {r_out:.3g} dh {r_dh:.3g} dbeta {r_db:.3g}")


@pytest.mark.xfail(strict=True, reason="the folded forms h scale + shift and c_g g + c_h h + c_1 round the cancelling terms "
                                       "|mean| rstd: up to ~7x torch's fp32 error on nearly constant / offset columns")
def test_adversarial_columns_no_less_accurate_than_torch():
    """The folded forms out = h scale + (beta - mean scale) and dh = c_g g + c_h h + c_1 cancel where |mean| rstd is large.
    Per column, the kernels' error against float64 held to torch's fp32 F.batch_norm on the same input -- the yardstick
    test_parity_gpu.py uses for std / var: kernel error <= max(1e-6 x the column's scale, 2 x torch's).  MEASURED (8,192
    rows): the forward output misses it -- 2.4e-5 against torch's exact result on a constant column, 5x torch's error on
    |mean| / std = 1e3, 7x on 1e5 -- and dh on one |mean| / std = 1e5 column (2.6x).  A tail that centres h on the mean (two
    floats) before scaling passes it; see the module docstring for why the tail does not yet.  Strict: when it does, this
    marker goes."""
    h, gamma, beta, dout, affine, out, out5, dh = _adversarial_case()
    t_out, t_dh = _torch_fp32_bn(h, gamma, beta, dout)
    h64 = h.double().requires_grad_(True)
    r_out = F.batch_norm(h64, None, None, gamma.double(), beta.double(), True, 0.1, EPS)
    r_out.backward(dout.double())
    r_out, r_dh = r_out.detach(), h64.grad
    nan_inf = lambda e: torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    rows, bad = [], []
    for what, got, tor, ref in (("out", out, t_out, r_out), ("dh", dh, t_dh, r_dh)):
        e_k = nan_inf((got.double() - ref).abs()).max(0).values
        e_t = nan_inf((tor.double() - ref).abs()).max(0).values
        scale = ref.abs().max(0).values
        allowed = torch.maximum(1e-6 * scale, 2 * e_t)
        for col, name in ADV_COLS.items():
            rows.append((what, name, float(e_k[col]), float(e_t[col])))
        bad += [(what, col, float(e_k[col]), float(e_t[col])) for col in range(128) if not bool(e_k[col] <= allowed[col])]
        fin = torch.isfinite(e_t) & (e_t > 0)
        print(what, "worst kernel / torch over the ordinary columns:", float((e_k / e_t)[8:][fin[8:]].max()))
    for row in rows:
        print("%-3s %-18s kernel %.3g  torch fp32 %.3g" % row)
    assert not bad, bad


def _planted_mask_inputs(n_cols=128, per_col=256, seed=0):
    """scale / shift per column and h planted where h scale + shift is exactly 0 or within a few float32 ulp of 0 -- under the
    fused (fma) and the separately rounded evaluation: the candidates are the float32 neighbours of -shift / scale."""
    rng = np.random.default_rng(seed)
    scale = (rng.uniform(0.3, 3.0, n_cols) * rng.choice([-1, 1], n_cols)).astype(np.float32)
    shift = (rng.standard_normal(n_cols) * np.logspace(-2, 4, n_cols)).astype(np.float32)
    scale[:4] = [1.0, 0.5, 3.0, -2.0]            # exact products: many exact zeros
    shift[:4] = [0.75, -1.5, 96.0, 8.0]
    root = (-shift.astype(np.float64) / scale.astype(np.float64)).astype(np.float32)
    h = np.empty((per_col, n_cols), np.float32)
    for c in range(n_cols):
        above = np.full(per_col // 2, root[c], np.float32)
        below = above.copy()
        for i in range(1, per_col // 2):
            above[i] = np.nextafter(above[i - 1], np.float32(np.inf))
            below[i] = np.nextafter(below[i - 1], np.float32(-np.inf))
        h[:, c] = np.concatenate([below[::-1], above])
    fused = (h.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)   # exact product, one rounding
    sep = (h * scale).astype(np.float32) + shift
    return h, scale, shift, fused, sep


def test_relu_mask_of_the_backward_equals_the_forward_decision():
    """Pre-activations at and next to 0, where a product rounded apart from its add and an fma can decide differently: the
    backward's recomputed mask (the elementwise pass and the moments pass) must equal the forward's decision on every element
    -- no gradient a g where the forward output 0, none lost where it passed."""
    lib = _lib()
    h_np, s_np, b_np, fused, sep = _planted_mask_inputs()
    assert (fused == 0).sum() > 0 and (sep == 0).sum() > 0
    assert ((fused > 0) != (sep > 0)).sum() > 0          # the planted set tells the two evaluations apart
    reps = 64                                            # several row blocks
    h = torch.from_numpy(np.tile(h_np, (reps, 1))).to(DEV).contiguous()
    n, c = h.shape
    scale, shift = torch.from_numpy(s_np).to(DEV), torch.from_numpy(b_np).to(DEV)
    ones = torch.ones_like(h)
    keep = torch.ones(n, c, dtype=torch.uint8, device=DEV)
    zero = torch.zeros(c, device=DEV)
    unit = torch.ones(c, device=DEV)
    for kp in (None, keep):
        fwd = _affine_act(h, scale, shift, None, True, kp, 1.0) > 0
        dh = torch.full_like(h, float("nan"))
        _check(lib.egc_affine_act_backward_f32(ones.data_ptr(), h.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, _p(kp), 1.0,
                                               unit.data_ptr(), zero.data_ptr(), zero.data_ptr(), n, c, dh.data_ptr(), None, _stream()),
               "egc_affine_act_backward_f32")
        parts = torch.empty((_n_parts(n), 2, c), dtype=torch.float64, device=DEV)
        _check(lib.egc_column_moments_f64(ones.data_ptr(), h.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, _p(kp), 1.0, n, c,
                                          parts.data_ptr(), parts.size(0), None, None, _stream()), "egc_column_moments_f64")
        torch.cuda.synchronize()
        assert torch.equal(dh == 1.0, fwd) and bool(((dh == 0) | (dh == 1)).all())
        assert torch.equal(parts[:, 0].sum(0), fwd.double().sum(0))
    print("planted: exact zeros fused %d / separate %d, decisions that differ %d" % ((fused == 0).sum(), (sep == 0).sum(),
                                                                                    ((fused > 0) != (sep > 0)).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# column sums: egc_column_sums_f32 + egc_sum_partials_f32

@pytest.mark.parametrize("n,c,ld", [(1, 4, 4), (1, 1024, 1024), (129, 12, 12), (129, 300, 308), (131073, 168, 168),
                                    (131073, 1024, 1024), (10 ** 6, 128, 128), (10 ** 6, 4, 12), (8193, 224, 352)])
def test_column_sums_against_float64(n, c, ld):
    """Column sums of [n, c] (a column block of [n, ld] when ld > c, as _column_sums passes d_cat[:, ldb:]) in n_parts partial
    rows, then added in a fixed order: within 2^-24 (rows per partial + n_parts) sum |x| (one rounding per add of each chain)."""
    lib = _lib()
    full = torch.randn(n, ld, device=DEV) * torch.logspace(-2, 2, ld, device=DEV) + torch.linspace(-5, 5, ld, device=DEV)
    off = (ld - c) // 8 * 4                     # a 16-byte aligned block inside the wider matrix
    x = full[:, off:off + c]
    parts = _n_parts(n)
    rows_per = -(-n // parts)
    pr = torch.full((parts, c), float("nan"), device=DEV)
    out = torch.full((c,), float("nan"), device=DEV)
    _check(lib.egc_column_sums_f32(x.data_ptr(), n, ld, c, pr.data_ptr(), parts, _stream()), "egc_column_sums_f32")
    _check(lib.egc_sum_partials_f32(pr.data_ptr(), parts, c, out.data_ptr(), _stream()), "egc_sum_partials_f32")
    torch.cuda.synchronize()
    ref = x.double().sum(0)
    r = _ratio((out.double() - ref).abs(), U * (rows_per + parts) * x.double().abs().sum(0))
    assert r <= 1.0, r
    from egc_amd import functional as Fn
    assert torch.equal(Fn._column_sums(x), out if parts > 1 else pr[0])     # the library path the backward takes
    print(f"column sums n={n} c={c} ld={ld}: ratio to budget {r:.3g}")


# ----------------------------------------------------------------------------------------------------------------------
# refusals: the status egc_hip.h promises

def test_tail_entries_refuse_what_they_do_not_implement():
    lib = _lib()
    n, c = 64, 8
    h = torch.randn(n, 1028, device=DEV)
    v = torch.ones(1028, device=DEV)
    parts = torch.zeros((1, 2, 1028), dtype=torch.float64, device=DEV)
    stats = torch.zeros((3, 1028), dtype=torch.float64, device=DEV)
    aff = torch.zeros((2, 1028), device=DEV)
    out5 = torch.zeros((5, 1028), device=DEV)
    out = torch.zeros(n, 1028, device=DEV)
    s = _stream()
    mis = h.data_ptr() + 4                               # 4-byte aligned, not 16

    def moments(a=h.data_ptr(), b=None, cols=c, parts_=parts.data_ptr()):
        return lib.egc_column_moments_f64(a, b, v.data_ptr(), v.data_ptr(), 1, None, 1.0, n, cols, parts_, 1, None, None, s)

    def fstats(hp=h.data_ptr(), cols=c, nr=n, rm=None, rv=None, mom=0.1, ntr=None, sync=None):
        return lib.egc_bn_forward_stats_f32(hp, nr, cols, parts.data_ptr(), 1, None, None, None, None, EPS, stats.data_ptr(),
                                            aff.data_ptr(), rm, rv, mom, ntr, sync, s)

    def ffin(cols=c, nr=n, rm=None, rv=None, mom=0.1, ntr=None):
        return lib.egc_bn_forward_finalize(parts.data_ptr(), 1, cols, nr, None, None, EPS, stats.data_ptr(), aff.data_ptr(), rm, rv, mom,
                                           ntr, None, s)

    def bstats(cols=c, hp=h.data_ptr(), sync=None, sums=False):
        if sums:
            return lib.egc_bn_backward_stats_sums_f32(h.data_ptr(), hp, v.data_ptr(), v.data_ptr(), 1, None, 1.0, n, cols, parts.data_ptr(), 1,
                                                      None, stats.data_ptr(), None, out5.data_ptr(), v.data_ptr(), sync, s)
        return lib.egc_bn_backward_stats_f32(h.data_ptr(), hp, v.data_ptr(), v.data_ptr(), 1, None, 1.0, n, cols, parts.data_ptr(), 1, None,
                                             stats.data_ptr(), None, out5.data_ptr(), sync, s)

    def fwd(cols=c, hp=h.data_ptr(), sc=v.data_ptr()):
        return lib.egc_affine_act_residual_f32(hp, sc, v.data_ptr(), None, 1, None, 1.0, n, cols, out.data_ptr(), None, s)

    def bwd(cols=c, hp=h.data_ptr(), cg=v.data_ptr()):
        return lib.egc_affine_act_backward_f32(h.data_ptr(), hp, v.data_ptr(), v.data_ptr(), 1, None, 1.0, cg, v.data_ptr(), v.data_ptr(),
                                               n, cols, out.data_ptr(), None, s)

    sync = torch.zeros(1, dtype=torch.int32, device=DEV)
    rm, rv = torch.zeros(1028, device=DEV), torch.ones(1028, device=DEV)
    # cols not a multiple of 4: every tail entry
    for call in (lambda: moments(cols=6), lambda: fstats(cols=6), lambda: fstats(cols=6, sync=sync.data_ptr()), lambda: bstats(cols=6),
                 lambda: bstats(cols=6, sync=sync.data_ptr()), lambda: bstats(cols=6, sums=True, sync=sync.data_ptr()),
                 lambda: fwd(cols=6), lambda: bwd(cols=6),
                 lambda: lib.egc_column_sums_f32(h.data_ptr(), n, 1028, 6, out.data_ptr(), 1, s),
                 lambda: lib.egc_sum_partials_f32(out.data_ptr(), 1, 6, out5.data_ptr(), s)):
        assert call() == UNSUPPORTED
    # cols above 1,024: the moments and statistics entries (the elementwise kernels have no such limit)
    for call in (lambda: moments(cols=1028), lambda: fstats(cols=1028), lambda: fstats(cols=1028, sync=sync.data_ptr()),
                 lambda: bstats(cols=1028), lambda: bstats(cols=1028, sync=sync.data_ptr()),
                 lambda: lib.egc_column_sums_f32(h.data_ptr(), n, 1028, 1028, out.data_ptr(), 1, s)):
        assert call() == UNSUPPORTED
    assert fwd(cols=1028) == OK and bwd(cols=1028) == OK
    # misaligned pointers
    for call in (lambda: moments(a=mis), lambda: moments(b=mis), lambda: moments(parts_=parts.data_ptr() + 8), lambda: fstats(hp=mis),
                 lambda: fstats(hp=mis, sync=sync.data_ptr()), lambda: bstats(hp=mis), lambda: bstats(hp=mis, sync=sync.data_ptr()),
                 lambda: fwd(hp=mis), lambda: fwd(sc=v.data_ptr() + 4), lambda: bwd(hp=mis), lambda: bwd(cg=v.data_ptr() + 4),
                 lambda: lib.egc_column_sums_f32(mis, n, 1028, c, out.data_ptr(), 1, s)):
        assert call() == UNSUPPORTED
    # running statistics with fewer than 2 rows; only one of the two; a cumulative average without the count
    for sy in (None, sync.data_ptr()):
        assert fstats(nr=1, rm=_p(rm), rv=_p(rv), sync=sy) == INVALID
        assert fstats(rm=_p(rm), sync=sy) == INVALID and fstats(rv=_p(rv), sync=sy) == INVALID
        assert fstats(rm=_p(rm), rv=_p(rv), mom=-1.0, sync=sy) == INVALID
    assert ffin(nr=1, rm=_p(rm), rv=_p(rv)) == INVALID
    assert ffin(rm=_p(rm)) == INVALID and ffin(rv=_p(rv)) == INVALID
    assert ffin(rm=_p(rm), rv=_p(rv), mom=-1.0) == INVALID
    torch.cuda.synchronize()
    assert int(sync) == 0 and bool((rm == 0).all()) and bool((rv == 1).all())     # the running statistics were not touched


# ----------------------------------------------------------------------------------------------------------------------
# the block in training, every route, against float64

def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def _named(conv, bn):
    return list(conv.named_parameters()) + [("bn." + k, q) for k, q in bn.named_parameters()]


def _ref_block(conv, bn, x, ei, aggrs, H, B, rm, rv, step, relu_mask, keep=None, p=0.0, residual=True, n_valid=None):
    """The block in float64 with autograd: the conv of oracle/egc_torch_ref.py, F.batch_norm on batch statistics (running
    statistics in float64), the ReLU as the block decided it, the block's own dropout mask, the residual.  (A float64 ReLU
    of its own would decide the pre-activations within float32 rounding of 0 differently, on millions of them a few -- and
    each such element moves the gradient of its whole column of the BatchNorm.)"""
    from oracle import egc_torch_ref as tref
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in _named(conv, bn)}
    x64 = x.detach().double().requires_grad_(True)
    xv = x64 if n_valid is None else x64[:n_valid]
    h = tref.egconv_forward(xv, ei.cpu().numpy(), p64["bases_weight"], p64["comb_weight.weight"], p64["comb_weight.bias"], p64["bias"],
                            H, B, aggrs)
    h = F.batch_norm(h, rm, rv, p64["bn.weight"], p64["bn.bias"], True, bn.momentum if bn.momentum is not None else 1.0 / (step + 1),
                     bn.eps)
    h = h * relu_mask[:h.size(0)].double()
    if keep is not None:
        h = h * keep[:h.size(0)].double() / (1.0 - p)
    out = h + xv if residual else h
    return out, x64, p64


def _block_case(block, x, g, ei, aggrs, H, B, steps=2, expect=None, n_valid=None, residual=True, p=0.0):
    """Two training steps of the block against the float64 block: the output element by element (elementwise_excess at 1e-5),
    x.grad and every parameter gradient within the suite's 5e-4 scale-relative bound for gradients, the running statistics."""
    conv, bn = block.conv, block.bn
    rm = bn.running_mean.double().clone()
    rv = bn.running_var.double().clone()
    nv = x.shape[0] if n_valid is None else int(n_valid)
    go = torch.randn(x.shape[0], conv.out_channels, device=DEV)
    for step in range(steps):
        for q in block.parameters():
            q.grad = None
        ref_conv, ref_bn = copy.deepcopy(conv), copy.deepcopy(bn)
        xa = x.clone().requires_grad_(True)
        out = block(xa, g, n_valid=n_valid) if n_valid is not None else block(xa, g)
        if expect is not None:
            expect(out)
        keep = block.last_keep_mask if p > 0 else None
        # the block's ReLU decision from its output: act = out - x with the residual, out without (dropped elements: any)
        act = out.detach() - x if residual else out.detach()
        ref, x64, p64 = _ref_block(ref_conv, ref_bn, x, ei, aggrs, H, B, rm, rv, step, act > 0, keep, p, residual, n_valid and nv)
        (out[:nv] * go[:nv]).sum().backward()
        (ref * go[:nv].double()).sum().backward()
        assert elementwise_excess(out.detach()[:nv].cpu().numpy(), ref.detach().cpu().numpy(), 1e-5) <= 1.0, step
        if n_valid is not None:
            assert bool((out.detach()[nv:] == 0).all())
        assert _rel(xa.grad, x64.grad) <= 5e-4, ("x", step, _rel(xa.grad, x64.grad))
        for k, q in _named(conv, bn):
            assert _rel(q.grad, p64[k].grad) <= 5e-4, (k, step, _rel(q.grad, p64[k].grad))
        assert _rel(bn.running_mean, rm) <= 1e-6 and _rel(bn.running_var, rv) <= 1e-6, step
        assert int(bn.num_batches_tracked) == step + 1


def _conv(f_in, f_out, H, B, aggrs, seed):
    import egc_amd
    torch.manual_seed(seed)
    conv = egc_amd.EGConv(f_in, f_out, aggrs=aggrs, num_heads=H, num_bases=B)
    with torch.no_grad():
        conv.bias.normal_()
    return conv


def _bn(c, momentum=0.1):
    bn = torch.nn.BatchNorm1d(c, momentum=momentum)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
    return bn


AGGRS = ["sum", "mean", "max", "symnorm"]
# The float64 conv decides each max on its own float32 rounding of x W, the kernels on their split-precision GEMM's: an
# entry within that rounding of its row's maximum can send one row's gradient to another source.  At molhiv size the
# 224-wide and the widening batch-node blocks with all four aggregators measured x.grad 6e-4 and 4e-3 off float64, while
# the same blocks pass with max alone and with the other three, and the arxiv-sized and one-launch blocks pass with all
# four.  Those two take the three others; max keeps its bit-exact arg tests (test_backward_gpu.py).
NO_MAX = ["sum", "mean", "symnorm"]


def _node(name):
    def expect(out):
        assert out.grad_fn is not None and name in out.grad_fn.name(), out.grad_fn.name()
    return expect


def _not_native(out):
    assert "BlockTrainFn" not in out.grad_fn.name(), out.grad_fn.name()


def _molhiv_batch(n_graphs=2048):
    """A molhiv-sized batch (BASELINE config 3): (edge_index, n, ptr)."""
    from egc_amd.workloads import molecule_batch
    ei, n, batch = molecule_batch(n_graphs, seed=3)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(batch, minlength=n_graphs).cumsum(0)])
    return ei, n, ptr


def _graph_batch(ei, ptr):
    import egc_amd
    return egc_amd.GraphBatch(ei.to(DEV), ptr=ptr.to(DEV), max_nodes=int((ptr[1:] - ptr[:-1]).max()))


def test_block_one_launch_node_on_a_molhiv_sized_batch_against_float64():
    import egc_amd
    ei, n, ptr = _molhiv_batch()
    block = egc_amd.FusedEGCBlock(_conv(128, 128, 8, 4, AGGRS, 1), _bn(128, momentum=None)).to(DEV).train()
    x = torch.randn(n, 128, device=DEV)
    _block_case(block, x, _graph_batch(ei, ptr), ei, AGGRS, 8, 4, expect=_node("BatchBlockTrainFn"))


def test_block_csr_node_at_the_full_arxiv_size_against_float64():
    import egc_amd
    from egc_amd.workloads import arxiv_like
    ei, n = arxiv_like(seed=0)
    block = egc_amd.FusedEGCBlock(_conv(128, 128, 8, 4, AGGRS, 2), _bn(128)).to(DEV).train()
    x = torch.randn(n, 128, device=DEV)
    _block_case(block, x, ei.to(DEV), ei, AGGRS, 8, 4, expect=_node("CsrBlockTrainFn"))


def test_block_csr_node_at_224_h4_b4_against_float64():
    """The reference's molhiv EGC-M width (224 / H4 / B4, cg = 56) on a GraphBatch: outside the one-launch envelope."""
    import egc_amd
    ei, n, ptr = _molhiv_batch()
    block = egc_amd.FusedEGCBlock(_conv(224, 224, 4, 4, NO_MAX, 3), _bn(224)).to(DEV).train()
    x = torch.randn(n, 224, device=DEV)
    _block_case(block, x, _graph_batch(ei, ptr), ei, NO_MAX, 4, 4, expect=_node("CsrBlockTrainFn"))


def test_block_python_functions_with_dropout_against_float64():
    import egc_amd
    from egc_amd.workloads import zinc_like_batch
    _, ei, n, _ = zinc_like_batch(256, seed=4)
    p = 0.2
    block = egc_amd.FusedEGCBlock(_conv(128, 128, 8, 4, AGGRS, 4), _bn(128), dropout=p).to(DEV).train()
    x = torch.randn(n, 128, device=DEV)
    _block_case(block, x, ei.to(DEV), ei, AGGRS, 8, 4, expect=_not_native, p=p)


def test_block_python_functions_with_padded_rows_against_float64():
    """n_valid (eager): the real rows first, isolated padding rows behind them; statistics and gradients are those of the
    unpadded batch, the padding rows' output is 0."""
    import egc_amd
    from egc_amd.workloads import zinc_like_batch
    _, ei, n, _ = zinc_like_batch(64, seed=6)
    block = egc_amd.FusedEGCBlock(_conv(64, 64, 4, 4, AGGRS, 6), _bn(64, momentum=None)).to(DEV).train()
    x = torch.zeros(n + 37, 64, device=DEV)
    x[:n] = torch.randn(n, 64, device=DEV)
    n_valid = torch.tensor(n, dtype=torch.int64, device=DEV)
    _block_case(block, x, ei.to(DEV), ei, AGGRS, 4, 4, expect=_not_native, n_valid=n_valid)


# ----------------------------------------------------------------------------------------------------------------------
# the compiled block paths decline modules whose widths do not match

@pytest.mark.parametrize("as_batch", [True, False])
def test_wrong_width_residual_block_raises_like_the_plain_composition(as_batch):
    import egc_amd
    ei, n, ptr = _molhiv_batch(512)
    g = _graph_batch(ei, ptr) if as_batch else ei.to(DEV)
    block = egc_amd.FusedEGCBlock(_conv(64, 128, 8, 4, AGGRS, 7), _bn(128), residual=True).to(DEV).train()
    x = torch.randn(n, 64, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError) as plain:
        block._plain(x, g)
    with pytest.raises(RuntimeError) as fused:
        block(x, g)
    assert str(fused.value) == str(plain.value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("as_batch", [True, False])
def test_widening_block_without_residual_runs_a_compiled_node_against_float64(as_batch):
    import egc_amd
    ei, n, ptr = _molhiv_batch()
    g = _graph_batch(ei, ptr) if as_batch else ei.to(DEV)
    aggrs = NO_MAX if as_batch else AGGRS
    block = egc_amd.FusedEGCBlock(_conv(64, 128, 8, 4, aggrs, 8), _bn(128), residual=False).to(DEV).train()
    x = torch.randn(n, 64, device=DEV)
    _block_case(block, x, g, ei, aggrs, 8, 4, residual=False, expect=_node("BatchBlockTrainFn" if as_batch else "CsrBlockTrainFn"))


class _Recorder:
    """Stands in for the compiled binding: records the arguments of one block op, then calls it."""
    def __init__(self, ops, name):
        self._ops, self._name, self.calls = ops, name, []

    def __getattr__(self, k):
        f = getattr(self._ops, k)
        if k != self._name:
            return f

        def rec(*a):
            self.calls.append(a)
            return f(*a)
        return rec


@pytest.mark.parametrize("op", ["batch_block_train", "csr_block_train"])
def test_direct_op_call_with_wrong_sized_operands_raises(op, monkeypatch):
    """A direct call through torch.ops with a wrong-sized x, gamma or beta: a TORCH_CHECK before anything is launched."""
    import egc_amd
    from egc_amd import _native
    ei, n, ptr = _molhiv_batch(512)
    c = 128 if op == "batch_block_train" else 224
    block = egc_amd.FusedEGCBlock(_conv(c, c, 8 if c == 128 else 4, 4, AGGRS, 9), _bn(c)).to(DEV).train()
    rec = _Recorder(_native.ops(), op)
    monkeypatch.setattr(_native, "ops", lambda: rec)
    x = torch.randn(n, c, device=DEV, requires_grad=True)
    block(x, _graph_batch(ei, ptr))
    torch.cuda.synchronize()
    assert len(rec.calls) == 1
    args = rec.calls[0]
    fn = getattr(torch.ops.egc_amd_native, op)
    tracked = int(block.bn.num_batches_tracked)
    for i, bad in ((0, torch.randn(n, c - 4, device=DEV)), (0, torch.randn(n, c + 4, device=DEV)),
                   (5, torch.ones(c - 4, device=DEV)), (5, torch.ones(c + 4, device=DEV)), (6, torch.zeros(c // 2, device=DEV))):
        a = list(args)
        a[i] = bad
        with pytest.raises(RuntimeError, match="egc_amd"):
            fn(*a)
    torch.cuda.synchronize()
    assert int(block.bn.num_batches_tracked) == tracked       # nothing ran
