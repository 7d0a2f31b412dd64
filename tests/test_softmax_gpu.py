"""The output head and loss on the device (egc_amd/csrc/egc_softmax.hip) against the float64 reference of softmax_ref.py.

Accuracy.  With u = 2^-24 and C = n_classes every log-probability is held to

    |err| <= u (|logp| + |lse| + 4 ln C + 3) + (C - 1) u

The kernel forms m = max_c x_c (exact), s = sum_c exp(x_c - m), lse = m + log s and logp = x - lse, one float32 rounding per
operation.  x_c - m rounds with relative error u, which exp turns into a relative error u |x_c - m| of that term; weighted
by the terms' shares of s this is u times the softmax-weighted mean of |x - m|, at most u ln C (the weights are
exp(-(m - x_c)) / s and -sum p log p <= ln C bounds it together with log s <= ln C).  expf and logf stay within 3 ulp each
(the OpenCL full-profile limit, which the device library is inside): 3u relative on every term of s, and 3u |log s| <=
3u ln C on the logarithm.  The C positive terms add up with a relative error of at most gamma_{C-1} ~ (C - 1) u in ANY
order.  A relative error of s is an absolute error of log s.  The last two roundings are u |lse| for m + log s and
u |logp| for x - lse.  Sum: u (ln C + 3) + (C - 1) u + 3u ln C + u |lse| + u |logp|, which is the bound above.

The loss and both gradients get bounds derived in the same way, written next to the reference (softmax_ref.loss_bound,
nll_grad_bound, log_softmax_grad_bound); the loss uses gamma_k with k the longest add chain of the documented order
(softmax_ref.loss_chain), not gamma_{M-1}.

Structure is checked exactly: zeros in the padding columns and on unselected rows, the first maximal column as arg-max,
duplicates counted as often as they occur, two runs equal to the bit, out-of-range labels and indices contributing nothing
and raising at the deferred check.  The padding columns of every input hold NaN: they are never read."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import egc_amd
import softmax_ref as ref
from softmax_ref import KINDS, logits as _logits
from egc_amd.graph import _IndexFlag

pytestmark = pytest.mark.gpu

SHAPES = [(40, 40), (10, 10), (349, 352), (349, 349), (1024, 1024), (1, 1), (7, 9)]
INDEX_MODES = ["none", "all", "p54", "p85"]


def _dev():
    return torch.device("cuda:0")


def _index(mode, n, seed):
    if mode == "none":
        return None
    if mode == "all":
        return torch.arange(n)
    g = torch.Generator().manual_seed(seed)
    keep = int(round(n * (0.54 if mode == "p54" else 0.85)))
    return torch.randperm(n, generator=g)[:keep]


def _flag_clear():
    torch.cuda.synchronize()
    try:
        _IndexFlag.poll()
    except RuntimeError:
        pass


# 1. log-softmax forward: accuracy of every element, lse, arg-max
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c,ld", SHAPES)
def test_log_softmax_every_element_within_the_float32_bound(c, ld, kind):
    x = _logits(1000, c, ld, kind, seed=c + ld)
    out, arg = egc_amd.log_softmax(x.to(_dev()), num_classes=c, return_argmax=True)
    assert out.shape == (1000, c) and out.is_contiguous() and arg.dtype == torch.int64
    want, lse = ref.log_softmax(x, c)
    err = (out.cpu().double() - want).abs()
    bound = ref.logp_bound(want, lse, c)
    worst = float((err / bound).max())
    print(f"log_softmax C={c} ld={ld} {kind}: max err / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), worst
    assert torch.equal(arg.cpu(), ref.first_argmax(x, c))


@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("c,ld", SHAPES)
def test_log_softmax_row_counts(c, ld, n):
    x = _logits(n, c, ld, "mixed", seed=n + c)
    out, arg = egc_amd.log_softmax(x.to(_dev()), num_classes=c, return_argmax=True)
    want, lse = ref.log_softmax(x, c)
    assert out.shape == (n, c) and arg.shape == (n,)
    assert bool(((out.cpu().double() - want).abs() <= ref.logp_bound(want, lse, c)).all())
    assert torch.equal(arg.cpu(), ref.first_argmax(x, c))


@pytest.mark.parametrize("c,ld", SHAPES)
def test_argmax_is_the_first_maximal_column_on_ties(c, ld):
    g = torch.Generator().manual_seed(c)
    x = torch.randint(0, 3, (1000, ld), generator=g).float()      # integer-valued rows: ties everywhere
    x[:, c:] = float("nan")
    _, arg = egc_amd.log_softmax(x.to(_dev()), num_classes=c, return_argmax=True)
    assert torch.equal(arg.cpu(), ref.first_argmax(x, c))


# 2. log-softmax backward
@pytest.mark.parametrize("c,ld", SHAPES)
def test_log_softmax_backward_within_bound_and_zero_padding(c, ld):
    dev = _dev()
    x = _logits(1000, c, ld, "mixed", seed=7 * c).to(dev).requires_grad_(True)
    out = egc_amd.log_softmax(x, num_classes=c)
    g = torch.randn(1000, c, generator=torch.Generator().manual_seed(c))
    out.backward(g.to(dev))
    dx = x.grad
    assert dx.shape == (1000, ld)
    assert not dx[:, c:].any()                                         # exactly zero, not NaN from the padding
    o = out.detach().cpu()
    want = ref.log_softmax_backward(g, o, ld)
    err = (dx.cpu().double() - want)[:, :c].abs()
    bound = ref.log_softmax_grad_bound(g, o, c)
    print(f"log_softmax backward C={c} ld={ld}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    x.grad = None
    egc_amd.log_softmax(x, num_classes=c).backward(g.to(dev))
    assert torch.equal(x.grad, dx)


# 3. fused NLL: loss, gradient, structure, determinism
def _check_nll(x, y, idx, c, reduction, g=1.0, sel=None, place=None):
    """Runs nll_log_softmax on the device twice and holds loss and gradient to the float64 reference's bounds.  `place`:
    how the CPU logits reach the device (default: a plain copy)."""
    dev = _dev()
    n, ld = x.shape
    xd = (x.to(dev) if place is None else place(x)).requires_grad_(True)
    yd = y.to(dev)
    index = sel if sel is not None else (idx.to(dev) if idx is not None else None)
    mean = reduction == "mean"
    results = []
    for _ in range(2):
        xd.grad = None
        loss = egc_amd.nll_log_softmax(xd, yd, index, num_classes=c, reduction=reduction)
        (loss * g).backward()
        results.append((loss.detach().clone(), xd.grad.clone()))
    assert torch.equal(results[0][0], results[1][0]) or bool(torch.isnan(results[0][0]) & torch.isnan(results[1][0]))
    assert torch.equal(results[0][1], results[1][1])
    loss, dx = results[0][0].cpu(), results[0][1].cpu()
    assert loss.shape == () and dx.shape == (n, ld)
    cnt = ref.counts(idx, n)
    m = int(cnt.sum())
    if m == 0:
        assert torch.isnan(loss) if mean else float(loss) == 0.0
        assert not dx.any()
        return loss, dx
    want, picked = ref.nll_forward(x, y, cnt, c, mean)
    _, lse = ref.log_softmax(x, c)
    lb = ref.loss_bound(picked, lse, cnt, n, c, mean)
    print(f"nll C={c} ld={ld} N={n} M={m} {reduction}: loss {float(loss):.7g} ref {float(want):.10g} "
          f"err {abs(float(loss) - float(want)):.3e} bound {lb:.3e} (chain {ref.loss_chain(n, c)})")
    assert abs(float(loss) - float(want)) <= lb
    want_dx = ref.nll_backward(g, x, y, cnt, c, mean)
    err = (dx.double() - want_dx).abs()
    bound = ref.nll_grad_bound(want_dx, x, y, cnt, g, c, mean)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert not dx[:, c:].any()                                         # padding columns: exactly zero
    assert not dx[cnt == 0].any()                                      # unselected rows: exactly zero
    return loss, dx


@pytest.mark.parametrize("mode", INDEX_MODES)
@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("c,ld", SHAPES)
def test_nll_loss_and_gradient(c, ld, n, mode):
    x = _logits(n, c, ld, "mixed", seed=n + 3 * c)
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(c + n))
    _check_nll(x, y, _index(mode, n, seed=c), c, "mean", g=1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c,ld", [(349, 352), (40, 40), (10, 10)])
def test_nll_sum_reduction_and_an_upstream_gradient(c, ld, kind):
    x = _logits(1000, c, ld, kind, seed=5 * c)
    y = torch.randint(0, c, (1000,), generator=torch.Generator().manual_seed(c))
    _check_nll(x, y, _index("p54", 1000, seed=1), c, "sum", g=-2.5)
    _check_nll(x, y, _index("p85", 1000, seed=2), c, "mean", g=3.0)


def test_nll_equals_torchs_composition_and_cross_entropy():
    dev = _dev()
    torch.manual_seed(0)
    x = torch.randn(1000, 352, device=dev)
    y = torch.randint(0, 349, (1000,), device=dev)
    idx = torch.randperm(1000, device=dev)[:600]
    for red in ("mean", "sum"):
        want = F.nll_loss(x[:, :349].log_softmax(-1)[idx], y[idx], reduction=red)
        got = egc_amd.nll_log_softmax(x, y, idx, num_classes=349, reduction=red)
        assert torch.allclose(got, want, rtol=1e-5, atol=0)
    b, t = torch.randn(128, 10, device=dev), torch.randint(0, 10, (128,), device=dev)
    assert torch.allclose(egc_amd.cross_entropy(b, t), F.cross_entropy(b, t), rtol=1e-5, atol=0)


def test_duplicate_indices_count_twice():
    dev = _dev()
    c, ld, n = 40, 40, 300
    x = _logits(n, c, ld, "randn10", seed=1)
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(2))
    idx = torch.tensor([5, 17, 5, 200, 5, 17])
    sel = egc_amd.RowSelection(idx.to(dev), n)
    assert sel.cnt.cpu().tolist() == ref.counts(idx, n).tolist() and sel.M.cpu().tolist() == [6]
    _, dx = _check_nll(x, y, idx, c, "mean", sel=sel)
    _, dx_plain = _check_nll(x, y, idx, c, "mean")                      # a plain tensor builds the same selection
    assert torch.equal(dx, dx_plain)
    once = _check_nll(x, y, torch.tensor([5, 17, 200]), c, "sum")[1]
    many = _check_nll(x, y, idx, c, "sum")[1]
    assert torch.equal(many[5], 3.0 * once[5]) and torch.equal(many[17], 2.0 * once[17]) and torch.equal(many[200], once[200])


# 4. out-of-range labels and indices: nothing contributed, the deferred check raises, never a fault
@pytest.mark.parametrize("bad_label", [-1, 349, 2 ** 40])
def test_label_out_of_range_contributes_nothing_and_raises_later(bad_label):
    dev = _dev()
    _flag_clear()
    c, ld, n = 349, 352, 500
    x = _logits(n, c, ld, "randn10", seed=3)
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(4))
    y[8] = bad_label            # selected: reported
    idx = torch.arange(0, n, 2)
    y_ok = y.clone()
    xd = x.to(dev).requires_grad_(True)
    loss = egc_amd.nll_log_softmax(xd, y.to(dev), idx.to(dev), num_classes=c)
    loss.backward()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="earlier call"):
        _IndexFlag.poll()
    cnt = ref.counts(idx, n)
    y_ok[8] = 0
    want, picked = ref.nll_forward(x, y, cnt, c, True)                  # the reference skips the label too; M counts the row
    _, lse = ref.log_softmax(x, c)
    assert abs(float(loss.detach()) - float(want)) <= ref.loss_bound(picked, lse, cnt, n, c, True)
    assert not xd.grad[8].any() and bool(xd.grad[6].any())
    # a bad label on an UNSELECTED row is nobody's business
    y2 = y_ok.clone()
    y2[9] = bad_label
    egc_amd.nll_log_softmax(xd, y2.to(dev), idx.to(dev), num_classes=c).backward()
    torch.cuda.synchronize()
    _IndexFlag.poll()


def test_index_out_of_range_is_not_counted_and_raises_later():
    dev = _dev()
    _flag_clear()
    n = 100
    idx = torch.tensor([3, n, -1, 3, 2 ** 40, 99])
    sel = egc_amd.RowSelection(idx.to(dev), n)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="earlier call"):
        _IndexFlag.poll()
    assert sel.cnt.cpu().tolist() == ref.counts(idx, n).tolist() and sel.M.cpu().tolist() == [3]
    x = _logits(n, 10, 10, "randn1", seed=0)
    y = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(1))
    _check_nll(x, y, idx, 10, "mean", sel=sel)


# 5. beyond the kernel's limit: torch's operators, same answer
def test_1025_classes_take_the_fallback_and_match():
    dev = _dev()
    torch.manual_seed(0)
    x = torch.randn(200, 1025, device=dev, requires_grad=True)
    y = torch.randint(0, 1025, (200,), device=dev)
    idx = torch.randperm(200, device=dev)[:150]
    loss = egc_amd.nll_log_softmax(x, y, idx)
    want = F.nll_loss(x.log_softmax(-1)[idx], y[idx])
    assert torch.equal(loss, want)
    out, arg = egc_amd.log_softmax(x, return_argmax=True)
    assert torch.equal(out, x.log_softmax(-1)) and torch.equal(arg, x.argmax(-1))
    loss.backward()
    assert x.grad.shape == x.shape
    from egc_amd import _C
    assert _C.load().egc_log_softmax_forward_f32(x.data_ptr(), 200, 1025, 1025, x.data_ptr(), None, None, None) == 4   # UNSUPPORTED


# 6. the full mag-sized case
def test_mag_sized_case():
    """N = 736,389 rows of 349 classes in a 352-wide row, about 630 k selected: every log-probability, the arg-max, the
    loss and every gradient element against float64 (the reference runs in row blocks on the CPU)."""
    dev = _dev()
    n, c, ld, m = 736_389, 349, 352, 629_571
    torch.manual_seed(11)
    xd = torch.randn(n, ld, device=dev) * 10.0
    xd[:, c:] = float("nan")
    yd = torch.randint(0, c, (n,), device=dev)
    idx = torch.randperm(n, device=dev)[:m]
    sel = egc_amd.RowSelection(idx, n)
    with torch.no_grad():
        out, arg = egc_amd.log_softmax(xd, num_classes=c, return_argmax=True)
    xd.requires_grad_(True)
    loss = egc_amd.nll_log_softmax(xd, yd, sel, num_classes=c)
    loss.backward()
    loss2 = egc_amd.nll_log_softmax(xd.detach(), yd, sel, num_classes=c)
    assert torch.equal(loss.detach(), loss2)
    x, y, dx, out, arg = xd.detach().cpu(), yd.cpu(), xd.grad.cpu(), out.cpu(), arg.cpu()
    cnt = ref.counts(idx.cpu(), n)
    assert int(cnt.sum()) == m and sel.M.cpu().tolist() == [m]
    total, abs_total, term_total = 0.0, 0.0, 0.0
    for r0 in range(0, n, 32768):
        r = slice(r0, min(r0 + 32768, n))
        want, lse = ref.log_softmax(x[r], c)
        assert bool(((out[r].double() - want).abs() <= ref.logp_bound(want, lse, c)).all()), r0
        assert torch.equal(arg[r], ref.first_argmax(x[r], c)), r0
        cb = cnt[r].double()
        picked = want[torch.arange(want.size(0)), y[r]]
        total += float((cb * picked).sum())
        abs_total += float((cb * picked.abs()).sum())
        term_total += float((cb * (ref.U * picked.abs() + ref.lse_bound(lse, c))).sum())
        # the block's gradient: the global M enters through g = 1 / M with the 'sum' form of the reference
        want_dx = ref.nll_backward(1.0 / m, x[r], y[r], cnt[r], c, False)
        bound = ref.nll_grad_bound(want_dx, x[r], y[r], cnt[r], 1.0 / m, c, False) + ref.U * want_dx.abs()   # (+ 1 / M rounded)
        assert bool(((dx[r].double() - want_dx).abs() <= bound).all()), r0
        assert not dx[r][:, c:].any() and not dx[r][cnt[r] == 0].any()
    want_loss = -total / m
    k = ref.loss_chain(n, c)
    lb = 1.01 * (term_total + (k + 1) * ref.U * abs_total) / m + ref.U * abs(want_loss)
    print(f"mag-sized: loss {float(loss):.8g} ref {want_loss:.12g} err {abs(float(loss) - want_loss):.3e} bound {lb:.3e} chain {k}")
    assert abs(float(loss) - want_loss) <= lb


# 7. inside a recorded step
@pytest.mark.parametrize("prebuilt", [True, False])
def test_nll_inside_a_recorded_step(prebuilt):
    """loss = nll_log_softmax(Linear(x)) recorded by egc_amd.GraphedStep: each replay on fresh contents of the static buffers
    gives the eager step's loss and gradients bit for bit (the selection is built inside the step when a plain index
    tensor is passed)."""
    dev = _dev()
    n, hidden, c, ld = 3000, 64, 349, 352
    torch.manual_seed(0)
    lin = nn.Linear(hidden, ld).to(dev)
    x = torch.randn(n, hidden, device=dev).requires_grad_(True)
    y = torch.randint(0, c, (n,), device=dev)
    idx = torch.randperm(n, device=dev)[:1800]
    index = egc_amd.RowSelection(idx, n) if prebuilt else idx
    leaves = list(lin.parameters()) + [x]
    kept = {}

    def step():
        kept["loss"] = egc_amd.nll_log_softmax(lin(x), y, index, num_classes=c)
        kept["loss"].backward()

    graphed = egc_amd.GraphedStep(step, params=leaves)
    recorded = kept["loss"]
    for trial in range(3):
        with torch.no_grad():
            x.copy_(torch.randn(n, hidden, device=dev))
            y.copy_(torch.randint(0, c, (n,), device=dev))
        graphed()
        got_loss, got = recorded.detach().clone(), [p.grad.detach().clone() for p in leaves]
        held = [p.grad for p in leaves]
        for p in leaves:
            p.grad = None
        step()
        assert torch.equal(got_loss, kept["loss"].detach()), trial
        for p, a in zip(leaves, got):
            assert torch.equal(a, p.grad), trial
        for p, h in zip(leaves, held):
            p.grad = h


# 8. the mag net of tests/callers.py with the fused loss behind its last layer
@pytest.mark.parametrize("name", ["net_mag_mean", "net_mag_symnorm"])
def test_mag_net_parameter_gradients_match_the_torch_composition(name):
    """MagNetLike (imported, not edited) ends in [:, :349].log_softmax(-1); the torch composition adds [idx] and F.nll_loss.
    Feeding the last layer's full-width output to nll_log_softmax(x, y, idx, num_classes=349) instead gives parameter
    gradients within the net fixtures' bounds (test_nets_golden.py: max(1e-5, 5 x the reference's own float32-to-float64
    distance) relative to max(1e-2 x the net's gradient scale, the parameter's largest gradient))."""
    import test_nets_golden as nets
    z, meta = nets._load(name)
    dev = _dev()
    n = meta["n"]
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, meta["out_true"], (n,), generator=g).to(dev)
    idx = torch.randperm(n, generator=g)[:int(0.6 * n)].to(dev)
    grads = {}
    for form in ("torch", "fused"):
        net = nets._build(meta)
        net.load_state_dict(nets._state(z), strict=True)
        net = net.to(dev).train()
        seen = []

        def conv_fn(conv, x, adj_t):
            seen.append(conv(x, adj_t))
            return seen[-1]
        out, _ = nets._call(net, meta, z, dev, torch.float32, True, conv_fn=conv_fn)
        if form == "torch":
            loss = F.nll_loss(out[idx], y[idx])
        else:
            assert seen[-1].shape == (n, 352)
            loss = egc_amd.nll_log_softmax(seen[-1], y, idx, num_classes=meta["out_true"])
        loss.backward()
        grads[form] = ({k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}, float(loss))
    assert abs(grads["torch"][1] - grads["fused"][1]) <= 1e-5 * abs(grads["torch"][1])
    gscale = max(float(v.abs().max()) for v in grads["torch"][0].values())
    for k, want in grads["torch"][0].items():
        bound = max(1e-5, 5.0 * meta["f32_vs_f64_grad"][k])
        denom = max(1e-2 * gscale, float(want.abs().max()))
        err = float((grads["fused"][0][k] - want).abs().max() / denom)
        assert err <= bound, (k, err, bound)
