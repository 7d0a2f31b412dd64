"""The token head on the device (egc_amd/csrc/egc_token_head.hip) against the float64 reference of token_head_ref.py, whose
docstring derives every bound used here (logit: gamma_{K+1} (sum |x w| + |b|); lse, loss and the three gradients from it).

Shapes: in_features 4, 36, 300, 304, 384 (one k tile, a part tile, the two ogbg-code widths -- 300 is no multiple of 16 --
and the widest); vocabularies 1, 7, one below / at / above the slab width and 5002; 1, 5 and 8 positions; 0, 1, 15, 17, 128
and 200 rows (one past a 16-row MFMA tile; 200 = two row blocks, where d_W and d_b are added across blocks).  Structure is
checked exactly: ties go to the smaller column, two runs are equal to the bit, a gradient that is not asked for is None,
labels out of range contribute nothing and raise at the deferred check, and no [G, V] array is allocated."""
import gc

import pytest
import torch
import torch.nn as nn

import egc_amd
from egc_amd import _C, _token_head
from egc_amd.graph import _IndexFlag
import token_head_ref as ref

pytestmark = pytest.mark.gpu

SLAB = _C.TOKEN_HEAD_SLAB
# (G, K, V, T, kind): a sparse product of the sizes above
CASES = [(128, 304, 5002, 5, "mixed"), (128, 300, 5002, 5, "large"), (17, 300, SLAB + 1, 1, "large"),
         (15, 36, SLAB - 1, 8, "mixed"), (1, 4, 1, 1, "mixed"), (200, 384, SLAB, 5, "mixed"), (200, 36, 7, 8, "large"),
         (17, 384, 5002, 1, "mixed"), (1, 304, SLAB + 1, 5, "large"), (15, 4, 7, 5, "large")]
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _case(g, k, v, t, kind):
    """(inputs, float64 reference) of a case, computed once and never written to."""
    key = (g, k, v, t, kind)
    if key not in _CACHE:
        inputs = ref.make_inputs(g, k, v, t, kind, seed=g + k + v + t)
        _CACHE[key] = (inputs, ref.reference(*inputs))
    return _CACHE[key]


def _flag_clear():
    torch.cuda.synchronize()
    try:
        _IndexFlag.poll()
    except RuntimeError:
        pass


def _leaves(x, ws, bs, dev, x_grad=True, p_grad=True):
    xd = x.to(dev).requires_grad_(x_grad)
    wd = [w.to(dev).requires_grad_(p_grad) for w in ws]
    bd = [b.to(dev).requires_grad_(p_grad) for b in bs]
    return xd, wd, bd


def _run(x, ws, bs, y, factor=None):
    dev = _dev()
    xd, wd, bd = _leaves(x, ws, bs, dev)
    loss = egc_amd.token_head_loss(xd, wd, bd, y.to(dev))
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), xd.grad, [w.grad for w in wd], [b.grad for b in bd]


def _within(name, got, want, bound):
    err = (got.cpu().double() - want).abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"  {name}: max err / bound = {worst:.3f}, max err = {float(err.max()) if err.numel() else 0.0:.3e}")
    assert bool((err <= bound).all()), (name, worst)


def _check_gradients(r, dx, dw, db):
    if dx is not None:
        _within("dx", dx, r["dx"], r["dx_bound"])
    for i in range(len(dw)):
        _within(f"dW[{i}]", dw[i], r["dw"][i], r["dw_bound"][i])
        _within(f"db[{i}]", db[i], r["db"][i], r["db_bound"][i])


# 1. loss, lse and every gradient at every shape; two runs equal to the bit
@pytest.mark.parametrize("g,k,v,t,kind", CASES)
def test_loss_lse_and_gradients_within_the_float32_bounds(g, k, v, t, kind):
    (x, ws, bs, y), r = _case(g, k, v, t, kind)
    print(f"token head G={g} K={k} V={v} T={t} {kind}")
    loss, dx, dw, db = _run(x, ws, bs, y)
    loss2, dx2, dw2, db2 = _run(x, ws, bs, y)
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2)
    assert all(torch.equal(a, b) for a, b in zip(dw + db, dw2 + db2))
    assert loss.shape == () and dx.shape == (g, k) and dw[0].shape == (v, k) and db[0].shape == (v,)
    err = abs(float(loss) - r["loss"])
    print(f"  loss: err / bound = {err / r['loss_bound']:.3f}, err = {err:.3e}")
    assert err <= r["loss_bound"]
    dev = _dev()
    _, lse, _ = _token_head.head_forward(x.to(dev), [w.to(dev) for w in ws], [b.to(dev) for b in bs], y.to(dev), False)
    assert lse.shape == (g, t)
    _within("lse", lse, r["lse"], r["lse_bound"])
    _check_gradients(r, dx, dw, db)


def test_no_rows_give_nan_and_zero_parameter_gradients():
    x, ws, bs, y = ref.make_inputs(0, 304, 7, 5, "mixed", seed=1)
    loss, dx, dw, db = _run(x, ws, bs, y)
    assert bool(torch.isnan(loss)) and dx.shape == (0, 304)
    assert all(not bool(p.any()) for p in dw + db)
    assert egc_amd.token_head_argmax(x.to(_dev()), [w.to(_dev()) for w in ws], [b.to(_dev()) for b in bs]).shape == (0, 5)


# 2. arg-max
@pytest.mark.parametrize("g,k,v,t,kind", CASES)
def test_argmax_is_a_column_within_twice_the_logit_bound_of_the_maximum(g, k, v, t, kind):
    (x, ws, bs, _), r = _case(g, k, v, t, kind)
    dev = _dev()
    head = egc_amd.TokenHead(k, v, t).to(dev)
    with torch.no_grad():
        for p, w, b in zip(head, ws, bs):
            p.weight.copy_(w)
            p.bias.copy_(b)
    pred = head.predict(x.to(dev))
    assert pred.dtype == torch.int64 and pred.shape == (g, t)
    pred = pred.cpu()
    assert bool(((pred >= 0) & (pred < v)).all())
    logits = r["logits"].permute(1, 0, 2)                                     # [G, T, V]
    picked = logits.gather(2, pred[..., None]).squeeze(2)
    gap = logits.max(dim=2).values - picked
    exact = float((pred == ref.first_argmax(r["logits"])).double().mean())
    print(f"argmax G={g} K={k} V={v} T={t} {kind}: {exact:.4f} equal to the float64 arg-max, largest gap {float(gap.max()):.3e}")
    assert bool((gap <= 2.0 * r["logit_bound_row"]).all())


@pytest.mark.parametrize("second", ["same_slab", "later_slab"])
def test_argmax_ties_go_to_the_smaller_column_exactly(second):
    g, k, v, t = 17, 36, 3 * SLAB + 5, 2
    x, ws, bs, _ = ref.make_inputs(g, k, v, t, "mixed", seed=5)
    first = SLAB + 3
    other = first + 7 if second == "same_slab" else 2 * SLAB + 9
    for w, b in zip(ws, bs):          # the pair is every row's maximum by a wide margin: both logits are the bias itself
        w[first] = 0.0
        b[first] = 1000.0
        w[other] = w[first]
        b[other] = b[first]
    dev = _dev()
    pred = egc_amd.token_head_argmax(x.to(dev), [w.to(dev) for w in ws], [b.to(dev) for b in bs]).cpu()
    assert bool((pred == first).all()), pred
    # ... and with weights that matter: the duplicated row is a real one, shifted up through the bias
    x, ws, bs, _ = ref.make_inputs(g, k, v, t, "mixed", seed=6)
    for w, b in zip(ws, bs):
        b[first] = 1000.0
        w[other] = w[first]
        b[other] = b[first]
    pred = egc_amd.token_head_argmax(x.to(dev), [w.to(dev) for w in ws], [b.to(dev) for b in bs]).cpu()
    assert bool((pred == first).all()), pred


# 3. structure
def test_an_upstream_factor_scales_the_gradients_within_bound():
    x, ws, bs, y = ref.make_inputs(17, 36, SLAB + 1, 5, "mixed", seed=3)
    r = ref.reference(x, ws, bs, y, grad_loss=3.0)
    loss, dx, dw, db = _run(x, ws, bs, y, factor=3.0)
    assert abs(float(loss) - r["loss"]) <= r["loss_bound"]
    _check_gradients(r, dx, dw, db)


def test_gradients_that_are_not_required_stay_none():
    x, ws, bs, y = ref.make_inputs(17, 36, SLAB + 1, 5, "mixed", seed=4)
    r = ref.reference(x, ws, bs, y)
    dev = _dev()
    xd, wd, bd = _leaves(x, ws, bs, dev, x_grad=True, p_grad=False)
    egc_amd.token_head_loss(xd, wd, bd, y.to(dev)).backward()
    assert all(p.grad is None for p in wd + bd)
    _within("dx alone", xd.grad, r["dx"], r["dx_bound"])
    xd, wd, bd = _leaves(x, ws, bs, dev, x_grad=False, p_grad=True)
    egc_amd.token_head_loss(xd, wd, bd, y.to(dev)).backward()
    assert xd.grad is None
    _check_gradients(r, None, [w.grad for w in wd], [b.grad for b in bd])
    xd, wd, bd = _leaves(x, ws, bs, dev, x_grad=False, p_grad=False)
    loss = egc_amd.token_head_loss(xd, wd, bd, y.to(dev))
    assert not loss.requires_grad and abs(float(loss) - r["loss"]) <= r["loss_bound"]


def test_labels_out_of_range_contribute_nothing_and_raise_at_the_deferred_check():
    g, k, v, t = 17, 36, SLAB + 1, 5
    x, ws, bs, y = ref.make_inputs(g, k, v, t, "mixed", seed=8)
    y[3, 1] = v
    y[9, 4] = -1
    y[16, 0] = 2 ** 40
    r = ref.reference(x, ws, bs, y)            # the reference drops those terms (and still divides by G T)
    _flag_clear()
    loss, dx, dw, db = _run(x, ws, bs, y)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="out of range"):
        _IndexFlag.poll()
    assert abs(float(loss) - r["loss"]) <= r["loss_bound"]
    _check_gradients(r, dx, dw, db)
    _flag_clear()


@pytest.mark.parametrize("k,t", [(302, 5), (304, 9)])
def test_shapes_outside_the_envelope_take_torch_and_match_it(k, t):
    g, v = 17, SLAB + 1
    x, ws, bs, y = ref.make_inputs(g, k, v, t, "mixed", seed=9)
    dev = _dev()
    xd, wd, bd = _leaves(x, ws, bs, dev)
    assert not _token_head.token_head_supported(xd, wd, bd)
    loss = egc_amd.token_head_loss(xd, wd, bd, y.to(dev))
    loss.backward()
    xt, wt, bt = _leaves(x, ws, bs, dev)
    want = ref.torch_composition(xt, wt, bt, y.to(dev))
    want.backward()
    assert torch.equal(loss, want) and torch.equal(xd.grad, xt.grad)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(wd + bd, wt + bt))
    pred = egc_amd.token_head_argmax(xd.detach(), wd, bd)
    assert torch.equal(pred, torch.stack([torch.argmax(nn.functional.linear(xt, w, b), dim=1) for w, b in zip(wt, bt)], dim=1))


# 4. inside a recorded step
def test_loss_inside_a_recorded_step():
    """TokenHead.loss + backward recorded by egc_amd.GraphedStep (one stream, no parallel branches): each replay on fresh
    contents of the static buffers gives the eager step's loss and gradients bit for bit."""
    dev = _dev()
    g, k, v, t = 128, 304, 5002, 5
    torch.manual_seed(0)
    head = egc_amd.TokenHead(k, v, t).to(dev)
    x = torch.randn(g, k, device=dev).requires_grad_(True)
    y = torch.randint(0, v, (g, t), device=dev)
    leaves = list(head.parameters()) + [x]
    kept = {}

    def step():
        kept["loss"] = head.loss(x, y)
        kept["loss"].backward()

    graphed = egc_amd.GraphedStep(step, params=leaves)
    recorded = kept["loss"]
    for trial in range(3):
        with torch.no_grad():
            x.copy_(torch.randn(g, k, device=dev))
            y.copy_(torch.randint(0, v, (g, t), device=dev))
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


# 5. behind the readout
def test_parameter_gradients_behind_global_mean_pool_match_the_composition():
    """nodes -> global_mean_pool -> TokenHead.loss at G = 128, K = 304: the head's parameter gradients against the float64
    composition on the pooled rows the device produced, and the nodes' gradient against d_x pushed through the mean
    (d node = d_x[graph] / count: one more rounding of the quotient)."""
    dev = _dev()
    g, k, v, t = 128, 304, 5002, 5
    gen = torch.Generator().manual_seed(11)
    counts = torch.randint(1, 40, (g,), generator=gen)
    batch = torch.repeat_interleave(torch.arange(g), counts)
    nodes = torch.randn(int(counts.sum()), k, generator=gen)
    _, ws, bs, y = ref.make_inputs(g, k, v, t, "mixed", seed=12)
    head = egc_amd.TokenHead(k, v, t).to(dev)
    with torch.no_grad():
        for p, w, b in zip(head, ws, bs):
            p.weight.copy_(w)
            p.bias.copy_(b)
    nd = nodes.to(dev).requires_grad_(True)
    pooled = egc_amd.global_mean_pool(nd, batch.to(dev), size=g)
    loss = head.loss(pooled, y.to(dev))
    loss.backward()
    r = ref.reference(pooled.detach().cpu(), ws, bs, y)
    assert abs(float(loss) - r["loss"]) <= r["loss_bound"]
    _check_gradients(r, None, [p.weight.grad for p in head], [p.bias.grad for p in head])
    c = counts.double()[batch][:, None]
    want = r["dx"][batch] / c
    bound = r["dx_bound"][batch] / c + 2.0 * ref.U * want.abs() + ref.TINY
    _within("d nodes", nd.grad, want, bound)


# 6. no [G, V] array
def test_no_logits_array_is_allocated():
    """Peak device memory of loss + backward at (128, 304, 5002, 5) above what is live before the call and above the
    gradients the call returns (d_W_t alone are 30.4 MB): the dx partials of this shape (198 workgroups x 155.6 KB = 30.8 MB,
    the workspace the query reports) exceed one 12.8 MB logits array, so the limit is workspace + 1 MB -- a single [G, V]
    array of one position (2.56 MB) would already break it."""
    dev = _dev()
    g, k, v, t = 128, 304, 5002, 5
    # torch counts whole BLOCKS as allocated, and its caching allocator hands out a free block of up to 1 MiB more than was asked
    # for unsplit: what earlier tests left in the cache is not this call's either, so the cache is emptied first
    gc.collect()
    torch.cuda.empty_cache()
    (x, ws, bs, y), _ = _case(g, k, v, t, "mixed")
    xd, wd, bd = _leaves(x, ws, bs, dev)
    yd = y.to(dev)
    egc_amd.token_head_loss(xd, wd, bd, yd).backward()                  # one-time work is not the call's
    xd.grad = None
    for p in wd + bd:
        p.grad = None
    workspace = int(_C.load().egc_token_head_workspace_bytes(g, k, v, t))
    assert workspace > g * v * t * 4                                     # (which is why the limit is workspace + 1 MB)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    egc_amd.token_head_loss(xd, wd, bd, yd).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    grads = sum(p.grad.numel() * 4 for p in [xd] + wd + bd)
    print(f"peak above the inputs {peak / 1e6:.2f} MB, gradients {grads / 1e6:.2f} MB, workspace {workspace / 1e6:.2f} MB")
    assert peak - grads < workspace + (1 << 20)
