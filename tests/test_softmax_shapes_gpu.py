"""The output head and loss (egc_amd/csrc/egc_softmax.hip) at every geometry its launcher distinguishes: the ten (lanes,
pieces per lane) cells in the vector form, in the scalar form and with the piece that straddles n_classes; rows padded far
beyond the registers' columns; row counts at the chunk edges; one to three trips of the finalize kernel; pointers that are
not 16-byte aligned at vector-eligible shapes; and outputs written inside sentinel-filled buffers.  The table is
softmax_ref.GEOMETRIES, guarded without a GPU by tests/test_softmax_shapes_cpu.py.

No tolerance of its own: every bound is one of tests/softmax_ref.py (derived there and in tests/test_softmax_gpu.py), a
function of n_classes; structure -- zeros in the padding and on unselected rows, the first maximal column, two runs equal --
is exact.  The padding columns of every input hold NaN."""
import pytest
import torch

import egc_amd
import softmax_ref as ref
from test_softmax_gpu import _check_nll

pytestmark = pytest.mark.gpu

N = ref.SWEEP_ROWS
GEOMS = [pytest.param(c, ld, id=f"{c}-{ld}") for c, ld in ref.GEOMETRIES]


def _dev():
    return torch.device("cuda:0")


def _offset_by_one(t):
    """The tensor's contents on the device as a dense view one element into a larger buffer: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def _check_forward(x, c, xd=None):
    out, arg = egc_amd.log_softmax(x.to(_dev()) if xd is None else xd, num_classes=c, return_argmax=True)
    n = x.size(0)
    assert out.shape == (n, c) and out.is_contiguous() and arg.shape == (n,) and arg.dtype == torch.int64
    want, lse = ref.log_softmax(x, c)
    err = (out.cpu().double() - want).abs()
    bound = ref.logp_bound(want, lse, c)
    print(f"log_softmax C={c} ld={x.size(1)} N={n}: max err / bound = {float((err / bound).max()) if n else 0.0:.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(arg.cpu(), ref.first_argmax(x, c))
    return out


def _check_backward(x, c, g, gd=None):
    """d x of log_softmax for the upstream gradient g [N, C] (gd: g as it is handed to the device)."""
    from egc_amd import functional as F
    dev = _dev()
    n, ld = x.shape
    with torch.no_grad():
        out = egc_amd.log_softmax(x.to(dev), num_classes=c)
    dx = F.log_softmax_backward(g.to(dev) if gd is None else gd, out, ld)
    assert dx.shape == (n, ld)
    assert not dx[:, c:].any()                                          # exactly zero, not NaN from the padding
    o = out.cpu()
    want = ref.log_softmax_backward(g, o, ld)
    err = (dx.cpu().double() - want)[:, :c].abs()
    bound = ref.log_softmax_grad_bound(g, o, c)
    print(f"log_softmax backward C={c} ld={ld}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(F.log_softmax_backward(g.to(dev) if gd is None else gd, out, ld), dx)
    return dx


# 1. every cell, every form
@pytest.mark.parametrize("c,ld", GEOMS)
def test_log_softmax_forward_at_every_geometry(c, ld):
    _check_forward(ref.logits(N, c, ld, "mixed", seed=3 * c + ld), c)


@pytest.mark.parametrize("c,ld", GEOMS)
def test_argmax_is_the_first_maximal_column_at_every_geometry(c, ld):
    x = ref.ties_logits(N, c, ld, seed=c)
    _, arg = egc_amd.log_softmax(x.to(_dev()), num_classes=c, return_argmax=True)
    assert torch.equal(arg.cpu(), ref.first_argmax(x, c))


@pytest.mark.parametrize("c,ld", GEOMS)
def test_log_softmax_backward_at_every_geometry(c, ld):
    x = ref.logits(N, c, ld, "mixed", seed=7 * c + ld)
    g = torch.randn(N, c, generator=torch.Generator().manual_seed(c))
    dev = _dev()
    dx = _check_backward(x, c, g)
    xd = x.to(dev).requires_grad_(True)                                 # and through autograd: the same bits
    egc_amd.log_softmax(xd, num_classes=c).backward(g.to(dev))
    assert torch.equal(xd.grad, dx)


@pytest.mark.parametrize("c,ld", GEOMS)
def test_nll_at_every_geometry(c, ld):
    x = ref.logits(N, c, ld, "mixed", seed=5 * c + ld)
    y = torch.randint(0, c, (N,), generator=torch.Generator().manual_seed(c + ld))
    idx = ref.sample_index(N, 0.54, seed=c)
    _check_nll(x, y, None, c, "mean", g=-2.5)
    _check_nll(x, y, idx, c, "mean", g=3.0)
    _check_nll(x, y, None, c, "sum", g=3.0)
    _check_nll(x, y, idx, c, "sum", g=-2.5)


# 2. row counts at the chunk edges; the finalize kernel's second and third trip
@pytest.mark.parametrize("n", ref.LADDER_ROWS)
@pytest.mark.parametrize("c,ld", ref.LADDER_GEOMETRIES)
def test_row_counts_at_the_chunk_edges(c, ld, n):
    x = ref.logits(n, c, ld, "mixed", seed=n + c)
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(n))
    _check_forward(x, c)
    _check_backward(x, c, torch.randn(n, c, generator=torch.Generator().manual_seed(n + 1)))
    _check_nll(x, y, None, c, "mean", g=-2.5)
    _check_nll(x, y, ref.sample_index(n, 0.54, seed=n), c, "sum", g=3.0)


@pytest.mark.parametrize("n", ref.FINALIZE_ROWS)
def test_finalize_trips(n):
    """One, two and three chunk sums in a thread of the second launch; the loss is held to loss_bound with loss_chain at
    that count (printed by _check_nll)."""
    c, ld = ref.FINALIZE_GEOMETRY
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, ld, generator=g) * 10.0
    y = torch.randint(0, c, (n,), generator=g)
    assert ref.loss_chain(n, c) == 1 + 9 + -(-(-(-n // 128)) // 256) + 9
    _check_nll(x, y, None, c, "mean", g=-2.5)
    _check_nll(x, y, ref.sample_index(n, 0.54, seed=1), c, "sum", g=3.0)


# 3. pointers one float off at shapes that would take the vector form
@pytest.mark.parametrize("c,ld", ref.UNALIGNED_GEOMETRIES)
def test_unaligned_logits_take_the_scalar_form(c, ld):
    x = ref.logits(N, c, ld, "mixed", seed=c)
    y = torch.randint(0, c, (N,), generator=torch.Generator().manual_seed(c))
    _check_forward(x, c, xd=_offset_by_one(x))
    _check_nll(x, y, ref.sample_index(N, 0.54, seed=c), c, "mean", g=-2.5, place=_offset_by_one)
    _check_nll(x, y, None, c, "sum", g=3.0, place=_offset_by_one)
    x2 = ref.ties_logits(N, c, ld, seed=c + 1)
    _, arg = egc_amd.log_softmax(_offset_by_one(x2), num_classes=c, return_argmax=True)
    assert torch.equal(arg.cpu(), ref.first_argmax(x2, c))


@pytest.mark.parametrize("c,ld", ref.UNALIGNED_GEOMETRIES)
def test_unaligned_grad_out_takes_the_scalar_form(c, ld):
    x = ref.logits(N, c, ld, "mixed", seed=2 * c)
    g = torch.randn(N, c, generator=torch.Generator().manual_seed(c))
    _check_backward(x, c, g, gd=_offset_by_one(g))


# 4. outputs inside sentinel-filled buffers, through the C entry points
SENTINEL = 12345.0
PAD = 64          # elements in front of and behind every output: 256 bytes, the view keeps a 16-byte alignment


def _guarded(numel, dtype=torch.float32):
    """(buffer, the NaN-prefilled (int: -7) output view inside it)"""
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=_dev())
    view = buf[PAD:PAD + numel]
    view.fill_(float("nan") if dtype.is_floating_point else -7)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _assert_guard(buf, view, what):
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + view.numel():] == SENTINEL).all()), (what, "sentinel overwritten")
    if view.dtype.is_floating_point:
        assert not bool(torch.isnan(view).any()), (what, "element not written")
    else:
        assert not bool((view == -7).any()), (what, "element not written")


@pytest.mark.parametrize("c,ld", [(40, 40), (10, 64), (10, 63), (513, 516)])
def test_outputs_stay_inside_their_buffers(c, ld):
    from egc_amd import _C
    lib = _C.load()
    dev = _dev()
    n = N
    x = ref.logits(n, c, ld, "randn10", seed=c).to(dev)
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(ld)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    ob, out = _guarded(n * c)
    lb, lse = _guarded(n)
    ab, arg = _guarded(n, torch.int32)
    assert lib.egc_log_softmax_forward_f32(x.data_ptr(), n, c, ld, out.data_ptr(), lse.data_ptr(), arg.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    for b, v, what in ((ob, out, "out"), (lb, lse, "lse"), (ab, arg, "argmax")):
        _assert_guard(b, v, what)
    assert torch.equal(out.view(n, c), egc_amd.log_softmax(x, num_classes=c))
    assert torch.equal(arg.cpu().long(), ref.first_argmax(x.cpu(), c))
    g = torch.randn(n, c, device=dev)
    db, dx = _guarded(n * ld)
    assert lib.egc_log_softmax_backward_f32(g.data_ptr(), out.data_ptr(), n, c, ld, dx.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    _assert_guard(db, dx, "log-softmax d_x")
    assert not dx.view(n, ld)[:, c:].any()
    # the fused loss: lse and d_x (every row, and a selection that leaves rows out)
    sel = egc_amd.RowSelection(ref.sample_index(n, 0.54, seed=3).to(dev), n)
    for cnt, total in ((None, None), (sel.cnt, sel.M)):
        lb2, lse2 = _guarded(n)
        sb, loss = _guarded(1)
        wb, ws = _guarded((n + 127) // 128)
        need = lib.egc_nll_log_softmax_workspace_bytes(n, c)
        assert need == ws.numel() * 4
        args = (x.data_ptr(), y.data_ptr(), cnt.data_ptr() if cnt is not None else None, total.data_ptr() if total is not None else None)
        assert lib.egc_nll_log_softmax_forward_f32(*args, n, c, ld, 1, loss.data_ptr(), lse2.data_ptr(), ws.data_ptr(), need,
                                                   None, stream) == 0
        torch.cuda.synchronize()
        for b, v, what in ((lb2, lse2, "nll lse"), (sb, loss, "loss"), (wb, ws, "chunk sums")):
            _assert_guard(b, v, what)
        go = torch.full((1,), 0.75, device=dev)
        db2, dx2 = _guarded(n * ld)
        assert lib.egc_nll_log_softmax_backward_f32(*args, lse2.data_ptr(), go.data_ptr(), n, c, ld, 1, dx2.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        _assert_guard(db2, dx2, "nll d_x")
        assert not dx2.view(n, ld)[:, c:].any()
        if cnt is not None:
            assert not dx2.view(n, ld)[sel.cnt == 0].any() and bool(dx2.view(n, ld)[sel.cnt > 0].any())
