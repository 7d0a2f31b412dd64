"""The readout kernels (egc_amd/csrc/egc_readout.hip) at every geometry they distinguish: segment lengths around one, two
and three batches of the 8 rows the forward requests together, empty segments first, in the middle and last; widths from one
lane to a group wider than a 256-thread workgroup in the 16-byte and in the 4-byte form; the NaN / Inf rule of the max
readout as the kernel's header states it; operands that are not 16-byte aligned at a multiple-of-4 width; outputs written
inside sentinel-filled buffers.  The ladder and the widths are those of tests/readout_ref.py, their properties asserted
without a GPU in tests/test_readout_shapes_cpu.py.

Bit for bit against the sequential float32 loop of tests/readout_ref.py: no tolerance appears anywhere.  (Where a float32
add MAKES a NaN -- Inf + -Inf in the sum readout -- its payload is not compared: a NaN equals a NaN.)"""
import math

import pytest
import torch

import readout_ref as ref
from test_readout_gpu import OPS, _check_pool

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# 1. the segment-length ladder at every width, in both orders
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("width", ref.WIDTHS)
def test_segment_length_ladder(width, order, op):
    batch, n_graphs = ref.ladder_batch(order)
    x = torch.randn(batch.numel(), width, generator=torch.Generator().manual_seed(width))
    want, arg, _ = _check_pool(op, x, batch, n_graphs)
    empty = [g for g, n in enumerate(ref.ladder_sizes(order)) if n == 0]
    assert not want[empty].any() and (op != "max" or bool((arg[empty] == -1).all()))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", [128, 77, 1030])
def test_segment_length_ladder_with_ties(width, op):
    batch, n_graphs = ref.ladder_batch("up")
    x = torch.randint(-1, 2, (batch.numel(), width), generator=torch.Generator().manual_seed(width)).to(torch.float32)
    _check_pool(op, x, batch, n_graphs)


# 2. NaN and +-Inf
def _special_input(width, seed):
    """The ladder batch with, per column c % 6: 0 a NaN in every segment's first row; 1 a NaN in a later row (the second,
    where there is one); 2 +Inf twice (second and last row); 3 all -Inf; 4 a NaN first AND +Inf later; 5 plain."""
    batch, n_graphs = ref.ladder_batch("up")
    seg = ref.seg_ptr_of(batch, n_graphs)
    x = torch.randn(batch.numel(), width, generator=torch.Generator().manual_seed(seed))
    col = torch.arange(width) % 6
    for g in range(n_graphs):
        r0, r1 = int(seg[g]), int(seg[g + 1])
        if r1 == r0:
            continue
        later = min(r0 + 1, r1 - 1)
        x[r0, col == 0] = math.nan
        if r1 - r0 > 1:
            x[later, col == 1] = math.nan
        x[later, col == 2] = math.inf
        x[r1 - 1, col == 2] = math.inf
        x[r0:r1, col == 3] = -math.inf
        x[r0, col == 4] = math.nan
        x[later, col == 4] = math.inf if r1 - r0 > 1 else math.nan
    return x, batch, n_graphs, seg, col


@pytest.mark.parametrize("width", [128, 77])
def test_max_follows_the_strict_compare_on_nan_and_inf(width):
    from egc_amd import functional as F
    dev = _dev()
    x, batch, n_graphs, seg, col = _special_input(width, 3)
    sizes = seg[1:] - seg[:-1]
    want, want_arg = ref.forward(x, seg, "max")
    out, arg = F.segment_reduce(x.to(dev), seg.to(dev), "max", want_arg=True)
    out, arg = out.cpu(), arg.cpu()
    assert torch.equal(arg, want_arg)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))           # a max only copies: the NaN's own bits too
    live, many = sizes > 0, sizes > 1
    first = seg[:-1].to(torch.int32)[:, None]
    # the rule itself, not only the reference's reading of it
    assert bool(torch.isnan(out[live][:, col == 0]).all()) and bool((arg[live][:, col == 0] == first[live]).all())
    assert not bool(torch.isnan(out[many][:, col == 1]).any())                  # a NaN in a later row is never taken
    assert bool((arg[many][:, col == 1] != first[many] + 1).all())
    assert bool((out[live][:, col == 2] == math.inf).all())
    assert bool((arg[many][:, col == 2] == first[many] + 1).all())              # the first +Inf, not the last
    assert bool((out[live][:, col == 3] == -math.inf).all()) and bool((arg[live][:, col == 3] == first[live]).all())
    assert bool(torch.isnan(out[live][:, col == 4]).all()) and bool((arg[live][:, col == 4] == first[live]).all())
    assert bool((arg[~live] == -1).all()) and not out[~live].any()
    # the backward routes the gradient to exactly that row
    go = torch.randn(n_graphs, width, generator=torch.Generator().manual_seed(4))
    dx = F.segment_reduce_backward(go.to(dev), seg.to(dev), "max", x.size(0), arg.to(dev)).cpu()
    assert torch.equal(dx, ref.backward(go, seg, "max", x.size(0), want_arg))
    assert int((dx != 0).sum()) == int(live.sum()) * width - int((go[live] == 0).sum())
    # and through the module with autograd
    import egc_amd
    xg = x.to(dev).requires_grad_(True)
    pooled = egc_amd.global_max_pool(xg, batch.to(dev), n_graphs)
    assert torch.equal(pooled.detach().cpu().view(torch.int32), want.view(torch.int32))
    pooled.backward(go.to(dev))
    assert torch.equal(xg.grad.cpu(), dx)


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("width", [128, 77])
def test_sum_and_mean_propagate_nan_and_inf(width, op):
    from egc_amd import functional as F
    dev = _dev()
    x, batch, n_graphs, seg, col = _special_input(width, 5)
    want, _ = ref.forward(x, seg, op)
    out = F.segment_reduce(x.to(dev), seg.to(dev), op).cpu()
    assert ref.same_bits_or_both_nan(out, want)
    live = (seg[1:] - seg[:-1]) > 0
    many = (seg[1:] - seg[:-1]) > 1
    assert bool(torch.isnan(out[live][:, col == 0]).all()) and bool(torch.isnan(out[many][:, col == 1]).all())
    assert bool((out[live][:, col == 2] == math.inf).all()) and bool((out[live][:, col == 3] == -math.inf).all())
    assert bool(torch.isfinite(out[:, col == 5]).all()) and not out[~live].any()


# 3. x, d_out and d_x one float off a 16-byte boundary at width 128: the 4-byte form, the same bits
def _offset_by_one(t):
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


@pytest.mark.parametrize("op", OPS)
def test_unaligned_operands_give_the_aligned_bits(op):
    from egc_amd import _C
    from egc_amd import functional as F
    dev = _dev()
    width = 128
    batch, n_graphs = ref.ladder_batch("up")
    n = batch.numel()
    seg = ref.seg_ptr_of(batch, n_graphs)
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(6))
    go = torch.randn(n_graphs, width, generator=torch.Generator().manual_seed(7))
    want, want_arg = ref.forward(x, seg, op)
    want_dx = ref.backward(go, seg, op, n, want_arg)
    xd, segd, god = x.to(dev), seg.to(dev), go.to(dev)
    assert xd.data_ptr() % 16 == 0 and god.data_ptr() % 16 == 0
    if op == "max":
        out, arg = F.segment_reduce(_offset_by_one(xd), segd, op, want_arg=True)
        assert torch.equal(arg.cpu(), want_arg)
    else:
        out, arg = F.segment_reduce(_offset_by_one(xd), segd, op), None
    assert torch.equal(out.cpu(), want)
    assert torch.equal(F.segment_reduce_backward(_offset_by_one(god), segd, op, n, arg).cpu(), want_dx)
    # d_x (and the forward's out and arg) are allocated by the wrappers: through the C entry points
    lib = _C.load()
    stream = torch.cuda.current_stream().cuda_stream
    code = F.READOUT_OPS[op]
    dx = _offset_by_one(torch.full((n, width), float("nan")))
    assert lib.egc_segment_reduce_backward_f32(god.data_ptr(), segd.data_ptr(), arg.data_ptr() if arg is not None else None,
                                               n_graphs, n, width, code, dx.data_ptr(), stream) == 0
    assert torch.equal(dx.cpu(), want_dx)
    out2 = _offset_by_one(torch.full((n_graphs, width), float("nan")))
    arg2 = _offset_by_one(torch.full((n_graphs, width), -7, dtype=torch.int32))
    assert lib.egc_segment_reduce_f32(xd.data_ptr(), segd.data_ptr(), n_graphs, n, width, code, out2.data_ptr(),
                                      arg2.data_ptr(), stream) == 0
    assert torch.equal(out2.cpu(), want)
    if op == "max":
        assert torch.equal(arg2.cpu(), want_arg)
        dx.fill_(float("nan"))
        assert lib.egc_segment_reduce_backward_f32(god.data_ptr(), segd.data_ptr(), arg2.data_ptr(), n_graphs, n, width, code,
                                                   dx.data_ptr(), stream) == 0
        assert torch.equal(dx.cpu(), want_dx)


# 4. out, arg and d_x inside sentinel-filled buffers, through the C entry points
SENTINEL = 12345
PAD = 64          # elements around every output: the views keep a 16-byte alignment


def _guarded(numel, dtype=torch.float32):
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=_dev())
    view = buf[PAD:PAD + numel]
    view.fill_(float("nan") if dtype.is_floating_point else -7)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _assert_guard(buf, view, what):
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + view.numel():] == SENTINEL).all()), (what, "sentinel overwritten")
    unwritten = torch.isnan(view) if view.dtype.is_floating_point else view == -7
    assert not bool(unwritten.any()), (what, "element not written")


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", [77, 128])
def test_outputs_stay_inside_their_buffers(width, op):
    from egc_amd import _C
    from egc_amd import functional as F
    dev = _dev()
    lib = _C.load()
    stream = torch.cuda.current_stream().cuda_stream
    code = F.READOUT_OPS[op]
    batch, n_graphs = ref.ladder_batch("down")
    seg = ref.seg_ptr_of(batch, n_graphs)
    n = batch.numel() + 8                                     # 3 rows in front of the first segment, 5 behind the last
    seg = seg + 3
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(8))
    go = torch.randn(n_graphs, width, generator=torch.Generator().manual_seed(9))
    want, want_arg = ref.forward(x, seg, op)
    xd, segd, god = x.to(dev), seg.to(dev), go.to(dev)
    ob, out = _guarded(n_graphs * width)
    ab, arg = _guarded(n_graphs * width, torch.int32)
    assert lib.egc_segment_reduce_f32(xd.data_ptr(), segd.data_ptr(), n_graphs, n, width, code, out.data_ptr(),
                                      arg.data_ptr() if op == "max" else None, stream) == 0
    torch.cuda.synchronize()
    _assert_guard(ob, out, "out")
    assert torch.equal(out.view(n_graphs, width).cpu(), want)
    if op == "max":
        _assert_guard(ab, arg, "arg")
        assert torch.equal(arg.view(n_graphs, width).cpu(), want_arg)
    db, dx = _guarded(n * width)
    assert lib.egc_segment_reduce_backward_f32(god.data_ptr(), segd.data_ptr(), arg.data_ptr() if op == "max" else None,
                                               n_graphs, n, width, code, dx.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    _assert_guard(db, dx, "d_x")
    dx = dx.view(n, width).cpu()
    assert torch.equal(dx, ref.backward(go, seg, op, n, want_arg))
    assert not dx[:3].any() and not dx[-5:].any()
