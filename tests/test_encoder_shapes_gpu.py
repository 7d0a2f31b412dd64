"""The node encoder kernels (egc_amd/csrc/egc_encoder.hip) at every geometry their launchers distinguish: one lane to 256
lanes per node in the 16-byte and in the 4-byte form, one to sixteen tables against the forward's batch of four, tables of
1 to 600 rows around the 256 partial slots of a chunk, list lengths around the 8 rows the first pass requests together,
node counts around the 256-node chunk and chunk counts around the 8 chunk sums the second pass requests together,
operands that are not 16-byte aligned at a multiple-of-4 width, an index outside its table in the 4-byte form, and outputs
written inside sentinel-filled buffers.  The lists are those of tests/encoder_ref.py, guarded without a GPU by
tests/test_encoder_shapes_cpu.py.

Everything is compared bit for bit: the forward with encoder_ref.forward, the table gradients with
encoder_ref.chunked_backward, the float32 restatement of the documented order (chunks of 256 nodes; ascending n inside a
chunk from the first row; ascending chunk after that).  The any-order bound of tests/test_encoder_gpu.py is asserted next
to it.  After every case the deferred index flag is clean."""
import ctypes as C

import pytest
import torch

import encoder_ref as ref
from test_encoder_gpu import _assert_grads_equal_the_documented_order, _assert_grads_within_bound, _tables

pytestmark = pytest.mark.gpu

DROP_SCALE = 1.0 / (1.0 - 0.2)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _keep(n, width, seed):
    return (torch.rand(n, width, generator=torch.Generator().manual_seed(seed)) < 0.8).to(torch.uint8)


def _check(tables, idx, clamp, d, keep=None, what=""):
    """Forward and backward of one case (with the dropout mask when given) against the restatements; the flag stays clean."""
    from egc_amd import functional as F
    dev = _dev()
    rows = [w.size(0) for w in tables]
    scale = DROP_SCALE if keep is not None else 1.0
    kd = keep.to(dev) if keep is not None else None
    got = F.encoder_forward([w.to(dev) for w in tables], idx.to(dev), clamp, kd, scale)
    want = ref.masked_rows(ref.forward(tables, idx, clamp), keep, scale)
    assert got.shape == want.shape and torch.equal(got.cpu(), want), (what, "forward")
    grads = F.encoder_backward(d.to(dev), idx.to(dev), rows, clamp, kd, scale)
    g = ref.masked_rows(d, keep, scale)
    _assert_grads_equal_the_documented_order(grads, g, idx, rows, clamp, what)
    _assert_grads_within_bound(grads, g, idx, rows, clamp, what)
    torch.cuda.synchronize()
    F._IndexFlag.poll()
    return got, grads


# 1. widths x table sets, uniform and skewed, with and without the dropout mask
@pytest.mark.parametrize("width, n_tables, dist", ref.sweep_cases())
def test_sweep_of_widths_and_table_sets(width, n_tables, dist):
    n = ref.SWEEP_NODES
    rows, clamp, beyond = ref.sweep_tables(n_tables)
    idx = ref.sweep_indices(n, rows, dist, 7 * width + n_tables, beyond)
    tables = _tables(rows, width, width + 1)
    d = torch.randn(n, width, generator=torch.Generator().manual_seed(width + 2))
    _check(tables, idx, clamp, d, None, f"{width}-T{n_tables}-{dist}")
    _check(tables, idx, clamp, d, _keep(n, width, width + 3), f"{width}-T{n_tables}-{dist}-dropout")


# 2. list lengths around the rows requested together; a chunk that is one list
@pytest.mark.parametrize("width", [128, 77])
def test_list_length_ladder(width):
    idx = ref.ladder_indices()
    tables = _tables(ref.LADDER_ROWS, width, 5)
    d = torch.randn(idx.size(0), width, generator=torch.Generator().manual_seed(6))
    _, grads = _check(tables, idx, None, d, None, f"ladder-{width}")
    assert not grads[0][ref.LADDER_ROWS[0] - 1].any()                   # the row nobody indexes
    _check(tables, idx, None, d, _keep(idx.size(0), width, 8), f"ladder-{width}-dropout")


# 3. node counts around the chunk, chunk counts around the chunk sums requested together
@pytest.mark.parametrize("n", ref.NODE_LADDER + ref.CHUNK_LADDER)
def test_node_and_chunk_ladder(n):
    width, rows = ref.LADDER_WIDTH, ref.NODE_LADDER_ROWS
    idx = ref.sweep_indices(n, rows, "uniform", n)
    tables = _tables(rows, width, 9)
    d = torch.randn(n, width, generator=torch.Generator().manual_seed(n + 1))
    _check(tables, idx, None, d, None, f"n{n}")
    _check(tables, idx, None, d, _keep(n, width, n + 2), f"n{n}-dropout")
    skew = ref.sweep_indices(n, rows, "skewed", n)                       # one destination row of every table in every chunk
    _check(tables, skew, None, d, None, f"n{n}-skewed")


# 4. operands one element off a 16-byte boundary at a multiple-of-4 width: the 4-byte form, the same bits
def _offset_by_one(t):
    buf = torch.empty(t.numel() + 32, dtype=t.dtype, device=_dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


@pytest.mark.parametrize("which", ["tables", "one_table", "d_out", "grad_tables", "keep"])
def test_unaligned_operands_give_the_aligned_bits(which):
    from egc_amd import functional as F
    dev = _dev()
    width, n = 128, ref.SWEEP_NODES
    rows, clamp, beyond = ref.sweep_tables(5)
    idx = ref.sweep_indices(n, rows, "uniform", 21, beyond)
    tables = _tables(rows, width, 22)
    d = torch.randn(n, width, generator=torch.Generator().manual_seed(23))
    keep = _keep(n, width, 24)
    fwd, grads = _check(tables, idx, clamp, d, keep, "aligned")
    dtab, dd, dk, di = [w.to(dev) for w in tables], d.to(dev), keep.to(dev), idx.to(dev)
    assert all(t.data_ptr() % 16 == 0 for t in dtab + [dd, dk])
    out = None
    if which == "tables":
        dtab = [_offset_by_one(w) for w in dtab]
    elif which == "one_table":
        dtab[3] = _offset_by_one(dtab[3])
    elif which == "d_out":
        dd = _offset_by_one(dd)
    elif which == "keep":
        dk = _offset_by_one(dk)
    else:
        out = [_offset_by_one(torch.full((r, width), float("nan"))) for r in rows]
    assert torch.equal(F.encoder_forward(dtab, di, clamp, dk, DROP_SCALE), fwd)
    got = F.encoder_backward(dd, di, rows, clamp, dk, DROP_SCALE, out=out)
    for t, (a, b) in enumerate(zip(got, grads)):
        assert torch.equal(a, b), (which, t)
        assert out is None or a is out[t]
    torch.cuda.synchronize()
    F._IndexFlag.poll()


# 5. an index outside its table in the 4-byte form
def test_index_outside_its_table_in_the_scalar_form():
    from egc_amd import functional as F
    dev = _dev()
    F._IndexFlag.poll()
    width, n = 77, 1000
    rows = [119, 4, 12, 12, 10, 6, 6, 2, 2]
    idx = ref.sweep_indices(n, rows, "uniform", 13)
    good = idx.clone()
    idx[5, 1] = rows[1]              # one past the end of table 1
    idx[9, 0] = -1                   # negative index into table 0
    idx[700, 8] = 2 ** 40
    tables = _tables(rows, width, 14)
    want = ref.forward(tables, idx, None)                                # the rule: such a table contributes a zero row
    rest5 = ref.forward([w for t, w in enumerate(tables) if t != 1], idx[5:6, [t for t in range(9) if t != 1]])
    assert torch.equal(want[5:6], rest5)
    dtab = [w.to(dev) for w in tables]
    got = F.encoder_forward(dtab, idx.to(dev))
    d = torch.randn(n, width, generator=torch.Generator().manual_seed(15))
    grads = F.encoder_backward(d.to(dev), idx.to(dev), rows)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got.cpu(), want)
    _assert_grads_equal_the_documented_order(grads, d, idx, rows, None, "bad index")
    _assert_grads_within_bound(grads, d, idx, rows, None, "bad index")
    with pytest.raises(RuntimeError, match="index outside its embedding table"):
        F.encoder_forward(dtab, good[:4].to(dev))                        # the deferred flag surfaces at the next call
    clean = F.encoder_forward(dtab, good.to(dev))                        # reported once
    # nothing else changes: every other node's output row and every table the bad indices do not touch
    others = torch.ones(n, dtype=torch.bool)
    others[[5, 9, 700]] = False
    assert torch.equal(got[others.to(dev)], clean[others.to(dev)])
    clean_grads = F.encoder_backward(d.to(dev), good.to(dev), rows)
    for t in (2, 3, 4, 5, 6, 7):
        assert torch.equal(grads[t], clean_grads[t]), t
    torch.cuda.synchronize()
    F._IndexFlag.poll()


# 6. outputs inside sentinel-filled buffers
SENTINEL = 12345.0
PAD = 64          # floats between and around the outputs: the views keep a 16-byte alignment


def _guarded(sizes):
    """(buffer, NaN-prefilled views of `sizes` elements inside it, PAD sentinels in front of, between and behind them)"""
    buf = torch.full((sum(sizes) + PAD * (len(sizes) + 1),), SENTINEL, device=_dev())
    views, at = [], PAD
    for m in sizes:
        views.append(buf[at:at + m])
        views[-1].fill_(float("nan"))
        at += m + PAD
    return buf, views


def _assert_guard(buf, views, what):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    at = PAD
    for v in views:
        inside[at:at + v.numel()] = True
        at += v.numel() + PAD
        assert not bool(torch.isnan(v).any()), (what, "element not written")
    assert bool((buf[~inside] == SENTINEL).all()), (what, "sentinel overwritten")


@pytest.mark.parametrize("width", [77, 128])
@pytest.mark.parametrize("masked", [False, True])
def test_outputs_stay_inside_their_buffers(width, masked):
    from egc_amd import _C
    from egc_amd import functional as F
    dev = _dev()
    lib = _C.load()
    n = ref.SWEEP_NODES
    rows, clamp, beyond = ref.sweep_tables(5)
    idx = ref.sweep_indices(n, rows, "uniform", 31, beyond).to(dev)
    tables = [w.to(dev) for w in _tables(rows, width, 32)]
    keep = _keep(n, width, 33).to(dev) if masked else None
    scale = DROP_SCALE if masked else 1.0
    t = len(rows)
    c_rows = (C.c_int32 * t)(*rows)
    c_clamp = (C.c_int32 * t)(*[-1 if c is None else c for c in clamp])
    ptrs = (C.c_void_p * t)(*[w.data_ptr() for w in tables])
    stream = torch.cuda.current_stream().cuda_stream
    buf, (out,) = _guarded([n * width])
    assert lib.egc_encoder_forward_f32(ptrs, c_rows, c_clamp, t, idx.data_ptr(), n, width, keep.data_ptr() if masked else None,
                                       scale, out.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    _assert_guard(buf, [out], "forward")
    assert torch.equal(out.view(n, width), F.encoder_forward(tables, idx, clamp, keep, scale))
    d = torch.randn(n, width, device=dev)
    gbuf, views = _guarded([r * width for r in rows])
    grads = [v.view(r, width) for v, r in zip(views, rows)]
    got = F.encoder_backward(d, idx, rows, clamp, keep, scale, out=grads)
    torch.cuda.synchronize()
    _assert_guard(gbuf, views, "table gradients")
    for a, b, want in zip(got, grads, F.encoder_backward(d, idx, rows, clamp, keep, scale)):
        assert a is b and torch.equal(a, want)
