"""Host side of the graph-level readouts: the name -> function map, the device requirement, and the argument checks of the C
entry points, which come before any launch (nothing here touches a GPU)."""
import ctypes as C

import pytest
import torch

import readout_ref as ref

EGC_ERR_INVALID = 1


def test_readout_maps_the_reference_constructor_names():
    import egc_amd
    assert egc_amd.readout("mean") is egc_amd.global_mean_pool
    assert egc_amd.readout("sum") is egc_amd.global_add_pool
    assert egc_amd.readout("max") is egc_amd.global_max_pool
    with pytest.raises(ValueError):
        egc_amd.readout("median")


@pytest.mark.parametrize("name", ["mean", "sum", "max"])
def test_cpu_tensors_are_refused(name):
    import egc_amd
    from egc_amd import functional as F
    x, batch = torch.randn(6, 8), torch.tensor([0, 0, 1, 1, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        egc_amd.readout(name)(x, batch, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.segment_reduce(x, torch.tensor([0, 2, 5, 6]), name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.segment_reduce_backward(torch.randn(3, 8), torch.tensor([0, 2, 5, 6]), name, 6,
                                  torch.zeros(3, 8, dtype=torch.int32) if name == "max" else None)
    with pytest.raises(ValueError):
        F.segment_reduce(x, torch.tensor([0, 2, 5, 6]), "median")


def test_header_codes_match_the_python_table():
    from egc_amd import _C, functional as F
    codes = {k: _C.ABI.constants["EGC_READOUT_" + k.upper()] for k in ("sum", "mean", "max")}
    assert codes == F.READOUT_OPS == {"sum": _C.READOUT_SUM, "mean": _C.READOUT_MEAN, "max": _C.READOUT_MAX}


def test_bad_arguments_are_refused_before_any_launch():
    """Host buffers stand in for device pointers: every call below must return at its argument check."""
    from egc_amd import _C
    lib = _C.load()
    x = (C.c_float * 8)()
    out = (C.c_float * 8)()
    arg = (C.c_int32 * 8)()
    seg = (C.c_int64 * 2)(0, 2)
    px, pout, parg, pseg = (C.addressof(b) for b in (x, out, arg, seg))
    fwd, bwd = lib.egc_segment_reduce_f32, lib.egc_segment_reduce_backward_f32
    assert fwd(px, pseg, 1, 2, 4, 7, pout, None, None) == EGC_ERR_INVALID          # unknown op
    assert fwd(px, pseg, 1, 2, 4, -1, pout, None, None) == EGC_ERR_INVALID
    assert fwd(px, pseg, 1, 2, 0, _C.READOUT_SUM, pout, None, None) == EGC_ERR_INVALID          # width 0
    assert fwd(px, None, 1, 2, 4, _C.READOUT_SUM, pout, None, None) == EGC_ERR_INVALID          # no seg_ptr
    assert fwd(px, pseg, 1, 2, 4, _C.READOUT_MAX, None, parg, None) == EGC_ERR_INVALID          # no out
    assert fwd(None, pseg, 1, 2, 4, _C.READOUT_MEAN, pout, None, None) == EGC_ERR_INVALID       # rows but no x
    assert fwd(px, pseg, 1, 1 << 31, 4, _C.READOUT_MAX, pout, parg, None) == 4                  # EGC_ERR_UNSUPPORTED: int32 arg
    assert bwd(pout, pseg, None, 1, 2, 4, _C.READOUT_MAX, px, None) == EGC_ERR_INVALID          # max backward without arg
    assert bwd(pout, pseg, parg, 1, 2, 4, 7, px, None) == EGC_ERR_INVALID
    assert bwd(pout, pseg, None, 1, 2, 0, _C.READOUT_SUM, px, None) == EGC_ERR_INVALID
    assert bwd(pout, pseg, None, 1, 2, 4, _C.READOUT_SUM, None, None) == EGC_ERR_INVALID        # no d_x
    # nothing to do is fine: no segments (forward), no rows (backward)
    assert fwd(None, None, 0, 0, 4, _C.READOUT_SUM, None, None, None) == 0
    assert bwd(None, None, None, 0, 0, 4, _C.READOUT_MEAN, None, None) == 0


@pytest.mark.parametrize("op", ["sum", "mean", "max"])
def test_the_sequential_reference_is_a_scatter_in_float64_to_rounding(op):
    """The reference the GPU tests compare with, bit for bit, is itself held against torch's scatter in float64 here."""
    g = torch.Generator().manual_seed(0)
    sizes = torch.randint(0, 30, (40,), generator=g)
    batch = torch.repeat_interleave(torch.arange(40), sizes)
    seg = ref.seg_ptr_of(batch, 40)
    x = torch.randn(batch.numel(), 12, generator=g)
    out, arg = ref.forward(x, seg, op)
    idx = batch[:, None].expand_as(x)
    if op == "max":
        want = torch.zeros(40, 12, dtype=torch.float64).scatter_reduce_(0, idx, x.double(), "amax", include_self=False)
        assert torch.equal(out.double(), want)
        live = arg >= 0
        assert torch.equal(live, (sizes > 0)[:, None].expand_as(live))
        cols = torch.arange(12)[None, :].expand_as(arg)
        assert torch.equal(x[arg[live].long(), cols[live]], out[live])
    else:
        want = torch.zeros(40, 12, dtype=torch.float64).index_add_(0, batch, x.double())
        if op == "mean":
            want = want / sizes.clamp(min=1)[:, None]
        assert float((out.double() - want).abs().max()) <= 1e-5
    go = torch.randn(40, 12, generator=g)
    dx = ref.backward(go, seg, op, x.size(0), arg)
    xr = x.double().requires_grad_(True)
    if op == "max":
        torch.zeros(40, 12, dtype=torch.float64).scatter_reduce(0, idx, xr, "amax", include_self=False).backward(go.double())
    else:
        s = torch.zeros(40, 12, dtype=torch.float64).index_add(0, batch, xr)
        (s / sizes.clamp(min=1)[:, None] if op == "mean" else s).backward(go.double())
    assert float((dx.double() - xr.grad).abs().max()) <= 1e-6          # (random normal input: no ties for amax to split)
