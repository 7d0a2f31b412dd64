"""Attention dropout of GATConv and GATv2Conv without a GPU: the mask of tests/gat_dropout_ref.py under the seed the GPU tests
use (kept fractions, nothing dropped at a tiny p), the per-edge composition with an all-ones mask against the float64
restatements of the plain kernels (tests/gat1_ref.py, tests/gat_ref.py), the argument checks of the four *_dropout_f32 entry
points, and the modules' host side."""
import numpy as np
import pytest
import torch

import egc_amd
import gat1_ref
import gat_ref
from egc_amd import _C
from egc_amd._gat import gat_aggregate, gatv2_aggregate
from gat_dropout_ref import (SEED, edge_list, gat_composition, gatv2_composition, keep_mask, multipliers, scale_of, threshold)
from mpnn_ref import csr_by_destination, rel_grad, rel_out

GRAPH_SEED, INPUT_SEED, N = 5, 7, 40
GPU_SHAPES = ((1, 1), (4, 1), (12, 5), (9, 7), (1, 256), (1, 257), (8, 33), (128, 3), (170, 3), (8, 19))   # tests/test_gat_dropout_gpu.py


def _csr():
    ei = gat_ref.sweep_graph(GRAPH_SEED, N)[0]
    rowptr, col, _ = csr_by_destination(ei, N)
    return ei, rowptr, col


@pytest.mark.parametrize("p", (0.1, 0.5, 0.9))
def test_kept_fraction_under_the_gpu_tests_seed(p):
    """Every draw of the sweep graph at H = 8 (1,234 entries and 40 self entries, 8 heads): the kept fraction is within four
    standard deviations of 1 - p, and the mask is a function of its arguments."""
    _, rowptr, _ = _csr()
    e = int(rowptr[-1])
    assert e == 1234
    keep_e, keep_s = keep_mask(e, N, 8, p, SEED)
    assert keep_e.shape == (e, 8) and keep_s.shape == (N, 8)
    n = keep_e.size + keep_s.size
    kept = (int(keep_e.sum()) + int(keep_s.sum())) / n
    bound = 4.0 * np.sqrt(p * (1.0 - p) / n)
    print(f"p {p}: kept {kept:.5f} of {n} draws, 1 - p = {1 - p:.5f}, bound {bound:.5f}")
    assert abs(kept - (1.0 - p)) <= bound
    again = keep_mask(e, N, 8, p, SEED)
    assert np.array_equal(again[0], keep_e) and np.array_equal(again[1], keep_s)
    other = keep_mask(e, N, 8, p, SEED + 1)
    assert not np.array_equal(other[0], keep_e)
    # heads beyond the first four come from a second call (counter word 1), the self entries from a stream of their own
    assert not np.array_equal(keep_e[:, :4], keep_e[:, 4:]) and not np.array_equal(keep_e[:N], keep_s)


def test_tiny_p_drops_nothing_and_scales_by_exactly_one():
    p = 1e-9
    assert threshold(p) == 4 and scale_of(p) == np.float32(1.0)
    _, rowptr, _ = _csr()
    for h, _ in GPU_SHAPES:
        keep_e, keep_s = keep_mask(int(rowptr[-1]), N, h, p, SEED)
        assert keep_e.all() and keep_s.all(), h


def test_thresholds_and_scales():
    assert threshold(0.5) == 2 ** 31 and threshold(0.25) == 2 ** 30 and threshold(1.0 - 2.0 ** -53) == 2 ** 32 - 1
    assert scale_of(0.5) == np.float32(2.0) and scale_of(0.6) == np.float32(2.5)


def test_edge_list_keeps_positions_and_appends_the_self_entries():
    _, rowptr, col = _csr()
    src, dst, pos = edge_list(rowptr, col, True)
    skipped = int((col == np.repeat(np.arange(N), np.diff(rowptr))).sum())
    assert skipped > 0 and len(src) == 1234 - skipped + N
    assert np.array_equal(pos[-N:], -1 - np.arange(N)) and np.array_equal(src[-N:], dst[-N:])
    assert np.array_equal(col[pos[:-N]], src[:-N]) and (np.diff(pos[:-N]) > 0).all()      # positions kept, gaps where skipped
    src, dst, pos = edge_list(rowptr, col, False)
    assert len(src) == 1234 and np.array_equal(pos, np.arange(1234))


@pytest.mark.parametrize("loops", (True, False))
@pytest.mark.parametrize("shape", ((12, 5), (4, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_ones_mask_is_the_plain_layer_in_float64(shape, loops):
    """With nothing dropped and scale 1 the float64 composition is the float64 restatement of the plain kernels, to rounding:
    the new truth is tied to the old one."""
    h, c = shape
    ei, rowptr, col = _csr()
    ones = (np.ones((1234, h), dtype=bool), np.ones((N, h), dtype=bool))
    mult = multipliers(rowptr, col, h, loops, 1e-9, SEED, mask=ones)
    assert mult.dtype == np.float32 and (mult == 1.0).all()
    # GAT v1
    xl, a_src, a_dst, gout = gat1_ref.sweep_inputs(h, c, N, INPUT_SEED)
    got = gat_composition(xl, a_src, a_dst, rowptr, col, mult, gout, loops=loops)
    ref = gat1_ref.sweep_reference(h, c, loops)[np.float64]
    assert rel_out(got[0], ref[0]) <= 1e-10 and gat1_ref.lse_distance(got[1], ref[1]) == (True, pytest.approx(0.0, abs=1e-10))
    for k in (2, 3, 4):
        assert rel_grad(got[k], ref[k]) <= 1e-10, k
    # GATv2
    xl, xr, gout, att = gat_ref.sweep_inputs(h, c, N, INPUT_SEED)
    got = gatv2_composition(xl, xr, att, rowptr, col, mult, gout, loops=loops)
    out, lse = gat_ref.aggregate_forward(xl, xr, att, ei, loops=loops)
    ref = (out, lse) + gat_ref.aggregate_backward(xl, xr, att, ei, out, lse, gout, loops=loops)
    assert rel_out(got[0], ref[0]) <= 1e-10 and gat1_ref.lse_distance(got[1], ref[1]) == (True, pytest.approx(0.0, abs=1e-10))
    for k in (2, 3, 4):
        assert rel_grad(got[k], ref[k]) <= 1e-10, k


def test_dropped_entries_stay_in_the_softmax():
    """The composition's alpha and lse are those of the unmasked row: masking changes out, never lse."""
    h, c = 4, 5
    _, rowptr, col = _csr()
    xl, a_src, a_dst, _ = gat1_ref.sweep_inputs(h, c, N, INPUT_SEED)
    plain = gat_composition(xl, a_src, a_dst, rowptr, col, multipliers(rowptr, col, h, True, 1e-9, SEED))
    dropped = gat_composition(xl, a_src, a_dst, rowptr, col, multipliers(rowptr, col, h, True, 0.5, SEED))
    assert np.array_equal(plain[1], dropped[1]) and not np.array_equal(plain[0], dropped[0])


def test_new_entry_points_reject_bad_arguments_without_device_work():
    lib = _C.load()
    names = ("egc_gat_forward_dropout_f32", "egc_gat_backward_dropout_f32", "egc_gatv2_forward_dropout_f32",
             "egc_gatv2_backward_dropout_f32")
    for sym in names:
        assert sym in _C.SYMBOLS and getattr(lib, sym) is not None
    INVALID = 1
    seed = torch.zeros(1, dtype=torch.int64).data_ptr()       # never followed: nothing is launched below
    idx = torch.zeros(4, dtype=torch.int32).data_ptr()

    def fwd1(p=0.5, seed=seed, n_rows=0):
        return lib.egc_gat_forward_dropout_f32(None, None, n_rows, 0, n_rows, None, 8, None, 2, None, 2, 2, 4, 0.2, 1, None, 8, None, None, 0,
                                               p, seed, None)

    def fwd2(p=0.5, seed=seed, n_rows=0):
        return lib.egc_gatv2_forward_dropout_f32(None, None, n_rows, 0, n_rows, None, 8, None, 8, None, 2, 4, 0.2, 1, None, 8, None, None, 0,
                                                 p, seed, None)

    def bwd1(p=0.5, seed=seed, t_rowptr=None, t_edge_id=None, n_rows=0, ld_xl=8):
        return lib.egc_gat_backward_dropout_f32(None, None, t_rowptr, None, t_edge_id, n_rows, 0, None, ld_xl, None, 2, None, 2, 2, 4, 0.2, 1,
                                                None, 8, None, None, 8, None, 8, None, 2, None, 2, None, 0, p, seed, None)

    def bwd2(p=0.5, seed=seed, t_rowptr=None, t_edge_id=None, n_rows=0, ld_xl=8):
        return lib.egc_gatv2_backward_dropout_f32(None, None, t_rowptr, None, t_edge_id, n_rows, 0, None, ld_xl, None, 8, None, 2, 4, 0.2, 1,
                                                  None, 8, None, None, 8, None, 8, None, 8, None, None, 0, p, seed, None)

    for f in (fwd1, fwd2, bwd1, bwd2):
        assert f() == 0, f.__name__                                       # nothing to do, and the arguments are fine
        for p in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
            assert f(p=p) == INVALID, (f.__name__, p)                     # p outside (0, 1)
        assert f(seed=None) == INVALID, f.__name__                        # no seed
        assert f(p=1e-9) == 0 and f(p=1.0 - 2.0 ** -53) == 0, f.__name__
    for f in (fwd1, fwd2):
        assert f(n_rows=4) == INVALID                                     # the plain checks still run: rows to do and no pointers
    for f in (bwd1, bwd2):
        assert f(t_rowptr=idx) == INVALID                                 # a transposed CSR without its entries' forward positions
        assert f(t_rowptr=idx, t_edge_id=idx) == 0
        assert f(ld_xl=7) == INVALID                                      # the plain checks still run


def test_functions_want_a_seed_with_dropout():
    xl, a, ei = torch.randn(5, 8), torch.randn(5, 2), torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="seed"):
        gat_aggregate(xl, a, a, ei, dropout=0.5)
    with pytest.raises(RuntimeError, match="seed"):
        gatv2_aggregate(xl, xl, torch.randn(2, 4), ei, dropout=0.5)
    with pytest.raises(RuntimeError, match="int64"):
        gat_aggregate(xl, a, a, ei, dropout=0.5, seed=torch.zeros(1))
    with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
        gat_aggregate(xl, a, a, ei, dropout=1.0, seed=torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("cls", (egc_amd.GATConv, egc_amd.GATv2Conv))
def test_modules_host_side(cls):
    """State dicts know nothing of dropout and no seed is drawn before a training forward.  What raised before the layers had a
    dropout path still raises the same way: dropout in training on a tensor off the device, and a ``.dropout`` assigned after
    construction (the layer's dropout is its constructor's); eval mode ignores both."""
    torch.manual_seed(0)
    layer, plain = cls(6, 4, heads=2, dropout=0.6), cls(6, 4, heads=2)
    assert layer.dropout == 0.6 and layer.last_dropout_seed is None
    assert set(layer.state_dict()) == set(plain.state_dict())
    plain.load_state_dict(layer.state_dict(), strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, plain.state_dict()[k]), k
    ei = torch.zeros((2, 3), dtype=torch.int64)
    for built in (layer, cls(6, 4, heads=2, dropout=1.0)):
        with pytest.raises(NotImplementedError, match="attention dropout .* not implemented for tensors on cpu"):
            built(torch.randn(5, 6), ei)
    assert layer.last_dropout_seed is None
    for changed, p in ((plain, 0.6), (layer, 0.3), (layer, 0.0)):
        changed.dropout = p
        with pytest.raises(NotImplementedError, match="attention dropout changed after construction"):
            changed(torch.randn(5, 6), ei)
        with pytest.raises(RuntimeError) as info:                # eval mode: past the dropout check, to the device check
            changed.eval()(torch.randn(5, 6), ei)
        assert not isinstance(info.value, NotImplementedError)
        changed.train()
