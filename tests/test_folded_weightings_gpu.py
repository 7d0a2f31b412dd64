"""The folded-weightings form of egc_layer_forward_packed (egc_hip.h): with sum and mean in the aggregator list the GEMM writes
w_sum + w_mean / max(cnt, 1) in place of the two weightings and the aggregate forms no mean.  Checked element by element against
the unfolded path through the same C ABI -- egc_basis_transform_packed (HBA weightings) + egc_aggregate_combine_f32 -- at 1e-6 of
the output scale (the products of sum and mean are reassociated, so the two are not bit-identical)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _graph_with_edge_cases(n, e, seed):
    """Heavy-tailed edges, plus a hub row of 3,000 entries (several long-row chunks, and past the 2,048 entries from which
    the graph build counts a row's entries with a whole block), a row made of self loops only, duplicate entries, and a block
    of rows without in-edges."""
    from egc_amd.workloads import heavy_tailed_graph
    ei = heavy_tailed_graph(n, e, seed=seed)
    dst = ei[1].clone()
    dst[dst >= n - 300] = 7                         # rows n-300 .. n-1 receive nothing (their entries go to row 7)
    rng = np.random.default_rng(seed)
    hub = torch.from_numpy(np.stack([rng.integers(0, n, 3000), np.full(3000, 11)]))
    selfs = torch.tensor([[13] * 5, [13] * 5])      # row 13: self loops only
    dup = torch.tensor([[5] * 4, [17] * 4])          # row 17: one source four times
    return torch.cat([torch.stack([ei[0], dst]), hub, selfs, dup], dim=1)


def _both_forms(aggrs, n, e, seed, heads=8, bases=4, module="EGConv"):
    import egc_amd
    from egc_amd import _C
    from egc_amd.functional import pack_weights
    dev = _dev()
    lib = _C.load()
    torch.manual_seed(seed)
    if module == "EGConv":
        conv = egc_amd.EGConv(128, 128, aggrs=aggrs, num_heads=heads, num_bases=bases)
    else:
        conv = egc_amd.EfficientGraphConv(128, 128, num_heads=heads, num_bases=bases, softmax_weights=False, aggrs=aggrs)
    with torch.no_grad():
        conv.bias.normal_()
    conv = conv.to(dev).eval()
    ei = _graph_with_edge_cases(n, e, seed).to(dev)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    spec = conv._spec_coo if module == "EGConv" else conv._spec
    with torch.no_grad():
        packed = conv._packed_weights()   # EGConv: (wcat, bcat); EfficientGraphConv: wcat, its Linear's bias in HBA order already
        wcat, bcat = packed if isinstance(packed, tuple) else (packed, conv.comb_weights.bias.detach())
        planes = pack_weights(spec, wcat)
        x = torch.randn(n, 128, device=dev)
    g = graph.c_struct()
    ws = torch.zeros(max(lib.egc_aggregate_workspace_bytes(C.byref(spec.c), n, ei.size(1)), 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    bias = conv.bias.detach()

    bases = torch.empty((n, spec.ldb), device=dev)
    wt = torch.empty((n, spec.w_cols), device=dev)
    ref = torch.empty((n, 128), device=dev)
    _C.check(lib.egc_basis_transform_packed(x.data_ptr(), planes.data_ptr(), bcat.data_ptr(), n, 128, spec.f_g, spec.w_cols,
                                            bases.data_ptr(), spec.ldb, wt.data_ptr(), stream), "egc_basis_transform_packed")
    _C.check(lib.egc_aggregate_combine_f32(C.byref(g), C.byref(spec.c), bases.data_ptr(), spec.ldb, wt.data_ptr(), bias.data_ptr(),
                                           ref.data_ptr(), None, None, ws.data_ptr(), ws.numel(), stream), "egc_aggregate_combine_f32")

    bases2 = torch.empty_like(bases)
    wt2 = torch.full_like(wt, float("nan"))          # whatever the layer entry leaves unwritten stays NaN
    out = torch.full((n, 128), float("nan"), device=dev)
    _C.check(lib.egc_layer_forward_packed(C.byref(g), C.byref(spec.c), x.data_ptr(), planes.data_ptr(), bcat.data_ptr(),
                                          bias.data_ptr(), bases2.data_ptr(), spec.ldb, wt2.data_ptr(), out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream), "egc_layer_forward_packed")
    torch.cuda.synchronize()
    return ref.cpu().numpy(), out.cpu().numpy(), wt.cpu().numpy(), wt2.cpu().numpy(), bases.cpu().numpy(), bases2.cpu().numpy()


def _scale_err(got, ref):
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("n,e", [(169343, 1164528), (20000, 150000)])
def test_folded_layer_matches_unfolded(n, e):
    """Config-2 shape (d = 128, H8 B4, sum+mean+max+symnorm): the folded layer forward against the unfolded two calls."""
    ref, out, wt, wt2, b, b2 = _both_forms(["sum", "mean", "max", "symnorm"], n, e, seed=3)
    assert np.array_equal(b, b2), "the bases columns of the GEMM are not part of the fold"
    err = _scale_err(out, ref)
    assert err <= TOL, f"folded vs unfolded: {err:.3e} of the output scale"
    # the folded intermediate is [N, H B 3]: (h, b) pairs in HBA order, (sum + mean / cnt, max, symnorm) in each
    w3 = wt2.reshape(-1)[: n * 96].reshape(n, 32, 3)
    w4 = wt.reshape(n, 32, 4)
    assert np.array_equal(w3[:, :, 1:], w4[:, :, 2:]), "the max / symnorm weightings pass through unchanged"
    assert np.isnan(wt2.reshape(-1)[n * 96:]).all(), "nothing written past N x 96"


def test_folded_layer_order_of_aggregators():
    """mean before sum in the list (a different place of each in the pair's quad); the fold must have been taken."""
    n = 20000
    ref, out, wt, wt2, *_ = _both_forms(["mean", "symnorm", "sum", "max"], n, 150000, seed=4)
    err = _scale_err(out, ref)
    assert err <= TOL, f"folded vs unfolded: {err:.3e} of the output scale"
    # folded [N, H B 3]: per pair (symnorm, sum + mean / cnt, max) -- the list without mean, in its order
    w3 = wt2.reshape(-1)[: n * 96].reshape(n, 32, 3)
    w4 = wt.reshape(n, 32, 4)
    assert np.array_equal(w3[:, :, 0], w4[:, :, 1]) and np.array_equal(w3[:, :, 2], w4[:, :, 3])
    assert not np.array_equal(w3[:, :, 1], w4[:, :, 2]), "the sum weighting carries the mean's"
    assert np.isnan(wt2.reshape(-1)[n * 96:]).all(), "nothing written past N x 96"


def test_rows_without_entries_and_hub_rows():
    """The edge-case rows alone: no in-edges, self loops only, duplicates and the hub of 3,000 entries."""
    n = 20000
    ref, out, *_ = _both_forms(["sum", "mean", "max", "symnorm"], n, 150000, seed=5)
    rows = np.r_[7, 11, 13, 17, n - 300:n]
    err = _scale_err(out[rows], ref[rows])
    assert err <= TOL, f"folded vs unfolded on the edge-case rows: {err:.3e}"


def test_without_mean_stays_unfolded():
    """No mean in the list: the layer entry is exactly the two unfolded calls (bit-identical output and weightings)."""
    ref, out, wt, wt2, *_ = _both_forms(["sum", "max", "min", "symnorm"], 20000, 150000, seed=6)
    assert np.array_equal(out, ref)
    assert np.array_equal(wt, wt2)


def test_raw_edge_set_is_not_folded_without_symnorm_over_it():
    """EfficientGraphConv's aggregators run over the RAW entries and symadd over the looped ones: the deg^-1/2 table of the
    RAW set is not the one the aggregate reads, so the layer is computed unfolded (bit-identical)."""
    ref, out, wt, wt2, *_ = _both_forms(["add", "mean", "max", "symadd"], 20000, 150000, seed=7, module="EfficientGraphConv")
    assert np.array_equal(out, ref)
    assert np.array_equal(wt, wt2)
