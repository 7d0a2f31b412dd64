"""The GATv2 aggregate kernels (egc_gatv2.hip) on the GPU at every head / channel geometry they dispatch on: the (H, C) table of
tests/gat_ref.py (all eight (S, VEC, SMALL) instances, every group size, heads across the slot boundary at column 256) on the
sweep graph (rows of three chunks both ways, self loops, duplicates, empty rows), plus the paths no fixture takes: misaligned
operands at an aligned width, the backward with only some gradients wanted, the d att sum over more than 64 workgroup partials,
rows landing elsewhere in the grid, and the forward on a rectangular graph.

Rule (a), the project's bound with the fixture constant replaced by a measurement of the REFERENCE made here: the truth is the
float64 restatement (gat_ref.aggregate_forward / aggregate_backward) on the same float32 inputs, the yardstick the same two
functions in float32, and per quantity  error <= max(1e-5, 5 x the float32 restatement's own distance from float64)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._gat import gatv2_aggregate, gatv2_aggregate_backward, gatv2_aggregate_lse
from gat_ref import (CHUNK, SWEEP_SHAPES, aggregate_backward, aggregate_forward, datt_partials, geometry, rel_grad, rel_out, sweep_graph,
                     sweep_inputs)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED = 5, 7
LOOPS = (True, False)


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def graph(n=40):
    return _frozen(sweep_graph(GRAPH_SEED, n)[0])[0]


@functools.lru_cache(maxsize=None)
def inputs(h, c, n=40):
    return _frozen(*sweep_inputs(h, c, n, INPUT_SEED))


@functools.lru_cache(maxsize=None)
def reference(h, c, loops, n=40):
    """{dtype: (out, lse, d xl, d xr, d att)} of the restatement in float64 (the truth) and float32 (the yardstick), each
    backward fed its own forward's out and lse."""
    xl, xr, gout, att = inputs(h, c, n)
    ref = {}
    for dtype in (np.float64, np.float32):
        out, lse = aggregate_forward(xl, xr, att, graph(n), loops=loops, dtype=dtype)
        ref[dtype] = _frozen(out, lse, *aggregate_backward(xl, xr, att, graph(n), out, lse, gout, loops=loops, dtype=dtype))
    return ref


def lse_distance(a, b):
    """(the -inf positions agree, max |a - b| over the finite entries relative to max(1, max |b|))"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    same = np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb])
    both = fa & fb
    return same, (rel_out(a[both], b[both]) if both.any() else 0.0)


def device_run(h, c, loops, n=40, ei=None, arrays=None):
    """(out, lse, d xl, d xr, d att) of the forward kernels and of the backward kernels fed the device's own out and lse."""
    xl, xr, gout, att = (_dev(a) for a in (inputs(h, c, n) if arrays is None else arrays))
    ei = _dev(graph(n) if ei is None else ei)
    out, lse = gatv2_aggregate_lse(xl, xr, att, ei, add_self_loops=loops)
    dxl, dxr, datt = gatv2_aggregate_backward(xl, xr, att, ei, out, lse, gout, add_self_loops=loops)
    assert out.shape == (n, h * c) and lse.shape == (n, h) and dxl.shape == dxr.shape == out.shape and datt.shape == (h, c)
    return out, lse, dxl, dxr, datt


def check_rule_a(tag, got, ref, names):
    """Prints measured / yardstick / bound of every named quantity, then asserts all of them."""
    dist = dict(out=rel_out, lse=lambda a, b: lse_distance(a, b)[1], dxl=rel_grad, dxr=rel_grad, datt=rel_grad)
    order = ("out", "lse", "dxl", "dxr", "datt")
    bad = []
    for k in names:
        truth, yard32 = ref[np.float64][order.index(k)], ref[np.float32][order.index(k)]
        measured, yard = dist[k](got[k], truth), dist[k](yard32, truth)
        bound = max(1e-5, 5.0 * yard)
        print(f"{tag} {k}: measured {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not measured <= bound:
            bad.append(f"{k}: error {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _tag(h, c, loops):
    g = geometry(h, c)
    return f"H {h} C {c} (S {g['S']} G {g['G']} {'vec' if g['vec_by_width'] else 'scalar'}{' small' if g['small'] else ''}) loops {int(loops)}"


# --------------------------------------------------------------------------------------------- a. the sweep against float64

@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=_id)
def test_forward_and_backward_match_float64(shape, loops):
    h, c = shape
    ref = reference(h, c, loops)
    got = dict(zip(("out", "lse", "dxl", "dxr", "datt"), (t.cpu().numpy() for t in device_run(h, c, loops))))
    same, _ = lse_distance(got["lse"], ref[np.float64][1])
    assert same, "lse is -inf at other positions than the reference's"
    empty = ~np.isfinite(got["lse"])                                             # [n, H]
    if loops:
        assert not empty.any()
    else:
        assert int(empty.all(axis=1).sum()) >= 3
        assert float(np.abs(got["out"].reshape(-1, h, c)[empty]).max()) == 0.0  # exactly 0 where lse is -inf
    assert all(np.isfinite(got[k]).all() for k in ("out", "dxl", "dxr", "datt"))
    check_rule_a(_tag(h, c, loops), got, ref, ("out", "lse", "dxl", "dxr", "datt"))


# ------------------------------------------------------------------------- b. misaligned operands at an aligned width

@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("shape", ((2, 8), (1, 256), (2, 256)), ids=_id)
def test_misaligned_operands_give_the_bits_of_aligned_ones(shape, loops):
    """xl, xr and d out as columns 1 .. w of [n, w + 3] arrays: pointers 4 bytes off a 16-byte boundary and strides that are no
    multiple of 4, so the 4-byte path runs at a width the 16-byte path takes otherwise.  Both promise the same order."""
    h, c = shape
    w = h * c
    assert geometry(h, c)["vec_by_width"]
    want = device_run(h, c, loops)
    xl, xr, gout, att = (_dev(a) for a in inputs(h, c))
    ei = _dev(graph())
    off = []
    for t in (xl, xr, gout):
        big = torch.full((t.size(0), w + 3), float("nan"), device=DEV)
        big[:, 1:1 + w] = t
        off.append(big[:, 1:1 + w])
        assert off[-1].data_ptr() % 16 == 4 and off[-1].stride(0) % 4 != 0 and off[-1].stride(1) == 1 and torch.equal(off[-1], t)
    out, lse = gatv2_aggregate_lse(off[0], off[1], att, ei, add_self_loops=loops)
    got = (out, lse) + tuple(gatv2_aggregate_backward(off[0], off[1], att, ei, out, lse, off[2], add_self_loops=loops))
    for k, a, b in zip(("out", "lse", "d xl", "d xr", "d att"), got, want):
        assert torch.equal(a, b), k


# ----------------------------------------------------------------------------------------- c. wanted-gradient subsets

@pytest.mark.parametrize("shape", ((4, 5), (1, 260), (7, 3)), ids=_id)
def test_every_subset_of_wanted_gradients_gives_the_bits_of_all_three(shape):
    h, c = shape
    ei, gout = _dev(graph()), _dev(inputs(h, c)[2])

    def run(needs):
        leaves = [_dev(a).requires_grad_(need) for a, need in zip((inputs(h, c)[0], inputs(h, c)[1], inputs(h, c)[3]), needs)]
        out = gatv2_aggregate(*leaves, ei, add_self_loops=True)
        out.backward(gout)
        return out.detach(), [t.grad for t in leaves]

    out_all, grads_all = run((True, True, True))
    assert all(g is not None for g in grads_all)
    subsets = [s for s in itertools.product((False, True), repeat=3) if any(s)]
    assert len(subsets) == 7
    for needs in subsets:
        out, grads = run(needs)
        assert torch.equal(out, out_all), needs
        for name, need, g, g_all in zip(("d xl", "d xr", "d att"), needs, grads, grads_all):
            if need:
                assert g is not None and g.shape == g_all.shape and torch.equal(g, g_all), (needs, name)
            else:
                assert g is None, (needs, name)


# ------------------------------------------------------------------------------------------ d. the two-level d att sum

@pytest.mark.parametrize("shape,levels", (((3, 43), 2), ((1, 3), 1)), ids=("3x43", "1x3"))
def test_d_att_summed_over_many_workgroups(shape, levels):
    """300 rows: at G = 64 (4 rows a workgroup) more than 64 partials, which the block sum takes in two levels; at G = 1 a
    workgroup's partial is itself the sum over 256 groups."""
    h, c = shape
    n, loops = 300, True
    parts = datt_partials(h, c, n, graph(n).shape[1])
    assert geometry(h, c)["G"] == (64 if levels == 2 else 1) and graph(n).shape[1] > CHUNK
    assert (64 < parts <= 64 * 64) if levels == 2 else parts == 3
    runs = [device_run(h, c, loops, n) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    got = dict(zip(("out", "lse", "dxl", "dxr", "datt"), (t.cpu().numpy() for t in runs[0])))
    check_rule_a(f"n {n}, {parts} partials, " + _tag(h, c, loops), got, reference(h, c, loops, n), ("out", "lse", "dxl", "dxr", "datt"))


# ---------------------------------------------------------------------------------------------------- e. row placement

@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("shape", ((12, 5), (3, 100), (128, 3)), ids=_id)
def test_a_row_gives_the_same_bits_wherever_it_lands(shape, loops):
    """Nodes relabelled i -> (i + 3) mod n, the edge list's order kept: out, lse and d xr of every row are the unshifted run's
    (the order of a row's sums depends on H and C only).  No claim for d xl and d att, whose entry order follows the labels."""
    h, c = shape
    n, shift = 40, 3
    base = device_run(h, c, loops)
    arrays = tuple(np.roll(a, shift, axis=0) for a in inputs(h, c)[:3]) + (inputs(h, c)[3],)
    moved = device_run(h, c, loops, ei=(graph() + shift) % n, arrays=arrays)
    for k, i in (("out", 0), ("lse", 1), ("d xr", 3)):
        assert torch.equal(moved[i], torch.roll(base[i], shift, dims=0)), k


# ------------------------------------------------------------------------------------------------ f. rectangular forward

N_DST, N_SRC = 40, 23


@functools.lru_cache(maxsize=None)
def rect_graph():
    """[2, E]: 200 random entries from 23 source rows into destinations 0 .. 36 and one destination of 2 CHUNK + 9 entries."""
    rng = np.random.default_rng(GRAPH_SEED + 1)
    hub, long_row = 4, 2 * CHUNK + 9
    dst = rng.choice(np.array([i for i in range(N_DST - 3) if i != hub]), 200)
    ei = np.concatenate([np.stack([rng.integers(0, N_SRC, 200), dst]), np.stack([rng.integers(0, N_SRC, long_row), np.full(long_row, hub)])],
                        axis=1).astype(np.int64)
    return _frozen(np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]))[0]


@pytest.mark.parametrize("shape", ((4, 5), (1, 260)), ids=_id)
def test_forward_on_a_rectangular_graph(shape):
    h, c = shape
    xl, xr, _, att = inputs(h, c, N_DST)
    xl, ei = xl[:N_SRC], rect_graph()
    assert ei[0].max() == N_SRC - 1 and ei[1].max() < N_DST - 3 and np.bincount(ei[1]).max() == 2 * CHUNK + 9
    ref = {dtype: aggregate_forward(xl, xr, att, ei, loops=False, dtype=dtype) for dtype in (np.float64, np.float32)}
    adj = egc_amd.SparseTensor(row=_dev(ei[1]), col=_dev(ei[0]), sparse_sizes=(N_DST, N_SRC))
    assert (adj.graph.n_nodes, adj.graph.n_src_rows) == (N_DST, N_SRC)
    out, lse = gatv2_aggregate_lse(_dev(xl), _dev(xr), _dev(att), adj, add_self_loops=False)
    assert out.shape == (N_DST, h * c) and lse.shape == (N_DST, h)
    got = dict(out=out.cpu().numpy(), lse=lse.cpu().numpy())
    same, _ = lse_distance(got["lse"], ref[np.float64][1])
    empty = ~np.isfinite(got["lse"])
    assert same and int(empty.all(axis=1).sum()) >= 3 and float(np.abs(got["out"].reshape(-1, h, c)[empty]).max()) == 0.0
    check_rule_a(f"[{N_DST}, {N_SRC}] " + _tag(h, c, False), got, ref, ("out", "lse"))
    with pytest.raises(RuntimeError, match="square"):
        gatv2_aggregate_lse(_dev(xl), _dev(xr), _dev(att), adj, add_self_loops=True)
