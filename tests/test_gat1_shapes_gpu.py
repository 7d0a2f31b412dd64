"""The GAT v1 aggregate kernels (egc_gat.hip) on their own on the GPU at every head / channel geometry they dispatch on: the
(H, C) table of tests/gat1_ref.py (all eight (S, VEC, SMALL) instances, every group size, heads across the slot boundary at
column 256, the reference's six shapes) on the sweep graph (n = 40, E = 1,234, rows of 2 CHUNK + 9 entries both ways, self loops,
duplicates, empty rows), with column-block strides and with misaligned 4-byte views; and the backward with only some of its
three gradients wanted.

The truth is the float64 restatement (gat1_ref.aggregate_forward / aggregate_backward) on the same float32 inputs, the yardstick
the same two functions in float32, and per quantity  error <= max(1e-5, 5 x the float32 restatement's own distance from float64)."""
import itertools

import numpy as np
import pytest
import torch

from egc_amd._gat import gat_aggregate, gat_aggregate_backward, gat_aggregate_lse
from gat1_ref import DISTANCE, QUANTITIES, SWEEP_SHAPES, geometry, lse_distance, sweep_graph, sweep_inputs, sweep_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED, N = 5, 7, 40
LOOPS = (True, False)


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tag(h, c, loops):
    g = geometry(h, c)
    return f"H {h} C {c} (S {g['S']} G {g['G']} {'vec' if g['vec_by_width'] else 'scalar'}{' small' if g['small'] else ''}) loops {int(loops)}"


def device_run(h, c, loops, layout):
    """(out, lse, d xl, d a_src, d a_dst) of the forward kernels and of the backward kernels fed the device's own out and lse.
    layout "dense": four contiguous arrays; "blocks": xl, a_src and a_dst as the column blocks of one [n, ext_width] array (the
    layer's layout) and d out as a column block too; "off": every operand as columns 1 .. of an array three columns wider --
    pointers 4 bytes off a 16-byte boundary and strides that are no multiple of 4, so the 4-byte path runs at every width."""
    xl, a_src, a_dst, gout = (_dev(a) for a in sweep_inputs(h, c, N, INPUT_SEED))
    ei = _dev(sweep_graph(GRAPH_SEED, N)[0])
    w = h * c
    if layout == "blocks":
        ext = torch.full((N, geometry(h, c)["ext_width"]), float("nan"), device=DEV)
        ext[:, :w], ext[:, w:w + h], ext[:, w + h:w + 2 * h] = xl, a_src, a_dst
        xl, a_src, a_dst = ext[:, :w], ext[:, w:w + h], ext[:, w + h:w + 2 * h]
        big = torch.full((N, w + 4), float("nan"), device=DEV)
        big[:, 4:] = gout
        gout = big[:, 4:]
        assert xl.stride(0) == ext.size(1) and gout.stride(0) == w + 4
    elif layout == "off":
        views = []
        for t in (xl, a_src, a_dst, gout):
            big = torch.full((t.size(0), t.size(1) + 3), float("nan"), device=DEV)
            big[:, 1:1 + t.size(1)] = t
            views.append(big[:, 1:1 + t.size(1)])
            assert views[-1].data_ptr() % 16 == 4 and views[-1].stride(1) == 1 and torch.equal(views[-1], t)
        xl, a_src, a_dst, gout = views
    out, lse = gat_aggregate_lse(xl, a_src, a_dst, ei, add_self_loops=loops)
    dxl, das, dad = gat_aggregate_backward(xl, a_src, a_dst, ei, out, lse, gout, add_self_loops=loops)
    assert out.shape == (N, w) == dxl.shape and lse.shape == (N, h) == das.shape == dad.shape
    return out, lse, dxl, das, dad


def check(tag, got, ref, h, c, loops):
    """Prints measured / yardstick / bound of every quantity, then asserts all of them."""
    same, _ = lse_distance(got["lse"], ref[np.float64][1])
    assert same, "lse is -inf at other positions than the reference's"
    empty = ~np.isfinite(got["lse"])                                             # [n, H]
    if loops:
        assert not empty.any()
    else:
        assert int(empty.all(axis=1).sum()) >= 3
        assert float(np.abs(got["out"].reshape(-1, h, c)[empty]).max()) == 0.0  # exactly 0 where lse is -inf
        assert float(np.abs(got["dad"][empty]).max()) == 0.0
    assert all(np.isfinite(got[k]).all() for k in ("out", "dxl", "das", "dad"))
    bad = []
    for i, k in enumerate(QUANTITIES):
        truth, yard32 = ref[np.float64][i], ref[np.float32][i]
        measured, yard = DISTANCE[k](got[k], truth), DISTANCE[k](yard32, truth)
        bound = max(1e-5, 5.0 * yard)
        print(f"{tag} {k}: measured {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not measured <= bound:
            bad.append(f"{k}: error {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=_id)
def test_forward_and_backward_match_float64(shape, loops):
    """Dense arrays against the float64 restatement; then the column-block layout and the misaligned 4-byte views, which promise
    the same order of every sum: the bits of the dense run, and so its distances."""
    h, c = shape
    dense = device_run(h, c, loops, "dense")
    check(_tag(h, c, loops), dict(zip(QUANTITIES, (t.cpu().numpy() for t in dense))), sweep_reference(h, c, loops), h, c, loops)
    for layout in ("blocks", "off"):
        for k, a, b in zip(QUANTITIES, device_run(h, c, loops, layout), dense):
            assert torch.equal(a, b), (layout, k)


@pytest.mark.parametrize("shape", ((4, 5), (1, 260), (7, 3)), ids=_id)
def test_every_subset_of_wanted_gradients_gives_the_bits_of_all_three(shape):
    """The backward skips what nobody wants (the destination pass's entries when only D is needed, the source pass's per-entry
    head sum without d a_src, either pass as a whole): what is left has the bits of the full backward."""
    h, c = shape
    arrays = sweep_inputs(h, c, N, INPUT_SEED)
    ei, gout = _dev(sweep_graph(GRAPH_SEED, N)[0]), _dev(arrays[3])

    def run(needs):
        leaves = [_dev(a).requires_grad_(need) for a, need in zip(arrays[:3], needs)]
        out = gat_aggregate(*leaves, ei, add_self_loops=True)
        out.backward(gout)
        return out.detach(), [t.grad for t in leaves]

    out_all, grads_all = run((True, True, True))
    assert all(g is not None for g in grads_all)
    subsets = [s for s in itertools.product((False, True), repeat=3) if any(s)]
    assert len(subsets) == 7
    for needs in subsets:
        out, grads = run(needs)
        assert torch.equal(out, out_all), needs
        for name, need, g, g_all in zip(("d xl", "d a_src", "d a_dst"), needs, grads, grads_all):
            if need:
                assert g is not None and g.shape == g_all.shape and torch.equal(g, g_all), (needs, name)
            else:
                assert g is None, (needs, name)
