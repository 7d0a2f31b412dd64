"""Attention dropout of GATConv and GATv2Conv on the GPU: the DROP instances of the kernels of egc_gat.hip and egc_gatv2.hip
through the functional API, and the two modules, on the sweep graph (n = 40, E = 1,234, rows of 2 CHUNK + 9 entries both ways,
self loops, duplicates, empty rows).

The truth is the plain per-edge float64 composition of tests/gat_dropout_ref.py under the numpy mask of the same seed (it knows
nothing of the kernels' summation order), the yardstick the same composition in float32, and per quantity
error <= max(1e-5, 5 x the float32 composition's own distance from float64).  The mask's CSR is the device CSRGraph's."""
import functools
import itertools

import numpy as np
import pytest
import torch

import egc_amd
import gat1_ref
import gat_ref
from egc_amd._gat import (gat_aggregate, gat_aggregate_backward, gat_aggregate_lse, gatv2_aggregate, gatv2_aggregate_backward,
                          gatv2_aggregate_lse)
from gat_dropout_ref import SEED, edge_list, gat_composition, gatv2_composition, layer_composition, multipliers
from mpnn_ref import rel_grad, rel_out

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED, N = 5, 7, 40
SHAPES = ((1, 1), (4, 1), (12, 5), (9, 7), (1, 256), (1, 257), (8, 33), (128, 3), (170, 3), (8, 19))
PS = (0.1, 0.5, 0.9)
LOOPS = (True, False)
KINDS = ("gat", "gatv2")
NAMES = dict(gat=("out", "lse", "dxl", "das", "dad"), gatv2=("out", "lse", "dxl", "dxr", "datt"))
FORWARD = dict(gat=gat_aggregate_lse, gatv2=gatv2_aggregate_lse)
BACKWARD = dict(gat=gat_aggregate_backward, gatv2=gatv2_aggregate_backward)
AGGREGATE = dict(gat=gat_aggregate, gatv2=gatv2_aggregate)
COMPOSITION = dict(gat=gat_composition, gatv2=gatv2_composition)


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seed(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def graph():
    """(the device CSRGraph, its rowptr and col on the host): built once."""
    g = egc_amd.CSRGraph.from_edge_index(_dev(gat_ref.sweep_graph(GRAPH_SEED, N)[0]), N)
    rowptr, col = g.rowptr.cpu().numpy().astype(np.int64), g.col.cpu().numpy().astype(np.int64)[:g.n_edges]
    assert g.n_edges == 1234 and len(rowptr) == N + 1 and rowptr[-1] == 1234
    rowptr.setflags(write=False), col.setflags(write=False)
    return g, rowptr, col


@functools.lru_cache(maxsize=None)
def inputs(kind, h, c):
    """gat: (xl, a_src, a_dst, gout); gatv2: (xl, xr, att, gout)."""
    if kind == "gat":
        arrays = gat1_ref.sweep_inputs(h, c, N, INPUT_SEED)
    else:
        xl, xr, gout, att = gat_ref.sweep_inputs(h, c, N, INPUT_SEED)
        arrays = (xl, xr, att, gout)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(kind, h, c, loops, p, seed=SEED):
    """{dtype: (out, lse, three gradients)} of the composition under the numpy mask, float64 and float32; computed once."""
    _, rowptr, col = graph()
    mult = multipliers(rowptr, col, h, loops, p, seed)
    *ops, gout = inputs(kind, h, c)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        ref[dtype] = COMPOSITION[kind](*ops, rowptr, col, mult, gout, loops=loops, dtype=dtype)
        for a in ref[dtype]:
            a.setflags(write=False)
    return ref


def _layout(kind, ops, gout, h, c, layout):
    """The operands as "dense" arrays; as column "blocks" of one wider array (the layers' layout) with d out a column block too;
    or "off": columns 1 .. of an array three columns wider (pointers 4 bytes off a 16-byte boundary, strides no multiple of 4)."""
    w = h * c
    if layout == "dense":
        return ops, gout
    if layout == "off":
        views = []
        for t in tuple(ops) + (gout,):
            if t.dim() != 2 or (kind == "gatv2" and t is ops[2]):
                views.append(t)                                                     # att: dense [H, C]
                continue
            big = torch.full((t.size(0), t.size(1) + 3), float("nan"), device=DEV)
            big[:, 1:1 + t.size(1)] = t
            views.append(big[:, 1:1 + t.size(1)])
            assert views[-1].data_ptr() % 16 == 4 and torch.equal(views[-1], t)
        return views[:-1], views[-1]
    assert layout == "blocks"
    big = torch.full((N, w + 4), float("nan"), device=DEV)
    big[:, 4:] = gout
    if kind == "gat":
        ext = torch.full((N, gat1_ref.geometry(h, c)["ext_width"]), float("nan"), device=DEV)
        ext[:, :w], ext[:, w:w + h], ext[:, w + h:w + 2 * h] = ops
        return [ext[:, :w], ext[:, w:w + h], ext[:, w + h:w + 2 * h]], big[:, 4:]
    lr = torch.full((N, 2 * w), float("nan"), device=DEV)
    lr[:, :w], lr[:, w:] = ops[0], ops[1]
    return [lr[:, :w], lr[:, w:], ops[2]], big[:, 4:]


def device_run(kind, h, c, loops, p, seed=SEED, layout="dense"):
    """(out, lse, three gradients) of the forward kernels and of the backward kernels fed the device's own out and lse; p = 0:
    the plain instances."""
    g, _, _ = graph()
    *ops, gout = (_dev(a) for a in inputs(kind, h, c))
    ops, gout = _layout(kind, ops, gout, h, c, layout)
    kw = dict(add_self_loops=loops) if p == 0 else dict(add_self_loops=loops, dropout=p, seed=_seed(seed))
    out, lse = FORWARD[kind](*ops, g, **kw)
    grads = BACKWARD[kind](*ops, g, out, lse, gout, **kw)
    assert out.shape == (N, h * c) and lse.shape == (N, h)
    return (out, lse) + tuple(grads)


def check(tag, kind, got, ref):
    """Prints measured / yardstick / bound of every quantity but lse, then asserts all of them."""
    bad = []
    for i, k in enumerate(NAMES[kind]):
        if k == "lse":
            continue
        dist = rel_out if k == "out" else rel_grad
        truth, yard32 = ref[torch.float64][i], ref[torch.float32][i]
        measured, yard = dist(got[i].reshape(truth.shape), truth), dist(yard32, truth)
        bound = max(1e-5, 5.0 * yard)
        print(f"{tag} {k}: measured {measured:.3e}, composition f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not measured <= bound:
            bad.append(f"{k}: error {measured:.3e}, composition f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_float64_composition(kind, shape, p, loops):
    h, c = shape
    got = [t.cpu().numpy() for t in device_run(kind, h, c, loops, p)]
    ref = reference(kind, h, c, loops, p)
    assert all(np.isfinite(a).all() for i, a in enumerate(got) if i != 1)
    check(f"{kind} H {h} C {c} p {p} loops {int(loops)}", kind, got, ref)
    # lse is the unmasked row's, in the unchanged order: the bits of the plain kernel's
    plain_lse = device_run(kind, h, c, loops, 0)[1].cpu().numpy()
    assert np.array_equal(got[1], plain_lse)
    same, dist = gat1_ref.lse_distance(got[1], ref[torch.float64][1])
    assert same and dist <= 1e-5
    empty = ~np.isfinite(got[1])
    if loops:
        assert not empty.any()
    else:
        assert int(empty.all(axis=1).sum()) >= 3 and (got[1][empty] == -np.inf).all()
        assert float(np.abs(got[0].reshape(N, h, c)[empty]).max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_and_head_with_every_entry_dropped(kind):
    """p = 0.9: some (row, head) with entries keeps none of them.  There out is exactly 0, lse is finite, every gradient finite."""
    h, c, p, loops = 8, 19, 0.9, True
    _, rowptr, col = graph()
    _, dst, _ = edge_list(rowptr, col, loops)
    mult = multipliers(rowptr, col, h, loops, p, SEED)
    entries, kept = np.zeros((N, h)), np.zeros((N, h))
    np.add.at(entries, dst, 1.0)
    np.add.at(kept, dst, (mult > 0).astype(np.float64))
    gone = (entries > 0) & (kept == 0)
    assert gone.any(), "choose another seed: no (row, head) lost all of its entries"
    got = [t.cpu().numpy() for t in device_run(kind, h, c, loops, p)]
    assert (got[0].reshape(N, h, c)[gone] == 0.0).all() and np.isfinite(got[1][gone]).all()
    assert all(np.isfinite(a).all() for a in got)
    check(f"{kind} all-dropped", kind, got, reference(kind, h, c, loops, p))


@pytest.mark.parametrize("loops", LOOPS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", KINDS)
def test_a_tiny_p_gives_the_bits_of_the_plain_kernels(kind, shape, loops):
    """p = 1e-9 drops nothing under this seed (tests/test_gat_dropout_cpu.py) and scales by exactly 1: the DROP instances run and
    are held to the plain instances' order rules, bit for bit."""
    h, c = shape
    for name, a, b in zip(NAMES[kind], device_run(kind, h, c, loops, 1e-9), device_run(kind, h, c, loops, 0)):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", ((12, 5), (8, 33)), ids=_id)
@pytest.mark.parametrize("kind", KINDS)
def test_layouts_give_the_bits_of_the_dense_run(kind, shape):
    h, c = shape
    dense = device_run(kind, h, c, True, 0.5)
    for layout in ("blocks", "off"):
        for name, a, b in zip(NAMES[kind], device_run(kind, h, c, True, 0.5, layout=layout), dense):
            assert torch.equal(a, b), (layout, name)


@pytest.mark.parametrize("shape", ((12, 5), (8, 33)), ids=_id)
@pytest.mark.parametrize("kind", KINDS)
def test_every_subset_of_wanted_gradients_gives_the_bits_of_all_three(kind, shape):
    h, c = shape
    g, _, _ = graph()
    *ops, gout = inputs(kind, h, c)
    gout = _dev(gout)

    def run(needs):
        leaves = [_dev(a).requires_grad_(need) for a, need in zip(ops, needs)]
        out = AGGREGATE[kind](*leaves, g, add_self_loops=True, dropout=0.5, seed=_seed())
        out.backward(gout)
        return out.detach(), [t.grad for t in leaves]

    out_all, grads_all = run((True, True, True))
    assert all(t is not None for t in grads_all)
    assert torch.equal(out_all, device_run(kind, h, c, True, 0.5)[0])
    for needs in [s for s in itertools.product((False, True), repeat=3) if any(s)]:
        out, grads = run(needs)
        assert torch.equal(out, out_all), needs
        for need, t, t_all in zip(needs, grads, grads_all):
            assert (t is None) if not need else torch.equal(t, t_all), needs


@pytest.mark.parametrize("kind", KINDS)
def test_seeds(kind):
    h, c = 8, 19
    a, b = device_run(kind, h, c, True, 0.5, seed=SEED), device_run(kind, h, c, True, 0.5, seed=SEED)
    for name, x, y in zip(NAMES[kind], a, b):
        assert torch.equal(x, y), name
    other = device_run(kind, h, c, True, 0.5, seed=SEED + 1)
    assert torch.equal(other[1], a[1])                                                  # lse does not know the mask
    for name, x, y in zip(NAMES[kind], a, other):
        assert name == "lse" or not torch.equal(x, y), name
    check(f"{kind} seed + 1", kind, [t.cpu().numpy() for t in other], reference(kind, h, c, True, 0.5, SEED + 1))
    big = -(2 ** 63) + 12345                                                             # a seed with its high half and sign bit set
    check(f"{kind} negative seed", kind, [t.cpu().numpy() for t in device_run(kind, h, c, True, 0.5, seed=big)],
          reference(kind, h, c, True, 0.5, big))


# ---------------------------------------------------------------------------------------------------------------- the modules

CLASSES = dict(gat=egc_amd.GATConv, gatv2=egc_amd.GATv2Conv)
F_IN, H, C = 12, 4, 5


def _module(kind, concat, dropout):
    torch.manual_seed(3)
    layer = CLASSES[kind](F_IN, C, heads=H, concat=concat, dropout=dropout)
    with torch.no_grad():
        layer.bias.normal_()
        if kind == "gatv2":
            layer.lin_l.bias.normal_(), layer.lin_r.bias.normal_()
    return layer.to(DEV)


def _step(layer, x, g, gout):
    layer.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    out = layer(xg, g)
    out.backward(gout)
    return out.detach(), xg.grad, {k: q.grad.clone() for k, q in layer.named_parameters()}


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("kind", KINDS)
def test_modules(kind, concat):
    g, rowptr, col = graph()
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(N, F_IN, generator=gen).to(DEV)
    gout = torch.randn(N, H * C if concat else C, generator=gen).to(DEV)
    layer = _module(kind, concat, 0.6)
    assert layer.training and layer.last_dropout_seed is None

    # torch.manual_seed governs the mask: two forwards differ, re-seeding reproduces both, gradients included
    torch.manual_seed(101)
    first, second = _step(layer, x, g, gout), _step(layer, x, g, gout)
    seed2 = layer.last_dropout_seed
    assert seed2.dtype == torch.int64 and seed2.shape == (1,) and seed2.device.type == "cuda"
    assert not torch.equal(first[0], second[0])
    torch.manual_seed(101)
    for want in (first, second):
        got = _step(layer, x, g, gout)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert set(got[2]) == set(want[2]) and all(torch.equal(got[2][k], want[2][k]) for k in want[2])
    assert torch.equal(layer.last_dropout_seed, seed2)

    # against the float64 composition under the mask of last_dropout_seed
    params = {k: v.detach().cpu().numpy() for k, v in layer.state_dict().items()}
    mult = multipliers(rowptr, col, H, True, 0.6, int(seed2.item()))
    ref = {dt: layer_composition(kind, x.cpu().numpy(), params, H, C, rowptr, col, mult, gout.cpu().numpy(), concat=concat, dtype=dt)
           for dt in (torch.float64, torch.float32)}
    out, _, grads = second
    bad = []
    quantities = [("out", rel_out, out.cpu().numpy(), ref[torch.float64][0], ref[torch.float32][0])]
    quantities += [(k, rel_grad, grads[k].cpu().numpy(), ref[torch.float64][1][k], ref[torch.float32][1][k]) for k in ref[torch.float64][1]]
    assert set(grads) == set(ref[torch.float64][1])
    for name, dist, got, truth, yard32 in quantities:
        measured, yard = dist(got, truth), dist(yard32, truth)
        bound = max(1e-5, 5.0 * yard)
        print(f"{kind} concat {int(concat)} {name}: measured {measured:.3e}, composition f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not measured <= bound:
            bad.append(f"{name}: error {measured:.3e}, bound {bound:.3e}")
    assert not bad, "; ".join(bad)

    # eval mode ignores dropout: the bits of a dropout = 0 module with the same state dict (strict round trip)
    plain = _module(kind, concat, 0.0)
    plain.load_state_dict(layer.state_dict(), strict=True)
    layer.load_state_dict(plain.state_dict(), strict=True)
    assert set(layer.state_dict()) == set(plain.state_dict())
    with torch.no_grad():
        assert torch.equal(layer.eval()(x, g), plain.eval()(x, g))
        assert torch.equal(layer.eval()(x, g), plain.train()(x, g))                      # and of its training forward
    assert torch.equal(layer.last_dropout_seed, seed2)                                    # eval mode draws nothing

    # the layer's dropout is its constructor's: one assigned afterwards raises in training, as it did before; eval mode ignores it
    plain.train().dropout = 0.6
    with pytest.raises(NotImplementedError, match="attention dropout changed after construction"):
        plain(x, g)
    with torch.no_grad():
        assert torch.equal(plain.eval()(x, g), layer.eval()(x, g))

    # dropout = 1: the bias alone, zero gradients for the layer's weights
    full = _module(kind, concat, 1.0)
    out, dx, grads = _step(full, x, g, gout)
    assert torch.equal(out, full.bias.detach().expand_as(out)) and float(dx.abs().max()) == 0.0
    for k, t in grads.items():
        assert k == "bias" or float(t.abs().max()) == 0.0, k
    assert torch.allclose(grads["bias"], gout.sum(dim=0), rtol=1e-5, atol=1e-5)
