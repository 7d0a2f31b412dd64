"""The Mpnn message kernels (egc_mpnn.hip) on the GPU at every row length and width they dispatch on: the ladder graph of
tests/mpnn_ref.py (one row of each of 0, 1, 7, 8, 9, 15, 16, 17, CHUNK - 1 .. CHUNK + 1, 2 CHUNK - 1 .. 2 CHUNK + 1, 3 CHUNK and
2 CHUNK + 18 entries; long rows first, last, adjacent, on / one past / one before a slot boundary; rectangular) and its flip
(the ladder in the transposed CSR the backward walks), add / mean / max, the 16-byte and the 4-byte path, one lane to more
lanes than a workgroup, plus what no fixture runs: the 4-byte path taken for an address or a stride, the backward with one
gradient wanted, and the same rows elsewhere in the grid.  tests/test_mpnn_shapes_cpu.py checks that the graph and the width
table reach what they claim.

Two checks per case.  Bits: m, arg, d P, d Q ``torch.equal`` to the sequential float32 restatement (message_forward /
message_backward) -- the kernels document their summation order.  Values, the project's rule with the fixture constant replaced by
a measurement made here: the truth is the same restatement in float64 on the same float32 inputs, the yardstick the float32
restatement's own distance from it, and per quantity  error <= max(1e-5, 5 x yardstick)  (rel_out for m, rel_grad for d P and
d Q); the max argument is compared exactly with both restatements."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from egc_amd._mpnn import _launch_backward, mpnn_message, mpnn_message_arg, mpnn_message_backward
from mpnn_ref import CHUNK, WIDTHS, ladder_graph, ladder_inputs, message_backward, message_forward, rel_grad, rel_out, tie_counts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED = 11, 12
AGGRS = ("add", "mean", "max")
BOTH = (False, True)                                     # the ladder in the forward CSR, in the transposed one
REDUCED = (("max_len", 2 * CHUNK + 1),)                  # the graph of the two widths above 1024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def graph(flip=False, variant=()):
    """(edge_index, n_dst, n_src) of ladder_graph(GRAPH_SEED, flip, **dict(variant))"""
    ei, n_dst, n_src = ladder_graph(GRAPH_SEED, flip=flip, **dict(variant))
    return _frozen(ei)[0], n_dst, n_src


@functools.lru_cache(maxsize=None)
def device_graph(flip=False, variant=()):
    ei, n_dst, n_src = graph(flip, variant)
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n_dst, n_src)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n_dst, n_src, ei.shape[1])
    return g


@functools.lru_cache(maxsize=None)
def inputs(flip, variant, width, ties=False):
    _, n_dst, n_src = graph(flip, variant)
    return _frozen(*ladder_inputs(n_dst, n_src, width, INPUT_SEED, ties=ties))


@functools.lru_cache(maxsize=None)
def reference(flip, variant, width, aggr, ties=False):
    """{dtype: (m, arg, d P, d Q)} of the restatement in float64 (the truth) and float32 (the bits, and the yardstick)."""
    ei, n_dst, n_src = graph(flip, variant)
    P, Q, dm = inputs(flip, variant, width, ties)
    ref = {}
    for dtype in (np.float64, np.float32):
        m, arg = message_forward(P, Q, ei, aggr, CHUNK, dtype)
        ref[dtype] = _frozen(m, arg, *message_backward(dm, ei, aggr, arg, CHUNK, dtype, n_src=n_src))
    if aggr == "max":      # comparing float32 values in float64 selects the same entries
        assert np.array_equal(ref[np.float32][1], ref[np.float64][1])
    return ref


def device_run(flip, variant, width, aggr, ties=False, arrays=None):
    """(m, arg or None, d P, d Q) of the forward and the backward kernel (the backward fed the device's own arg)."""
    g = device_graph(flip, variant)
    P, Q, dm = (_dev(a) for a in inputs(flip, variant, width, ties)) if arrays is None else arrays
    arg = None
    m = mpnn_message(P, Q, g, aggr)
    if aggr == "max":
        m2, arg = mpnn_message_arg(P, Q, g)
        assert torch.equal(m2, m) and arg.dtype == torch.int32
    dP, dQ = mpnn_message_backward(dm, g, aggr, arg)
    assert m.shape == dQ.shape == (g.n_nodes, width) and dP.shape == (g.n_src_rows, width)      # rectangular: d P has P's rows
    assert arg is None or arg.shape == m.shape
    return m, arg, dP, dQ


def check(tag, got, ref):
    """Bits against the float32 restatement, then measured / yardstick / bound of m, d P, d Q against the float64 one."""
    m, arg, dP, dQ = got
    want, truth = ref[np.float32], ref[np.float64]
    if want[1] is not None:
        assert torch.equal(arg.cpu(), torch.from_numpy(want[1])), f"{tag}: arg"
        assert np.array_equal(arg.cpu().numpy(), truth[1]), f"{tag}: arg against float64"
    else:
        assert arg is None
    bad = []
    for k, i, t, dist in (("m", 0, m, rel_out), ("d P", 2, dP, rel_grad), ("d Q", 3, dQ, rel_grad)):
        measured, yard = dist(t.cpu().numpy(), truth[i]), dist(want[i], truth[i])
        bound = max(1e-5, 5.0 * yard)
        print(f"{tag} {k}: measured {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not torch.equal(t.cpu(), torch.from_numpy(want[i])):
            bad.append(f"{k}: not the bits of the documented order ({int((t.cpu() != torch.from_numpy(want[i])).sum())} elements differ)")
        if not measured <= bound:
            bad.append(f"{k}: error {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _tag(flip, variant, width, aggr, ties=False):
    lanes = (width + 3) // 4
    return (f"{aggr} width {width} ({lanes} lane{'s' if lanes > 1 else ''}, {'vec' if width % 4 == 0 else 'scalar'}) "
            f"{'flip' if flip else 'ladder'}{''.join(' ' + k for k, _ in variant)}{' ties' if ties else ''}")


# ------------------------------------------------------------------------------------------------------ a. the degree sweep

DEGREE_CASES = (((), 8), ((), 6), ((("tail_empty", True),), 8), ((("pad_to_chunk", True),), 8))


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("variant,width", DEGREE_CASES, ids=lambda v: str(v) if isinstance(v, int) else ("-".join(k for k, _ in v) or "default"))
def test_degree_sweep(variant, width, aggr, flip):
    ei, n_dst, n_src = graph(flip, variant)
    assert n_dst != n_src and (ei.shape[1] % CHUNK == 0) == (variant == (("pad_to_chunk", True),))
    check(_tag(flip, variant, width, aggr), device_run(flip, variant, width, aggr), reference(flip, variant, width, aggr))


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (8, 6))
def test_degree_sweep_max_with_ties(width, flip):
    """P of small integers: maxima tied between different edges and, on the ladder, between different chunks of one row -- the
    first entry wins inside a chunk, the first chunk between chunks, and the backward routes d m to that one edge."""
    ei, n_dst, n_src = graph(flip)
    edges, chunks = tie_counts(inputs(flip, (), width, True)[0], ei, n_dst)
    assert edges > 0 and (flip or chunks > 0)
    check(_tag(flip, (), width, "max", True), device_run(flip, (), width, "max", True), reference(flip, (), width, "max", True))


# ------------------------------------------------------------------------------------------------------- b. the width sweep

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("aggr", ("mean", "max"))
@pytest.mark.parametrize("width", WIDTHS)
def test_width_sweep(width, aggr, flip):
    variant = REDUCED if width > 1024 else ()
    check(_tag(flip, variant, width, aggr), device_run(flip, variant, width, aggr), reference(flip, variant, width, aggr))


# ----------------------------------------------------------------------------------- c. the 4-byte path taken for an address

def _block(t, cols, col):
    """t as columns col .. col + width of a fresh [rows, cols] array of sentinels"""
    big = torch.full((t.size(0), cols), -77.0, device=DEV)
    big[:, col:col + t.size(1)] = t
    return big, big[:, col:col + t.size(1)]


def _sentinels_kept(big, col, width):
    return bool((big[:, :col] == -77.0).all()) and bool((big[:, col + width:] == -77.0).all())


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("how", ("pointer", "out", "stride"))
def test_misaligned_operands_at_width_8_give_the_bits_of_aligned_ones(how, aggr, flip):
    """``pointer``: P, Q, d m are wide[:, 1:9] of a [n, 12] array (4 bytes off a 16-byte boundary, the stride a multiple of 16);
    ``out``: m, d P, d Q are written at column 1 of such an array; ``stride``: every operand is wide[:, 0:8] of a [n, 11] array
    (aligned at row 0, a stride of 44 bytes).  Each takes the 4-byte path at a width the 16-byte path takes otherwise."""
    width = 8
    g = device_graph(flip)
    want = device_run(flip, (), width, aggr)
    P, Q, dm = (_dev(a) for a in inputs(flip, (), width))
    cols, col = (11, 0) if how == "stride" else (12, 1)
    if how in ("pointer", "stride"):
        ops = []
        for t in (P, Q, dm):
            big, view = _block(t, cols, col)
            assert torch.equal(view, t) and view.stride(1) == 1
            assert (view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0) if how == "pointer" else (view.data_ptr() % 16 == 0 and view.stride(0) % 4 != 0)
            ops.append(view)
        got = device_run(flip, (), width, aggr, arrays=ops)
        for k, a, b in zip(("m", "arg", "d P", "d Q"), got, want):
            assert (a is None and b is None) or torch.equal(a, b), k
    if how in ("out", "stride"):
        big = torch.full((g.n_nodes, cols), -77.0, device=DEV)
        block = mpnn_message(P, Q, g, aggr, out=big, out_col=col)
        assert block.data_ptr() == big.data_ptr() + 4 * col and (block.data_ptr() % 16 != 0 or block.stride(0) % 4 != 0)
        assert torch.equal(block, want[0]) and _sentinels_kept(big, col, width)
        big_p = torch.full((g.n_src_rows, cols), -77.0, device=DEV)
        big_q = torch.full((g.n_nodes, cols), -77.0, device=DEV)
        _launch_backward(dm, g, {"add": _C.MPNN_ADD, "mean": _C.MPNN_MEAN, "max": _C.MPNN_MAX}[aggr], want[1],
                         big_p[:, col:col + width], big_q[:, col:col + width])
        assert torch.equal(big_p[:, col:col + width], want[2]) and _sentinels_kept(big_p, col, width)
        assert torch.equal(big_q[:, col:col + width], want[3]) and _sentinels_kept(big_q, col, width)


# ------------------------------------------------------------------------------------------------------- d. partial wants

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("width", (8, 6))
def test_one_wanted_gradient_gives_the_half_of_the_full_backward(width, aggr, flip):
    g = device_graph(flip)
    m, _, dP, dQ = device_run(flip, (), width, aggr)
    for needs in ((True, False), (False, True), (True, True)):
        P, Q, dm = (_dev(a) for a in inputs(flip, (), width))
        P.requires_grad_(needs[0]), Q.requires_grad_(needs[1])
        out = mpnn_message(P, Q, g, aggr)
        out.backward(dm)
        assert torch.equal(out.detach(), m), needs
        assert (P.grad is not None and torch.equal(P.grad, dP)) if needs[0] else P.grad is None, needs
        assert (Q.grad is not None and torch.equal(Q.grad, dQ)) if needs[1] else Q.grad is None, needs


# ------------------------------------------------------------------------------ e. the same rows elsewhere in the grid

SHIFTED = (("prepend", 300),)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("width", (8, 6, 260))
def test_rows_landing_elsewhere_in_the_grid(width, aggr, flip):
    """300 one-entry rows first: every long row's groups fall into later workgroups and its slots 300 / CHUNK further on, no
    longer aligned as in the sweep."""
    ei, n_dst, n_src = graph(flip, SHIFTED)
    assert max(n_dst, n_src) == 579 and min(n_dst, n_src) == 386
    check(_tag(flip, SHIFTED, width, aggr), device_run(flip, SHIFTED, width, aggr), reference(flip, SHIFTED, width, aggr))
