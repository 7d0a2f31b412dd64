"""The PNA aggregate kernels (egc_pna.hip) on the GPU at every row length and width they dispatch on: the ladder graph of
tests/mpnn_ref.py (one row of each of 0, 1, 7, 8, 9, 15, 16, 17, CHUNK - 1 .. CHUNK + 1, 2 CHUNK - 1 .. 2 CHUNK + 1, 3 CHUNK and
2 CHUNK + 18 entries; long rows first, last, adjacent, on / one past / one before a slot boundary; rectangular) and its flip (the
ladder in the transposed CSR the backward's source pass walks), with ``tail_empty`` and ``pad_to_chunk``; the full six-aggregator
list at every width of WIDTHS (the 16-byte and the 4-byte path, one lane to more lanes than a workgroup), every single aggregator
and the reference's four at widths 4, 5 and 128 (every instantiation of the kernels), and integer-valued P whose extrema tie
between edges and between chunks.

Two checks per case.  Bits: agg, arg_min, arg_max, mu, v, d P, d Q ``torch.equal`` to the sequential float32 restatement
(tests/pna_ref.py).  Values: every quantity within 1e-5 of the same restatement in float64 on the same float32 inputs, in the
distances of the Mpnn and GAT sweeps -- rel_out (max |a - b| over max(1, max |b|)) for agg, mu and v, rel_grad (over max |b|)
for d P and d Q; the bound is the flat 1e-5, not widened by the restatement's own float32 distance, which is printed beside it.
The args are compared exactly with both restatements."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._pna import pna_aggregate_saved
from pna_ref import (ALL_AGGREGATORS, CHUNK, REF_AGGREGATORS, WIDTHS, aggregate_backward, aggregate_forward, ladder_graph, ladder_inputs,
                     rel_grad, rel_out)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED = 21, 22
BOTH = (False, True)                                     # the ladder in the forward CSR, in the transposed one
REDUCED = (("max_len", 2 * CHUNK + 1),)                  # the graph of the two widths above 1024
LISTS = tuple((a,) for a in ALL_AGGREGATORS) + (REF_AGGREGATORS,)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def graph(flip=False, variant=()):
    return ladder_graph(GRAPH_SEED, flip=flip, **dict(variant))


@functools.lru_cache(maxsize=None)
def device_graph(flip=False, variant=()):
    ei, n_dst, n_src = graph(flip, variant)
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n_dst, n_src)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n_dst, n_src, ei.shape[1])
    return g


@functools.lru_cache(maxsize=None)
def inputs(flip, variant, width, n_aggr, ties=False):
    _, n_dst, n_src = graph(flip, variant)
    P, Q, _ = ladder_inputs(n_dst, n_src, width, INPUT_SEED, ties=ties)
    dagg = np.random.default_rng(INPUT_SEED + 1).standard_normal((n_dst, n_aggr * width)).astype(np.float32)
    return P, Q, dagg


def reference(flip, variant, width, aggregators, ties, dtype):
    ei, n_dst, n_src = graph(flip, variant)
    P, Q, dagg = inputs(flip, variant, width, len(aggregators), ties)
    fwd = aggregate_forward(P, Q, ei, aggregators, CHUNK, dtype)
    dP, dQ = aggregate_backward(dagg, ei, aggregators, P, fwd, CHUNK, dtype, n_src=n_src)
    return dict(fwd, dP=dP, dQ=dQ)


def run_case(flip, variant, width, aggregators, ties=False):
    g = device_graph(flip, variant)
    P, Q, dagg = (_dev(a) for a in inputs(flip, variant, width, len(aggregators), ties))
    agg, arg_min, arg_max, mu, var = pna_aggregate_saved(P, Q, g, aggregators)
    assert torch.equal(egc_amd.pna_aggregate(P, Q, g, aggregators), agg)                      # the inference form: the same bits
    dP, dQ = egc_amd.pna_aggregate_backward(dagg, g, aggregators, P=P, arg_min=arg_min, arg_max=arg_max, mu=mu, var=var)
    assert agg.shape == (g.n_nodes, len(aggregators) * width) and dP.shape == (g.n_src_rows, width) and dQ.shape == (g.n_nodes, width)
    got = dict(agg=agg, arg_min=arg_min, arg_max=arg_max, mu=mu, var=var, dP=dP, dQ=dQ)
    want, truth = (reference(flip, variant, width, aggregators, ties, dt) for dt in (np.float32, np.float64))
    tag = f"{'+'.join(aggregators)} width {width} {'flip' if flip else 'ladder'}{''.join(' ' + k for k, _ in variant)}{' ties' if ties else ''}"
    bad = []
    for k, t in got.items():
        if want[k] is None:
            assert t is None, k
            continue
        t = t.cpu().numpy()
        if not np.array_equal(t, want[k]):
            bad.append(f"{k}: not the bits of the documented order ({int((t != want[k]).sum())} of {t.size} elements differ)")
        if k.startswith("arg"):
            if not np.array_equal(t, truth[k]):
                bad.append(f"{k}: differs from the float64 restatement")
            continue
        dist = rel_grad if k in ("dP", "dQ") else rel_out
        err, yard = dist(t, truth[k]), dist(want[k], truth[k])
        print(f"{tag} {k}: measured {err:.3e}, restatement f32-vs-f64 {yard:.3e}, bound 1e-5")
        if not err <= 1e-5:
            bad.append(f"{k}: error {err:.3e} > 1e-5")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", WIDTHS)
def test_width_sweep_of_the_full_list(width, flip):
    run_case(flip, REDUCED if width > 1024 else (), width, ALL_AGGREGATORS)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (8, 6))
@pytest.mark.parametrize("variant", ((("tail_empty", True),), (("pad_to_chunk", True),)), ids=("tail_empty", "pad_to_chunk"))
def test_graph_variants_of_the_full_list(variant, width, flip):
    ei, _, _ = graph(flip, variant)
    assert (ei.shape[1] % CHUNK == 0) == (variant == (("pad_to_chunk", True),))
    run_case(flip, variant, width, ALL_AGGREGATORS)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (4, 5, 128))
@pytest.mark.parametrize("aggregators", LISTS, ids=lambda a: "+".join(a))
def test_every_instantiation(aggregators, width, flip):
    run_case(flip, (), width, aggregators)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (8, 6))
def test_ties_between_edges_and_between_chunks(width, flip):
    """P of small integers: extrema tied between different edges and, on the ladder, between different chunks of one row -- the
    first entry wins inside a chunk, the first chunk between chunks, and the backward routes the gradient to that one edge."""
    from mpnn_ref import tie_counts
    ei, n_dst, _ = graph(flip)
    edges, chunks = tie_counts(inputs(flip, (), width, 6, True)[0], ei, n_dst)
    assert edges > 0 and (flip or chunks > 0)
    run_case(flip, (), width, ALL_AGGREGATORS, ties=True)
