"""The gather plan of a static graph (egc_gather_plan_build) and the aggregate's PLAN form on the GPU.

Two properties, on small graphs that hit every edge the builder and the kernel have:
  * the plan read back satisfies its invariants against numpy: the table is the distinct values of the edge set's deg^-1/2 table,
    ascending by bit pattern; every entry's low bits are col[p] and table[high bits] equals edge_dis[p] bit for bit; the header's
    form is egc_gather_plan_form's answer, and a graph whose distinct values do not fit the spare bits keeps no plan;
  * the layer output with the plan is BIT-IDENTICAL to the output with EGC_NO_GATHER_PLAN=1, and the launch with the plan DID take
    the PLAN form (egc_gather_plan_launches moves by one; by none with the switch, without a plan, or for a layer whose kernel has
    no PLAN form) -- the north-star layer through both entry points (aggregate alone, unfolded four aggregators; the packed layer
    forward, which folds mean into sum), one run-time configuration each at 32- and 64-lane groups, and the ogbn-mag layer
    (44 slots: one row per wavefront) on a graph of more than 32768 rows, where a wavefront takes four row groups in turn.
Graphs: 1, 3, 5 and 67 rows; empty rows; rows of exactly 64 and 65 entries; self entries; a hub of a few hundred entries next to
short rows; sources of one degree only; more distinct degrees than the spare bits hold (min_col_bits); exactly as many as they hold
(a path: two degrees at 31 source-id bits, the index in bit 31 of the word) and one more; exactly 64 and 65 rows, most entries
reading the highest-numbered rows."""
import functools
import os

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from egc_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, M, X, Y, STD = _C.AGGR_SUM, _C.AGGR_MEAN, _C.AGGR_MAX, _C.AGGR_SYMNORM, _C.AGGR_STD
BIG_ROWS = 32768 + 37      # launch_fast gives one-row groups four rows per wavefront from 32768 rows on


def _random_graph(n, e, seed, empty_every=0):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    if empty_every:
        keep = dst % empty_every != 0          # rows without entries
        src, dst = src[keep], dst[keep]
    k = max(1, n // 3)
    loops = rng.integers(0, n, k)              # self entries
    if empty_every:
        loops = loops[loops % empty_every != 0]
    return np.stack([np.concatenate([src, loops]), np.concatenate([dst, loops])]).astype(np.int64), n


def _threshold_graph():
    """67 rows: row 3 has exactly 64 entries, row 4 exactly 65, row 10 is a hub of 300 entries, the others are short or empty."""
    rng = np.random.default_rng(5)
    n = 67
    parts = [(rng.integers(0, n, 64), np.full(64, 3)), (rng.integers(0, n, 65), np.full(65, 4)),
             (rng.integers(0, n, 300), np.full(300, 10))]
    rows = np.array([r for r in range(n) if r not in (3, 4, 10) and r % 5 != 0])
    dst = np.repeat(rows, rng.integers(1, 9, rows.size))
    parts.append((rng.integers(0, n, dst.size), dst))
    parts.append((rows[::4], rows[::4]))       # self entries
    return np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])]).astype(np.int64), n


def _regular_graph():
    """A ring with two entries per row: every source has one degree, the table one value."""
    n = 67
    r = np.arange(n)
    return np.stack([np.concatenate([(r + 1) % n, (r + n - 1) % n]), np.concatenate([r, r])]).astype(np.int64), n


def _big_graph():
    """More than 32768 rows, 0 .. 70 entries each (so some are long), a hub, self entries."""
    rng = np.random.default_rng(9)
    n = BIG_ROWS
    deg = rng.integers(0, 6, n)
    deg[rng.integers(0, n, 40)] = rng.integers(60, 71, 40)
    deg[n - 2] = 500
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, dst.size)
    src[::17] = dst[::17]
    return np.stack([src, dst]).astype(np.int64), n


def _path_graph(n=40, three_at=None):
    """A path: the end rows have one entry, the inner rows two -- two distinct degrees in either edge set, exactly what ONE spare
    bit holds.  ``three_at``: that row gets a third entry, and the graph a third degree."""
    r = np.arange(n)
    src, dst = np.concatenate([r[:-1], r[1:]]), np.concatenate([r[1:], r[:-1]])
    if three_at is not None:
        src, dst = np.append(src, (three_at + 7) % n), np.append(dst, three_at)
    return np.stack([src, dst]).astype(np.int64), n


def _top_source_graph(n):
    """Exactly ``n`` rows (64: six source-id bits, 65: seven); most entries read row 63 (and row 64 where there is one), whose own
    single entry gives it the largest deg^-1/2, the LAST table index: an all-ones source id next to a non-zero index."""
    rng = np.random.default_rng(n)
    deg = rng.integers(0, 9, n)
    deg[5], deg[63:] = 40, 1
    dst = np.repeat(np.arange(n), deg)
    hot = rng.integers(63, n, dst.size)
    src = np.where(rng.random(dst.size) < 0.6, hot, rng.integers(0, n, dst.size))
    return np.stack([src, dst]).astype(np.int64), n


GRAPHS = {
    "two_degree": _path_graph,
    "three_degree": lambda: _path_graph(three_at=11),
    "n64": lambda: _top_source_graph(64),
    "n65": lambda: _top_source_graph(65),
    "n1": lambda: (np.array([[0, 0], [0, 0]], dtype=np.int64), 1),
    "n3": lambda: _random_graph(3, 7, 1),
    "n5_empty_rows": lambda: _random_graph(5, 12, 2, empty_every=2),
    "n67": lambda: _random_graph(67, 600, 3, empty_every=7),
    "threshold_and_hub": _threshold_graph,
    "one_degree": _regular_graph,
    "big": _big_graph,
}
# (graph, min_col_bits): 31 leaves one spare bit -- two table values -- to graphs with more distinct degrees: no plan is kept
SMALL = [("n1", 0), ("n3", 0), ("n5_empty_rows", 0), ("n67", 0), ("threshold_and_hub", 0), ("one_degree", 0), ("one_degree", 31)]
UNFIT = [("n67", 31), ("threshold_and_hub", 31)]
# the exact fit n_table == 1 << (32 - cb) on a BUILT plan: two values at 31 source-id bits put the index in bit 31 of the word;
# three values there keep no plan.  64 / 65 rows: the source-id field full of ones, and one bit wider
SMALL += [("two_degree", 31), ("n64", 0), ("n65", 0)]
UNFIT += [("three_degree", 31)]
IDS = dict(ids=lambda p: f"{p[0]}-cb{p[1]}")


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The big case's arrays (46 MB of output) would stay behind as cached blocks of odd sizes; tests of other modules that
    measure peak device memory see an allocation served from such a block at the block's size.  Hand everything back."""
    yield
    static_graph.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def static_graph(name, min_col_bits=0):
    ei, n = GRAPHS[name]()
    g = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(ei).to(DEV), n).trim_launches()
    if min_col_bits:
        g.rebuild_gather_plans(min_col_bits=min_col_bits)
    torch.cuda.synchronize()
    return g


def check_plan(g, edge_set, min_col_bits=0):
    lib = _C.load()
    n, e = g.n_nodes, g.n_edges
    plan, header = g.gather_plans[edge_set]
    p = plan.cpu().numpy()
    off = [int(lib.egc_gather_plan_offset(n, e, k)) for k in range(3)]
    col = g.col.cpu().numpy()[:e]
    edis = (g.edge_dis_raw if edge_set == "raw" else g.edge_dis_looped).cpu().numpy()[:e]
    dis = (g.dis_raw if edge_set == "raw" else g.dis_looped).cpu().numpy()[:n]
    table = p[off[0]:off[0] + header[_C.GP_TABLE_SIZE]].view(np.uint32)
    words = p[off[1]:off[1] + e].view(np.uint32)
    form = int(lib.egc_gather_plan_form(n, header[_C.GP_TABLE_SIZE], min_col_bits))
    assert (header[_C.GP_FORM], header[_C.GP_COL_BITS]) == (form & 0xff, form >> 8) and header[_C.GP_FORM] == _C.GP_PACKED
    assert np.array_equal(table, np.unique(dis.view(np.uint32)))
    cb = header[_C.GP_COL_BITS]
    assert np.array_equal(words & np.uint32((1 << cb) - 1), col.astype(np.uint32))
    assert np.array_equal(table[words >> np.uint32(cb)], edis.view(np.uint32))


@pytest.mark.parametrize("case", SMALL + [("big", 0)], **IDS)
@pytest.mark.parametrize("edge_set", ["raw", "looped"])
def test_plan_invariants(case, edge_set):
    check_plan(static_graph(*case), edge_set, case[1])


@pytest.mark.parametrize("case", UNFIT, **IDS)
def test_no_plan_where_the_values_do_not_fit(case):
    g = static_graph(*case)
    n_values = np.unique(g.dis_looped.cpu().numpy()[:g.n_nodes]).size
    assert n_values > 2 and int(_C.load().egc_gather_plan_form(g.n_nodes, n_values, 31)) & 0xff == _C.GP_UNFIT
    st = g.c_struct()
    assert g.gather_plans == {} and not st.gather_plan_raw and not st.gather_plan_looped


def test_cases_reach_what_they_name():
    assert static_graph("one_degree").gather_plans["raw"][1][_C.GP_TABLE_SIZE] == 1
    assert static_graph("one_degree", 31).gather_plans["looped"][1][_C.GP_COL_BITS] == 31
    deg = np.diff(static_graph("threshold_and_hub").rowptr.cpu().numpy())
    assert {64, 65} <= set(deg.tolist()) and deg.max() >= 300
    big = np.diff(static_graph("big").rowptr.cpu().numpy())
    assert big.size >= 32768 and big.max() >= 500 and (big == 0).any() and ((big > 64) & (big < 256)).any()


def _read_back(g, edge_set):
    """(header, table, entry words) of a kept plan"""
    lib = _C.load()
    plan, header = g.gather_plans[edge_set]
    p = plan.cpu().numpy()
    off = [int(lib.egc_gather_plan_offset(g.n_nodes, g.n_edges, k)) for k in range(2)]
    return header, p[off[0]:off[0] + header[_C.GP_TABLE_SIZE]].view(np.uint32), p[off[1]:off[1] + g.n_edges].view(np.uint32)


@pytest.mark.parametrize("edge_set", ["raw", "looped"])
def test_the_exact_fit_puts_the_index_in_bit_31(edge_set):
    """two values at 31 source-id bits: n_table == 1 << (32 - cb), the plan is kept and its index bit is the word's sign bit"""
    g = static_graph("two_degree", 31)
    header, table, words = _read_back(g, edge_set)
    assert (header[_C.GP_FORM], header[_C.GP_COL_BITS], header[_C.GP_TABLE_SIZE]) == (_C.GP_PACKED, 31, 2) and len(table) == 2
    assert header[_C.GP_TABLE_SIZE] == 1 << (32 - header[_C.GP_COL_BITS])
    assert int(_C.load().egc_gather_plan_form(g.n_nodes, 3, 31)) & 0xff == _C.GP_UNFIT
    top = (words >> np.uint32(31)).astype(bool)
    assert top.any() and not top.all()
    check_plan(g, edge_set, 31)
    deg = np.diff(g.rowptr.cpu().numpy()[:g.n_nodes + 1])
    assert sorted(set(deg.tolist())) == [1, 2] and (deg[[0, -1]] == 1).all()
    three = np.diff(static_graph("three_degree", 31).rowptr.cpu().numpy()[:g.n_nodes + 1])
    assert sorted(set(three.tolist())) == [1, 2, 3] and (three == 3).sum() == 1


@pytest.mark.parametrize("layer", ["northstar_folded", "rt_32_lanes", "mag_44_slots"])
def test_aggregate_bit_identical_with_the_index_in_bit_31(layer):
    """16-, 32- and 64-lane groups; the raw plan (rt_32_lanes) and the looped one"""
    aggregate_case(static_graph("two_degree", 31), layer, 1)


@pytest.mark.parametrize("rows", [64, 65])
@pytest.mark.parametrize("edge_set", ["raw", "looped"])
def test_the_source_field_full_of_ones_next_to_an_index(rows, edge_set):
    g = static_graph(f"n{rows}")
    header, table, words = _read_back(g, edge_set)
    cb = header[_C.GP_COL_BITS]
    assert g.n_nodes == rows and cb == {64: 6, 65: 7}[rows] and len(table) > 2
    src, idx = words & np.uint32((1 << cb) - 1), words >> np.uint32(cb)
    hot = src >= 63
    assert 2 * hot.sum() > words.size and (idx[hot] != 0).all() and (src == rows - 1).any() and (src == 63).any()


# ---- the kernel: bit-identical with and without the plan, and the PLAN form did launch ----------------------------------------
LAYERS = {
    # north star (StCfg<8, 4, 16, ...>): the four aggregators unfolded; the folded list of the packed layer forward
    "northstar_unfolded": dict(f_out=128, H=8, B=4, aggrs=[S, M, X, Y], sets=(_C.SET_LOOPED, _C.SET_LOOPED)),
    "northstar_folded": dict(f_out=128, H=8, B=4, aggrs=[S, X, Y], sets=(_C.SET_LOOPED, _C.SET_LOOPED)),
    # run-time configurations: 24 slots -> 32-lane groups (raw sets: the raw plan), 48 slots -> 64-lane groups
    "rt_32_lanes": dict(f_out=96, H=4, B=4, aggrs=[S, X, Y], sets=(_C.SET_RAW, _C.SET_RAW)),
    "rt_64_lanes": dict(f_out=192, H=4, B=4, aggrs=[Y, X], sets=(_C.SET_LOOPED, _C.SET_LOOPED)),
    # the ogbn-mag layer (StCfg<8, 4, 44, 1, symnorm>): one row per wavefront
    "mag_44_slots": dict(f_out=352, H=8, B=4, aggrs=[Y], sets=(_C.SET_LOOPED, _C.SET_LOOPED)),
    # std keeps a sum of squares: its kernels have no PLAN form, the launch walks col / edge_dis
    "std_no_plan_form": dict(f_out=128, H=8, B=4, aggrs=[S, STD, X, Y], sets=(_C.SET_LOOPED, _C.SET_LOOPED)),
}


def spec_of(layer, f_in=16):
    d = LAYERS[layer]
    return F.make_spec(f_in, d["f_out"], d["H"], d["B"], d["aggrs"], d["sets"][0], d["sets"][1], True, _C.LAYOUT_HBA, _C.ACT_NONE)


def both_ways(fn, plan_launches):
    """fn() with the plan and with EGC_NO_GATHER_PLAN=1; the first takes the PLAN form ``plan_launches`` times, the second never"""
    lib = _C.load()
    assert "EGC_NO_GATHER_PLAN" not in os.environ
    c0 = int(lib.egc_gather_plan_launches())
    with_plan = fn()
    c1 = int(lib.egc_gather_plan_launches())
    os.environ["EGC_NO_GATHER_PLAN"] = "1"
    try:
        without = fn()
    finally:
        del os.environ["EGC_NO_GATHER_PLAN"]
    c2 = int(lib.egc_gather_plan_launches())
    torch.cuda.synchronize()
    assert (c1 - c0, c2 - c1) == (plan_launches, 0), "the launch did not take the form it should"
    assert torch.isfinite(without).all()
    assert torch.equal(with_plan, without), f"{(with_plan != without).sum().item()} outputs differ"


def aggregate_case(g, layer, plan_launches):
    spec = spec_of(layer)
    gen = torch.Generator().manual_seed(11)
    bases = torch.randn(g.n_nodes, spec.ldb, generator=gen).to(DEV)
    wt = torch.randn(g.n_nodes, spec.w_cols, generator=gen).to(DEV)
    bias = torch.randn(spec.f_out, generator=gen).to(DEV)

    def run():
        out = torch.full((g.n_nodes, spec.f_out), float("nan"), device=DEV)
        return F.egc_aggregate_combine(g, spec, bases, wt, bias, out=out)

    both_ways(run, plan_launches)


@pytest.mark.parametrize("case", SMALL, **IDS)
@pytest.mark.parametrize("layer", list(LAYERS))
def test_aggregate_bit_identical(case, layer):
    aggregate_case(static_graph(*case), layer, 0 if layer == "std_no_plan_form" else 1)


@pytest.mark.parametrize("layer", ["mag_44_slots", "northstar_folded"])
def test_aggregate_bit_identical_four_row_groups_per_wavefront(layer):
    aggregate_case(static_graph("big"), layer, 1)


@pytest.mark.parametrize("case", UNFIT, **IDS)
def test_aggregate_without_a_kept_plan(case):
    aggregate_case(static_graph(*case), "northstar_folded", 0)


@pytest.mark.parametrize("case", SMALL, **IDS)
def test_packed_layer_forward_bit_identical(case):
    """the folded entry point (egc_layer_forward_packed: mean folded into sum by the GEMM, three aggregators in the aggregate)"""
    g = static_graph(*case)
    spec = spec_of("northstar_unfolded", f_in=128)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(g.n_nodes, 128, generator=gen).to(DEV)
    wcat = (torch.randn(128, spec.f_g + spec.w_cols, generator=gen) / 11).to(DEV)
    bcat = torch.randn(spec.w_cols, generator=gen).to(DEV)
    bias = torch.randn(spec.f_out, generator=gen).to(DEV)
    packed = F.pack_weights(spec, wcat)
    both_ways(lambda: F.egc_layer_forward(g, spec, x, wcat, bcat, bias, packed=packed).clone(), 1)


def test_row_range_and_untrimmed_graph_take_no_plan():
    lib = _C.load()
    g = static_graph("n67")
    spec = spec_of("northstar_folded")
    bases, wt = torch.randn(67, spec.ldb, device=DEV), torch.randn(67, spec.w_cols, device=DEV)
    c0 = int(lib.egc_gather_plan_launches())
    part = F.egc_aggregate_combine(g, spec, bases, wt, None, rows=(0, 40))
    part = F.egc_aggregate_combine(g, spec, bases, wt, None, rows=(40, 67), out=part)
    ei, n = GRAPHS["n67"]()
    plain = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(ei).to(DEV), n)
    st = plain.c_struct()
    assert plain.gather_plans == {} and not st.gather_plan_raw and not st.gather_plan_looped
    whole = F.egc_aggregate_combine(plain, spec, bases, wt, None)
    assert int(lib.egc_gather_plan_launches()) == c0
    assert torch.equal(part, whole) and torch.equal(whole, F.egc_aggregate_combine(g, spec, bases, wt, None))
    assert int(lib.egc_gather_plan_launches()) == c0 + 1
    st = g.c_struct()
    assert set(g.gather_plans) == {"raw", "looped"} and st.gather_plan_raw and st.gather_plan_looped
    assert (st.gather_plan_form_looped & 0xff) == _C.GP_PACKED
    assert all(any(t is p for t in g.tensors()) for p, _ in g.gather_plans.values())     # kept alive with the C view


def test_refresh_edge_dis_rebuilds_the_plans():
    """a static graph whose deg^-1/2 tables change: the plans follow with the per-entry copies"""
    ei, n = GRAPHS["n67"]()
    g = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(ei).to(DEV), n).trim_launches()
    old = g.gather_plans["looped"][0]
    g.dis_looped.mul_(0.5)
    g.dis_raw[::2] = 0.25
    g.refresh_edge_dis()
    assert g.gather_plans["looped"][0] is not old
    check_plan(g, "raw")
    check_plan(g, "looped")
    aggregate_case(g, "northstar_folded", 1)
