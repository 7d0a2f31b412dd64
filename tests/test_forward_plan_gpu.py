"""The PLAN form of agg_fast_kernel -- what every cached layer's inference runs on a static graph -- against float64 at every
instance the library compiles (tests/forward_ref.py: plan_form, plan_instances; tests/test_forward_plan_cpu.py holds the case
list to the compiled set).  tests/test_forward_shapes_gpu.py never trims its graphs, so it launches no PLAN kernel; the cases,
operands, float64 restatement and bound here are that file's, the graphs are SEPARATE trimmed ones (trim_launches() mutates a
graph in place: the other file's cached graphs are never touched).

Three checks for every launch: egc_gather_plan_launches() moves by exactly one where ``plan_form`` says so and by none otherwise
(a plan silently not kept fails, it cannot hide); the output meets the float64 restatement at the sweep's own bound
(``held``: elementwise_excess <= 1 at 1e-5); and it is torch.equal to the same call under EGC_NO_GATHER_PLAN=1.

Beyond the other file's graphs: ``lanes`` (32 rows; rows of 31 / 32 / 33 and 15 / 16 / 17 entries, the reload boundary of the 32-
and 16-lane groups; every row's entries start at the highest-numbered source, whose id is all ones in the word's source field) and
the ladder with its plan REBUILT at the fewest spare bits its table fits, so that the table index reaches bit 31 of the word the
kernel carries in a signed int."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from egc_amd import functional as F
from forward_ref import (BIG_CASE, CASES, GRAPH_SEED, INPUT_SEED, PLAN_CASES, PLAN_FORMS, PLAN_SWITCH, POST_SEED, SETS, STRIDED_CASES,
                         TIE_CASES, aggregate_combine, dispatch, edges, family, graph_key, hba_columns, home, make_inputs, make_post,
                         need_of, plan_form)
from test_forward_shapes_gpu import DEV, FORM_NAMES, device_graph, expected, held, on_device, operands, reference, spec_of

pytestmark = pytest.mark.gpu
LANES = ("lanes",)
LANES_ROWS = 32
# in CSR order; row 31 -- the all-ones source id -- has ONE entry: the smallest degree is the LARGEST deg^-1/2, the last table index
LANES_LENGTHS = (33, 31, 32, 0, 17, 15, 16, 1, 32, 33, 31, 2, 16, 17, 15, 0, 3, 31, 5, 33, 1, 32, 2, 15, 4, 17, 0, 16, 7, 1, 9, 1)
assert len(LANES_LENGTHS) == LANES_ROWS
WORST = {}


@functools.lru_cache(maxsize=None)
def lanes_edges():
    """(edge_index, n, n): row r's entries are the sources n - 1, n - 2, ... (a row of more than n entries starts over: duplicate
    edges), so every non-empty row reads source n - 1 and rows that reach their own number hold a self entry; shuffled."""
    rng = np.random.default_rng(GRAPH_SEED)
    n = LANES_ROWS
    lengths = np.array(LANES_LENGTHS, dtype=np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), lengths)
    src = np.concatenate([(n - 1 - np.arange(k)) % n for k in lengths]).astype(np.int64)
    ei = np.stack([src, dst])
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]), n, n


def edges_of(case, kind):
    return lanes_edges() if kind == LANES else edges(*graph_key(case, kind, False))


@functools.lru_cache(maxsize=None)
def _lanes_reference(case):
    """``reference`` of tests/test_forward_shapes_gpu.py on the module's own graph (loops_all cases only: n_loop = n)."""
    ei, n, n_src = lanes_edges()
    assert case.loops_all
    bases, wt, gout = make_inputs(case, n, n_src, INPUT_SEED)
    ops = make_post(case, n, POST_SEED)
    if not case.bias:
        ops["bias"] = None
    with torch.no_grad():
        z = {dt: aggregate_combine(torch.from_numpy(bases).to(dt), hba_columns(torch.from_numpy(wt).to(dt), case), ei, n, case, n)
             for dt in (torch.float64, torch.float32)}
    return dict(ei=ei, n=n, n_src=n_src, n_loop=n, bases=bases, wt=wt, gout=gout, ops=ops, z=z)


def reference_of(case, kind, ties=False):
    return _lanes_reference(case) if kind == LANES else reference(case, kind, False, ties)


def expects_plan(case, kind, env=()):
    """``plan_form``; the module's own graph is square and small like the ladder, which the rule knows."""
    return plan_form(case, ("ladder",) if kind == LANES else kind, env=env)


# ---- the trimmed graphs: this module's own ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trimmed(kind, reduced):
    ei, n, n_src = lanes_edges() if kind == LANES else edges(kind, False, reduced)
    g = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(np.ascontiguousarray(ei)).to(DEV), n, n_src).trim_launches()
    torch.cuda.synchronize()
    if n_src == n:
        assert set(g.gather_plans) == {"raw", "looped"}, f"{kind}: a plan was not kept"
    return g


def trimmed(case, kind):
    return _trimmed(*graph_key(case, kind, False)[::2])


def plan_parts(g, name):
    """(header, table [T] uint32, words [e] uint32) of a kept plan, read back."""
    lib = _C.load()
    plan, header = g.gather_plans[name]
    p = plan.cpu().numpy()
    off = [int(lib.egc_gather_plan_offset(g.n_nodes, g.n_edges, k)) for k in range(2)]
    return header, p[off[0]:off[0] + header[_C.GP_TABLE_SIZE]].view(np.uint32), p[off[1]:off[1] + g.n_edges].view(np.uint32)


@functools.lru_cache(maxsize=None)
def top_bit_graph(name):
    """The trimmed ladder with its plans rebuilt at min_col_bits = 32 - ceil(log2(T)), T the table size of the ``name`` plan as
    first kept: exactly the bits its indices need, so with T >= 2 more than half -- at least one -- of the table's indices have
    their top bit, bit 31 of the word, set.  (The other edge set's plan is kept or not as its own table fits.)"""
    ei, n, n_src = edges(("ladder",))
    g = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(ei).to(DEV), n, n_src).trim_launches()
    T = g.gather_plans[name][1][_C.GP_TABLE_SIZE]
    assert T >= 2
    bits = math.ceil(math.log2(T))
    g.rebuild_gather_plans(min_col_bits=32 - bits)
    torch.cuda.synchronize()
    return g, T, bits


def plan_read_by(case):
    """aggregate_combine_impl: the sym set's plan for a layer with symnorm, else the looped one (both are kept here)."""
    return "looped" if "symnorm" not in case.aggrs or SETS[case.sets][1] == _C.SET_LOOPED else "raw"


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """As tests/test_gather_plan_gpu.py: the graphs (the 32768-row one among them) go back to the device, so that modules which
    measure peak device memory do not see this one's cached blocks."""
    yield
    if WORST:
        print(f"PLAN sweep: largest measured excess {WORST['excess']:.3f} ({WORST['tag']}), bound 1")
    _trimmed.cache_clear()
    top_bit_graph.cache_clear()
    torch.cuda.empty_cache()


# ---- one launch, three checks -----------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def switch_on(name):
    assert name not in os.environ
    os.environ[name] = "1"
    try:
        yield
    finally:
        del os.environ[name]


def launches():
    return int(_C.load().egc_gather_plan_launches())


def plan_check(case, kind, variant="plain", ties=False, env=(), graph=None, want_plan=None, note=""):
    """The call on the trimmed graph with and without the plan: the counter, float64, bit-identity.  Returns the output."""
    ref = reference_of(case, kind, ties)
    g = trimmed(case, kind) if graph is None else graph
    want_plan = expects_plan(case, kind, env) if want_plan is None else want_plan
    bases, wt, bias, post = operands(case, ref, variant)
    spec = spec_of(case)

    def call():
        out = torch.full((ref["n"], case.out), float("nan"), device=DEV)
        return F.egc_aggregate_combine(g, spec, bases, wt, bias, post=post, out=out)
    c0 = launches()
    with_plan = on_device(call)
    c1 = launches()
    with switch_on(PLAN_SWITCH):
        without = on_device(call)
    c2 = launches()
    tag = (f"{case.name} {'/'.join(str(k) for k in kind)}{' ties' if ties else ''} {variant}{' ' + FORM_NAMES[env] if env else ''}"
           f"{' ' + note if note else ''} trimmed")
    assert (c1 - c0, c2 - c1) == (int(want_plan), 0), f"{tag}: PLAN launches {c1 - c0} (expected {int(want_plan)}), with the switch {c2 - c1}"
    excess = held(with_plan.cpu().numpy(), expected(ref, variant), expected(ref, variant, torch.float32), tag,
                  family(case, ref["n"], env) + (" PLAN" if want_plan else ""))
    if want_plan and excess > WORST.get("excess", -1.0):
        WORST.update(excess=excess, tag=tag)
    differ = int((with_plan != without).sum())
    assert torch.equal(with_plan, without), f"{tag}: {differ} outputs differ from the launch without the plan"
    return with_plan


def _set_env(env, monkeypatch):
    for name in env:
        monkeypatch.setenv(name, "1")


def _plan_forms(cases=CASES):
    return [pytest.param(c, env, id=f"{c.name}-{FORM_NAMES[env] if env else 'default'}") for c in cases for env in PLAN_FORMS
            if plan_form(c, home(c), env=env)]


def _one_per_lane_group():
    """One case with symnorm per lane-group size (the table lookup feeds only the symnorm fold), each on the full ladder: the
    north star (16 lanes, the looped plan), rt<5,1,0> (32 lanes, raw sets: the raw plan, a padded basis, sigmoid weightings) and
    the 136 / H4 / B4 configuration (36 of 64 lanes, the looped plan)."""
    got = []
    for lg, cell, name in ((4, CASES[0].cell, "looped"), (5, "rt<5,1,0>", "raw"), (6, "st<4,4,34,symnorm+max+mean,none,lay>", "looped")):
        case = next(c for c in PLAN_CASES if c.cell == cell and c.loops_all and not c.ldw)
        assert dispatch(case, 32).lpr_log2 == lg and "symnorm" in case.aggrs and case.graph == "ladder" and plan_read_by(case) == name
        got.append(case)
    return got


IDS = dict(ids=lambda c: c.name)


@pytest.mark.parametrize("case,env", _plan_forms())
def test_every_plan_instance_against_float64(case, env, monkeypatch):
    """Every case with a PLAN form on its home graph (rows of 0, 1, 15 / 16 / 17, 63 / 64 / 65 entries and long rows that stay on
    col / edge_dis; the isolated tail where the case has no loops_all), by default and on its rt<...,0> fallback: one test per
    compiled kernel the case reaches, plain and with the full post-op."""
    _set_env(env, monkeypatch)
    for variant in ("plain", "full"):
        plan_check(case, home(case), variant, env=env)


@pytest.mark.parametrize("case,env", _plan_forms())
def test_every_plan_instance_on_low_degree_and_edgeless_graphs(case, env, monkeypatch):
    """161 rows of at most 17 entries, and no entry at all: the pack kernel is not launched, a plan is kept all the same and
    the PLAN kernel streams nothing."""
    _set_env(env, monkeypatch)
    g = trimmed(case, ("edgeless",))
    assert g.n_edges == 0 and all(h[_C.GP_FORM] == _C.GP_PACKED for _, h in g.gather_plans.values())
    for kind in (("sparse",), ("edgeless",)):
        for variant in ("plain", "full"):
            plan_check(case, kind, variant, env=env)


@pytest.mark.parametrize("case,env", _plan_forms(TIE_CASES))
def test_ties_through_the_plan(case, env, monkeypatch):
    _set_env(env, monkeypatch)
    plan_check(case, home(case), "full", ties=True, env=env)


@pytest.mark.parametrize("case,env", _plan_forms(STRIDED_CASES))
def test_a_strided_weightings_block_through_the_plan(case, env, monkeypatch):
    """The weightings as a column block of a wider array whose surround is NaN."""
    _set_env(env, monkeypatch)
    for kind in (("ladder",), ("sparse",)):
        for variant in ("plain", "full"):
            plan_check(case, kind, variant, env=env)


def test_four_row_groups_per_wavefront_through_the_plan():
    case, kind = BIG_CASE, ("big",)
    assert plan_form(case, kind) and dispatch(case, reference_of(case, kind)["n"]).rows_per_wave == 4
    plan_check(case, kind, "plain")


@pytest.mark.parametrize("case", _one_per_lane_group(), **IDS)
def test_the_reload_boundary_of_every_lane_group(case):
    """Rows of 15 / 16 / 17 and 31 / 32 / 33 entries whose entries start at the all-ones source id: one lane group exactly, one
    entry fewer, one more -- the second batch re-reads the words and must re-derive the source ids from them."""
    ei, n, _ = lanes_edges()
    g = trimmed(case, LANES)
    deg = np.diff(g.rowptr.cpu().numpy()[:n + 1])
    assert {0, 1, 15, 16, 17, 31, 32, 33} <= set(deg.tolist()) and deg.max() <= 64
    header, table, words = plan_parts(g, plan_read_by(case))
    cb = header[_C.GP_COL_BITS]
    ones = (words & np.uint32((1 << cb) - 1)) == (1 << cb) - 1
    assert n == 1 << cb and ones.sum() >= (deg > 0).sum() and ((words >> np.uint32(cb))[ones] != 0).all() and len(table) >= 8
    for variant in ("plain", "full"):
        plan_check(case, LANES, variant)


@pytest.mark.parametrize("case", _one_per_lane_group(), **IDS)
def test_a_table_index_in_bit_31(case):
    """The plan rebuilt with exactly the spare bits its table needs: the words of more than half the table's values have bit 31
    set, and the kernel's ``(unsigned)word >> cb`` must not see a sign."""
    name = plan_read_by(case)
    g, T, bits = top_bit_graph(name)
    assert name in g.gather_plans, "the rebuilt plan was not kept"
    header, table, words = plan_parts(g, name)
    assert header[_C.GP_FORM] == _C.GP_PACKED and header[_C.GP_COL_BITS] == 32 - bits and header[_C.GP_TABLE_SIZE] == T == len(table)
    assert 1 << (bits - 1) < T <= 1 << bits
    assert (words >> np.uint32(31)).any()
    edis = (g.edge_dis_raw if name == "raw" else g.edge_dis_looped).cpu().numpy()[:g.n_edges]
    assert np.array_equal(table[words >> np.uint32(32 - bits)], edis.view(np.uint32))
    for variant in ("plain", "full"):
        plan_check(case, ("ladder",), variant, graph=g, note="top bit")


def _no_plan_cases():
    by_family = {}
    for c in CASES:
        cell = dispatch(c, 32)
        key = cell.family if cell.family != "reg" else ("reg SQ" if need_of(c) == "SQ" else None)
        if key is not None and c.loops_all and not c.ldw:
            by_family.setdefault(key, c)
    return [by_family[k] for k in ("wide", "lds", "reg SQ")]


@pytest.mark.parametrize("case", _no_plan_cases(), **IDS)
def test_kernels_without_a_plan_form_leave_the_plan_alone(case):
    """The two-slots-per-lane kernel, the LDS kernels and a register instance that keeps squares: on the trimmed graph the
    counter does not move and the output is the untrimmed graph's bit for bit."""
    kind = home(case)
    assert not plan_form(case, kind)
    got = plan_check(case, kind, "full")
    ref = reference(case, kind)
    bases, wt, bias, post = operands(case, ref, "full")
    out = torch.full((ref["n"], case.out), float("nan"), device=DEV)
    plain = device_graph(case, kind)
    assert plain.gather_plans == {}
    c0 = launches()
    want = on_device(lambda: F.egc_aggregate_combine(plain, spec_of(case), bases, wt, bias, post=post, out=out))
    assert launches() == c0 and torch.equal(got, want)


def test_a_cached_layer_runs_the_plan_form():
    """egc_amd.EGConv at 128 / H8 / B4 with the north-star aggregators and cached=True: the layer trims the graph it pins, and
    every inference forward after that launches the PLAN form."""
    ei, n, _ = edges(("ladder",))
    torch.manual_seed(5)
    conv = egc_amd.EGConv(128, 128, aggrs=["sum", "mean", "max", "symnorm"], num_heads=8, num_bases=4, cached=True).to(DEV).eval()
    x = torch.randn(n, 128, generator=torch.Generator().manual_seed(6)).to(DEV)
    edge_index = torch.from_numpy(ei).to(DEV)
    with torch.no_grad():
        first = on_device(lambda: conv(x, edge_index).clone())
        assert set(conv._cached_graph[0].gather_plans) == {"raw", "looped"}
        c0 = launches()
        second = on_device(lambda: conv(x, edge_index).clone())
        c1 = launches()
        with switch_on(PLAN_SWITCH):
            without = on_device(lambda: conv(x, edge_index).clone())
        c2 = launches()
    assert (c1 - c0, c2 - c1) == (1, 0)
    assert torch.isfinite(second).all() and torch.equal(first, second) and torch.equal(second, without)
