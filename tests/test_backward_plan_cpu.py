"""The host side of the layer backward (egc_amd/csrc/egc_backward_host.h: which kernels a call launches for a layer on a graph,
the workspace's tables and records, and the launch geometry), run without a GPU by tests/backward_plan/backward_plan_check.cpp.

(a) the C++ plan names the kernels ``backward_ref.dispatch`` names -- the restatement written against the inline chain the plan
    replaced, which indexes the GPU sweep -- over every cell of that sweep and over a seeded sample of GRID below; where the
    restatement raises "unsupported" the plan refuses with EGC_ERR_UNSUPPORTED.  A mismatch is a behaviour change in the C++;
(b) the compared set reaches every instance, record mode, basis kind and refusal -- by the restatement alone, too;
(c) the plan's numbers hold together, and its two workspace sizes are what the library answers;
(d) the lists the launches expand from are what backward_ref parses and what COMPILED_DST / COMPILED_SRC state.

GRID is the product of H, B, L (the basis stride from padded_basis_stride), LISTS, the edge-set pairs, the nonlinearities, SWITCHES
and four (n, e) pairs per ldb: no entry, exactly on the record rule (ldb n = 10 e), one entry short of it, and e 64 >= 2^31.  The
last is e = 2^26: the library compares e 64 with 0xFFFFFFF0 (a 32-bit buffer offset), ``records_apply`` with 2^31, and they agree
from 2^26 on and below 2^25 -- in between the restatement is wrong about the library before and after the plan (no graph of the
sweep is near it).  The product is 571,536 layers, 11.4 million lines -- the sanitized check program walks all of it (``full_grid_lines``, DESIGN.md
section 3.22), this file SAMPLE layers of it at every switch set and (n, e) pair."""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

from backward_ref import (ACTS, ALL7, CASES, CODES, COMPILED_DST, COMPILED_SRC, GRAPH_SEED, RECORD_CASES, SETS, Case, case_graph,
                          dispatch, extrema, geometry, records_apply, source_instances, sparse)
from egc_amd import _C
from egc_amd.functional import make_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "backward_plan", "_build", "backward_plan_check")
UNSUPPORTED = _C.ERR_UNSUPPORTED
SWITCH_NAMES = ("EGC_BWD_GENERIC", "EGC_BWD_NO_REC", "EGC_BWD_REC_SEPARATE")
MODES = ((), ("EGC_BWD_NO_REC",), ("EGC_BWD_REC_SEPARATE",), ("EGC_BWD_GENERIC",))     # of tests/test_backward_shapes_cpu.py
SWITCHES = MODES + (("EGC_BWD_NO_REC", "EGC_BWD_GENERIC"),)

HEADS = (1, 2, 4, 6, 8, 16, 32)
BASES = (1, 2, 3, 4, 8, 16)
LENGTHS = (1, 3, 4, 7, 8, 9, 12, 16, 17, 31, 32, 34, 37, 40, 56, 64, 74, 128)
_COMPILED = sorted({lst for lists in COMPILED_DST.values() for lst in lists})        # six lists in nine (lane group, H, A) rows
LISTS = tuple(dict.fromkeys(
    [(a,) for a in ALL7] + _COMPILED + [p for lst in _COMPILED for p in itertools.permutations(lst)] +
    # 2, 4, 5 and 7 aggregators without and with max / min / std / symnorm (a list may name an aggregator twice)
    [("sum", "mean"), ("max", "symnorm"), ("sum", "mean", "var", "mean"), ("max", "min", "std", "symnorm"),
     ("sum", "mean", "var", "sum", "mean"), ("sum", "max", "min", "std", "symnorm"), ("sum", "mean", "var", "sum", "mean", "var", "sum"), ALL7]))
SAMPLE, SAMPLE_SEED = 20000, 322
BIG_E = 1 << 26


def layers():
    """GRID's layers, lazily: Case(out, H, B, aggrs, sets, "", act)."""
    for H, B, L, aggrs, sets, act in itertools.product(HEADS, BASES, LENGTHS, LISTS, SETS, ACTS):
        yield Case(H * L, H, B, aggrs, sets, "", act)


def graph_counts(ldb):
    return ((50, 0), (50, 5 * ldb), (50, 5 * ldb - 1), (50, BIG_E))


def line(case, n, e, env, n_src=None, te=None, ws=-1, has_plan=1, d_chunks=-1, t_chunks=-1):
    agg_set, sym_set = SETS[case.sets]
    return "%d %d %d %d %d %d %d %d %s  %d %d %d %d %d %d %d %d  %d %d %d\n" % (
        case.out, case.H, case.B, geometry(case)[1], ACTS[case.act], agg_set, sym_set, len(case.aggrs),
        " ".join(str(CODES[a]) for a in case.aggrs), n, n if n_src is None else n_src, e, d_chunks, e if te is None else te, t_chunks,
        ws, has_plan, *(int(s in env) for s in SWITCH_NAMES))


def full_grid_lines():
    for c in layers():
        for n, e in graph_counts(geometry(c)[2]):
            for env in SWITCHES:
                yield line(c, n, e, env)


def run_plan(lines):
    """input lines -> one dict per line: every field the check program prints (numbers as int)."""
    subprocess.run(["bash", os.path.join(ROOT, "tests", "backward_plan", "build.sh")], check=True, capture_output=True)
    r = subprocess.run([BIN], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    names = out[0].split()[1:]
    plans = [dict(zip(names, (int(v) if v.lstrip("-").isdigit() else v for v in row.split()[1:]))) for row in out[1:] if row]
    assert len(plans) == len(lines) and all(len(p) == len(names) for p in plans)
    return plans


def reference(case, n, e, env):
    try:
        return dispatch(case, n, e, env)
    except AssertionError as err:
        assert str(err).startswith("unsupported")
        return None


@pytest.fixture(scope="module")
def compared():
    """[(case, n, e, env, reference Cell or None, plan)]: the cells of the GPU sweep, then the sample of GRID."""
    keys = []
    for c in CASES:
        ei, n, _ = case_graph(c)
        keys += [(c, n, ei.shape[1], env) for env in MODES]
        if c in RECORD_CASES:
            ei, n, _ = sparse(GRAPH_SEED)
            keys.append((c, n, ei.shape[1], ()))
    every = list(layers())
    assert len(every) == len(HEADS) * len(BASES) * len(LENGTHS) * len(LISTS) * len(SETS) * len(ACTS) and len(every) > SAMPLE
    for c in random.Random(SAMPLE_SEED).sample(every, SAMPLE):
        keys += [(c, n, e, env) for n, e in graph_counts(geometry(c)[2]) for env in SWITCHES]
    plans = run_plan([line(*k) for k in keys])
    return [k + (reference(*k), p) for k, p in zip(keys, plans)]


def _reach(cells, refused):
    """What a set of (Cell, refusal) reaches, and the assertion that it is everything."""
    src = source_instances()
    fast = {c.dst for c in cells if c.dst.startswith("fast")}
    assert fast == src["dst"] and len(fast) == 16
    assert {c.dst for c in cells if c.dst.startswith("lds")} == {"lds/4", "lds/1"}
    assert {c.src for c in cells} == src["src"] and len(src["src"]) == 13 + 4
    assert {c.rec for c in cells} == {"off", "fused", "sep<1>", "sep<2>", "sep<3>", "sep<4>"}
    for lg in (4, 5, 6):
        assert {c.basis for c in cells if c.dst.startswith(f"fast<{lg}")} == {"p2:H%P", "p2:H<P", "np2"}, lg
    assert refused >= {"lds", "slots"}


def test_the_grid_reaches_everything_by_the_restatement_alone(compared):
    """No C++ in this one: the restatement's own cells, and which of its two "unsupported" assertions a refused layer meets."""
    refused = set()
    for case, n, e, env, ref, _ in compared:
        if ref is None:
            _, _, ldb, slots, A, W = geometry(case)
            floats = A * ldb + ((case.out + 3) & ~3) + 2 * ((W + 3) & ~3)
            refused.add("lds" if (16 * floats if 16 * floats <= 48 * 1024 else 4 * floats) > 64 * 1024 else "slots")
            assert slots > 256 or floats * 4 > 64 * 1024
    _reach([ref for *_, ref, _ in compared if ref is not None], refused)
    assert len({(c.name, c.act) for c, *_ in compared}) >= SAMPLE


def test_the_plan_names_the_kernels_the_restatement_names(compared):
    for case, n, e, env, ref, p in compared:
        key = (case.name, case.act, n, e, env)
        if ref is None:
            assert p["status"] == UNSUPPORTED and p["refusal"] in ("lds", "slots"), key
            continue
        assert p["status"] == 0 and p["refusal"] == "-", key
        got = (p["dst"], p["basis"].replace("-", ""), p["src"], p["lpr_log2"], p["rec"])
        assert got == tuple(ref), (key, got, ref)
        assert bool(p["rule"]) == bool(records_apply(case, n, e, env)), key
    _reach([type(ref)(p["dst"], p["basis"].replace("-", ""), p["src"], p["lpr_log2"], p["rec"]) for *_, ref, p in compared if ref is not None],
           {p["refusal"] for *_, p in compared})


def _chunk_blocks(n, e, hint=-1):
    cap_long = min(e // (_C.LONG_ROW_THRESHOLD + 1) + 1, n + 1)
    cap = e // _C.LONG_ROW_CHUNK + cap_long
    return -(-(hint if 0 <= hint <= cap else cap) // 4)


def _hold_together(p, n, n_src, e, te, d_hint=-1, t_hint=-1):
    ldb, ext = p["ldb"], p["extrema"]
    assert p["ws_tables"] == ((5 * n * ldb * 4 + 255) & ~255) + 256 and p["table_floats"] == n * ldb
    assert p["ws_total"] == p["ws_tables"] + (ext * e * 64 if p["rule"] else 0) and p["rec_offset"] == p["ws_tables"]
    assert ext == p["has_x"] + p["has_n"]
    if p["status"] != 0:
        return
    fused, off = p["rec"] == "fused", p["rec"] == "off"
    assert p["dst_lds"] <= 64 * 1024 and p["rec_lds"] <= 64 * 1024
    if p["dst"].startswith("fast"):
        G = 64 >> p["dst_lpr_log2"]
        assert p["slots"] <= 64 >> 0 and p["slots"] <= (1 << p["dst_lpr_log2"]) and p["dst_threads"] == 256
        assert p["dst_row_blocks"] == -(-n // (4 * G)) and p["dst_grid"] == p["dst_row_blocks"] + p["rec_chunk_blocks"]
        assert p["rec_chunk_blocks"] == (_chunk_blocks(n, e, d_hint) if fused else 0)
        assert p["dst_lds"] == 16 * G * p["dst_group_floats"]
        if fused:                                 # the record builder's LDS: 64 entries a lane group, 256 a wavefront
            assert p["dst_group_floats"] >= p["rec_group_u32"] and G * p["dst_group_floats"] >= p["rec_group_u32"] + 384
    else:
        assert not fused and p["rec_chunk_blocks"] == p["dst_row_blocks"] == 0
        assert p["dst_grid"] == -(-n // p["wpb"]) and p["dst_threads"] == 64 * p["wpb"] and p["dst_lds"] == 4 * p["wpb"] * p["lds_floats_per_wave"]
    assert (p["rec_grid"] == 0) == (fused or off) and (p["rec_entry_bytes"] == 0) == off
    if not off:
        assert p["rec_entry_bytes"] == e * 64 and p["rec_group_u32"] == 128 + ldb + ldb // 4 + 4 and p["rec_lds"] == 64 * p["rec_group_u32"]
        assert p["rec_blocks"] == _chunk_blocks(n, e, d_hint) and p["rec_short_rows"] == (not fused)
        assert fused or p["rec_grid"] == p["rec_blocks"] + -(-n // 16)
    for pre, rows, edges, hint in (("src", n_src, te, t_hint), ("arg", n, e, d_hint)):
        lg = p["lpr_log2" if pre == "src" else "arg_lpr_log2"]
        assert lg == p["arg_lpr_log2"] and p[pre + "_ns"] == -(-p["slots"] // (1 << lg)) <= 4 and p["arg_status"] == 0
        assert p[pre + "_chunk_blocks"] == _chunk_blocks(rows, edges, hint)
        assert p[pre + "_grid"] == p[pre + "_chunk_blocks"] + -(-rows // (4 * (64 >> lg)))


def test_the_plans_numbers_hold_together(compared, monkeypatch):
    lib = _C.load()
    asked = {}
    for case, n, e, env, _, p in compared:
        _hold_together(p, n, n, e, e)
        key = (case, n, e, "EGC_BWD_NO_REC" in env)
        if key not in asked:                       # the library's two sizes: no device call; EGC_BWD_NO_REC is read on every call
            if key[3]:
                monkeypatch.setenv("EGC_BWD_NO_REC", "1")
            else:
                monkeypatch.delenv("EGC_BWD_NO_REC", raising=False)
            agg_set, sym_set = SETS[case.sets]
            spec = make_spec(16, case.out, case.H, case.B, [CODES[a] for a in case.aggrs], agg_set, sym_set, True, _C.LAYOUT_HBA,
                             ACTS[case.act], basis_stride=geometry(case)[1])
            g = _C.EgcGraph(n, e, None, None, None, None, None, None, None, -1, n, None, None)
            asked[key] = (lib.egc_backward_workspace_bytes(C.byref(spec.c), n), lib.egc_backward_workspace_bytes_for(C.byref(spec.c), C.byref(g)))
        assert asked[key] == (p["ws_tables"], p["ws_total"]), key[1:]


def test_counts_the_square_sweep_does_not_have():
    """Rectangular graphs, host-known chunk counts on either side (honoured up to the capacity), a workspace without room for
    the records or for the tables, a destination graph without a plan: the record mode follows, the numbers still hold."""
    c = next(c for c in CASES if c.name == "64-H8-B4-sum+mean+max-raw")
    n, n_src, e = 300, 450, 40000
    cap = _chunk_blocks(n, e) * 4
    kw = dict(n_src=n_src, te=e)
    plans = run_plan([line(c, n, e, (), **kw), line(c, n, e, (), d_chunks=7, t_chunks=9, **kw), line(c, n, e, (), d_chunks=cap + 400, **kw),
                      line(c, n, e, (), ws=-2, **kw), line(c, n, e, (), has_plan=0, **kw), line(c, n, e, (), ws=1000, **kw),
                      line(c, n, e, ("EGC_BWD_REC_SEPARATE",), d_chunks=7, **kw)])
    for p, hints in zip(plans, ((-1, -1), (7, 9), (cap + 400, -1), (-1, -1), (-1, -1), (-1, -1), (7, -1))):
        _hold_together(p, n, n_src, e, e, *hints)
    assert [p["rec"] for p in plans] == ["fused", "fused", "fused", "off", "off", "off", "sep<1>"]
    assert [p["src"] for p in plans[:5]] == ["src<1,T|X|REC>"] * 3 + ["src<1>"] * 2            # (T X without records: not a compiled word)
    assert plans[1]["rec_chunk_blocks"] == 2 and plans[1]["src_chunk_blocks"] == 3 and plans[2]["rec_chunk_blocks"] == cap // 4
    assert [(p["status"], p["size_status"], p["refusal"]) for p in plans[4:6]] == [(0, 0, "-"), (2, 2, "workspace")]
    big = run_plan([line(c, 1 << 25, 0, ()), line(c, (1 << 25) - 1, 0, ()), line(c, 1 << 25, 0, (), ws=0)])   # n ldb 4 (ldb = 32) against 0xFFFFFFF0
    assert [(p["status"], p["size_status"], p["refusal"]) for p in big] == [(4, 4, "offsets"), (0, 0, "-"), (2, 2, "workspace")]


def test_the_lists_are_what_the_launches_expand_from():
    src = source_instances()
    subprocess.run(["bash", os.path.join(ROOT, "tests", "backward_plan", "build.sh")], check=True, capture_output=True)
    rows = [r.split() for r in subprocess.run([BIN, "--instances"], capture_output=True, text=True, check=True).stdout.split("\n") if r]
    printed = {k: [v for kind, v in rows if kind == k] for k in ("dst", "src", "rec", "arg")}
    assert all(len(v) == len(set(v)) for v in printed.values())                       # no row twice
    assert {k: set(v) for k, v in printed.items()} == {**src, "arg": {str(a) for a in src["arg"]}}
    want = {f"fast<{lg},{h},{a}>" for lg, h, a in COMPILED_DST} | {f"fast<{lg},{h},{a},{'+'.join(lst)}>" for (lg, h, a), lists in
                                                                    COMPILED_DST.items() for lst in lists}
    assert src["dst"] == want and len(want) == 16
    order = ("T", "S", "V", "X", "N", "XL", "YL", "REC")
    assert src["src"] == {"src<1," + "|".join(f for f in order if f in fl) + ">" for fl in COMPILED_SRC} | {f"src<{ns}>" for ns in (1, 2, 3, 4)}
    assert src["rec"] == {f"sep<{ns}>" for ns in (1, 2, 3, 4)} and src["arg"] == {1, 2, 3, 4}
