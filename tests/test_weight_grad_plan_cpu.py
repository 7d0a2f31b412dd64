"""The host side of the weight-gradient GEMM (egc_gemm_xt.hip: xt_plan and the workspace record), pinned against the library
of the commit BEFORE its plan and envelope got one owner: egc_weight_grad_plan's plan8 and the two workspace queries (host
only, no GPU touched) over a grid of shapes, with EGC_GEMM_EXACT unset and set, and with every compiled tile forced through
EGC_XT_TILE.  The callers size their workspaces by these numbers and the launchers take their grids from the same plan: a
value that moves here is a launch that changed.

tests/golden/weight_grad_plan.json was recorded ONCE, by tests/golden/make_weight_grad_plan.py, from the library built at the
commit it names.  A mismatch is a behaviour change of the host code: find it and remove it, never re-record."""
import ctypes as C
import json
import os

import pytest

from egc_amd import _C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_grad_plan.json")
TM, TN, ES = _C.WEIGHT_GRAD_TILE_ROWS, _C.WEIGHT_GRAD_TILE_COLS, _C.WEIGHT_GRAD_MAX_SUM_COLS

ROWS = (0, 1, 17, 31, 32, 33, 65, 200, 257, 1000, 3000, 8300, 20000, 169343, 736389)
# A thinned 4 .. 400 x 4 .. 640.  The one-tile envelope's edges and their neighbours:
EDGES = tuple((f, k) for f in (4, TM - 4, TM, TM + 4) for k in (4, TN - 4, TN, TN + 4))
# ... walking rows, f_in, k in that order over the full grid in steps of 4, the (f_in, k) at which each compiled tile is first chosen
# (32 x 64 at 0 rows; 64 x 64, 64 x 128, 64 x 192 at 0; 32 x 128 at 1000; 32 x 192, 128 x 64, 128 x 128, 160 x 128 at 3000; 128 x 192,
# 224 x 128 at 8300; 160 x 192, 224 x 144, 224 x 192, 224 x 288, 224 x 320 at 20000):
FIRST = ((4, 196), (100, 516), (196, 580), (388, 580), (4, 516), (4, 324), (68, 260), (132, 424), (132, 388), (324, 516), (324, 388),
         (132, 516), (388, 132), (196, 516), (324, 260), (388, 292))
# ... and the nets' own widths
SHAPES = tuple(dict.fromkeys(EDGES + FIRST + ((224, 272), (296, 180), (352, 208))))
E_COLS = (0, 4, ES)
XT_TILES = ((1, 1, 4), (1, 2, 4), (1, 3, 4), (2, 1, 4), (2, 2, 4), (2, 3, 4), (4, 1, 4), (4, 2, 4), (4, 3, 4), (5, 2, 4), (5, 3, 4),
            (7, 2, 4), (7, 3, 3), (7, 3, 4), (7, 5, 4), (7, 3, 6))
FORCED_SHAPES = ((TM, TN), (TM + 4, TN + 4), (224, 272), (296, 180))     # (the first is one tile: the forced one is not taken)
FORCED_ROWS = (1, 3000, 169343)


def grid():
    """[(EGC_GEMM_EXACT or None, EGC_XT_TILE or None, n, f_in, k)]: the table has one line per (switches, shape)"""
    g = [(exact, None, n, f, k) for exact in (None, "1") for f, k in SHAPES for n in ROWS]
    g += [(None, "%d,%d,%d" % t, n, f, k) for t in XT_TILES for f, k in FORCED_SHAPES for n in FORCED_ROWS]
    return g


def answers(lib, monkeypatch, cases):
    """[[rc, plan8 ..., workspace bytes, ex workspace bytes at each of E_COLS]] for the cases, in order"""
    plan = (C.c_int32 * 8)()
    out = []
    for exact, tile, n, f, k in cases:
        for name, value in (("EGC_GEMM_EXACT", exact), ("EGC_XT_TILE", tile)):
            monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
        rc = lib.egc_weight_grad_plan(n, f, k, C.cast(plan, C.c_void_p))
        out.append([rc, *plan, lib.egc_weight_grad_workspace_bytes(n, f, k),
                    *(lib.egc_weight_grad_ex_workspace_bytes(n, f, k, e) for e in E_COLS)])
    return out


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        t = json.load(f)
    t["expect"] = [e for line in t["expect"] for e in line]
    return t


def test_table_covers_the_grid(table):
    assert len(table["commit"]) == 40
    axes = dict(rows=ROWS, shapes=SHAPES, e_cols=E_COLS, tiles=XT_TILES, forced_shapes=FORCED_SHAPES, forced_rows=FORCED_ROWS)
    assert all(table[name] == json.loads(json.dumps(axis)) for name, axis in axes.items())
    cases = grid()
    assert len(table["expect"]) == len(cases) and set(EDGES + FIRST) <= set(SHAPES)
    unforced = [e for c, e in zip(cases, table["expect"]) if c[0] is None and c[1] is None]
    assert {e[1] for e in unforced} == {0, 1}                                       # plan8[0]: both kernels
    # (mt, nt, wn) of a row [rc, plan8 ...]: a tile is 32 mt x 16 wn nt on 128 wn threads
    assert {(e[2] // 32, e[3] * 8 // e[8], e[8] // 128) for e in unforced if e[1] == 0} == set(XT_TILES)
    for c, e in zip(cases, table["expect"]):
        if c[1] is not None:
            mt, nt, wn = (int(v) for v in c[1].split(","))
            assert e[:4] == ([0, 1, TM, TN] if c[3] <= TM else [0, 0, 32 * mt, 16 * wn * nt]), c


def test_plan_and_workspace_match_the_recorded_table(table, monkeypatch):
    cases = grid()
    got = answers(_C.load(), monkeypatch, cases)
    wrong = [(c, want, g) for c, want, g in zip(cases, table["expect"], got) if want != g]
    assert not wrong, (len(wrong), wrong[:5])


def test_weight_gradient_plan_keeps_every_xcd_at_one_round(monkeypatch):
    """egc_weight_grad_plan (host only): the tile grid covers the output, the row ranges cover the rows, the workspace holds one
    record per range, and -- the round-6 fix -- the tiles of the ranges that land on one XCD fit its 32 CUs whenever the output has
    at most 32 tiles (86 ranges of three tiles used to put 33 workgroups on some XCDs: two rounds)."""
    lib = _C.load()
    monkeypatch.delenv("EGC_XT_TILE", raising=False)
    monkeypatch.delenv("EGC_GEMM_EXACT", raising=False)
    plan = (C.c_int32 * 8)()
    for n in (0, 1, 700, 2998, 52771, 169343, 736389):
        for f, k in ((TM, TN), (168, 116), (224, 272), (296, 180), (136, 184), (304, 368), (352, 208), (4, 4), (384, 384)):
            assert lib.egc_weight_grad_plan(n, f, k, C.cast(plan, C.c_void_p)) == 0
            x3, tm, tn, mt, nt, ranges, rows, threads = list(plan)
            assert x3 == int(f <= TM and k <= TN)
            assert mt * tm >= f and nt * tn >= k and ranges * rows >= n and rows % 32 == 0 and threads in (384, 512, 768)
            assert lib.egc_weight_grad_workspace_bytes(n, f, k) == ranges * (f * k + k) * 4
            if not x3 and mt * nt <= 32:
                assert -(-ranges // 8) * mt * nt <= 32, (n, f, k, list(plan))
    monkeypatch.setenv("EGC_XT_TILE", "3,3,3")          # not a compiled tile
    assert lib.egc_weight_grad_plan(1000, 224, 272, C.cast(plan, C.c_void_p)) == 4
    assert lib.egc_weight_grad_plan(1000, 0, 272, C.cast(plan, C.c_void_p)) == 1
