"""The host side of the packed basis transform (egc_amd/csrc/egc_gemm_host.h: which kernel family serves a shape, its sizes,
and the launch geometry of every kernel whose geometry is a run-time value), run without a GPU by
tests/gemm_plan/gemm_plan_check.cpp over a dense grid of shapes and both flag values.

(a) the plan's workspace bound is the library's egc_basis_pack_bytes;
(b) layout and pack bytes are what the library of the commit BEFORE the plan existed answered: tests/golden/gemm_plan.json was
    recorded ONCE, by tests/golden/make_gemm_plan.py, from that commit's library and headers.  A mismatch is a behaviour change
    (the planes of a family are read by that family alone): find it and remove it, never re-record;
(c) every launch description obeys the limits the kernels state, a shape planned for the long-k kernels has no refused launch,
    and the grid reaches every kernel instance that any shape can reach."""
import ctypes as C
import json
import os
import subprocess

import pytest

from egc_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "gemm_plan", "_build", "gemm_plan_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")

# every value at which the host code takes another path, with its neighbours, over two strides that between them put a multiple
# of four and a non-multiple into every k-step count of the long-k kernels (5 .. 12 steps of 32)
_EDGES = (4, 32, 33, 64, 65, 96, 97, 128, 129, 132, 160, 224, 225, 228, 256, 257, 260, 288, 289, 292, 352, 384, 385, 388, 389)
F_IN = sorted({v for e in _EDGES for v in (e - 1, e, e + 1)} | set(range(4, 401, 12)) | set(range(1, 401, 29)) | {400})
COLS = (0, 1, 7, 16, 20, 32, 64, 124, 168, 176, 192, 208, 224, 300, 320, 512)     # f_g and w_cols
FLAGS = (0, _C.GEMM_24BIT)
ROWS = 200
LAYOUT_CODE = {"BF16X3": "B", "F16X2": "H", "F16X2K": "K"}
LDS_MAX = 160 * 1024

# The kernel instances the three translation units compile (egc_gemm_bf16x3.hip, egc_gemm_f16x2k.hip) ...
WS_INSTANCES = {("ws", k) for k in (2, 4, 6, 8)}
STAGED_INSTANCES = {("staged", 1, 7), ("staged", 1, 6), ("staged", 0, 6), ("staged", 1, 4), ("staged", 1, 0), ("staged", 0, 0)}
LONGK_INSTANCES = ({("all_in_one", ks, w) for ks in range(5, 13) for w in (12, 16)} |
                   {("roles", ks, w) for ks in range(5, 13) for w in (12, 16)} | {("two_tiles", ks, 12) for ks in (5, 6, 7)})


# ... and those of them that no shape launches: with 12 wavefronts (at most 9 column tiles) the all-in-one form is taken only
# where two workgroups share a CU, which needs KS <= 9, and the separated roles only where they do not, which these tile counts
# allow from KS = 9 on; at KS = 12 a launch has at most 12 column tiles and always four helpers
UNREACHED_LONGK = ({("all_in_one", ks, 12) for ks in (10, 11, 12)} | {("all_in_one", 12, 16)} | {("roles", ks, 12) for ks in (5, 6, 7, 8)})


def run_plan(shapes):
    """[(f_in, f_g, w_cols, flags, rows)] -> one dict per shape: the plan's fields, "longk" / "bf16x3" (lists of launches, or
    the refusal's status) and "ranges" {tile rows: [(r0, rows)]}."""
    subprocess.run(["bash", os.path.join(ROOT, "tests", "gemm_plan", "build.sh")], check=True, capture_output=True)
    text = "".join("%d %d %d %d %d\n" % s for s in shapes)
    r = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = []
    for w in (line.split() for line in r.stdout.split("\n") if line):
        if w[0] == "plan":
            f = [int(v) for v in w[1:6]] + [w[6]] + [int(v) for v in w[7:]]
            out.append(dict(zip(("f_in", "f_g", "w_cols", "flags", "valid", "layout", "ldb", "NV", "KS", "TB", "NT", "pack_bytes",
                                 "pack_bytes_max"), f), longk=[], bf16x3=[], ranges={}, refused=None))
        elif w[0] == "longk" and len(w) == 2 or w[0] == "bf16x3" and len(w) == 2:
            out[-1]["refused"] = int(w[1])
        elif w[0] == "longk":
            keys = ("status", "form", "waves", "tile0", "tiles", "mult", "per_cu", "LDX", "R", "slot_bytes", "ring", "lds", "threads", "grid")
            out[-1]["longk"].append(dict(zip(keys, [int(w[1]), w[2]] + [int(v) for v in w[3:]])))
        elif w[0] == "bf16x3":
            keys = ("status", "kernel", "ksub", "vec4", "nt", "vblock0", "grid_x", "grid_y", "threads", "pieces", "lds")
            out[-1]["bf16x3"].append(dict(zip(keys, [int(w[1]), w[2]] + [int(v) for v in w[3:]])))
        else:
            assert w[0] == "ranges"
            out[-1]["ranges"][int(w[1])] = [tuple(int(v) for v in x.split(":")) for x in w[2:]]
    assert [(p["f_in"], p["f_g"], p["w_cols"], p["flags"]) for p in out] == [s[:4] for s in shapes]
    return out


def grid():
    return [(f_in, f_g, w, flags, ROWS) for f_in in F_IN for f_g in COLS for w in COLS for flags in FLAGS]


def instances(plans):
    """the kernel instances the launches of these plans name"""
    seen = set()
    for p in plans:
        for g in p["longk"]:
            seen.add((g["form"], p["KS"], g["waves"]))
        for g in p["bf16x3"]:
            seen.add(("ws", g["ksub"]) if g["kernel"] == "ws" else ("staged", g["vec4"], g["nt"]))
    return seen


@pytest.fixture(scope="module")
def plans():
    return run_plan(grid())


def test_pack_bytes_are_the_librarys(plans):
    lib = _C.load()
    lib.egc_basis_pack_bytes.restype = C.c_size_t
    lib.egc_basis_pack_bytes.argtypes = [C.c_int32] * 3
    for p in plans:
        assert p["pack_bytes_max"] == lib.egc_basis_pack_bytes(p["f_in"], p["f_g"], p["w_cols"]), p
        assert p["pack_bytes"] <= p["pack_bytes_max"] and (p["pack_bytes"] > 0) == bool(p["valid"]), p


def test_layout_and_pack_bytes_are_the_recorded_ones(plans):
    with open(GOLDEN) as f:
        table = json.load(f)
    assert table["f_in"] == F_IN and table["cols"] == list(COLS) and table["flags"] == list(FLAGS)
    by_shape = {(p["f_in"], p["f_g"], p["w_cols"], p["flags"]): p for p in plans}
    n = 0
    for f_in, row in zip(table["f_in"], table["rows"]):
        for i, f_g in enumerate(COLS):
            for j, w in enumerate(COLS):
                for flags, layouts in zip(FLAGS, row["layout"]):
                    p = by_shape[(f_in, f_g, w, flags)]
                    assert LAYOUT_CODE[p["layout"]] == layouts[i * len(COLS) + j], (f_in, f_g, w, flags)
                    assert p["pack_bytes_max"] == row["pack_bytes"][i * len(COLS) + j], (f_in, f_g, w, flags)
                    n += 1
    assert n == len(plans)


def test_launch_descriptions_obey_the_kernels_limits(plans):
    for p in plans:
        key = (p["f_in"], p["f_g"], p["w_cols"], p["flags"])
        if not p["valid"]:
            assert not p["longk"] and not p["bf16x3"], key
            continue
        assert p["ldb"] == (p["f_g"] + 3) // 4 * 4 and p["NV"] % 32 == 0 and 0 <= p["NV"] - p["ldb"] - p["w_cols"] < 32, key
        assert p["KS"] == -(-p["f_in"] // 32) and p["NT"] == -(-p["ldb"] // 16) + -(-p["w_cols"] // 16), key
        assert p["refused"] is None, key                    # rows = 200: no family refuses a shape planned for it
        if p["flags"] & _C.GEMM_24BIT:
            assert p["layout"] == "BF16X3", key
        if p["layout"] == "F16X2K":
            assert 1 <= len(p["longk"]) <= 2 and sum(g["tiles"] for g in p["longk"]) == p["NT"], key
            t0 = 0
            for g in p["longk"]:
                assert g["status"] == 0 and g["tile0"] == t0, key
                t0 += g["tiles"]
                assert g["lds"] <= LDS_MAX and 1 <= g["R"] <= 16 and 2 <= g["ring"] <= 4 and g["threads"] <= 1024, (key, g)
                assert g["threads"] <= 64 * g["waves"] and g["per_cu"] * g["lds"] <= LDS_MAX and g["LDX"] == 32 * p["KS"] + 16, (key, g)
                stagers = g["threads"] // 64 - (0 if g["form"] == "all_in_one" else g["mult"])
                assert stagers >= (1 if g["form"] == "all_in_one" else 2), (key, g)
                assert g["R"] * stagers * 64 >= 16 * (p["f_in"] // 4) and g["slot_bytes"] == g["R"] * stagers * 64 * 16, (key, g)
                assert g["mult"] * (2 if g["form"] == "two_tiles" else 1) >= g["tiles"], (key, g)
                assert g["grid"] == min(256 * g["per_cu"], -(-ROWS // 16)), (key, g)
        elif p["layout"] == "BF16X3":
            assert 1 <= len(p["bf16x3"]) <= 2, key
            cols = 0
            for g in p["bf16x3"]:
                assert g["lds"] <= LDS_MAX and g["threads"] <= 1024, (key, g)
                if g["kernel"] == "ws":
                    assert g["threads"] * 4 >= g["pieces"] and g["threads"] == 2 * p["NV"] and p["f_in"] <= 16 * g["ksub"], (key, g)
                    assert g["pieces"] == 32 * 16 * g["ksub"] // 4 and g["grid_x"] == -(-ROWS // 32), (key, g)
                    cols = p["NV"]
                else:
                    assert g["threads"] == 256 and g["grid_x"] == -(-ROWS // 128) and g["vblock0"] * 192 == cols, (key, g)
                    assert g["vec4"] == (p["f_in"] % 4 == 0), (key, g)
                    cols += {7: 224, 6: 192 * g["grid_y"], 4: 128}.get(g["nt"], p["NV"] - cols)
            assert cols == p["NV"], key                     # the launches cover every virtual column once
        else:
            assert p["layout"] == "F16X2" and not p["longk"] and not p["bf16x3"], key
        for tile_rows in (64, 16):
            assert p["ranges"][tile_rows] == [(0, ROWS)], key


def test_the_grid_reaches_every_instance_a_shape_can_reach(plans):
    """Every compiled instance of the bf16x3 kernels is reached.  Of the long-k instances the grid reaches every one that ANY
    shape reaches: the second run below walks the whole domain of the long-k kernels (every F_in, every split of 1 .. 32 column
    tiles that changes a launch) and must name the same set.  What it does not name is compiled and never launched:
    UNREACHED_LONGK, which only shrinks."""
    seen = instances(plans)
    assert {i for i in seen if i[0] in ("ws", "staged")} == WS_INSTANCES | STAGED_INSTANCES
    domain = run_plan([(f_in, 16 * tb, 16 * tw, 0, ROWS) for f_in in range(132, 385, 4) for tb in range(1, 33)
                       for tw in range(0, 33 - tb)])
    reachable = {i for i in instances(domain) if i[0] not in ("ws", "staged")}
    assert {i for i in seen if i[0] not in ("ws", "staged")} == reachable
    assert LONGK_INSTANCES - reachable == UNREACHED_LONGK and reachable <= LONGK_INSTANCES


def test_row_ranges_are_whole_tiles_below_2_gib(monkeypatch):
    big = 3 * (1 << 30)
    for f_in, f_g, w in ((128, 64, 128), (352, 176, 32)):
        p = run_plan([(f_in, f_g, w, 0, big)])[0]
        widest = max(f_in, p["ldb"], w)
        for tile_rows, ranges in p["ranges"].items():
            assert ranges[0][0] == 0 and sum(n for _, n in ranges) == big
            for (r0, n), nxt in zip(ranges, ranges[1:] + [(big, 0)]):
                assert r0 + n == nxt[0] and n * widest * 4 <= 0x7FFFFFF0 and (n % tile_rows == 0 or r0 + n == big)
            assert len(ranges) == -(-big // (0x7FFFFFF0 // (4 * widest) // tile_rows * tile_rows))
    for hook, expect in (("192", {64: [(0, 192), (192, 8)], 16: [(0, 192), (192, 8)]}),
                         ("96", {64: [(0, 64), (64, 64), (128, 64), (192, 8)], 16: [(0, 96), (96, 96), (192, 8)]}),
                         ("1", {64: [(0, 64), (64, 64), (128, 64), (192, 8)], 16: [(i, min(16, 200 - i)) for i in range(0, 200, 16)]})):
        monkeypatch.setenv("EGC_GEMM_MAX_ROWS", hook)
        assert run_plan([(128, 64, 128, 0, ROWS)])[0]["ranges"] == expect
