"""The (H, C) table of the GAT v1 geometry sweep without a GPU (tests/gat1_ref.py: SWEEP_SHAPES, geometry, sweep_reference).  This
guards the TABLE, not the kernel: that its shapes reach every template instance, every group size and both access widths of
egc_gat.hip, the heads whose row-end sum straddles lanes or crosses column 256, and the reference's six shapes; that
``geometry`` restates the library's own (where the library can be asked without a device); and that on every sweep shape the
float32 restatement -- the GPU sweep's yardstick, the factored destination-pass sums included -- stays within the project's bound of the
float64 one."""
import itertools

import numpy as np
import pytest

from egc_amd import _C
from egc_amd._gat import _ext_width
from gat1_ref import (CHUNK, DISTANCE, QUANTITIES, REFERENCE_SHAPES, SHAPES, SWEEP_SHAPES, aggregate_forward, geometry, lse_distance,
                      per_edge_backward, rel_grad, rel_out, sweep_graph, sweep_inputs, sweep_reference, workspace_bytes)

BOUND = 1e-5        # the floor of the project's rule max(1e-5, 5 x the reference's own float32 distance)


def _id(s):
    return f"{s[0]}x{s[1]}"


def test_the_table_holds_the_shapes_it_was_set_up_with():
    assert len(set(SWEEP_SHAPES)) == len(SWEEP_SHAPES) and all(1 <= h * c <= 512 for h, c in SWEEP_SHAPES)
    assert REFERENCE_SHAPES == ((8, 19), (1, 152), (8, 30), (1, 240), (8, 38), (1, 304)) and set(REFERENCE_SHAPES) <= set(SWEEP_SHAPES)
    assert {s for s in SHAPES.values() if s[0] * s[1] >= 152} <= set(REFERENCE_SHAPES)


def test_the_table_covers_every_instance_group_size_and_access_width():
    geoms = {s: geometry(*s) for s in SWEEP_SHAPES}
    triples = {(g["S"], g["vec_by_width"], g["small"]) for g in geoms.values()}
    assert triples == set(itertools.product((1, 2), (True, False), (True, False)))
    assert {g["G"] for g in geoms.values()} == {1, 2, 4, 8, 16, 32, 64}
    assert {g["vec_by_width"] for g in geoms.values()} == {True, False}
    assert all(g["V"] == g["S"] * g["G"] and (g["S"] == 1 or g["G"] == 64) for g in geoms.values())
    # a head's row-end sum across lanes: heads that start inside a quad, at both access widths and both slot counts
    for s, vec in itertools.product((1, 2), (True, False)):
        assert any(g["straddles"] and g["S"] == s and g["vec_by_width"] == vec for g in geoms.values()), (s, vec)
    assert sum(g["spans_256"] for g in geoms.values()) >= 4 and sum(g["boundary_256"] for g in geoms.values()) >= 1
    assert not any(g["spans_256"] or g["boundary_256"] for g in geoms.values() if g["S"] == 1)
    for (h, c), head in (((3, 100), 2), ((8, 33), 7), ((37, 13), 19), ((128, 3), 85), ((8, 38), 6)):
        assert head < h and head * c < 256 < (head + 1) * c and geoms[(h, c)]["spans_256"]
    assert geoms[(2, 256)]["boundary_256"] and geoms[(1, 304)]["spans_256"]
    for s in (1, 2):
        assert {c for (h, c), g in geoms.items() if g["small"] and g["S"] == s} >= {1, 3}
    # the reference's shapes: all 16-byte rows; H = 8 fills the extended array, H = 1 leaves two pad columns
    for h, c in REFERENCE_SHAPES:
        g = geoms[(h, c)]
        assert g["vec_by_width"] and g["G"] == 64 and g["S"] == (2 if h * c > 256 else 1)
        assert g["ext_width"] - (h * c + 2 * h) == (0 if h == 8 else 2)


@pytest.mark.parametrize("shape", SWEEP_SHAPES + tuple(sorted(set(SHAPES.values()) - set(SWEEP_SHAPES))), ids=_id)
def test_geometry_agrees_with_the_library(shape):
    h, c = shape
    lib = _C.load()
    fwd, bwd = workspace_bytes(h, c, 40, 1000)
    assert lib.egc_gat_forward_workspace_bytes(1000, h, c) == fwd == 4 * geometry(h, c)["V"] * 48
    assert lib.egc_gat_backward_workspace_bytes(40, 1000, h, c) == bwd
    assert lib.egc_gat_backward_workspace_bytes(40, CHUNK, h, c) == workspace_bytes(h, c, 40, CHUNK)[1] == 4 * ((40 * h + 3) // 4 * 4)
    assert lib.egc_gatv2_forward_workspace_bytes(1000, h, c) == fwd                 # one mapping for both attention kernels
    assert _ext_width(h, c) == geometry(h, c)["ext_width"] >= h * c + 2 * h and _ext_width(h, c) % 4 == 0


def test_sweep_inputs():
    xl, a_src, a_dst, gout = sweep_inputs(3, 43, 40, 7)
    assert xl.shape == gout.shape == (40, 129) and a_src.shape == a_dst.shape == (40, 3)
    assert all(a.dtype == np.float32 for a in (xl, a_src, a_dst, gout))
    assert not np.array_equal(a_src, a_dst) and np.array_equal(xl, sweep_inputs(3, 43, 40, 7)[0])


@pytest.mark.parametrize("loops", (True, False))
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=_id)
def test_float32_restatement_is_within_the_bound_of_the_float64_one(shape, loops):
    h, c = shape
    ref = sweep_reference(h, c, loops)
    same, _ = lse_distance(ref[np.float32][1], ref[np.float64][1])
    assert same and (loops or int((~np.isfinite(ref[np.float64][1])).all(axis=1).sum()) >= 3)
    for k, a32, a64 in zip(QUANTITIES, ref[np.float32], ref[np.float64]):
        d = DISTANCE[k](a32, a64)
        print(f"H {h} C {c} loops {int(loops)} {k}: float32 restatement against float64 {d:.3e}, bound {BOUND:.0e}")
        assert d <= BOUND, (k, d)


@pytest.mark.parametrize("shape", ((12, 5), (2, 3), (8, 38), (128, 3)), ids=_id)
@pytest.mark.parametrize("loops", (True, False))
def test_restatement_is_the_per_edge_form_beyond_rounding(shape, loops):
    """One shape per (S, small) pair: the float64 truth of the sweep hinges neither on the chunk and batch cuts it shares with
    the kernel nor on the factoring of the backward sums."""
    h, c = shape
    g = geometry(h, c)
    assert (g["S"], g["small"]) == {(12, 5): (1, False), (2, 3): (1, True), (8, 38): (2, False), (128, 3): (2, True)}[shape]
    ei, n = sweep_graph(5)
    xl, a_src, a_dst, gout = sweep_inputs(h, c, n, 7)
    out, lse, dxl, das, dad = sweep_reference(h, c, loops)[np.float64]
    b, lb = aggregate_forward(xl, a_src, a_dst, ei, loops=loops, chunk=10 ** 9, ahead=1)
    fin = np.isfinite(lse)
    assert np.array_equal(fin, np.isfinite(lb)) and (loops or int((~fin).sum()) >= 3 * h)
    assert rel_out(out, b) <= 1e-12 and rel_out(lse[fin], lb[fin]) <= 1e-12
    for got, want in zip((dxl, das, dad), per_edge_backward(xl, a_src, a_dst, ei, out, lse, gout, loops=loops)):
        assert rel_grad(got, want) <= 1e-11
