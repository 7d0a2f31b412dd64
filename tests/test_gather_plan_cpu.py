"""Host-side logic of the gather plan (egc_gather_plan.hip, egc_amd/graph.py), no GPU: the bit-width arithmetic and the decision
not to pack (egc_gather_plan_form is the function the device builder decides with), the plan's layout, which graphs get a plan at
all -- trim_launches() on a partition, a rectangular adjacency or a GraphBatch builds nothing -- and that the binding documented
in INTEGRATION.md declares the same egc_graph as egc_amd/_C.py."""
import ctypes as C
import os
import re

import pytest
import torch

import egc_amd
from egc_amd import _C
from egc_amd.graph import CSRGraph, GraphBatch


def form(n, n_table, min_col_bits=0):
    v = int(_C.load().egc_gather_plan_form(n, n_table, min_col_bits))
    return v & 0xff, v >> 8


@pytest.mark.parametrize("n,cb", [(1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (67, 7), (128, 7), (129, 8), (169343, 18), (1 << 18, 18),
                                  ((1 << 18) + 1, 19), ((1 << 31) - 2, 31)])
def test_source_id_bits(n, cb):
    assert form(n, 1) == (_C.GP_PACKED, cb)          # cb = ceil(log2(n)), at least 1
    assert (1 << cb) >= n and (cb == 1 or (1 << (cb - 1)) < n)


def test_packed_while_the_table_fits_the_spare_bits():
    # the benchmark's graph: 18 bits of source id leave 14 bits -- 16,384 table entries; it has 358
    assert form(169343, 358) == (_C.GP_PACKED, 18)
    assert form(169343, 1 << 14) == (_C.GP_PACKED, 18)
    assert form(169343, (1 << 14) + 1) == (_C.GP_UNFIT, 18)
    # one spare bit holds two values; no spare bit holds none
    assert form(67, 2, 31) == (_C.GP_PACKED, 31)
    assert form(67, 3, 31) == (_C.GP_UNFIT, 31)
    assert form(67, 1, 32) == (_C.GP_UNFIT, 32)
    assert form((1 << 31) - 2, 2) == (_C.GP_PACKED, 31) and form((1 << 31) - 2, 3) == (_C.GP_UNFIT, 31)
    # min_col_bits only ever widens
    assert form(169343, 358, 7) == (_C.GP_PACKED, 18) and form(169343, 358, 24) == (_C.GP_UNFIT, 24)
    # refused arguments
    assert int(_C.load().egc_gather_plan_form(-1, 1, 0)) == 0 and int(_C.load().egc_gather_plan_form(5, 1, 33)) == 0


@pytest.mark.parametrize("n,e", [(1, 0), (1, 2), (5, 12), (67, 600), (169343, 2329056)])
def test_layout(n, e):
    lib = _C.load()
    table, ent, end = (int(lib.egc_gather_plan_offset(n, e, k)) for k in range(3))
    assert table == _C.GP_HEADER_INTS and all(o % 4 == 0 for o in (table, ent, end))     # 16-byte aligned parts
    assert ent - table >= n and end - ent >= e and table < ent < end
    assert int(lib.egc_gather_plan_bytes(n, e)) == 4 * end
    assert int(lib.egc_gather_plan_offset(n, e, 3)) == -1 and int(lib.egc_gather_plan_offset(-1, e, 0)) == -1


def host_graph(n, n_src=None):
    """A CSRGraph over host tensors (an empty CSR; plan[1] = 0 chunks): enough for the decisions trim_launches takes."""
    z = torch.zeros(max(n, 1) + 1, dtype=torch.int32)
    one = torch.zeros(1, dtype=torch.int32)
    f = torch.zeros(max(n, n_src or n, 1), dtype=torch.float32)
    return CSRGraph(n, 0, z, one, one, f, f.clone(), torch.full((1,), -1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), n_src)


def test_partitions_and_rectangular_graphs_get_no_plan(monkeypatch):
    def no_build(*a, **k):
        raise AssertionError("the library must not be asked for a plan")
    monkeypatch.setattr(_C, "load", no_build)
    part = host_graph(5)
    part.halo = object()                               # one rank's share of a partition
    assert part.trim_launches() is part and part.gather_plans == {} and part._n_chunks == 0
    rect = host_graph(5, n_src=9)                      # rows and sources of two node types
    assert rect.trim_launches() is rect and rect.gather_plans == {}
    asked = host_graph(5)
    assert asked.trim_launches(gather_plan=False).gather_plans == {}
    with pytest.raises(AssertionError):
        host_graph(5).trim_launches()                  # a square, whole graph does ask


def test_graph_batch_builds_nothing():
    gb = object.__new__(GraphBatch)
    assert gb.trim_launches() is gb and not hasattr(gb, "gather_plans")


def test_c_view_without_a_plan():
    g = host_graph(5)
    st = g.c_struct()
    assert not st.gather_plan_raw and not st.gather_plan_looped
    assert (st.gather_plan_form_raw, st.gather_plan_form_looped) == (0, 0)
    assert C.sizeof(_C.EgcGraph) == 13 * 8 + 2 * 8 + 2 * 4    # the trailing fields of include/egc_hip.h's egc_graph


def test_the_documented_binding_declares_the_same_graph_struct():
    """INTEGRATION.md's ctypes stub is what a caller outside this package copies: a struct that ends early would have the library
    read past it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    body = text[text.index("class EgcGraph(C.Structure):"):]
    body = body[:body.index("class EgcLayer(C.Structure):")]
    documented = re.findall(r'\("(\w+)", C\.(\w+)\)', body)
    assert [(name, getattr(C, t)) for name, t in documented] == list(_C.EgcGraph._fields_)
