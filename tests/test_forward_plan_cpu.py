"""The gather plan's place in the table of the inference-aggregate sweep, without a GPU (tests/forward_ref.py: plan_form,
plan_instances).  agg_fast_kernel<..., PLAN> is a separately compiled kernel per instance; tests/test_forward_plan_gpu.py runs
every case ``plan_form`` names against float64 on trimmed graphs.  This file guards that the cases so named reach EVERY compiled
PLAN instance -- by default and under EGC_NO_STATIC_CFG, where a compiled-in configuration runs its rt<...,0> fallback --, so that
an EGC_STATIC_CFG(..., 0) row added to egc_aggregate_fast.hip without a case fails here, and that ``plan_form`` says no wherever
launch_one / aggregate_combine_impl offer no plan."""
import numpy as np

import backward_ref
from forward_ref import (BIG_CASE, CASES, NOLOOP_CASES, PLAN_CASES, PLAN_FORMS, PLAN_SWITCH, RECT_CASES, STRIDED_CASES, TIE_CASES,
                         dispatch, edges, graph_key, home, need_of, plan_form, plan_instances, static_rows)


def _rows(case, kind=None):
    return edges(*graph_key(case, kind or home(case), False))[1]


def _reached(cases=CASES):
    return {dispatch(c, _rows(c), False, env).instance for c in cases for env in PLAN_FORMS if plan_form(c, home(c), env=env)}


def test_the_cases_reach_every_compiled_plan_instance():
    want = plan_instances()
    static = {n for n in want if n.startswith("st<")}
    assert len(static) == 16 and len(want - static) == 9                      # what the file holds today
    assert static == {r.name for r in static_rows() if r.kind == "reg" and r.need == "0"}
    assert _reached() == want
    assert _reached(PLAN_CASES) == want and all(not plan_form(c, home(c), env=env) for c in CASES if c not in PLAN_CASES for env in PLAN_FORMS)
    # the compiled-in configurations are reached by default, each one's fallback without them
    assert {dispatch(c, _rows(c)).instance for c in PLAN_CASES} >= static
    assert {dispatch(c, _rows(c), False, PLAN_FORMS[1]).instance for c in PLAN_CASES} == want - static


def test_a_plan_row_added_to_the_source_without_a_case_is_noticed():
    source = backward_ref.source_text("egc_aggregate_fast.hip")
    anchor = "    // EGConv / EGC-S default"
    line = "    EGC_STATIC_CFG(8, 4, 16, 2, agg_pack(S, X), EGC_ACT_NONE, false, false, true, 0)\n"
    more = source.replace(anchor, line + anchor)
    assert more != source and plan_instances(more) - _reached() == {"st<8,4,16,sum+max,none,raw>"}
    # ... a row with optional aggregates has no PLAN form and adds none
    sq = source.replace(anchor, line.replace("agg_pack(S, X)", "agg_pack(S, EGC_AGGR_STD)").replace("true, 0)", "true, NEED_SQ)") + anchor)
    assert sq != source and plan_instances(sq) == plan_instances()
    # dropping the only case of an instance is noticed too
    for lone in ("rt<5,4,0>", "st<8,4,44,mean,none,looped>"):
        fewer = tuple(c for c in CASES if c.cell != lone)
        assert len(fewer) == len(CASES) - 1 and plan_instances() - _reached(fewer) == {lone}


def test_plan_form_is_the_offer_of_the_launcher():
    by_cell = {c.cell: c for c in CASES}
    north = CASES[0]
    assert plan_form(north, ("ladder",)) and plan_form(north, ("sparse",)) and plan_form(north, ("edgeless",)) and plan_form(north, ("tail",))
    n = _rows(north)
    assert plan_form(north, ("ladder",), rows=(0, n)) and not plan_form(north, ("ladder",), rows=(0, n - 1))
    assert not plan_form(north, ("ladder",), rows=(1, n))
    assert not plan_form(north, ("ladder",), env=(PLAN_SWITCH,)) and not plan_form(north, ("ladder",), env=("EGC_FORCE_GENERIC",))
    raw = next(c for c in RECT_CASES if need_of(c) == "0" and dispatch(c, 32).family == "reg")
    assert plan_form(raw, ("ladder",)) and not plan_form(raw, ("rect", True)) and not plan_form(raw, ("rect", False))
    for cell in ("rt<4,1,SQ>", "rt<5,2,MN>", "rt<6,4,SQ|MN>", "st<8,4,16,sum+std+max+symnorm,none,looped>", "wide<1,0>", "lds<1>/4", "lds<3>/4"):
        assert not plan_form(by_cell[cell], home(by_cell[cell])), cell
    assert plan_form(BIG_CASE, ("big",)) and dispatch(BIG_CASE, _rows(BIG_CASE, ("big",))).rows_per_wave == 4


def test_the_plan_cases_cover_what_the_gpu_file_runs_them_for():
    cells = {c.name: dispatch(c, _rows(c)) for c in PLAN_CASES}
    assert {cells[c.name].lpr_log2 for c in PLAN_CASES} == {4, 5, 6}
    for lg in (4, 5, 6):
        group = [c for c in PLAN_CASES if cells[c.name].lpr_log2 == lg]
        assert {cells[c.name].store for c in group} == {"contig", "padded"}, lg
    assert {c.act for c in PLAN_CASES} == {"none", "sigmoid", "hardtanh"} and {c.bias for c in PLAN_CASES} == {True, False}
    assert {c.sets for c in PLAN_CASES} == {"raw", "looped", "lay"}
    assert {4} <= {-(-c.H // c.B) for c in PLAN_CASES}                                    # four heads per lane
    noloop = [c for c in NOLOOP_CASES if c in PLAN_CASES]
    assert len(noloop) >= 2 and all(home(c) == ("tail",) for c in noloop)
    assert {cells[c.name].lpr_log2 for c in STRIDED_CASES if c in PLAN_CASES} == {4, 5}
    assert any(c in PLAN_CASES for c in TIE_CASES)
    # both plans are read: a layer with symnorm takes its sym set's, one without the looped one where it exists
    assert any("symnorm" in c.aggrs and c.sets == "raw" for c in PLAN_CASES) and any("symnorm" in c.aggrs and c.sets != "raw" for c in PLAN_CASES)
    # the ladder has the rows the reload of more than one lane group's entries needs at 16 and 64 lanes; 32 lanes: the module's own graph
    deg = set(np.bincount(edges(("ladder",))[0][1]).tolist())
    assert {0, 1, 15, 16, 17, 63, 64, 65} <= deg and not {31, 32, 33} & deg
