"""The host side of the one-launch batch kernel (egc_amd/csrc/egc_fused_tile_host.h: form and envelope, the fields of FusedTileArgs,
the LDS image, the tile test, the capacities, the packed operands' layouts, the grid), run without a GPU by
tests/fused_tile_plan/fused_tile_plan_check.cpp and held to tests/fused_tile_ref.py, the transcription of the arithmetic the
planner replaced.

(a) every field of both plans, the image, the tile test's status, both capacities, the pack layouts and the grid are the
    transcription's -- with ONE permitted difference, asserted in both directions: the transcription keeps the old split between a
    capacity query (which never looked at the launch's bound on ``emax``) and its launch; the planner's capacity is 0 beyond the
    bound.  Every line where they differ has ``emax`` beyond the bound, and every such line with a positive old capacity differs;
(b) the compared set reaches all three forms, both quanta, one and two passes, one to three slabs, the backward's 6- and 8-chunk
    caps and each refusal code;
(c) the library's own queries answer the plan's numbers for the launch-envelope grid.

GRID is the layers of test_launch_envelope_cpu.grid() and the product HEADS x BASES x LENGTHS x LISTS x F_INS, each with both
``with_post``, every TCAPS and every EMAXS: 6.5 million lines.  The sanitized check program walks all of it
(``full_grid_lines``); this file the envelope layers and SAMPLE layers of the product."""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

import fused_tile_ref as ref
from egc_amd import _C
from egc_amd.functional import padded_basis_stride
from test_launch_envelope_cpu import grid as envelope_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "fused_tile_plan", "_build", "fused_tile_plan_check")

S, M, X, N, V, D, Y = (_C.AGGR_SUM, _C.AGGR_MEAN, _C.AGGR_MAX, _C.AGGR_MIN, _C.AGGR_VAR, _C.AGGR_STD, _C.AGGR_SYMNORM)
HEADS = (1, 2, 4, 8, 16)
BASES = (1, 2, 3, 4, 8)
LENGTHS = (4, 12, 16, 21, 24, 37, 40, 56, 64)
LISTS = ((S,), (X,), (D,), (Y,), (S, M), (S, X), (S, D), (S, Y), (S, M, N), (S, M, X), (S, D, X), (Y, X, M),
         (S, M, N, V), (S, M, X, Y), (S, D, X, Y), (S, M, X, D))     # 1 .. 4 aggregators without and with max / std / symnorm
F_INS = (4, 6, 100, 128, 132, 256, 260, 320, 324)
TCAPS = (0, 8, 16, 32, 48, 96, 112, 128, 144, 160, 176)
EMAXS = (-1, 0, 1, 4096, 16384, 16385, 20000, 65535, 65536)
BATCHES = ((100, 3000, 0, None), (1, 5, 1, 7), (1000, 100000, 0, 0), (3, 1000, 0, 1000), (0, 0, 1, None), (40, 200, 0, 64))
SAMPLE, SAMPLE_SEED = 1200, 323
FORMS = {0: "none", 1: "narrow", 2: "wide"}
IMAGE = ("off_rec", "off_planes", "off_rowinv", "off_bases", "off_wt", "off_col", "off_rowptr", "off_cnt", "off_dis", "csr_stride",
         "off_db", "off_rowinv2", "total")
DERIVED_F = ("n_ct", "n_slabs", "k16", "ldbp", "w_aw", "wl_floats", "nsets", "p0", "magic0", "magic1", "k2")
DERIVED_B = ("n_ct", "w_aw", "wl_floats", "nsets", "k2")            # (the old backward launch left the wide-only fields unset)


def product_layers():
    """ref.Layer for every cell of the product (the basis stride the layer classes choose), lazily."""
    for H, B, L, aggrs, f_in in itertools.product(HEADS, BASES, LENGTHS, LISTS, F_INS):
        yield ref.layer_fields(H * L, H, B, aggrs, padded_basis_stride(H * L, H, B), ref.ACT_NONE, f_in)


def envelope_layers():
    return [ref.layer_fields(s["out_channels"], s["num_heads"], s["num_bases"], s["aggr_codes"], s["basis_stride"], s["weight_act"],
                             s["in_channels"]) for s in envelope_grid()]


def line(a, with_post, tcap, emax, batch):
    n_graphs, n_nodes, no_static, ft_grid = batch
    return "%d %d %d %d %d %d %d %d %d %s  %d %d  %d %d  %d %d  %d %s\n" % (
        a.H, a.B, a.A, a.L, a.Ls, a.ldb, a.slots, a.W, a.act, " ".join(map(str, a.aggr)), a.f_in, with_post, tcap, emax, n_graphs, n_nodes,
        no_static, "-" if ft_grid is None else ft_grid)


def layer_lines(a, i=0):
    for with_post, tcap, emax in itertools.product((0, 1), TCAPS, EMAXS):
        i += 1
        yield (a, with_post, tcap, emax, BATCHES[i % len(BATCHES)])


def full_grid_lines():
    for a in itertools.chain(envelope_layers(), product_layers()):
        for k in layer_lines(a):
            yield line(*k)


def run_plan(lines):
    subprocess.run(["bash", os.path.join(ROOT, "tests", "fused_tile_plan", "build.sh")], check=True, capture_output=True)
    r = subprocess.run([BIN], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    names = out[0].split()[1:]
    plans = [dict(zip(names, map(int, row.split()[1:]))) for row in out[1:] if row]
    assert len(plans) == len(lines) and all(len(p) == len(names) for p in plans)
    return plans


@pytest.fixture(scope="module")
def compared():
    """[(layer, with_post, tcap, emax, batch, plan)]: the envelope layers, then the sample of the product."""
    every = list(product_layers())
    assert len(every) == len(HEADS) * len(BASES) * len(LENGTHS) * len(LISTS) * len(F_INS) and len(every) > SAMPLE
    layers = envelope_layers() + random.Random(SAMPLE_SEED).sample(every, SAMPLE)
    keys = [k for i, a in enumerate(layers) for k in layer_lines(a, i)]
    return [k + (p,) for k, p in zip(keys, run_plan([line(*k) for k in keys]))]


def _check_direction(p, pre, a, status, image, derived, names, cap_old, bound, emax, key):
    """One direction of one line against the transcription; returns whether the capacity differs from the old query's."""
    get = lambda n: p[pre + n]
    assert get("ok") == status, key
    want = image if image is not None else dict.fromkeys(IMAGE, 0)       # (refused before the image: the program prints zeros)
    assert {n: get(n) for n in IMAGE} == {n: want[n] for n in IMAGE}, key
    if derived is not None:
        assert {n: get(n) for n in names} == {n: derived[n] for n in names}, key
    differs = get("cap") != cap_old
    if differs:
        assert emax > bound and get("cap") == 0, key
    if emax > bound and cap_old > 0:
        assert differs, key
    return differs


def compare(compared):
    """Every line against the transcription; returns how many capacities differ from the old queries', per direction."""
    caps, differing = {}, {"f_": 0, "b_": 0}
    for a, with_post, tcap, emax, batch, p in compared:
        key = (a, with_post, tcap, emax)
        ck = (a, with_post, emax)
        if ck not in caps:
            caps[ck] = (ref.capacity(a, emax, bool(with_post)), ref.bwd_capacity(a, emax))
        # forward
        assert FORMS[p["f_form"]] == ref.form(a) and p["f_quantum"] == ref.quantum(a), key
        st, img, der = ref.launch(a, tcap, emax, bool(with_post))
        if der is None and ref.form(a) != "none":              # (an INVALID launch derived nothing; the plan's fields do not depend on the tile)
            der = ref.derived(a, ref.form(a) == "wide", ref.ftw_aw(a) if ref.form(a) == "wide" else 4)
        differing["f_"] += _check_direction(p, "f_", a, st, img, der, DERIVED_F, caps[ck][0], 65535, emax, key)
        assert p["f_pk_bytes"] == ref.pack_bytes(a), key
        if ref.form(a) != "none":
            assert p["f_max_emax"] == 65535 and p["f_quantum"] * p["f_max_chunks"] == 160, key
            assert p["f_pk_tail_at"] * 2 + p["f_pk_tail_floats"] * 4 == p["f_pk_bytes"] and p["f_pk_bias_at"] * 2 == p["f_pk_tail_floats"], key
            assert p["f_pk_columns"] == (192 if ref.form(a) == "narrow" else 32 * der["n_ct"]), key
            assert p["f_pk_k_rows"] == (128 if ref.form(a) == "narrow" else 16 * der["k16"]), key
        # backward
        assert p["b_form"] == int(ref.bwd_shape(a)), key
        st, img, der = ref.bwd_launch(a, tcap, emax)
        if der is None and ref.bwd_shape(a):
            der = ref.derived(a, False, 4)
        differing["b_"] += _check_direction(p, "b_", a, st, img, der, DERIVED_B, caps[ck][1], 16384, emax, key)
        assert p["b_pk_bytes"] == ref.bwd_pack_bytes(a), key
        if ref.bwd_shape(a):
            assert (p["b_quantum"], p["b_max_chunks"], p["b_max_emax"]) == (16, ref.bwd_chunks(a), 16384), key
            assert (p["b_pk_columns"], p["b_pk_k_rows"], p["b_pk_tail_at"], p["b_pk_tail_floats"]) == (128, 192, 8 * 6 * 2 * 64 * 8, 128), key
        # a capacity is a tile its launch runs
        for pre, launch in (("f_", lambda t: ref.launch(a, t, emax, bool(with_post))[0]), ("b_", lambda t: ref.bwd_launch(a, t, emax)[0])):
            if p[pre + "cap"] > 0 and tcap == TCAPS[0]:
                assert launch(p[pre + "cap"]) == ref.OK and launch(p[pre + "cap"] + p[pre + "quantum"]) != ref.OK, key
        # the switches and the grid
        n_graphs, n_nodes, no_static, ft_grid = batch
        assert p["static_cfg"] == (not no_static) and p["grid"] == ref.grid(n_graphs, n_nodes, ft_grid), key
    return differing


def test_the_plan_is_the_old_arithmetic(compared):
    # the permitted difference exists on the backward side (H = 4 at 20000 edges: 48 rows by the old query, refused by every launch);
    # the forward's image never fits beyond its bound, so its query already answered 0 there
    differing = compare(compared)
    assert differing["b_"] > 0 and differing["f_"] == 0


def test_the_compared_set_reaches_everything(compared):
    plans = [p for *_, p in compared]
    assert {p["f_form"] for p in plans} == {0, 1, 2} and {p["b_form"] for p in plans} == {0, 1}
    assert {p["f_quantum"] for p in plans} == {0, 16, 32}
    assert {p["f_nsets"] for p in plans if p["f_form"]} == {1, 2}
    assert {p["f_n_slabs"] for p in plans if p["f_form"] == 2} == {1, 2, 3}
    assert {p["b_max_chunks"] for p in plans if p["b_form"]} == {6, 8}
    for pre in ("f_", "b_"):
        assert {p[pre + "ok"] for p in plans} == {ref.OK, ref.INVALID, ref.UNSUPPORTED}
        # UNSUPPORTED for either reason: outside the envelope, and an image beyond the LDS
        assert any(p[pre + "ok"] == ref.UNSUPPORTED and p[pre + "form"] for p in plans) and any(not p[pre + "form"] for p in plans)
        assert len({p[pre + "cap"] for p in plans}) > 3
    assert {p["f_w_aw"] for p in plans if p["f_form"] == 2} == {1, 2, 4}


def test_the_library_answers_the_plans_numbers(monkeypatch):
    monkeypatch.delenv("EGC_STDVAR_REFERENCE", raising=False)
    lib = _C.load()
    specs = envelope_grid()
    edges = (-1, 0, 1, 4096, 16384, 16385, 20000, 65535, 65536)
    keys = [(a, post, 16, e, BATCHES[0]) for a in envelope_layers() for post in (0, 1) for e in edges]
    plans = iter(run_plan([line(*k) for k in keys]))
    positive = 0
    for spec, a in zip(specs, envelope_layers()):
        lay = _C.make_layer(**spec)
        p = C.byref(lay)
        looped = (spec["agg_set"] == _C.SET_LOOPED, spec["sym_set"] == _C.SET_LOOPED)
        fwd_in, bwd_in = (ref.gate(a, *looped, spec["weight_layout"], two) for two in (True, False))
        for post in (0, 1):
            for e in edges:
                pl = next(plans)
                assert lib.egc_batch_fused_tile_nodes(p, e, post) == (pl["f_cap"] if fwd_in else 0), (spec, post, e)
                assert lib.egc_batch_fused_bwd_tile_nodes(p, e) == (pl["b_cap"] if bwd_in else 0), (spec, e)
                positive += pl["f_cap"] > 0 and fwd_in
        assert lib.egc_batch_fused_tile_quantum(p) == (pl["f_quantum"] if fwd_in else 0), spec
        assert lib.egc_batch_fused_pack_bytes(p) == (pl["f_pk_bytes"] if fwd_in else 0), spec
        assert lib.egc_batch_fused_bwd_pack_bytes(p) == (pl["b_pk_bytes"] if bwd_in else 0), spec
    assert positive > 100
