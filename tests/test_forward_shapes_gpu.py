"""The full-graph inference aggregate + combine on the GPU at every form it dispatches on: the table of tests/forward_ref.py
(every compiled-in configuration and the whole run-time ladder of agg_fast_kernel, both configurations and the ladder of
agg_wide_kernel, the LDS kernels at one to four chunks, four and one wavefronts a block and every small lane group), each case
plain and with the full fused post-op ``relu((z + bias) * scale + shift) + residual``, on the square ladder graph (rows of
0 .. 768 entries: long rows first, last and adjacent, 63 / 64 / 65 around the hand-over to chunks) and on its transpose.

The operands go in directly -- no GEMM in front -- through the Python entry points of egc_amd.functional, ``out`` is full of NaN
before every call, and EVERY output is held to the restatement in float64 on the same float32 operands at the project's 1e-5 on the
scale of the element's OWN row (golden_util.elementwise_excess <= 1): a few wrong columns of a short row cannot hide behind a hub.
std / var layers are held to the same bound; their inputs are rounded to eighths, so that it holds for any correct float32
evaluation.  Each form of a case -- by default, without compiled-in configurations, without the two-slots-per-lane kernel, on the
LDS kernels -- is held to float64 itself, so nothing here depends on forward_ref.dispatch being right.  The measured excess is
printed next to the float32 restatement's own (tests/test_forward_shapes_cpu.py keeps that one below one half)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from backward_ref import arg_positions, gradients, real_columns, rel_grad, rel_out
from egc_amd import functional as F
from forward_ref import (ACTS, BIG_CASE, CASES, CODES, FAMILIES, INPUT_SEED, LAYOUTS, NOLOOP_CASES, POST_SEED, RECT_CASES, RPW_ROWS, SETS,
                         STRIDED_CASES, TAIL_ROWS, THRESHOLD, TIE_CASES, VARIANTS, aggregate_combine, dispatch, edges, family, forms,
                         geometry, graph_key, hba_columns, home, make_inputs, make_post, n_loop_of, post_of, post_op)
from golden_util import elementwise_excess

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOTH = (False, True)
IDS = dict(ids=lambda c: c.name)
FLIPS = dict(ids=("ladder", "flip"))
FORM_NAMES = {(): "default", ("EGC_NO_STATIC_CFG",): "no_static", ("EGC_NO_WIDE",): "no_wide", ("EGC_FORCE_GENERIC",): "generic"}
BLOCK_AT = 4          # first column of a strided weightings block inside the wider array (16 bytes)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device_graph(kind, flip, reduced):
    ei, n, n_src = edges(kind, flip, reduced)
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n, n_src)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n, n_src, ei.shape[1])
    return g


def device_graph(case, kind, flip=False):
    return _device_graph(*graph_key(case, kind, flip))


def spec_of(case):
    agg_set, sym_set = SETS[case.sets]
    return F.make_spec(16, case.out, case.H, case.B, [CODES[a] for a in case.aggrs], agg_set, sym_set, case.loops_all,
                       LAYOUTS[case.layout], ACTS[case.act], basis_stride=geometry(case)[1])


@functools.lru_cache(maxsize=None)
def reference(case, kind, flip=False, ties=False):
    """Operands and the restatement before the post-op in float64 (the truth) and float32 (the yardstick): computed once per
    (case, graph, input set) and shared by every form and post variant."""
    ei, n, n_src = edges(*graph_key(case, kind, flip))
    bases, wt, gout = make_inputs(case, n, n_src, INPUT_SEED, ties)
    ops = make_post(case, n, POST_SEED)
    if not case.bias:
        ops["bias"] = None
    n_loop = n_loop_of(case, ei, n)
    with torch.no_grad():
        z = {dt: aggregate_combine(torch.from_numpy(bases).to(dt), hba_columns(torch.from_numpy(wt).to(dt), case), ei, n, case, n_loop)
             for dt in (torch.float64, torch.float32)}
    return dict(ei=ei, n=n, n_src=n_src, n_loop=n_loop, bases=bases, wt=wt, gout=gout, ops=ops, z=z)


def expected(ref, variant, dtype=torch.float64):
    return post_op(ref["z"][dtype], *post_of(ref["ops"], variant, dtype)).numpy()


def on_device(fn):
    """A failing HIP call ends the whole run: nothing more is started on a device that has reported an error."""
    try:
        got = fn()
        torch.cuda.synchronize()
        return got
    except RuntimeError as exc:
        pytest.exit(f"HIP error, the sweep stops here: {exc}", returncode=3)


def operands(case, ref, variant):
    """(bases, weightings, bias, PostOp) on the device.  A strided case's weightings are a column block of a wider array full of
    NaN: a read outside the block shows in the output."""
    n, W = ref["n"], geometry(case)[5]
    wt = _dev(ref["wt"])
    if case.ldw:
        wide = torch.full((n, case.ldw), float("nan"), device=DEV)
        wide[:, BLOCK_AT:BLOCK_AT + W] = wt
        wt = wide[:, BLOCK_AT:BLOCK_AT + W]
        assert wt.stride(0) == case.ldw != W and wt.data_ptr() % 16 == 0
    ops, parts = ref["ops"], VARIANTS[variant]
    post = None
    if parts:
        post = F.PostOp(scale=_dev(ops["scale"]) if "affine" in parts else None, shift=_dev(ops["shift"]) if "affine" in parts else None,
                        residual=_dev(ops["residual"]) if "residual" in parts else None, relu="relu" in parts)
    return _dev(ref["bases"]), wt, (_dev(ops["bias"]) if ops["bias"] is not None else None), post


def run(case, kind, flip=False, variant="plain", ties=False, rows=None, out=None):
    """One inference call through egc_amd.functional.egc_aggregate_combine into an ``out`` full of NaN (or the caller's)."""
    ref = reference(case, kind, flip, ties)
    g = device_graph(case, kind, flip)
    bases, wt, bias, post = operands(case, ref, variant)
    if out is None:
        out = torch.full((ref["n"], case.out), float("nan"), device=DEV)
    if rows is not None:
        wt = wt.contiguous()                                    # (a row range reads dense weightings)
    return on_device(lambda: F.egc_aggregate_combine(g, spec_of(case), bases, wt, bias, post=post, rows=rows, out=out))


def held(got, want, yard, tag, fam):
    """The element-wise excess of ``got`` over float64 ``want``, printed next to the float32 restatement's, asserted <= 1."""
    assert got.shape == want.shape and np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} outputs are not finite"
    excess, own = elementwise_excess(got, want, tol=1e-5), elementwise_excess(yard, want, tol=1e-5)
    print(f"{tag} [{fam}]: measured excess {excess:.3f}, restatement f32-vs-f64 {own:.3f}, bound 1")
    assert excess <= 1.0, f"{tag} [{fam}]: element-wise excess {excess:.3f} > 1 (1e-5 on the scale of the element's own row)"
    return excess


def check(case, kind, flip=False, variant="plain", ties=False, env=()):
    ref = reference(case, kind, flip, ties)
    out = run(case, kind, flip, variant, ties).cpu().numpy()
    tag = (f"{case.name} {'/'.join(str(k) for k in kind)}{' flip' if flip else ''}{' ties' if ties else ''} {variant}"
           f"{' ' + FORM_NAMES[env] if env else ''}")
    return held(out, expected(ref, variant), expected(ref, variant, torch.float32), tag, family(case, ref["n"], env))


def _forms():
    return [pytest.param(c, env, id=f"{c.name}-{FORM_NAMES[env]}") for c in CASES for env in forms(c, 32)]


@pytest.mark.parametrize("flip", BOTH, **FLIPS)
@pytest.mark.parametrize("variant", ("plain", "full"))
@pytest.mark.parametrize("case,env", _forms())
def test_every_cell_in_every_form_against_float64(case, env, variant, flip, monkeypatch):
    """Every case plain and with the full post-op, on the ladder (with the isolated tail where the case has no loops_all) and
    its transpose: by default, and under every switch that sends the case to other kernels."""
    for name in env:
        monkeypatch.setenv(name, "1")
    check(case, home(case), flip, variant, env=env)


def _family_cases(k=3):
    return [c for fam in FAMILIES for c in [c for c in CASES if family(c) == fam][:k]]


@pytest.mark.parametrize("variant", ("affine", "relu", "residual"))
@pytest.mark.parametrize("case", _family_cases(), **IDS)
def test_the_parts_of_the_post_op_one_at_a_time(case, variant):
    """Scale + shift only, relu only, residual only, on three cases of each epilogue: register contiguous, register padded,
    two slots per lane, LDS with one chunk, LDS with several."""
    check(case, home(case), variant=variant)


def test_one_of_scale_and_shift_alone_is_refused():
    case = CASES[0]
    ref = reference(case, home(case))
    g = device_graph(case, home(case))
    bases, wt, bias, post = operands(case, ref, "full")
    for lone in (F.PostOp(scale=post.scale), F.PostOp(shift=post.shift, relu=True)):
        with pytest.raises(RuntimeError, match="EGC_ERR_INVALID"):
            F.egc_aggregate_combine(g, spec_of(case), bases, wt, bias, post=lone)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", TIE_CASES, **IDS)
def test_ties_between_entries_and_between_chunks(case):
    """Small-integer bases: nearly every extremum is attained by several entries, in several chunks of a long row and by the
    row's own features."""
    check(case, home(case), variant="full", ties=True)


def _noloop_forms():
    return [pytest.param(c, env, id=f"{c.name}-{FORM_NAMES[env]}") for c in NOLOOP_CASES for env in forms(c, 32)]


@pytest.mark.parametrize("case,env", _noloop_forms())
def test_rows_beyond_the_largest_index_get_no_self_loop(case, env, monkeypatch):
    """loops_all = 0 on the ladder with five rows that appear in no edge: those rows are the epilogue of an EMPTY row -- bias,
    post-op and residual applied once to the empty row's aggregates --, every other row meets the float64 bound."""
    for name in env:
        monkeypatch.setenv(name, "1")
    ref = reference(case, ("tail",))
    n, n_loop = ref["n"], ref["n_loop"]
    assert n_loop == n - TAIL_ROWS
    with torch.no_grad():
        b, w = torch.from_numpy(ref["bases"]).double(), hba_columns(torch.from_numpy(ref["wt"]).double(), case)
        empty = aggregate_combine(b, w, np.zeros((2, 0), dtype=np.int64), n, case, 0)
    for variant in ("plain", "full"):
        want = expected(ref, variant)
        alone = post_op(empty, *post_of(ref["ops"], variant, torch.float64)).numpy()
        assert np.array_equal(want[n_loop:], alone[n_loop:])
        out = run(case, ("tail",), variant=variant).cpu().numpy()
        yard = expected(ref, variant, torch.float32)
        tag = f"{case.name} tail {variant} {FORM_NAMES[env]}"
        held(out[n_loop:], alone[n_loop:], yard[n_loop:], tag + " (rows in no edge)", family(case, n, env))
        held(out[:n_loop], want[:n_loop], yard[:n_loop], tag + " (rows of the ladder)", family(case, n, env))


@pytest.mark.parametrize("case", [next(c for c in NOLOOP_CASES if family(c) == f) for f in ("reg contig", "lds one chunk", "lds chunks")], **IDS)
def test_training_forward_and_backward_without_loops_all(case):
    """egc_aggregate_combine_train + egc_aggregate_combine_backward with loops_all = 0 on the same graph: ``out``, ``d_bases``,
    ``d_weightings`` and the arg positions against float64 autograd through the restatement, at the bounds of
    tests/test_backward_shapes_gpu.py (whose table passes loops_all = 1 everywhere)."""
    from test_backward_shapes_gpu import bound_of
    ref = reference(case, ("tail",))
    ei, n, n_loop = ref["ei"], ref["n"], ref["n_loop"]
    ins = (ref["bases"], ref["wt"], ref["gout"])
    f64, f32 = (gradients(*ins, ei, n, case, dt, n_loop) for dt in (torch.float64, torch.float32))
    g = device_graph(case, ("tail",))
    spec = spec_of(case)
    bases, wt, gout = (_dev(a) for a in ins)

    def call():
        out, saved = F.egc_aggregate_combine_train(g, spec, bases, wt, None)
        d_b, d_w, _ = F.egc_aggregate_combine_backward(g, spec, bases, wt, gout, saved)
        return out, d_b, d_w, saved[2], saved[3]
    out, d_b, d_w, arg_max, arg_min = on_device(call)
    L, Ls, _, _, _, _ = geometry(case)
    e = g.n_edges
    edge_id = g.edge_id.cpu().numpy().astype(np.int64)
    for which, arg in (("max", arg_max), ("min", arg_min)):
        if which not in case.aggrs:
            assert arg is None
            continue
        got = real_columns(arg.cpu().numpy().astype(np.int64), case.B, L, Ls)
        assert got.min() >= -1 and got.max() <= e
        got = np.where((got >= 0) & (got < e), edge_id[np.clip(got, 0, e - 1)], got)
        want = arg_positions(ins[0], ei, n, case, which, n_loop)
        assert (want[n_loop:] == -1).all()                                       # a row in no edge attains its extrema nowhere
        assert np.array_equal(got, want), f"arg_{which}: {int((got != want).sum())} positions differ"
    err = rel_out(out.cpu().numpy(), f64[0])
    print(f"{case.name} tail train out: measured {err:.3e}, bound 1e-5")
    assert err <= 1e-5
    held(out.cpu().numpy()[n_loop:], f64[0][n_loop:], f32[0][n_loop:], f"{case.name} tail train out (rows in no edge)", "train")
    short = np.bincount(ei[0], minlength=n) <= THRESHOLD
    d_b, d_w = d_b.cpu().numpy(), d_w.cpu().numpy()
    assert np.isfinite(d_b).all() and np.isfinite(d_w).all()
    for name, got, yard, truth in (("d_bases", d_b, f32[1], f64[1]), ("d_bases (short source rows)", d_b[short], f32[1][short], f64[1][short]),
                                   ("d_weightings", d_w, f32[2], f64[2])):
        err, y = rel_grad(got, truth), rel_grad(yard, truth)
        bound = bound_of(case, y)
        print(f"{case.name} tail train {name}: measured {err:.3e}, restatement f32-vs-f64 {y:.3e}, bound {bound:.1e}")
        assert err <= bound, name


def _cuts(deg):
    """Row-range boundaries: 0 and n; directly before, on and after a long row between short ones; between two adjacent long rows."""
    n = len(deg)
    long = deg > THRESHOLD
    r = next(r for r in range(1, n - 1) if long[r] and not long[r - 1] and not long[r + 1])
    a = next(a for a in range(n - 1) if long[a] and long[a + 1])
    return sorted({0, n, r - 1, r, r + 1, a + 1})


@pytest.mark.parametrize("case", _family_cases(1), **IDS)
def test_row_ranges(case):
    """egc_aggregate_combine_rows_f32 over [0, k) and then [k, n): rows outside a range keep their NaN, rows inside meet the
    float64 bound, and the two halves together are the single full call bit for bit (a row's entries are folded in the same
    order whichever wavefront and lane group the range gives it to)."""
    kind = home(case)
    ref = reference(case, kind)
    n = ref["n"]
    want, yard = expected(ref, "plain"), expected(ref, "plain", torch.float32)
    full = run(case, kind)
    cuts = _cuts(np.bincount(ref["ei"][1], minlength=n))
    assert len(cuts) >= 6
    for k in cuts:
        out = run(case, kind, rows=(0, k))
        assert bool(torch.isnan(out[k:]).all()), f"k = {k}: rows outside [0, k) were written"
        if k > 0:
            held(out[:k].cpu().numpy(), want[:k], yard[:k], f"{case.name} rows [0, {k})", family(case, k))
        kept = out[:k].clone()
        out = run(case, kind, rows=(k, n), out=out)
        assert torch.equal(out[:k], kept), f"k = {k}: rows outside [k, n) were written"
        assert torch.equal(out, full), f"k = {k}: the two ranges together are not the full call"


@pytest.mark.parametrize("flip", BOTH, **FLIPS)
@pytest.mark.parametrize("more", (True, False), ids=("more_sources", "fewer_sources"))
@pytest.mark.parametrize("case", RECT_CASES, **IDS)
def test_rectangular_graphs(case, more, flip):
    """n_src != n (raw sets, no symnorm): the bases have the sources' rows."""
    for variant in ("plain", "full"):
        check(case, ("rect", more), flip, variant)


@pytest.mark.parametrize("kind", (("sparse",), ("edgeless",)), ids=("sparse", "edgeless"))
@pytest.mark.parametrize("case", CASES, **IDS)
def test_low_degree_and_edgeless_graphs(case, kind):
    """Many rows of at most 17 entries (no long row: the chunk role has nothing to do), and a graph without any edge: a LOOPED
    set leaves every row its own features, or -- without loops_all, the largest index being -1 -- nothing."""
    for variant in ("plain", "full"):
        check(case, kind, variant=variant)


@pytest.mark.parametrize("env", ((), ("EGC_FORCE_GENERIC",)), ids=("default", "generic"))
@pytest.mark.parametrize("case", STRIDED_CASES, **IDS)
def test_a_strided_weightings_block_against_float64(case, env, monkeypatch):
    """The weightings as a column block of a wider array whose surround is NaN, against float64 (not against the dense call)."""
    for name in env:
        monkeypatch.setenv(name, "1")
    for variant in ("plain", "full"):
        check(case, ("ladder",), variant=variant, env=env)
        check(case, ("sparse",), variant=variant, env=env)


def test_four_row_groups_per_wavefront():
    """Exactly 32768 rows at 33 .. 64 slots: launch_fast gives a wavefront four one-row groups; one row fewer in range, one."""
    case, kind = BIG_CASE, ("big",)
    ref = reference(case, kind)
    n = ref["n"]
    assert n == RPW_ROWS and (dispatch(case, n).rows_per_wave, dispatch(case, n - 1).rows_per_wave) == (4, 1)
    for variant in ("plain", "full"):
        check(case, kind, variant=variant)
    out = run(case, kind, rows=(0, n - 1))
    assert bool(torch.isnan(out[n - 1:]).all())
    held(out[:n - 1].cpu().numpy(), expected(ref, "plain")[:n - 1], expected(ref, "plain", torch.float32)[:n - 1],
         f"{case.name} big rows [0, {n - 1})", "reg contig")
    assert torch.equal(out[:n - 1], run(case, kind)[:n - 1])                     # either schedule folds a row in the same order


@pytest.mark.parametrize("case", _family_cases(1), **IDS)
def test_two_calls_are_bit_identical(case):
    """Long rows are merged in chunk order, not in arrival order."""
    a = run(case, home(case), variant="full")
    b = run(case, home(case), variant="full")
    assert torch.equal(a, b)
