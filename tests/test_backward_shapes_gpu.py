"""The kernels of the layer backward (egc_amd/csrc/egc_backward.hip) and the arg pass of the training forward on the GPU at every
form they dispatch on: the table of tests/backward_ref.py (every instance of bwd_dst_fast_kernel, bwd_dst_kernel at four and one
wavefronts a block, every compiled flag word and the four run-time forms of bwd_src_kernel, the records fused, separate and off,
arg_extrema_kernel<1..4>), on the square ladder graph (rows of 0 .. 768 entries on both sides: 3 / 4 / 5 around the source
kernel's load pipeline, 63 / 64 / 65 around the hand-over to atomic chunks, 255 / 256 / 257 on the chunk boundary of a hub) and on
its transpose, with normal inputs and with small-integer bases whose extrema tie between entries and between chunks.

Each case runs egc_aggregate_combine_train, then egc_aggregate_combine_backward, and holds ``d_bases`` and ``d_weightings``
THEMSELVES -- no GEMM and no parameter gradient behind which a few wrong columns could hide -- to autograd through the operand-level
restatement in float64 on the same float32 inputs.  Distance: max |a - b| / max |b|, per array and once more over the short source
rows alone (at most 64 out-entries), so that a hub's magnitude cannot cover a short row.  Bound: the project's 1e-5; with std / var
twice the float32 restatement's own distance from float64 on that case (kernel and restatement are two float32 evaluations, in
different orders, of the same amplified rounding), at least 1e-5 and never more than the 2e-4 of tests/test_backward_gpu.py.
arg_max / arg_min equal the restatement's first attaining entry exactly.  Measured distance, yardstick and bound are printed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import egc_amd
from backward_ref import (ACTS, BOUNDARY_CASES, CASES, CODES, GRAPH_SEED, INPUT_SEED, RECORD_CASES, RECT_CASES, SETS, THRESHOLD,
                          arg_positions, boundary, extrema, geometry, gradients, ladder, make_inputs, real_columns, rect, rel_grad,
                          rel_out, sparse, stdvar)
from egc_amd import _C
from egc_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOTH = (False, True)
IDS = dict(ids=lambda c: c.name)
NO_REC, SEPARATE, GENERIC = ("EGC_BWD_NO_REC",), ("EGC_BWD_REC_SEPARATE",), ("EGC_BWD_GENERIC", "EGC_FORCE_GENERIC")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def edges(kind, flip, reduced=False, ldb=0):
    """(edge_index, n, n_src) of a graph key: ("ladder",) / ("rect", more) / ("sparse",) / ("boundary", on)."""
    if kind[0] == "ladder":
        return ladder(GRAPH_SEED, flip, reduced)
    if kind[0] == "rect":
        return rect(GRAPH_SEED, kind[1], flip)
    if kind[0] == "sparse":
        return sparse(GRAPH_SEED, flip)
    return boundary(GRAPH_SEED, ldb, kind[1])


def _key(case, kind, flip):
    return kind, flip, kind[0] == "ladder" and case.graph == "reduced", geometry(case)[2] if kind[0] == "boundary" else 0


@functools.lru_cache(maxsize=None)
def _device_graph(kind, flip, reduced, ldb):
    ei, n, n_src = edges(kind, flip, reduced, ldb)
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n, n_src)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n, n_src, ei.shape[1])
    return g


def device_graph(case, kind=("ladder",), flip=False):
    return _device_graph(*_key(case, kind, flip))


def spec_of(case):
    agg_set, sym_set = SETS[case.sets]
    return F.make_spec(16, case.out, case.H, case.B, [CODES[a] for a in case.aggrs], agg_set, sym_set, True, _C.LAYOUT_HBA,
                       ACTS[case.act], basis_stride=geometry(case)[1])


@functools.lru_cache(maxsize=None)
def reference(case, kind, flip, ties):
    """Inputs, the float64 truth, the float32 yardstick and the arg positions of one (case, graph, input set): computed once."""
    ei, n, n_src = edges(*_key(case, kind, flip))
    ins = make_inputs(case, n, n_src, INPUT_SEED, ties)
    f64, f32 = (gradients(*ins, ei, n, case, dt) for dt in (torch.float64, torch.float32))
    args = {w: arg_positions(ins[0], ei, n, case, w) for w in ("max", "min") if w in case.aggrs}
    short = np.bincount(ei[0], minlength=n_src) <= THRESHOLD
    return dict(ei=ei, n=n, n_src=n_src, ins=ins, f64=f64, f32=f32, args=args, short=short)


def on_device(fn):
    """A failing HIP call ends the whole run: nothing more is started on a device that has reported an error."""
    try:
        got = fn()
        torch.cuda.synchronize()
        return got
    except RuntimeError as exc:
        pytest.exit(f"HIP error, the sweep stops here: {exc}", returncode=3)


def run(case, kind=("ladder",), flip=False, ties=False):
    """One train + backward call through the Python entry points: (out, d_bases, d_weightings, arg_max, arg_min, graph)."""
    ref = reference(case, kind, flip, ties)
    g = device_graph(case, kind, flip)
    spec = spec_of(case)
    bases, wt, gout = (_dev(a) for a in ref["ins"])

    def call():
        out, saved = F.egc_aggregate_combine_train(g, spec, bases, wt, None)
        d_b, d_w, _ = F.egc_aggregate_combine_backward(g, spec, bases, wt, gout, saved)
        return out, d_b, d_w, saved[2], saved[3], g
    return on_device(call)


def bound_of(case, yardstick):
    return min(2e-4, max(1e-5, 2 * yardstick)) if stdvar(case) else 1e-5


def check(case, kind=("ladder",), flip=False, ties=False, mode=""):
    ref = reference(case, kind, flip, ties)
    out, d_b, d_w, arg_max, arg_min, g = run(case, kind, flip, ties)
    L, Ls, ldb, _, _, W = geometry(case)
    tag = f"{case.name} {'/'.join(str(k) for k in kind)}{' flip' if flip else ''}{' ties' if ties else ''}{' ' + mode if mode else ''}"
    bad = []
    # ---- the arg rule: CSR position -> input edge; the appended self loop reads as n_edges, an empty row as -1
    e = g.n_edges
    edge_id = g.edge_id.cpu().numpy().astype(np.int64)
    for which, arg in (("max", arg_max), ("min", arg_min)):
        if which not in case.aggrs:
            assert arg is None
            continue
        got = real_columns(arg.cpu().numpy().astype(np.int64), case.B, L, Ls)
        assert got.min() >= -1 and got.max() <= e
        got = np.where((got >= 0) & (got < e), edge_id[np.clip(got, 0, e - 1)], got)
        if not np.array_equal(got, ref["args"][which]):
            bad.append(f"arg_{which}: {int((got != ref['args'][which]).sum())} of {got.size} positions are not the first attaining entry")
    # ---- distances
    o64, b64, w64 = ref["f64"]
    _, b32, w32 = ref["f32"]
    short = ref["short"]
    assert d_b.shape == b64.shape and d_w.shape == w64.shape and bool(torch.isfinite(d_b).all()) and bool(torch.isfinite(d_w).all())
    err = rel_out(out.cpu().numpy(), o64)
    print(f"{tag} out: measured {err:.3e}, bound 1e-5")
    if not err <= 1e-5:
        bad.append(f"out: error {err:.3e} > 1e-5")
    d_b, d_w = d_b.cpu().numpy(), d_w.cpu().numpy()
    for name, got, yard, truth in (("d_bases", d_b, b32, b64), ("d_bases (short source rows)", d_b[short], b32[short], b64[short]),
                                   ("d_weightings", d_w, w32, w64)):
        err, y = rel_grad(got, truth), rel_grad(yard, truth)
        bound = bound_of(case, y)
        print(f"{tag} {name}: measured {err:.3e}, restatement f32-vs-f64 {y:.3e}, bound {bound:.1e}")
        if not err <= bound:
            bad.append(f"{name}: error {err:.3e} > {bound:.1e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("case", CASES, **IDS)
def test_every_cell_against_float64(case, flip):
    check(case, flip=flip)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("case", [c for c in CASES if extrema(c)], **IDS)
def test_ties_between_entries_and_between_chunks(case, flip):
    """Small-integer bases: nearly every extremum is attained by several entries, in several chunks of a hub row, and by the row's
    own features under a LOOPED set -- the first entry takes the whole gradient."""
    ref = reference(case, ("ladder",), flip, True)
    if case.sets == "looped":                                                    # the appended self loop does win columns
        assert all(int((a == ref["ei"].shape[1]).sum()) > 0 for a in ref["args"].values())
    check(case, flip=flip, ties=True)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("mode", (NO_REC, SEPARATE), ids=("no_rec", "separate"))
@pytest.mark.parametrize("case", RECORD_CASES, **IDS)
def test_every_record_mode_against_float64(case, mode, flip, monkeypatch):
    """The extremum gradients as arg bytes (no records) and as records built by bwd_records_kernel: each held to float64 itself,
    on rows of one and two entries (records overflow), 8 / 9 entries (the ballot ranking limit) and hub chunks."""
    monkeypatch.setenv(mode[0], "1")
    check(case, flip=flip, ties=flip, mode=mode[0])


@pytest.mark.parametrize("case", CASES, **IDS)
def test_generic_forms_against_float64(case, monkeypatch):
    """EGC_BWD_GENERIC=1 (bwd_dst_kernel, the run-time source form at every slot count) under EGC_FORCE_GENERIC=1 (the generic
    training forward, whose arg positions come from arg_extrema_kernel<1..4>)."""
    for name in GENERIC:
        monkeypatch.setenv(name, "1")
    check(case, ties=bool(extrema(case)), mode="generic")


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("case", RECORD_CASES, **IDS)
def test_low_degree_graph_without_records(case, flip):
    """Many rows of at most 17 entries, more than ten basis columns per entry: no records, the compiled arg-byte source forms."""
    check(case, kind=("sparse",), flip=flip, ties=flip)


@pytest.mark.parametrize("on", (True, False), ids=("last_with_records", "first_without"))
@pytest.mark.parametrize("case", BOUNDARY_CASES, **IDS)
def test_either_side_of_the_record_rule(case, on):
    """ldb N = 10 E exactly (records) and one entry fewer (none): the workspace query and the backward take the same side."""
    ref = reference(case, ("boundary", on), False, True)
    g = device_graph(case, ("boundary", on))
    spec, gs = spec_of(case), g.c_struct()
    lib = _C.load()
    extra = lib.egc_backward_workspace_bytes_for(C.byref(spec.c), C.byref(gs)) - lib.egc_backward_workspace_bytes(C.byref(spec.c), ref["n"])
    assert extra == (extrema(case) * g.n_edges * 64 if on else 0)
    check(case, kind=("boundary", on), ties=True)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("more", (True, False), ids=("more_sources", "fewer_sources"))
@pytest.mark.parametrize("case", RECT_CASES, **IDS)
def test_rectangular_graphs_against_float64(case, more, flip):
    """n_src != n (raw sets): d_bases has the sources' rows, is zero-filled by the caller and added to."""
    check(case, kind=("rect", more), flip=flip, ties=bool(extrema(case)) and more)


def _direct(case, g, ins, saved, fill, zero_db):
    """egc_aggregate_combine_backward_f32 itself with the outputs and the whole workspace holding ``fill`` on entry."""
    lib = _C.load()
    spec = spec_of(case)
    _, _, ldb, _, _, W = geometry(case)
    bases, wt, gout = ins
    stats, cnt, arg_max, arg_min = saved
    tg = g.transposed()
    cg, ct = g.c_struct(), tg.c_struct()
    nbytes = lib.egc_backward_workspace_bytes_for(C.byref(spec.c), C.byref(cg))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV).fill_(fill)
    d_b = torch.full((g.n_src_rows, ldb), 0.0 if zero_db else fill, device=DEV)
    d_w = torch.full((g.n_nodes, W), fill, device=DEV)
    on_device(lambda: _C.check(lib.egc_aggregate_combine_backward_f32(
        C.byref(cg), C.byref(ct), C.byref(spec.c), bases.data_ptr(), ldb, wt.data_ptr(), gout.data_ptr(), stats.data_ptr(),
        cnt.data_ptr(), arg_max.data_ptr() if arg_max is not None else None, arg_min.data_ptr() if arg_min is not None else None,
        d_b.data_ptr(), ldb, d_w.data_ptr(), W, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream),
        "egc_aggregate_combine_backward_f32"))
    return d_b, d_w


@pytest.mark.parametrize("case", CASES, **IDS)
def test_nothing_is_read_before_it_is_written(case):
    """d_bases, d_weightings and the whole workspace full of NaN on entry (square graph: the C ABI promises that every row of
    d_bases is written): both come back finite everywhere, the padding columns of a padded basis included -- they are an operand of
    the gradient GEMMs -- and equal to the run on zeros: bit for bit on short source rows and in d_weightings (no atomics there),
    within 1e-6 on hub rows (float atomics in arrival order)."""
    ties = bool(extrema(case))
    ref = reference(case, ("ladder",), False, ties)
    g = device_graph(case)
    ins = tuple(_dev(a) for a in ref["ins"])
    _, saved = on_device(lambda: F.egc_aggregate_combine_train(g, spec_of(case), ins[0], ins[1], None))
    zb, zw = _direct(case, g, ins, saved, 0.0, False)
    nb, nw = _direct(case, g, ins, saved, float("nan"), False)
    assert bool(torch.isfinite(nb).all()) and bool(torch.isfinite(nw).all())
    short = torch.from_numpy(ref["short"]).to(DEV)
    assert torch.equal(nb[short], zb[short]) and torch.equal(nw, zw)
    assert rel_out(nb.cpu().numpy(), zb.cpu().numpy()) <= 1e-6
    assert rel_grad(nb.cpu().numpy(), ref["f64"][1]) <= bound_of(case, rel_grad(ref["f32"][1], ref["f64"][1]))


@pytest.mark.parametrize("case", RECT_CASES[:2], **IDS)
def test_rectangular_d_bases_is_added_to_a_zero_filled_array(case):
    """Rectangular graph: d_bases zero-filled as the API requires, d_weightings and the workspace full of NaN."""
    ref = reference(case, ("rect", True), False, False)
    g = device_graph(case, ("rect", True))
    ins = tuple(_dev(a) for a in ref["ins"])
    _, saved = on_device(lambda: F.egc_aggregate_combine_train(g, spec_of(case), ins[0], ins[1], None))
    nb, nw = _direct(case, g, ins, saved, float("nan"), True)
    assert bool(torch.isfinite(nb).all()) and bool(torch.isfinite(nw).all())
    assert rel_grad(nb.cpu().numpy(), ref["f64"][1]) <= 1e-5 and rel_grad(nw.cpu().numpy(), ref["f64"][2]) <= 1e-5
