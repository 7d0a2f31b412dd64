"""Every host branch of the packed basis transform -- each plane layout, each kernel instance family and launch form that
egc_gemm_host.h describes, the folded form, EGC_GEMM_24BIT, the addend and transposed-pack entry points, the row-range walk --
at rows 1, 17, 65 and 200, held to the BITS the library produced at the commit before the plan existed: the SHA-256 of `bases`
and `weightings` against tests/golden/gemm_forms.json (recorded on the MI355X by tests/golden/make_gemm_forms.py, which runs
everything twice and requires every digest to repeat: these kernels have no atomics).  Operands come from numpy's default_rng,
so they do not depend on the device.  tests/test_gemm_plan_cpu.py shows, without a GPU, which branch each shape takes."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from egc_amd import _C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_forms.json")
ROWS = (1, 17, 65, 200)
GEMM_24BIT = _C.GEMM_24BIT

# (f_in, f_g, w_cols, flags): what the plan program prints for each is behind it
SHAPES = [
    (128, 64, 128, 0),    # fp16x2, the north star
    (100, 64, 126, 0),    # fp16x2, F_in < 128, ragged weightings
    (128, 168, 0, 0),     # fp16x2 without weightings, ldb % 32 != 0
    (224, 224, 48, 0),    # long k, 17 tiles: two tiles per wavefront
    (200, 150, 30, 0),    # long k, 12 tiles: two tiles per wavefront, padded bases
    (192, 128, 0, 0),     # long k, 8 tiles: all-in-one, two workgroups per CU
    (168, 84, 32, 0),     # long k, 8 tiles: all-in-one, two per CU, padded bases
    (352, 176, 32, 0),    # long k, 13 tiles: separated roles, 16 wavefronts
    (384, 64, 128, 0),    # long k, 12 tiles, the longest k: separated roles
    (320, 64, 64, 0),     # long k, 8 tiles at KS = 10: separated roles, 12 wavefronts
    (256, 192, 64, 0),    # long k, 16 tiles: all-in-one with 16 wavefronts, no helpers
    (192, 320, 16, 0),    # long k, 21 tiles: two launches (roles, then all-in-one two per CU)
    (300, 300, 48, 0),    # long k, 22 tiles: two launches of separated roles
    (384, 16, 0, 0),      # long k refused (one column tile cannot stage its x tile): bf16x3, staged, run-time tile count
    (384, 208, 0, 0),     # long k refused (13 tiles at KS = 12): bf16x3, 6-tile block + 32-column remainder
    (7, 5, 3, 0),         # weight-stationary, 2 sub-steps, scalar x loads
    (32, 64, 64, 0),      # weight-stationary, 2 sub-steps
    (64, 64, 64, 0),      # weight-stationary, 4 sub-steps
    (96, 64, 96, 0),      # weight-stationary, 6 sub-steps
    (124, 124, 48, 0),    # weight-stationary, 8 sub-steps
    (128, 20, 7, 0),      # weight-stationary refused (one wavefront cannot stage the tile): staged, run-time tile count
    (388, 192, 32, 0),    # staged, one 7-tile block
    (388, 64, 64, 0),     # staged, 128 columns
    (388, 300, 48, 0),    # staged, 6-tile block + remainder of 160 columns
    (389, 192, 32, 0),    # staged, not vec4: 6-tile block + 32-column remainder
    (128, 64, 128, GEMM_24BIT),   # the fp16x2 shape on three bf16 planes: weight-stationary, 8 sub-steps
    (352, 176, 32, GEMM_24BIT),   # the long-k shape on three bf16 planes: staged, one 7-tile block
]
FOLDED = (["mean", "sum", "max", "symnorm"], ["sum", "mean", "max", "symnorm"], ["sum", "max", "mean", "symnorm"],
          ["sum", "max", "symnorm", "mean"])       # the mean at each place of the quad
MAX_ROWS = ((128, 64, 128, "192"), (128, 64, 128, "96"), (352, 176, 32, "192"), (352, 176, 32, "96"))   # EGC_GEMM_MAX_ROWS, rows = 200


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def _operands(n, f_in, cols, w_cols, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n, f_in), dtype=np.float32)).to(DEV)
    wcat = torch.from_numpy(rng.standard_normal((f_in, cols), dtype=np.float32) * np.float32(0.2)).to(DEV)
    bcat = torch.from_numpy(rng.standard_normal(max(w_cols, 1), dtype=np.float32)).to(DEV)
    return x, wcat, bcat


def _gemm(n, f_in, f_g, w_cols, flags, addend=False, transposed=False):
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    x, wcat, bcat = _operands(n, f_in, f_g + w_cols, w_cols, seed=1000 * n + f_in + 7 * f_g + w_cols)
    ldb = (f_g + 3) & ~3
    nb = lib.egc_basis_pack_bytes(f_in, f_g, w_cols)
    planes = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    if transposed:
        wt_src = wcat.t().contiguous()               # [f_g + w_cols][f_in]
        _C.check(lib.egc_basis_pack_transposed(wt_src.data_ptr(), f_in, f_in, f_g, w_cols, planes.data_ptr(), nb, st), "pack_transposed")
    else:
        _C.check(lib.egc_basis_pack_ex(wcat.data_ptr(), f_in, f_g, w_cols, flags, planes.data_ptr(), nb, st), "pack")
    bases = torch.full((n, ldb), float("nan"), device=DEV)
    wt = torch.full((n, w_cols), float("nan"), device=DEV)
    if addend:
        add = torch.from_numpy(np.random.default_rng(n).standard_normal((n, ldb), dtype=np.float32)).to(DEV)
        _C.check(lib.egc_basis_transform_packed_add(x.data_ptr(), planes.data_ptr(), bcat.data_ptr(), n, f_in, f_g, w_cols, flags,
                                                    add.data_ptr(), bases.data_ptr(), ldb, wt.data_ptr(), st), "packed_add")
    else:
        _C.check(lib.egc_basis_transform_packed_ex(x.data_ptr(), planes.data_ptr(), bcat.data_ptr(), n, f_in, f_g, w_cols, flags,
                                                   bases.data_ptr(), ldb, wt.data_ptr(), st), "packed_ex")
    torch.cuda.synchronize()
    return _sha(bases, wt)


def _folded(aggrs, n=65):
    """egc_layer_forward_packed at d = 128 / H8 / B4 on an n-node graph: the bases and the [n, H B 3] weightings of its GEMM."""
    import egc_amd
    from egc_amd import _C
    from egc_amd.functional import pack_weights
    lib = _C.load()
    conv = egc_amd.EGConv(128, 128, aggrs=aggrs, num_heads=8, num_bases=4).to(DEV).eval()
    spec = conv._spec_coo
    rng = np.random.default_rng(65)
    ei = torch.from_numpy(rng.integers(0, n, (2, 6 * n))).to(DEV)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    x, wcat, bcat = _operands(n, 128, spec.f_g + spec.w_cols, spec.w_cols, seed=165)
    with torch.no_grad():
        assert tuple(conv._packed_weights()[0].shape) == tuple(wcat.shape)
        planes = pack_weights(spec, wcat)
    g = graph.c_struct()
    ws = torch.zeros(max(lib.egc_aggregate_workspace_bytes(C.byref(spec.c), n, ei.size(1)), 1), dtype=torch.uint8, device=DEV)
    bias = torch.zeros(128, device=DEV)
    bases = torch.full((n, spec.ldb), float("nan"), device=DEV)
    wt = torch.full((n, spec.w_cols), float("nan"), device=DEV)
    out = torch.empty((n, 128), device=DEV)
    _C.check(lib.egc_layer_forward_packed(C.byref(g), C.byref(spec.c), x.data_ptr(), planes.data_ptr(), bcat.data_ptr(),
                                          bias.data_ptr(), bases.data_ptr(), spec.ldb, wt.data_ptr(), out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "egc_layer_forward_packed")
    torch.cuda.synchronize()
    flat = wt.reshape(-1)
    assert bool(torch.isnan(flat[n * 96:]).all()) and not bool(torch.isnan(flat[: n * 96]).any()), "the folded form was taken"
    return _sha(bases, wt)


def case_ids():
    ids = ["%d,%d,%d,%d" % s for s in SHAPES]
    ids += ["folded," + "-".join(a) for a in FOLDED]
    ids += ["add,208,352,0", "transposed,352,176,32", "transposed,128,64,128"]
    ids += ["max_rows=%s,%d,%d,%d" % (m, a, b, c) for a, b, c, m in MAX_ROWS]
    return ids


def digest(case):
    """case id -> {rows or name: sha256}; run with EGC_GEMM_MAX_ROWS unset but for the max_rows cases, which set it themselves"""
    w = case.split(",")
    if w[0] == "folded":
        return {"65": _folded(w[1].split("-"))}
    if w[0] == "add":                  # the d x GEMM of the 352-wide layer with its residual gradient: long k, 22 tiles, two launches
        return {str(n): _gemm(n, int(w[1]), int(w[2]), int(w[3]), 0, addend=True) for n in ROWS}
    if w[0] == "transposed":
        return {str(n): _gemm(n, int(w[1]), int(w[2]), int(w[3]), 0, transposed=True) for n in ROWS}
    if w[0].startswith("max_rows="):
        old = os.environ.get("EGC_GEMM_MAX_ROWS")
        os.environ["EGC_GEMM_MAX_ROWS"] = w[0].split("=")[1]
        try:
            return {"200": _gemm(200, int(w[1]), int(w[2]), int(w[3]), 0)}
        finally:
            os.environ.pop("EGC_GEMM_MAX_ROWS") if old is None else os.environ.__setitem__("EGC_GEMM_MAX_ROWS", old)
    return {str(n): _gemm(n, *(int(v) for v in w)) for n in ROWS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", case_ids())
def test_bits_are_those_of_the_commit_before_the_plan(golden, case):
    assert digest(case) == golden[case]


def test_row_ranges_give_the_bits_of_one_launch(golden):
    """the row-range walk cuts at whole row tiles: the same bits as the single launch of the same 200 rows"""
    for f_in, f_g, w, m in MAX_ROWS:
        assert golden["max_rows=%s,%d,%d,%d" % (m, f_in, f_g, w)]["200"] == golden["%d,%d,%d,0" % (f_in, f_g, w)]["200"]


def test_transposed_pack_gives_the_planes_of_the_plain_pack(golden):
    for s in ("352,176,32", "128,64,128"):
        assert golden["transposed," + s] == golden[s + ",0"]
