"""Every host branch of the weight-gradient GEMM (egc_gemm_xt.hip) -- the one-tile split-bf16 kernel with and without the third
stream, the exact-fp32 tile grid unforced and with every compiled tile forced, EGC_GEMM_EXACT, wide row strides, the scatter into
the parameters' gradients -- at rows 1, 17, 65, 200 and 8300, held to the BITS the library produced at the commit before its plan
and envelope got one owner: the SHA-256 of everything the entry points wrote against tests/golden/weight_grad_forms.json
(recorded on the MI355X by tests/golden/make_weight_grad_forms.py, which runs everything twice and requires every digest to
repeat: the reduction adds the row ranges in a fixed order).  Operands come from numpy's default_rng, so they do not depend on
the device.  Rows 1 .. 200 walk the 16-row sub-tiles and the 32-row stage edges; at 8300 the one-tile plan has 130 ranges of 64
rows, so a range takes two stages and the reduction crosses more than eight ranges.  tests/test_weight_grad_plan_cpu.py shows,
without a GPU, which plan each shape takes."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from egc_amd import _C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_grad_forms.json")
ROWS = (1, 17, 65, 200, 8300)
TM, TN, ES = _C.WEIGHT_GRAD_TILE_ROWS, _C.WEIGHT_GRAD_TILE_COLS, _C.WEIGHT_GRAD_MAX_SUM_COLS

ONE_TILE = ((TM, TN), (100, 64), (4, 4))                    # x (0, 4, ES) columns of the third array
GRID = ((132, 196), (136, 184), (224, 272), (296, 180), (352, 208))
XT_TILES = ((1, 1, 4), (1, 2, 4), (1, 3, 4), (2, 1, 4), (2, 2, 4), (2, 3, 4), (4, 1, 4), (4, 2, 4), (4, 3, 4), (5, 2, 4), (5, 3, 4),
            (7, 2, 4), (7, 3, 3), (7, 3, 4), (7, 5, 4), (7, 3, 6))
FORCED = ((224, 272), (296, 180), (132, 196))               # the shapes of test_weight_grad_every_compiled_tile
STRIDED = ((TM, TN), (132, 196))                            # x sums 0 / 1; row strides f + 32 and k + 64
# (f_in, H, A, B, L, Ls, permute, n_parts) of egc_weight_grad_params_f32, the third array f_out = H L columns (rounded up to 4) wide
PARAMS = ((128, 8, 4, 4, 16, 16, 1, 1), (128, 8, 4, 4, 16, 16, 0, 4), (48, 4, 3, 4, 8, 8, 0, 4), (48, 4, 3, 4, 8, 8, 1, 1),
          (64, 2, 1, 2, 21, 24, 0, 2))


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=4)
def _operands(n, f, k, e, pad_x=0, pad_d=0):
    """x [n, f], d [n, k] (columns of very different size), e [n, e]; x and d as column blocks of wider arrays with pad_*"""
    rng = np.random.default_rng(100003 * n + 1009 * f + 7 * k + e)
    x = torch.from_numpy(rng.standard_normal((n, f + pad_x), dtype=np.float32)).to(DEV)
    d = torch.from_numpy(rng.standard_normal((n, k + pad_d), dtype=np.float32) * np.logspace(-4, 2, k + pad_d, dtype=np.float32)).to(DEV)
    ex = torch.from_numpy(rng.standard_normal((n, max(e, 4)), dtype=np.float32) * np.float32(3) + np.float32(0.5)).to(DEV)
    return x[:, pad_x // 2: pad_x // 2 + f], d[:, pad_d: pad_d + k], ex


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _workspace(n, f, k, e):
    nb = int(_C.load().egc_weight_grad_ex_workspace_bytes(n, f, k, e))
    return _nan(max(nb, 16) // 4)                           # contents irrelevant on entry


def _ex(n, f, k, e, sums=True, pad_x=0, pad_d=0):
    """egc_weight_grad_ex_f32 (e > 0) or egc_weight_grad_f32 -> the digest of out, col_sums, e_sums"""
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    x, d, ex = _operands(n, f, k, e, pad_x, pad_d)
    out, cs, es, ws = _nan(f, k), _nan(k) if sums else None, _nan(e) if e else None, _workspace(n, f, k, e)
    csp = cs.data_ptr() if sums else None
    if e:
        _C.check(lib.egc_weight_grad_ex_f32(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), n, f, k, out.data_ptr(), csp,
                                            ex.data_ptr(), ex.stride(0), e, es.data_ptr(), ws.data_ptr(), ws.numel() * 4, st), "ex")
    else:
        _C.check(lib.egc_weight_grad_f32(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), n, f, k, out.data_ptr(), csp,
                                         ws.data_ptr(), ws.numel() * 4, st), "plain")
    torch.cuda.synchronize()
    return _sha(*(t for t in (out, cs, es) if t is not None))


def _params(n, f_in, H, A, B, L, Ls, permute, n_parts):
    """egc_weight_grad_params_f32 with e riding -> the digest of the basis parts, d comb weight, d comb bias, e_sums"""
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    W, k, e = H * B * A, B * Ls + H * B * A, (H * L + 3) // 4 * 4
    x, d, ex = _operands(n, f_in, k, e)
    parts = [_nan(f_in, B * L if n_parts == 1 else L) for _ in range(n_parts)]
    cw, cb, es, ws = _nan(W, f_in), _nan(W), _nan(e), _workspace(n, f_in, k, e)
    ptrs = (C.c_void_p * n_parts)(*[p.data_ptr() for p in parts])
    _C.check(lib.egc_weight_grad_params_f32(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), n, f_in, H, A, B, L, Ls, permute, ptrs,
                                            n_parts, cw.data_ptr(), cb.data_ptr(), None, ex.data_ptr(), ex.stride(0), e, es.data_ptr(),
                                            ws.data_ptr(), ws.numel() * 4, st), "params")
    torch.cuda.synchronize()
    return _sha(*parts, cw, cb, es)


def case_ids():
    ids = ["one_tile,%d,%d,%d" % (f, k, e) for f, k in ONE_TILE for e in (0, 4, ES)]
    ids += ["grid,%d,%d" % s for s in GRID]
    ids += ["exact,%d,%d" % (TM, TN)]
    ids += ["tile=%d-%d-%d,%d,%d" % (*t, f, k) for t in XT_TILES for f, k in FORCED]
    ids += ["strided,%d,%d,%d" % (f, k, sums) for f, k in STRIDED for sums in (0, 1)]
    ids += ["params,%d,%d,%d,%d,%d,%d,%d,%d" % p for p in PARAMS]
    return ids


def digest(case, monkeypatch):
    """case id -> {rows: sha256}; EGC_GEMM_EXACT and EGC_XT_TILE unset but where the case sets one"""
    w = case.split(",")
    v = [int(a) for a in w[1:]]
    monkeypatch.delenv("EGC_XT_TILE", raising=False)
    monkeypatch.delenv("EGC_GEMM_EXACT", raising=False)
    if w[0] == "exact":
        monkeypatch.setenv("EGC_GEMM_EXACT", "1")
    if w[0].startswith("tile="):
        monkeypatch.setenv("EGC_XT_TILE", w[0][5:].replace("-", ","))
    if w[0] == "one_tile":
        return {str(n): _ex(n, *v) for n in ROWS}
    if w[0] == "strided":
        return {str(n): _ex(n, v[0], v[1], 0, sums=bool(v[2]), pad_x=32, pad_d=64) for n in ROWS}
    if w[0] == "params":
        return {str(n): _params(n, *v) for n in ROWS}
    return {str(n): _ex(n, v[0], v[1], 0) for n in ROWS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", case_ids())
def test_bits_are_those_of_the_commit_before_the_plan_had_one_owner(golden, case, monkeypatch):
    assert digest(case, monkeypatch) == golden[case]


def test_the_unforced_call_gives_the_bits_of_one_forced_tile(golden):
    """the plan chooses among the compiled tiles: forcing the one it chose changes nothing"""
    for f, k in set(FORCED) & set(GRID):
        forced = [golden["tile=%d-%d-%d,%d,%d" % (*t, f, k)] for t in XT_TILES]
        for n in ROWS:
            assert golden["grid,%d,%d" % (f, k)][str(n)] in {d[str(n)] for d in forced}
