"""The three packed weight operands of the one-launch batch kernel (egc_batch_fused_pack: narrow and wide; egc_batch_fused_bwd_pack /
egc_batch_fused_train_pack: transposed), byte for byte against a numpy restatement of the kernels that wrote them BEFORE the
layouts moved into egc_fused_tile_host.h -- the restatement, not the code under test, says what "the same bytes" are (this file
passes unchanged against the library of that commit).

Restated: the column scale from the biased exponent of the column's largest magnitude (clamped at 253; scale 2^(127 - be), inverse
2^(be - 127), the inverse of an all-zero or all-denormal column 0), h = fp16(s), l = fp16((s - h) 2048) (both round to nearest
even, as numpy's float32 -> float16 does), the fragment order [tile][k-step][plane][lane][8] and the tail of floats.

The buffer is prefilled with 0xA5.  Every byte inside pack_bytes is overwritten but for the ones no column owns: the wide
operand's tail holds col_inv[384] and col_bias[384] and the pack writes the n_ct * 32 columns in use -- floats [32 n_ct, 384) of
either array keep the prefill (the kernel reads none of them), before and after.  Narrow and transposed: every byte written.
Nothing is written behind pack_bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from egc_amd import _C
from egc_amd.functional import _stream_ptr, padded_basis_stride

S, M, X, Y = _C.AGGR_SUM, _C.AGGR_MEAN, _C.AGGR_MAX, _C.AGGR_SYMNORM
FILL, GUARD = 0xA5, 256
FT_NV, FT_KP, FTW_MAX_COLS, FTB_K2 = 192, 128, 384, 192

NARROW = ((128, 8, 4, (S, M, X, Y), 4), (128, 8, 4, (S, M, X, Y), 100), (128, 8, 4, (S, M, X, Y), 128), (64, 4, 4, (S, M, X, Y), 64))
WIDE = ((168, 8, 4, (Y,), 132),         # ldb 96
        (136, 4, 4, (Y, X, M), 136),    # ldb 144 -> ldbp 160: the padding columns
        (296, 8, 4, (Y,), 320))         # k16 = 20, three slabs
BACKWARD = ((128, 8, 4, (S, M, X, Y), 100), (64, 4, 4, (S, M, X, Y), 64))


def make(f_out, heads, bases, aggrs, f_in):
    stride = padded_basis_stride(f_out, heads, bases)
    Ls = stride
    lay = _C.make_layer(in_channels=f_in, out_channels=f_out, num_heads=heads, num_bases=bases, aggr_codes=list(aggrs),
                        agg_set=_C.SET_LOOPED, sym_set=_C.SET_LOOPED, loops_all_nodes=1, weight_layout=_C.LAYOUT_HBA,
                        weight_act=_C.ACT_NONE, basis_stride=0 if stride == f_out // heads else stride)
    dims = dict(K=f_in, F_g=bases * Ls, ldb=(bases * Ls + 3) & ~3, W=heads * bases * len(aggrs), A=len(aggrs), H=heads, B=bases)
    return lay, dims


def weights(d, seed):
    """wcat [K][F_g + W], bcat [W]: normal entries over 40 binades, and in the bases and in the weightings an all-zero column, a column
    whose largest entry is 2^127, a column holding a denormal among normal entries and a column of denormals only."""
    rng = np.random.default_rng(seed)
    n = d["F_g"] + d["W"]
    w = (rng.standard_normal((d["K"], n)) * np.exp2(rng.integers(-20, 20, (1, n)))).astype(np.float32)
    for c0 in (0, d["F_g"]):
        w[:, c0 + 1] = 0.0
        w[rng.integers(d["K"]), c0 + 2] = np.float32(2.0 ** 127)
        w[rng.integers(d["K"]), c0 + 3] = np.float32(1e-40)
        w[:, c0 + 5] = ((np.arange(d["K"]) % 7 - 3) * 1e-41).astype(np.float32)
    assert (w[:, 5] != 0).any() and (np.abs(w[:, 5]) < np.finfo(np.float32).tiny).all()
    return w, rng.standard_normal(d["W"]).astype(np.float32)


def split(cols):
    """cols [n][k] float32, one operand column per row -> (h bits [n][k], l bits, inverse scale [n])."""
    bits = np.ascontiguousarray(cols).view(np.uint32) & np.uint32(0x7FFFFFFF)
    be = np.minimum(bits.max(axis=1, initial=0) >> 23, 253).astype(np.uint32)
    scale, inv = ((254 - be) << 23).astype(np.uint32).view(np.float32), (be << 23).astype(np.uint32).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = cols * scale[:, None]
        h = s.astype(np.float16)
        l = ((s - h.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return h.view(np.uint16), l.view(np.uint16), inv


def fragments(h, l, tw, ksteps):
    """[columns][k rows] bits of both planes -> the halves [tile][k-step][plane][lane][8]."""
    n, kr = h.shape
    kw = 512 // tw
    assert n % tw == 0 and kr == ksteps * kw
    v, k = np.meshgrid(np.arange(n), np.arange(kr), indexing="ij")
    base = ((((v // tw) * ksteps + k // kw) * 2) * 64 + tw * ((k % kw) >> 3) + v % tw) * 8 + (k & 7)
    out = np.full((n // tw) * ksteps * 2 * 512, 1 << 16, dtype=np.uint32)
    out[base] = h
    out[base + 512] = l
    assert (out < (1 << 16)).all()                       # every half of the operand is some (column, k, plane)
    return out.astype(np.uint16)


def forward_operand(d, w, bcat, wide):
    """(expected bytes, written mask) of the narrow / wide forward operand."""
    wcol0 = (d["ldb"] + 31) & ~31 if wide else d["ldb"]
    n_cols = (wcol0 + d["W"] + 31) // 32 * 32 if wide else FT_NV
    k_rows = ((((d["K"] + 15) // 16) + 3) & ~3) * 16 if wide else FT_KP
    cols = np.zeros((n_cols, k_rows), dtype=np.float32)
    cols[:d["F_g"], :d["K"]] = w[:, :d["F_g"]].T
    cols[wcol0:wcol0 + d["W"], :d["K"]] = w[:, d["F_g"]:].T
    h, l, inv = split(cols)
    tw = 32 if wide else 16
    halves = fragments(h, l, tw, k_rows // (512 // tw))
    stride = FTW_MAX_COLS if wide else FT_NV
    tail = np.zeros(2 * stride, dtype=np.float32)
    written = np.zeros(2 * stride, dtype=bool)
    tail[:n_cols] = inv
    if bcat is not None:
        tail[stride + wcol0:stride + wcol0 + d["W"]] = bcat
    written[:n_cols] = written[stride:stride + n_cols] = True
    return np.concatenate([halves.view(np.uint8), tail.view(np.uint8)]), np.concatenate([np.ones(halves.size * 2, bool), np.repeat(written, 4)])


def transposed_operand(d, w):
    k2 = d["ldb"] + d["H"] * d["B"] * 4
    cols = np.zeros((FT_KP, FTB_K2), dtype=np.float32)          # [output feature f][image column k]
    for k in range(k2):
        if k < d["ldb"]:
            c = k if k < d["F_g"] else -1
        else:
            hb, aa = (k - d["ldb"]) >> 2, (k - d["ldb"]) & 3
            c = d["F_g"] + hb * d["A"] + aa if aa < d["A"] and hb * d["A"] + aa < d["W"] else -1
        if c >= 0:
            cols[:d["K"], k] = w[:, c]
    h, l, inv = split(cols)
    out = np.concatenate([fragments(h, l, 16, FTB_K2 // 32).view(np.uint8), inv.view(np.uint8)])
    return out, np.ones(out.size, bool)


def device_buffer(nbytes, dev):
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)


def check(buf, nbytes, want, written, what):
    got = buf.cpu().numpy()
    assert want.size == nbytes == written.size, (what, want.size, nbytes)
    assert (got[nbytes:] == FILL).all(), what + ": bytes written behind pack_bytes"
    body = got[:nbytes]
    bad = np.flatnonzero(written & (body != want))
    assert bad.size == 0, (what, "first differing byte", int(bad[0]), "of", bad.size)
    assert (body[~written] == FILL).all(), what + ": a byte no column owns was written"
    # (a written byte may equal the prefill by value; as 16-bit halves 0xA5A5 = -0.0221 is not what any case packs in bulk)
    assert (body[written].view(np.uint16) == 0xA5A5).mean() < 0.01, what


@pytest.fixture(scope="module")
def lib():
    return _C.load()


def test_numpy_split_is_the_restated_one():
    """The special columns: zero -> inverse 0 and zero planes; 2^127 -> be 254 clamped to 253, s = 2 exactly; denormals scale by 2^127."""
    cols = np.zeros((4, 8), dtype=np.float32)
    cols[1, 3] = 2.0 ** 127
    cols[2, :2] = (1.0, 1e-40)
    cols[3, 0] = 3e-41
    h, l, inv = split(cols)
    assert inv.tolist() == [0.0, 2.0 ** 126, 1.0, 0.0] and not h[0].any() and not l[0].any()
    assert h[1, 3] == np.float16(2.0).view(np.uint16) and l[1, 3] == 0
    assert h[2, 0] == np.float16(1.0).view(np.uint16) and h[2, 1] == 0                      # 1e-40 against a column of magnitude 1: below fp16
    assert np.float16(np.float32(3e-41) * np.float32(2.0 ** 127)).view(np.uint16) == h[3, 0] != 0
    x = np.array([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -13]], dtype=np.float32)   # two ties (to even: down, up) and past one
    hh, ll, _ = split(x)
    assert hh.view(np.float16).tolist() == [[1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10]] and ll.view(np.float16).tolist() == [[1.0, -1.0, -0.75]]


@pytest.mark.gpu
@pytest.mark.parametrize("with_bcat", (False, True))
@pytest.mark.parametrize("case", NARROW + WIDE, ids=lambda c: "%d-H%d-B%d-A%d-fin%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_forward_operand(lib, case, with_bcat):
    dev = torch.device("cuda")
    lay, d = make(*case)
    w, b = weights(d, 11)
    want, written = forward_operand(d, w, b if with_bcat else None, case in WIDE)
    nbytes = int(lib.egc_batch_fused_pack_bytes(C.byref(lay)))
    buf = device_buffer(nbytes, dev)
    wt, bt = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    _C.check(lib.egc_batch_fused_pack(C.byref(lay), wt.data_ptr(), bt.data_ptr() if with_bcat else None, buf.data_ptr(), nbytes,
                                      _stream_ptr(dev)), "egc_batch_fused_pack")
    torch.cuda.synchronize()
    assert (case in WIDE) == (not written.all())
    check(buf, nbytes, want, written, "forward operand")


@pytest.mark.gpu
@pytest.mark.parametrize("with_bcat", (False, True))
@pytest.mark.parametrize("case", BACKWARD, ids=lambda c: "%d-H%d-fin%d" % (c[0], c[1], c[4]))
def test_transposed_operand(lib, case, with_bcat):
    dev = torch.device("cuda")
    lay, d = make(*case)
    w, b = weights(d, 12)
    want_t, all_t = transposed_operand(d, w)
    want_f, all_f = forward_operand(d, w, b if with_bcat else None, False)
    nb, nbt = int(lib.egc_batch_fused_pack_bytes(C.byref(lay))), int(lib.egc_batch_fused_bwd_pack_bytes(C.byref(lay)))
    wt, bt = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)
    alone = device_buffer(nbt, dev)
    _C.check(lib.egc_batch_fused_bwd_pack(C.byref(lay), wt.data_ptr(), alone.data_ptr(), nbt, _stream_ptr(dev)), "egc_batch_fused_bwd_pack")
    fwd, both = device_buffer(nb, dev), device_buffer(nbt, dev)
    _C.check(lib.egc_batch_fused_train_pack(C.byref(lay), wt.data_ptr(), bt.data_ptr() if with_bcat else None, fwd.data_ptr(), nb,
                                            both.data_ptr(), nbt, _stream_ptr(dev)), "egc_batch_fused_train_pack")
    torch.cuda.synchronize()
    check(alone, nbt, want_t, all_t, "transposed operand")
    check(both, nbt, want_t, all_t, "transposed operand of the training pack")
    check(fwd, nb, want_f, all_f, "forward operand of the training pack")
