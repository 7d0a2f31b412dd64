"""The host arithmetic of the one-launch batch kernel as it stood BEFORE egc_amd/csrc/egc_fused_tile_host.h: a transcription of
egc_fused_tile.hip's ft_narrow_shape, ft_wide_shape, fused_tile_bwd_shape, ft_lds, ftw_k16, ftw_n_ct, ftw_aw, the three capacity
loops, the range checks of launch_fused_tile / launch_fused_tile_bwd, the *_pack_bytes functions, p0 / magic0 / magic1 and the
grid clamp of ft_tile_args, written from that source before it was touched.  It keeps that source's split: ``capacity`` never
looks at the launch's ``emax`` bound, ``launch_status`` restates the ``tcap`` range -- tests/test_fused_tile_plan_cpu.py holds the
planner to both and states the one place they may differ.  Also the entry points' gate in front of either (tile_layer_args:
fast_path_supported / wide_path_supported of egc_aggregate_fast.hip, without their per-launch terms)."""
from collections import namedtuple

from egc_amd import _C

OK, INVALID, UNSUPPORTED = _C.OK, _C.ERR_INVALID, _C.ERR_UNSUPPORTED
SUM, MEAN, MAX, MIN, VAR, STD, SYMNORM = range(7)  # EGC_AGGR_*
ACT_NONE, ACT_SOFTMAX = 0, 1
LAYOUT_HBA = 0
AMAX, HPB_MAX = 4, 4

FT_MFMA_WAVES, FT_KP, FT_CHUNK, FT_RING, FT_PBUF = 12, 128, 16, 10, 3
FT_NV = FT_MFMA_WAVES * 16
FT_PLANE_BYTES = FT_CHUNK * FT_KP * 2
FT_PLANES_BYTES = FT_PBUF * 2 * FT_PLANE_BYTES
FTB_ROW_BYTES = 192 * 2 + 16
FTB_PLANES_BYTES = 2 * 2 * FT_CHUNK * FTB_ROW_BYTES
FTW_CH, FTW_PP, FTW_SLAB = 32, 10, 128
FTW_MAX_FIN = 8 * FTW_PP * 4
FTW_LDX = FTW_SLAB + 8
FTW_PLANES_BYTES = 2 * 2 * FTW_CH * FTW_LDX * 2
FTW_MAXCH = FT_CHUNK * FT_RING // FTW_CH
FTW_MAX_CT = FT_MFMA_WAVES
FT_LDS_BUDGET = 160 * 1024 - 256

# the layer fields the host side reads (AggArgs' share after agg_layer_fields, and the layer's in_channels)
Layer = namedtuple("Layer", "H B A L Ls ldb slots W act aggr f_in")


def layer_fields(out_channels, heads, bases, aggrs, basis_stride, act, f_in):
    """agg_layer_fields: basis_stride 0 (or not above the basis length) = contiguous bases."""
    L = out_channels // heads
    Ls = basis_stride if basis_stride > L else L
    ldb = (bases * Ls + 3) & ~3
    return Layer(heads, bases, len(aggrs), L, Ls, ldb, ldb // 4, heads * bases * len(aggrs), act, tuple(aggrs), f_in)


def narrow_shape(a):
    return 4 <= a.f_in <= FT_KP and a.f_in % 4 == 0 and a.ldb + a.W <= FT_NV and a.slots <= 64 and a.A <= AMAX


def wide_shape(a):
    if a.slots > 64 and (a.slots > 128 or a.B * (((a.Ls >> 2) + 1) // 2) > 64):
        return False
    return 4 <= a.f_in <= FTW_MAX_FIN and a.f_in % 4 == 0 and ((a.ldb + 31) & ~31) + a.W <= FTW_MAX_CT * 32 and a.A <= AMAX


def bwd_shape(a):
    if not narrow_shape(a) or a.act != ACT_NONE:
        return False
    if a.B != 4 or a.L != 16 or a.Ls != 16 or a.ldb != 64 or a.H not in (4, 8):
        return False
    return all(g in (SUM, MEAN, MAX, SYMNORM) for g in a.aggr)


def form(a):
    return "narrow" if narrow_shape(a) else "wide" if wide_shape(a) else "none"


def ftw_k16(f_in):
    return (((f_in + 15) // 16) + 3) & ~3


def ftw_n_ct(a):
    return (((a.ldb + 31) & ~31) + a.W + 31) // 32


def ftw_aw(a):
    return 4 if a.A >= 3 else a.A


def magic(d):
    return ((1 << 32) // d + 1) & 0xFFFFFFFF


def lds(a, wl_floats, tcap, emax, with_post, wide=False, bwd=False):
    """ft_lds: the LDS image's byte offsets, in its order, and the total."""
    def up16(v):
        return (v + 15) & ~15
    L = dict.fromkeys(("off_rec", "off_planes", "off_rowinv", "off_bases", "off_wt", "off_col", "off_rowptr", "off_cnt", "off_dis",
                       "csr_stride", "off_db", "off_rowinv2"), 0)
    at = up16((2 if with_post else 1) * ((a.H * a.Ls + 3) & ~3) * 4)
    L["off_rec"] = at; at += 128
    L["off_planes"] = at; at += FTW_PLANES_BYTES if wide else (max(FT_PLANES_BYTES, FTB_PLANES_BYTES) if bwd else FT_PLANES_BYTES)
    L["off_rowinv"] = at; at += up16(2 * FTW_CH * 4) if wide else up16(FT_PBUF * FT_CHUNK * 4)
    if bwd:
        L["off_rowinv2"] = at; at += up16(2 * FT_CHUNK * 4)
    L["off_bases"] = at; at += up16((tcap + 1) * a.ldb * 4)
    L["off_wt"] = at; at += up16(tcap * wl_floats * 4)
    if bwd:
        L["off_db"] = at; at += up16((tcap + 1) * a.ldb * 8)
    csr0 = at
    L["off_col"] = at; at += up16(emax * 2)
    L["off_rowptr"] = at; at += up16((tcap + 1) * 4)
    L["off_cnt"] = at; at += up16(tcap * 4)
    L["off_dis"] = at; at += up16(tcap * 4)
    L["csr_stride"] = at - csr0
    L["total"] = at + L["csr_stride"]
    return L


def pack_bytes(a):
    if narrow_shape(a):
        return FT_MFMA_WAVES * 4 * 2 * 64 * 8 * 2 + 2 * FT_NV * 4
    if wide_shape(a):
        return ftw_n_ct(a) * ftw_k16(a.f_in) * 2 * 64 * 8 * 2 + 2 * FTW_MAX_CT * 32 * 4
    return 0


def bwd_pack_bytes(a):
    return 8 * 6 * 2 * 64 * 8 * 2 + 128 * 4 if bwd_shape(a) else 0


def quantum(a):
    return FT_CHUNK if narrow_shape(a) else FTW_CH if wide_shape(a) else 0


def capacity(a, emax, with_post):
    """fused_tile_capacity: no look at the launch's emax bound."""
    if emax < 0:
        return 0
    best = 0
    if narrow_shape(a):
        for tcap in range(FT_CHUNK, FT_CHUNK * FT_RING + 1, FT_CHUNK):
            if lds(a, a.H * a.B * 4, tcap, emax, with_post)["total"] > FT_LDS_BUDGET:
                break
            best = tcap
    elif wide_shape(a):
        for tcap in range(FTW_CH, FTW_CH * FTW_MAXCH + 1, FTW_CH):
            if lds(a, a.H * a.B * ftw_aw(a), tcap, emax, with_post, True)["total"] > FT_LDS_BUDGET:
                break
            best = tcap
    return best


def bwd_chunks(a):
    return 6 if a.H == 8 else 8


def bwd_capacity(a, emax):
    if not bwd_shape(a) or emax < 0:
        return 0
    best = 0
    for tcap in range(FT_CHUNK, FT_CHUNK * bwd_chunks(a) + 1, FT_CHUNK):
        if lds(a, a.H * a.B * 4, tcap, emax, False, False, True)["total"] > FT_LDS_BUDGET:
            break
        best = tcap
    return best


def launch(a, tcap, emax, with_post):
    """launch_fused_tile up to the launch: (status, image or None, the FusedTileArgs fields it derives or None)."""
    if form(a) == "none":
        return UNSUPPORTED, None, None
    wide = not narrow_shape(a)
    w_aw = ftw_aw(a) if wide else 4
    if tcap < FT_CHUNK or tcap > FT_CHUNK * FT_RING or tcap % (FTW_CH if wide else FT_CHUNK) != 0 or emax < 0 or emax > 65535:
        return INVALID, None, None
    L = lds(a, a.H * a.B * w_aw, tcap, emax, with_post, wide)
    return (UNSUPPORTED if L["total"] > FT_LDS_BUDGET else OK), L, derived(a, wide, w_aw)


def bwd_launch(a, tcap, emax):
    if not bwd_shape(a):
        return UNSUPPORTED, None, None
    if tcap < FT_CHUNK or tcap > FT_CHUNK * bwd_chunks(a) or tcap % FT_CHUNK != 0 or emax < 0 or emax > 16384:
        return INVALID, None, None
    L = lds(a, a.H * a.B * 4, tcap, emax, False, False, True)
    return (UNSUPPORTED if L["total"] > FT_LDS_BUDGET else OK), L, derived(a, False, 4)


def derived(a, wide, w_aw):
    """ft_tile_args and the lines behind it in launch_fused_tile (the backward leaves the wide-only fields unset: not compared)."""
    p0 = ((a.Ls >> 2) + 1) // 2
    return dict(n_ct=ftw_n_ct(a) if wide else (a.ldb + a.W + 15) // 16, w_aw=w_aw, wl_floats=a.H * a.B * w_aw,
                nsets=2 if a.slots > 64 else 1, n_slabs=(a.f_in + FTW_SLAB - 1) // FTW_SLAB, k16=ftw_k16(a.f_in),
                ldbp=(a.ldb + 31) & ~31, p0=p0, magic0=magic(p0), magic1=magic(max(1, (a.Ls >> 2) - p0)),
                k2=a.ldb + a.H * a.B * 4)


def grid(n_graphs, n_nodes, ft_grid=None):
    """ft_tile_args' grid: 256 (or EGC_FT_GRID, at least 1), clamped by the graphs and by n_nodes / 16."""
    g = 256 if ft_grid is None else max(1, ft_grid)
    return min(g, max(1, n_graphs), max(1, n_nodes // 16))


def gate(a, x_looped, y_looped, layout, two_sets_ok):
    """tile_layer_args behind validate_layer: fast_path_supported, or (the forward) wide_path_supported, at n_nodes = 1."""
    if layout != LAYOUT_HBA or a.act == ACT_SOFTMAX or (x_looped and not y_looped):
        return False
    if a.Ls % 4 != 0 or a.ldb != a.B * a.Ls or a.B & (a.B - 1) or not 1 <= a.A <= AMAX or -(-a.H // a.B) > HPB_MAX:
        return False
    if 1 <= a.slots <= 64:
        return a.W <= 8 * (16 if a.slots <= 16 else 32 if a.slots <= 32 else 64)
    if not two_sets_ok or not 64 < a.slots <= 128 or a.W > 512 or a.B * ((a.Ls // 4 + 1) // 2) > 64:
        return False
    return 4 * (((a.H * a.Ls + 3) & ~3) + ((a.W + 3) & ~3)) * 4 <= 64 * 1024      # (the strips of launch_wide_rows, no post-op)
