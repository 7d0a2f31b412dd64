"""GCNConv, SAGEConv, GINConv and the neighbour sum without a GPU: the properties the fixtures are named for, the chunked
restatement against the plain one, the transpose identities the backward rests on (sum <-> sum, mean <-> mean_t, sym <-> sym, with
and without skipped self entries), the restated layers against the fixtures in float64, the modules' contract (constructors,
repr, state dict, eps, errors), and the C ABI's argument errors, which come back before any device call."""
import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from nbr_ref import (CASES, CHUNK, FORMS, TRANSPOSE, build_layer, csr_by_destination, dis_tables, ladder_graph, load_gnn_golden, nbr_sum, nbr_sum_plain,
                     nbr_sum_transposed, rel_grad, rel_out, transposed_csr)


# -------------------------------------------------------------------------------------------------------------- the fixtures

def test_chunk_is_the_librarys():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    assert (_C.NBR_SUM, _C.NBR_MEAN, _C.NBR_MEAN_T, _C.NBR_SYM) == (0, 1, 2, 3)


def test_fixtures_have_the_properties_they_are_named_for():
    seen = set()
    for name in CASES:
        g = load_gnn_golden(name)
        m, (src, dst) = g["meta"], g["ei"]
        n, fin, fout, opt = m["n"], m["in_channels"], m["out_channels"], m["options"]
        assert g["x"].shape == (n, fin) and g["gout"].shape == g["out64"].shape == g["out32"].shape == (n, fout)
        assert g["x"].dtype == g["out32"].dtype == np.float32 and g["out64"].dtype == g["grad_x64"].dtype == np.float64
        assert set(g["grad64"]) == set(g["params"]) - ({"eps"} if m["layer"] == "gin" and not opt["train_eps"] else set())
        assert set(m["f32_vs_f64_grad"]) == set(g["grad64"]) and m["chunk"] == CHUNK
        indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
        if "messy" in name:
            pairs = src * n + dst
            assert (src == dst).sum() >= 9 and len(pairs) - len(np.unique(pairs)) >= 20
            assert (indeg[-3:] == 0).all() and (outdeg[-3:] == 0).all()
        if "hub" in name:
            assert indeg.max() > 2 * CHUNK + 1 and outdeg.max() > 2 * CHUNK + 1
        seen.add((m["layer"], tuple(sorted(opt.items(), key=str)) if m["layer"] != "gin" else opt["train_eps"]))
    by_name = {name: load_gnn_golden(name)["meta"] for name in CASES}
    assert by_name["gcn_messy_narrow_in"]["in_channels"] < by_name["gcn_messy_narrow_in"]["out_channels"]
    assert by_name["gcn_messy_wide_in"]["in_channels"] > by_name["gcn_messy_wide_in"]["out_channels"]
    for name in ("gcn_messy_narrow_in", "gcn_messy_wide_in", "sage_mean_messy", "gin_train_eps"):
        assert by_name[name]["in_channels"] % 4 != 0
    flags = {(m["options"]["normalize"], m["options"]["add_self_loops"]) for m in by_name.values() if m["layer"] == "gcn"}
    assert flags == {(True, True), (True, False), (False, True), (False, False)}
    assert {m["options"]["aggr"] for m in by_name.values() if m["layer"] == "sage"} == {"mean", "sum"}
    assert not by_name["sage_no_root"]["options"]["root_weight"] and by_name["sage_normalize"]["options"]["normalize"]
    assert by_name["gin_train_eps"]["options"]["train_eps"] and by_name["gin_train_eps"]["options"]["eps"] != 0.0
    assert not by_name["gin_buffer_eps"]["options"]["train_eps"] and by_name["gin_buffer_eps"]["options"]["eps"] != 0.0


# ------------------------------------------------------------------------------------------------------- the restatement

def _case(square, seed=5, width=5, flip=False):
    """a reduced ladder graph (rows up to 2 CHUNK + 1 entries), its CSR, and seeded operands"""
    ei, n_dst, n_src = ladder_graph(seed, flip=flip, square=square, max_len=2 * CHUNK + 1)
    rowptr, col, _ = csr_by_destination(ei, n_dst)
    rng = np.random.default_rng(seed + 1)
    return rowptr, col, n_dst, n_src, rng.standard_normal((n_src, width)), rng.standard_normal((n_dst, width))


def _configs(rowptr, col, n_dst, n_src, square):
    """(form, keyword arguments) of every configuration the layers launch, forward"""
    t_rowptr, _ = transposed_csr(rowptr, col, n_src)
    out = [("sum", {}), ("mean", {}), ("mean_t", dict(deg_rowptr=t_rowptr)), ("sum", dict(self=True, s=1.3))]
    if square:
        raw, looped = dis_tables(rowptr, col)
        out += [("sum", dict(self=True, skip=True)), ("sym", dict(row_scale=raw, src_scale=raw)),
                ("sym", dict(self=True, skip=True, row_scale=looped, src_scale=looped)),
                ("sym", dict(self=True, skip=True, row_scale=looped, edge_scale=looped[col]))]
    return out


@pytest.mark.parametrize("square", (True, False), ids=("square", "rectangular"))
def test_chunked_restatement_equals_the_plain_one_in_float64(square):
    rowptr, col, n_dst, n_src, x, xs = _case(square)
    assert np.diff(rowptr).max() > 2 * CHUNK and (square or n_dst != n_src)
    for form, kw in _configs(rowptr, col, n_dst, n_src, square):
        kw = dict(kw)
        x_self = xs if kw.pop("self", False) else None
        got = nbr_sum(x, rowptr, col, form, x_self=x_self, dtype=np.float64, **kw)
        want = nbr_sum_plain(x, rowptr, col, form, x_self=x_self, **kw)
        assert rel_out(got, want) <= 1e-13, (form, kw.keys())
        one_chunk = nbr_sum(x, rowptr, col, form, x_self=x_self, dtype=np.float64, chunk=10 ** 9, **kw)
        assert rel_out(got, one_chunk) <= 1e-13
    # the chunks are real: in float32 a row of more than one chunk does not have the bits of one running sum
    a = nbr_sum(x, rowptr, col, "sum", dtype=np.float32)
    b = nbr_sum(x, rowptr, col, "sum", dtype=np.float32, chunk=10 ** 9)
    long_rows = np.diff(rowptr) > CHUNK
    assert np.array_equal(a[~long_rows], b[~long_rows]) and not np.array_equal(a[long_rows], b[long_rows])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("skip", (False, True), ids=("all_entries", "skip_self"))
def test_transpose_identity(form, skip):
    """<d out, F(x)> = <F^T(d out), x>: the form TRANSPOSE[form] on the transposed CSR is the adjoint, and with x_self = x the
    self term transposes to itself in the same pass."""
    rowptr, col, n, n_src, x, dout = _case(True, seed=8)
    assert n == n_src and (col == np.repeat(np.arange(n), np.diff(rowptr))).sum() > 0          # self entries to skip
    t_rowptr, t_col = transposed_csr(rowptr, col, n)
    _, looped = dis_tables(rowptr, col)
    kw = dict(deg_rowptr=t_rowptr) if form == "mean_t" else dict(row_scale=looped, src_scale=looped) if form == "sym" else {}
    for shared in (False, True):
        out = nbr_sum(x, rowptr, col, form, x_self=x if shared else None, s=0.7, skip=skip, dtype=np.float64, **kw)
        dx = nbr_sum_transposed(dout, rowptr, col, n, form, shared_self=shared, s=0.7, skip=skip, scale=looped, dtype=np.float64)
        lhs, rhs = float((dout * out).sum()), float((dx * x).sum())
        assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (form, skip, shared, lhs, rhs)
        # and entry by entry against the dense transpose
        basis = nbr_sum_plain(np.eye(n), rowptr, col, form, x_self=np.eye(n) if shared else None, s=0.7, skip=skip, **kw)
        assert rel_grad(dx, basis.T @ dout) <= 1e-12
    assert TRANSPOSE[TRANSPOSE[form]] == form
    # transposing twice gives the rows back, each with its entries sorted by source
    tt_rowptr, tt_col = transposed_csr(t_rowptr, t_col, n)
    assert np.array_equal(tt_rowptr, rowptr)
    assert all(np.array_equal(tt_col[a:b], np.sort(col[a:b])) for a, b in zip(rowptr[:-1], rowptr[1:]))


def test_skipped_entries_keep_their_place_in_the_chunk_layout():
    """Row 0 holds CHUNK + 1 entries, the first CHUNK of them self entries: with skip the one live entry still sits in chunk 1,
    and the float32 bits are those of (0) + (0 + t), not of a re-packed row."""
    n, d = 3, 4
    col = np.concatenate([np.zeros(CHUNK, dtype=np.int64), [1], [2, 0]])
    rowptr = np.array([0, CHUNK + 1, CHUNK + 3, CHUNK + 3])
    x = np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)
    out = nbr_sum(x, rowptr, col, "sum", skip=True)
    assert np.array_equal(out[0], x[1]) and np.array_equal(out[1], x[2] + x[0]) and np.array_equal(out[2], np.zeros(d, dtype=np.float32))
    mean = nbr_sum(x, rowptr, col, "mean", skip=True)                  # deg_i is the walked row's entry count, skipped ones included
    assert np.array_equal(mean[0], x[1] / np.float32(CHUNK + 1))


# ------------------------------------------------------------------------------------- the layers, restated, against the fixtures

def restated_layer(g, dtype=np.float64):
    """The layer of a fixture through nbr_sum in the package's order of operations (numpy, forward only)."""
    m, p = g["meta"], {k: v.astype(dtype) for k, v in g["params"].items()}
    opt, n = m["options"], m["n"]
    x = g["x"].astype(dtype)
    rowptr, col, _ = csr_by_destination(g["ei"], n)
    if m["layer"] == "gcn":
        raw, looped = dis_tables(rowptr, col)
        loops = opt["add_self_loops"]

        def propagate(h):
            if opt["normalize"]:
                scale = looped if loops else raw
                return nbr_sum(h, rowptr, col, "sym", x_self=h if loops else None, skip=loops, row_scale=scale, src_scale=scale, dtype=dtype)
            return nbr_sum(h, rowptr, col, "sum", x_self=h if loops else None, skip=loops, dtype=dtype)
        if m["out_channels"] <= m["in_channels"]:
            return propagate(x @ p["lin.weight"].T) + p["bias"]
        return propagate(x) @ p["lin.weight"].T + p["bias"]
    if m["layer"] == "sage":
        out = nbr_sum(x, rowptr, col, opt["aggr"], dtype=dtype) @ p["lin_l.weight"].T + p["lin_l.bias"]
        if opt["root_weight"]:
            out = out + x @ p["lin_r.weight"].T
        return out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12) if opt["normalize"] else out
    h = nbr_sum(x, rowptr, col, "sum", x_self=x, s=dtype(1) + p["eps"][0], dtype=dtype)
    n_lin = len(opt["hidden"]) + 1
    for k in range(n_lin):
        h = h @ p[f"nn.{2 * k}.weight"].T + p[f"nn.{2 * k}.bias"]
        h = np.maximum(h, 0) if k + 1 < n_lin else h
    return h


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    g = load_gnn_golden(name)
    err = rel_out(restated_layer(g), g["out64"])
    print(name, f"{err:.1e}")
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------------------- the modules

@pytest.mark.parametrize("name", CASES)
def test_state_dict_names_shapes_and_strict_load(name):
    g = load_gnn_golden(name)
    layer = build_layer(g)
    assert sorted(layer.state_dict().keys()) == sorted(g["params"].keys())
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in layer.state_dict().items():
        assert v.shape == g["params"][k].shape and np.array_equal(v.numpy(), g["params"][k]), k


def test_constructors_and_repr():
    gcn = egc_amd.GCNConv(12, 7, cached=True)
    assert gcn.lin.weight.shape == (7, 12) and gcn.lin.bias is None and gcn.bias.shape == (7,) and float(gcn.bias.detach().abs().max()) == 0.0
    assert "12, 7" in repr(gcn) and "normalize=True" in repr(gcn) and gcn.cached
    assert list(egc_amd.GCNConv(4, 4, bias=False).state_dict()) == ["lin.weight"]
    sage = egc_amd.SAGEConv(12, 7, aggr="add")
    assert sage.lin_l.weight.shape == sage.lin_r.weight.shape == (7, 12) and sage.lin_l.bias.shape == (7,) and sage.lin_r.bias is None
    assert "aggr=add" in repr(sage)
    assert sorted(egc_amd.SAGEConv(3, 5, root_weight=False, bias=False).state_dict()) == ["lin_l.weight"]
    gin = egc_amd.GINConv(torch.nn.Linear(3, 5), eps=0.25, train_eps=True)
    assert "train_eps=True" in repr(gin) and "Linear" in repr(gin)


def test_eps_is_a_parameter_or_a_buffer():
    trained = egc_amd.GINConv(torch.nn.Linear(3, 5), eps=0.25, train_eps=True)
    fixed = egc_amd.GINConv(torch.nn.Linear(3, 5), eps=0.25)
    for layer in (trained, fixed):
        assert layer.eps.shape == (1,) and layer.eps.dtype == torch.float32 and float(layer.eps.detach()) == 0.25
        assert "eps" in layer.state_dict()
    assert isinstance(trained.eps, torch.nn.Parameter) and trained.eps.requires_grad and "eps" in dict(trained.named_parameters())
    assert not isinstance(fixed.eps, torch.nn.Parameter) and "eps" in dict(fixed.named_buffers()) and "eps" not in dict(fixed.named_parameters())
    fixed.load_state_dict(trained.state_dict(), strict=True)


def test_unsupported_options_raise():
    with pytest.raises(NotImplementedError, match="improved"):
        egc_amd.GCNConv(4, 4, improved=True)
    with pytest.raises(NotImplementedError, match="project"):
        egc_amd.SAGEConv(4, 4, project=True)
    for aggr in ("max", "lstm", None):
        with pytest.raises(ValueError, match="aggr"):
            egc_amd.SAGEConv(4, 4, aggr=aggr)
    ei = torch.zeros((2, 0), dtype=torch.int64)
    for layer in (egc_amd.GCNConv(8, 4), egc_amd.SAGEConv(8, 4)):
        with pytest.raises(RuntimeError, match="expected"):
            layer(torch.zeros(5, 7), ei)
        with pytest.raises(RuntimeError, match="ROCm device"):        # the package's usual error for a host tensor
            layer(torch.zeros(5, 8), ei)
    with pytest.raises(RuntimeError, match="expected"):
        egc_amd.GINConv(torch.nn.Linear(8, 4))(torch.zeros(5), ei)
    with pytest.raises(ValueError, match="form"):
        egc_amd.neighbor_sum(torch.zeros(3, 4), ei, "max")
    with pytest.raises(RuntimeError):
        egc_amd.neighbor_sum(torch.zeros(3, 4), ei, "sum")


# -------------------------------------------------------------------------------------------------------------- the C ABI

def _call(lib, n_rows=4, n_edges=0, n_src=4, x=None, ld_x=8, x_self=None, ld_self=8, width=8, form=0, skip=0, deg_rowptr=None,
          row_scale=None, src_scale=None, edge_scale=None, out=None, ld_out=8, rowptr=None):
    return lib.egc_nbr_sum_f32(rowptr, None, n_rows, n_edges, n_src, x, ld_x, x_self, ld_self, width, form, skip, 1.0, None, deg_rowptr,
                               row_scale, src_scale, edge_scale, out, ld_out, None, 0, None)


def test_abi_argument_errors_come_back_without_a_device():
    lib = _C.load()
    OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 2, 4
    P = 4096                                     # a non-NULL address; no call below gets as far as using it
    assert lib.egc_nbr_sum_workspace_bytes(CHUNK, 30) == 0                  # no row can be longer than a chunk
    assert lib.egc_nbr_sum_workspace_bytes(1000, 30) == 4 * 8 * 16          # ceil(1000 / 256) slots of 8 lanes
    assert lib.egc_nbr_sum_workspace_bytes(1000, 0) == 0 and lib.egc_nbr_sum_workspace_bytes(-1, 8) == 0
    assert _call(lib, n_rows=0) == OK                                       # nothing to do
    for kw in (dict(width=0), dict(width=-4), dict(n_rows=-1), dict(n_edges=-1), dict(n_src=-1), dict(form=4), dict(form=-1),
               dict(ld_x=7), dict(ld_out=7), dict(x_self=P, ld_self=7), dict(rowptr=P), dict(out=P),
               dict(rowptr=P, out=P, n_edges=5),                                      # entries without col and x
               dict(form=_C.NBR_MEAN_T, rowptr=P, out=P),                            # MEAN_T without deg_rowptr
               dict(form=_C.NBR_SYM, rowptr=P, out=P),                               # SYM without scales
               dict(form=_C.NBR_SYM, rowptr=P, out=P, row_scale=P),                  # ... without a source of e_p
               dict(form=_C.NBR_SYM, rowptr=P, out=P, src_scale=P, edge_scale=P)):   # ... without row_scale
        assert _call(lib, **kw) == INVALID, kw
    for kw in (dict(skip=1),                                                          # SUM + skip without x_self
               dict(form=_C.NBR_MEAN, x_self=P), dict(form=_C.NBR_MEAN, skip=1),
               dict(form=_C.NBR_MEAN_T, deg_rowptr=P, skip=1, x_self=P),
               dict(form=_C.NBR_SYM, row_scale=P, src_scale=P, x_self=P),            # SYM: the self term comes with skip only
               dict(form=_C.NBR_SYM, row_scale=P, edge_scale=P, skip=1),
               dict(rowptr=P, out=P, n_rows=2 ** 31), dict(rowptr=P, out=P, n_src=2 ** 31)):
        assert _call(lib, **kw) == UNSUPPORTED, kw
    # a CSR of more than one chunk of entries needs its workspace before anything is launched
    assert lib.egc_nbr_sum_f32(P, P, 4, 1000, 4, P, 8, None, 0, 8, 0, 0, 1.0, None, None, None, None, None, P, 8, None, 0, None) == WORKSPACE
    assert lib.egc_nbr_sum_f32(P, P, 4, 1000, 4, P, 8, None, 0, 8, 0, 0, 1.0, None, None, None, None, None, P, 8, 4096, 16, None) == WORKSPACE
