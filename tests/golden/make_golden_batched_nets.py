#!/usr/bin/env python3
"""Generate tests/golden/bnets/*.npz: forward, loss and backward of the REFERENCE's molhiv, CIFAR and ogbg-code nets.

Same arrangement as make_golden_nets.py (whose install / _randomise / _run / _collect are used, not copied): the reference's
model files are imported as they are --

    mol/pna_style_models.py   EgcHIVNet, MpnnHIVNet   (AtomEncoder -> L x [conv, BatchNorm1d, ReLU, + x] -> pool -> mlp)
    cifar/models.py           EgcCifarNet             (Linear(5, h) -> L x [Dropout, conv, bn, relu, + identity] -> pool -> mlp)
    code/models.py            EgcCodeNet, MpnnCodeNet (ASTNodeEncoder -> L x [conv, bn, relu, + x] -> pool -> 5 x Linear)

-- over the reference's own layers.py / utils.py, with the shims of make_golden_nets.py, the ``propagate`` of
make_golden_mpnn.py that ends in ``update()``, and, written here: ogb's ``AtomEncoder`` (nine xavier-uniform tables of
egc_amd.encoders.ATOM_FEATURE_DIMS rows under ``atom_embedding_list``, summed from 0 in table order), ``global_add_pool`` /
``global_max_pool`` over the batch vector, and empty stand-ins for the modules the model files import and never use here
(``ogb``, ``torch_geometric.transforms``, ``torch_geometric.data``).

What is differentiated is the scalar LOSS of the reference's training loops (mol/configs.py:64-68: BCE with logits over the
entries with ``y == y``; cifar/configs.py:57: cross-entropy; code/configs.py:63-66: the mean of the five positions'
cross-entropies), from 1.0: no separate cotangent.  The loops cast the net's output to float32 first; here it stays in the
run's dtype, or there would be no float64 fixture.  Dropout probabilities are 0.

Per case, in float32 and float64: inputs, state dict, the net's output in evaluation and in training mode (``net_eval*`` /
``net_train*``; for the code nets the five positions' logits as [G, 5, classes]), the loss in both modes, every parameter's
gradient, the BatchNorm running statistics after the ONE training forward (``stat*:``), the seed, and the reference's own
float32-vs-float64 distances of all of these (``meta``).  A gradient of more than 4096 rows of which fewer than a quarter are
non-zero is stored as ``grad*:<key>:ids`` / ``grad*:<key>:rows`` (the 10030-row attribute table of the code nets).

While generating, every max / min (an aggregator's, Mpnn's, the max readout's) is checked in the float64 run: per (row, channel)
the best candidate and the best candidate of another VALUE must differ by more than 1e-4 of their magnitude, so that no float32
evaluation can route a gradient to another element than the fixture did.  A draw that fails is passed over for the next one,
one layer's convolution at a time (``separate``).

Only vectors are committed: per case ``<name>.npz`` and the gradients in ``<name>.grad.npz`` (each below the repository's limit
for a committed file), written with fixed zip timestamps: a rerun reproduces them byte for byte.
Runs only in the build container (needs /root/reference).  Usage:  python tests/golden/make_golden_batched_nets.py
"""
from __future__ import annotations

import copy
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden_grad as mgg  # noqa: E402
import make_golden_mpnn as mgm  # noqa: E402
import make_golden_nets as mgn  # noqa: E402
from egc_amd.encoders import ATOM_FEATURE_DIMS  # noqa: E402
from egc_amd.workloads import code_like_batch, knn_superpixel_batch, molecule_batch  # noqa: E402

REF = mgn.REF
OUT = os.path.join(HERE, "bnets")
SEPARATION = 1e-4
MAX_FILE_BYTES = 2_000_000            # per case
MAX_COMMITTED_BYTES = 1 << 20         # per file
MAX_TOTAL_BYTES = 10_000_000
SPARSE_ROWS = 4096


# ---------------------------------------------------------------------------------------------------------------------
# shims
# ---------------------------------------------------------------------------------------------------------------------
class NotSeparated(AssertionError):
    pass


def assert_separated(src, index, n, reduce):
    """float64 candidates src [E, F] of rows index [E]: best against the best of another value, per (row, channel)."""
    v = src.detach() if reduce == "max" else -src.detach()
    idx = index.view(-1, 1).expand(-1, v.size(1))
    top = torch.full((n, v.size(1)), -np.inf, dtype=v.dtype).scatter_reduce(0, idx, v, "amax", include_self=True)
    rest = torch.where(v == top[index], torch.full_like(v, -np.inf), v)
    second = torch.full((n, v.size(1)), -np.inf, dtype=v.dtype).scatter_reduce(0, idx, rest, "amax", include_self=True)
    has = torch.isfinite(second)
    gap = (top - second)[has]
    mag = torch.maximum(top.abs(), second.abs())[has]
    if bool((gap <= SEPARATION * mag).any()):
        raise NotSeparated(LAYER[0], f"{int((gap <= SEPARATION * mag).sum())} of {gap.numel()} {reduce} candidates closer than {SEPARATION}")


LAYER = [0]          # the graph layer whose convolution ran last (set by separate()'s hooks): whom a failed check blames


def checked_scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    # (the training forward only: the evaluation forward takes no gradient, so there is none to route elsewhere)
    if reduce in ("max", "min") and src.dtype == torch.float64 and torch.is_grad_enabled():
        assert_separated(src, index, int(dim_size), reduce)
    return mgg.diff_scatter(src, index, dim, out, dim_size, reduce)


class CheckedMessagePassing(mgm.UpdatingMessagePassing):
    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        return checked_scatter(inputs, index, self.node_dim, None, dim_size, self.aggr)


def global_add_pool(x, batch, size=None):
    n = int(batch.max()) + 1 if size is None else int(size)
    return torch.zeros(n, x.size(1), dtype=x.dtype).index_add(0, batch, x)


def global_max_pool(x, batch, size=None):
    n = int(batch.max()) + 1 if size is None else int(size)
    assert int(torch.bincount(batch, minlength=n).min()) >= 1          # every graph has a row: no -inf, no empty maximum
    return checked_scatter(x, batch, 0, None, n, "max")


class AtomEncoder(torch.nn.Module):
    """ogb.graphproppred.mol_encoder.AtomEncoder, restated: one table per atom feature, summed from 0 in table order."""

    def __init__(self, emb_dim):
        super().__init__()
        self.atom_embedding_list = torch.nn.ModuleList()
        for rows in ATOM_FEATURE_DIMS:
            emb = torch.nn.Embedding(rows, emb_dim)
            torch.nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)

    def forward(self, x):
        out = 0
        for i in range(x.shape[1]):
            out = out + self.atom_embedding_list[i](x[:, i])
        return out


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install():
    mgn.install()
    tg = sys.modules["torch_geometric.nn"]
    tg.MessagePassing = sys.modules["torch_geometric.nn.conv"].MessagePassing = CheckedMessagePassing
    tg.global_add_pool, tg.global_max_pool = global_add_pool, global_max_pool
    sys.modules["torch_scatter"].scatter = checked_scatter
    mgn._load("experiments.layers", os.path.join(REF, "layers.py"))         # again: it binds the two names above on import
    _stand_in("ogb")
    _stand_in("ogb.graphproppred", PygGraphPropPredDataset=None)
    _stand_in("ogb.graphproppred.mol_encoder", AtomEncoder=AtomEncoder)
    _stand_in("torch_geometric.transforms")
    _stand_in("torch_geometric.data", DataLoader=None)
    for sub in ("mol", "cifar", "code"):
        pkg = types.ModuleType(f"experiments.{sub}")
        pkg.__path__ = [os.path.join(REF, sub)]
        sys.modules[f"experiments.{sub}"] = pkg
    mgn._load("experiments.code.utils", os.path.join(REF, "code", "utils.py"))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def single_node_graph(ei, batch, k):
    """Graph k of the batch rewritten to ONE node without edges (its first node stays)."""
    first = int(torch.nonzero(batch == k)[0])
    keep = (batch != k)
    keep[first] = True
    new_id = torch.cumsum(keep.long(), 0) - 1
    e_keep = (batch[ei[0]] != k)
    return new_id[ei[:, e_keep]], int(keep.sum()), batch[keep]


def mol_inputs(rng, seed, n_graphs, lone):
    ei, n, batch = molecule_batch(n_graphs, seed=seed)
    if lone is not None:
        ei, n, batch = single_node_graph(ei, batch, lone)
    x = np.stack([rng.integers(0, rows, size=n) for rows in ATOM_FEATURE_DIMS], axis=1).astype(np.int64)
    y = rng.integers(0, 2, size=(n_graphs, 1)).astype(np.float32)
    y[::5] = np.nan                                                   # unlabelled: mol/configs.py:64 masks them out
    return dict(x=x, edge_index=ei.numpy(), batch=batch.numpy(), y=y)


def cifar_inputs(rng, seed, n_graphs):
    ei, n, batch = knn_superpixel_batch(n_graphs, seed=seed)
    x = rng.standard_normal((n, 5)).astype(np.float32)
    y = rng.integers(0, 10, size=n_graphs).astype(np.int64)
    return dict(x=x, edge_index=ei.numpy(), batch=batch.numpy(), y=y)


def code_inputs(rng, seed, n_graphs, n_classes, seq_len):
    ei, n, batch = code_like_batch(n_graphs, mean_nodes=40, min_nodes=5, max_nodes=80, seed=seed)
    x = np.stack([rng.integers(0, 98, size=n), rng.integers(0, 10030, size=n)], axis=1).astype(np.int64)
    depth = rng.integers(0, 26, size=n).astype(np.int64)              # past MAX_DEPTH = 20: the encoder clamps
    y_arr = rng.integers(0, n_classes, size=(n_graphs, seq_len)).astype(np.int64)
    return dict(x=x, edge_index=ei.numpy(), batch=batch.numpy(), node_depth=depth, y_arr=y_arr)


# ---------------------------------------------------------------------------------------------------------------------
# losses of the reference's training loops, in the run's dtype
# ---------------------------------------------------------------------------------------------------------------------
def mol_loss(out, data, dtype):
    is_labeled = data.y == data.y
    return F.binary_cross_entropy_with_logits(out.to(dtype)[is_labeled], data.y.to(dtype)[is_labeled])


def cifar_loss(out, data, dtype):
    return F.cross_entropy(out, data.y)


def code_loss(pred_list, data, dtype):
    loss = 0
    for i in range(len(pred_list)):
        loss += F.cross_entropy(pred_list[i].to(dtype), data.y_arr[:, i])
    loss /= len(pred_list)
    return loss


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def cases():
    egc = lambda H, B, aggrs: dict(heads=H, bases=B, aggrs=aggrs)                                     # noqa: E731
    return [
        # name, family, class, hidden, layers, readout, conv arguments, first seed, (mol: the graph made a single node)
        ("hiv_egc_mean", "mol", "EgcHIVNet", 56, 4, "mean", egc(4, 4, ["add", "std", "max"]), 5100, None),
        ("hiv_egc_max", "mol", "EgcHIVNet", 64, 4, "max", egc(8, 4, ["symadd"]), 5200, 7),
        ("hiv_egc_sum", "mol", "EgcHIVNet", 48, 4, "sum", egc(4, 4, ["mean", "min"]), 5300, None),
        ("hiv_mpnn_add", "mol", "MpnnHIVNet", 48, 4, "mean", dict(aggr="add"), 5400, None),
        ("hiv_mpnn_max", "mol", "MpnnHIVNet", 48, 4, "mean", dict(aggr="max"), 5500, 3),
        ("cifar_egc", "cifar", "EgcCifarNet", 64, 4, "mean", egc(8, 4, ["symadd", "max", "mean"]), 5600, None),
        ("cifar_egc_max", "cifar", "EgcCifarNet", 64, 4, "max", egc(8, 4, ["symadd", "max", "mean"]), 5700, None),
        ("code_egc", "code", "EgcCodeNet", 32, 4, "mean", egc(4, 4, ["symadd", "min", "max"]), 5800, None),
        ("code_mpnn", "code", "MpnnCodeNet", 32, 4, "mean", dict(aggr="add"), 5900, None),
    ]


VOCAB, SEQ_LEN = 130, 5
FAMILY = {
    "mol": dict(file=("mol", "pna_style_models.py"), n_graphs=24, loss=mol_loss, ref="mol/pna_style_models.py:21-79"),
    "cifar": dict(file=("cifar", "models.py"), n_graphs=6, loss=cifar_loss, ref="cifar/models.py:18-75"),
    "code": dict(file=("code", "models.py"), n_graphs=24, loss=code_loss, ref="code/models.py:27-125"),
}


def _convs(net):
    return [[m for m in layer if not isinstance(m, (torch.nn.Dropout, torch.nn.BatchNorm1d, torch.nn.ReLU))][0]
            for layer in net.graph_layers]


def separate(net, call, seed, tries=6000):
    """Make every max / min of the float64 training forward separated (the module docstring), layer by layer: a whole-net seed
    would have to clear about 1e5 (row, channel) pairs at once, each failing with probability about 1e-4, so instead the
    convolution of the FIRST layer that fails is drawn again (seed, layer and attempt name its generator; a failed max
    readout blames the last layer) until the forward passes; the layers in front of it stay as they are.  Returns the
    attempts per layer."""
    attempts = [0] * len(net.graph_layers)
    for _ in range(tries):
        probe = copy.deepcopy(net).double().train()
        for i, conv in enumerate(_convs(probe)):
            conv.register_forward_pre_hook(lambda m, a, i=i: LAYER.__setitem__(0, i))
        try:
            with torch.enable_grad():
                call(probe, torch.float64, True)
            return attempts
        except NotSeparated as e:
            layer = e.args[0]
        attempts[layer] += 1
        conv = _convs(net)[layer]
        draw = seed * 100003 + layer * 10007 + attempts[layer]
        torch.manual_seed(draw)
        if hasattr(conv, "reset_parameters"):
            conv.reset_parameters()
        else:
            for m in conv.modules():
                if isinstance(m, torch.nn.Linear):
                    m.reset_parameters()
        mgn._randomise(conv, np.random.default_rng(draw))
    raise SystemExit(f"seed {seed}: no separated draw of layer {layer} in {tries} attempts")


def build_net(mod, family, cls, hidden, layers, readout, conv):
    if family == "mol":
        return getattr(mod, cls)(hidden, layers, 0.0, True, readout=readout, **conv)
    if family == "cifar":
        return getattr(mod, cls)(hidden, layers, True, readout=readout, dropout=0.0, **conv)
    return getattr(mod, cls)(hidden, layers, 0.0, True, vocab_size=VOCAB, seq_len=SEQ_LEN, readout=readout, **conv)


def run_case(mod, case, seed):
    name, family, cls, hidden, layers, readout, conv, _, lone = case
    fam = FAMILY[family]
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    g = fam["n_graphs"]
    if family == "mol":
        inputs = mol_inputs(rng, seed, g, lone)
    elif family == "cifar":
        inputs = cifar_inputs(rng, seed, g)
    else:
        inputs = code_inputs(rng, seed, g, VOCAB + 2, SEQ_LEN)
    net = build_net(mod, family, cls, hidden, layers, readout, conv)
    mgn._randomise(net, rng)
    tensors = {k: torch.from_numpy(v) for k, v in inputs.items()}
    taps = {}

    def call(net, dtype, train):
        data = types.SimpleNamespace(**{k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in tensors.items()})
        out = net(data)
        taps[(dtype, train)] = (torch.stack(out, dim=1) if isinstance(out, list) else out).detach().clone()
        return fam["loss"](out, data, dtype), None

    if family == "code":
        # the rows of the 10030-row attribute table that no node of the batch reads take no part in forward or backward, and
        # 1.1 MB of incompressible noise would take the file past its cap: they are zeroed (a wrong row read on the device
        # still shows: the rows that ARE read keep their N(0, 1) values)
        with torch.no_grad():
            table = net.embedding.attribute_encoder.weight
            unread = torch.ones(table.size(0), dtype=torch.bool)
            unread[tensors["x"][:, 1]] = False
            table[unread] = 0.0
    attempts = separate(net, call, seed)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    one = torch.ones(())
    res, stats = {}, {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        res[tag] = mgn._run(net, call, one, dtype, state)
        stats[tag] = {k: v.detach().clone() for k, v in net.state_dict().items()
                      if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    net.float()
    meta = dict(net=cls, family=family, ref=fam["ref"], hidden=hidden, layers=layers, readout=readout, residual=True, seed=seed,
                n=int(inputs["x"].shape[0]), n_edges=int(inputs["edge_index"].shape[1]), n_graphs=g,
                single_node_graph=lone, conv_draws=attempts, **({k: v for k, v in conv.items()}),
                **(dict(n_classes=VOCAB + 2, seq_len=SEQ_LEN) if family == "code" else {}))
    arrays, meta = mgn._collect(meta, inputs, state, one, res["32"], res["64"])
    del arrays["gout"]
    # what _run differentiates is the loss: its "out" is the loss, the net's outputs are the taps
    for tag in ("32", "64"):
        arrays[f"loss_eval{tag}"] = arrays.pop(f"out_eval{tag}")
        arrays[f"loss_train{tag}"] = arrays.pop(f"out_train{tag}")
        dtype = torch.float32 if tag == "32" else torch.float64
        arrays[f"net_eval{tag}"] = taps[(dtype, False)].numpy()
        arrays[f"net_train{tag}"] = taps[(dtype, True)].numpy()
        arrays.update({f"stat{tag}:{k}": v.numpy() for k, v in stats[tag].items()})
    meta["f32_vs_f64_loss"] = meta.pop("f32_vs_f64_out_train")

    def dist(a, b):          # _collect's distance of an output
        a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
        return float((a - b).abs().max() / max(1.0, float(b.abs().max())))
    meta["f32_vs_f64_out_train"] = dist(arrays["net_train32"], arrays["net_train64"])
    meta["f32_vs_f64_loss_eval"] = dist(arrays["loss_eval32"], arrays["loss_eval64"])
    meta["f32_vs_f64_out_eval"] =dist(arrays["net_eval32"], arrays["net_eval64"])
    meta["f32_vs_f64_stat"] = {k: dist(stats["32"][k], v) for k, v in stats["64"].items() if not k.endswith("tracked")}
    for k in [k for k in arrays if k.startswith("grad64:")]:
        key = k[len("grad64:"):]
        g64 = arrays[k]
        if g64.ndim == 2 and g64.shape[0] > SPARSE_ROWS:
            ids = np.nonzero(np.abs(g64).sum(axis=1) + np.abs(arrays[f"grad32:{key}"]).sum(axis=1))[0].astype(np.int64)
            if 4 * len(ids) < g64.shape[0]:
                for tag in ("32", "64"):
                    dense = arrays.pop(f"grad{tag}:{key}")
                    arrays[f"grad{tag}:{key}:ids"], arrays[f"grad{tag}:{key}:rows"] = ids, dense[ids]
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return arrays, meta


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    os.makedirs(OUT, exist_ok=True)
    install()
    mods = {fam: mgn._load(f"experiments.{v['file'][0]}.{v['file'][1][:-3]}", os.path.join(REF, *v["file"]))
            for fam, v in FAMILY.items()}
    manifest, total = {}, 0
    for case in cases():
        name, family, seed0 = case[0], case[1], case[7]
        seed = seed0
        arrays, meta = run_case(mods[family], case, seed)
        # two files per case, each inside the repository's limit for a committed file: the gradients, and everything else
        grads = {k: arrays.pop(k) for k in [k for k in arrays if k.startswith("grad")]}
        size = 0
        for path, part in ((os.path.join(OUT, f"{name}.npz"), arrays), (os.path.join(OUT, f"{name}.grad.npz"), grads)):
            write_npz(path, part)
            assert os.path.getsize(path) <= MAX_COMMITTED_BYTES, (path, os.path.getsize(path))
            size += os.path.getsize(path)
        assert size <= MAX_FILE_BYTES, (name, size)
        total += size
        manifest[name] = dict({k: v for k, v in meta.items() if k not in ("f32_vs_f64_grad", "f32_vs_f64_stat")}, bytes=size)
        print(f"{name:14s} seed {seed} N={meta['n']:4d} E={meta['n_edges']:5d} {size / 1e6:.2f} MB  loss f32-vs-f64 "
              f"{meta['f32_vs_f64_loss']:.2e}  out {meta['f32_vs_f64_out_train']:.2e}  worst gradient {meta['f32_vs_f64_grad_max']:.2e}")
    assert total <= MAX_TOTAL_BYTES, total
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
