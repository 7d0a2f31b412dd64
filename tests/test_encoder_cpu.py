"""The node encoders without a GPU: state-dict compatibility with the modules they replace, the CPU path (torch's
operators, composed as the reference composes them), and argument errors."""
import pytest
import torch
import torch.nn as nn

import egc_amd

ATOM_ROWS = [119, 4, 12, 12, 10, 6, 6, 2, 2]     # output/pretrained.txt:460-470 of the reference


class _RefAtomEncoder(nn.Module):
    """The structure of ogb's AtomEncoder (nine nn.Embedding in a ModuleList, summed from 0)."""

    def __init__(self, emb_dim):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList([nn.Embedding(r, emb_dim) for r in ATOM_ROWS])

    def forward(self, x):
        out = 0
        for i in range(x.shape[1]):
            out = out + self.atom_embedding_list[i](x[:, i])
        return out


class _RefASTNodeEncoder(nn.Module):
    """The structure of the reference's ASTNodeEncoder (code/models.py:27-45), in-place clamp included."""

    def __init__(self, emb_dim, num_nodetypes, num_nodeattributes, max_depth):
        super().__init__()
        self.max_depth = max_depth
        self.type_encoder = nn.Embedding(num_nodetypes, emb_dim)
        self.attribute_encoder = nn.Embedding(num_nodeattributes, emb_dim)
        self.depth_encoder = nn.Embedding(max_depth + 1, emb_dim)

    def forward(self, x, depth):
        depth[depth > self.max_depth] = self.max_depth
        return self.type_encoder(x[:, 0]) + self.attribute_encoder(x[:, 1]) + self.depth_encoder(depth)


def _atom_idx(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, r, (n,), generator=g) for r in ATOM_ROWS], dim=1)


def test_state_dict_keys_and_shapes():
    sd = egc_amd.Embedding(28, 20).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"weight": (28, 20)}
    sd = egc_amd.AtomEncoder(24).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {f"atom_embedding_list.{i}.weight": (r, 24)
                                                          for i, r in enumerate(ATOM_ROWS)}
    sd = egc_amd.ASTNodeEncoder(16, 98, 10030, 20).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"type_encoder.weight": (98, 16), "attribute_encoder.weight": (10030, 16),
                                                          "depth_encoder.weight": (21, 16)}
    sd = egc_amd.NodeEncoder([5, 7], 8).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"tables.0.weight": (5, 8), "tables.1.weight": (7, 8)}


def test_initialisation_matches_the_replaced_modules():
    torch.manual_seed(3)
    a = egc_amd.AtomEncoder(40)
    for emb in a.atom_embedding_list:     # xavier_uniform_: |w| <= sqrt(6 / (rows + dim)), and not all zero
        bound = (6.0 / (emb.weight.size(0) + 40)) ** 0.5
        assert float(emb.weight.detach().abs().max()) <= bound and float(emb.weight.detach().abs().max()) > 0.5 * bound
    torch.manual_seed(5)
    mine = egc_amd.Embedding(28, 12)
    torch.manual_seed(5)
    theirs = nn.Embedding(28, 12)
    assert torch.equal(mine.weight, theirs.weight)
    torch.manual_seed(7)
    mine = egc_amd.ASTNodeEncoder(8, 9, 11, 4)
    torch.manual_seed(7)
    theirs = _RefASTNodeEncoder(8, 9, 11, 4)
    for (ka, va), (kb, vb) in zip(mine.state_dict().items(), theirs.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_reference_checkpoints_load_strict_and_cpu_path_reproduces_them():
    torch.manual_seed(0)
    ref = _RefAtomEncoder(36)
    enc = egc_amd.AtomEncoder(36)
    enc.load_state_dict(ref.state_dict(), strict=True)
    x = _atom_idx(301)
    assert torch.equal(enc(x), ref(x))

    ref = nn.Embedding(28, 20)
    enc = egc_amd.Embedding(28, 20)
    enc.load_state_dict(ref.state_dict(), strict=True)
    atom = torch.randint(0, 28, (77,))
    assert torch.equal(enc(atom), ref(atom))

    ref = _RefASTNodeEncoder(12, 98, 500, 20)
    enc = egc_amd.ASTNodeEncoder(12, 98, 500, 20)
    enc.load_state_dict(ref.state_dict(), strict=True)
    x = torch.stack([torch.randint(0, 98, (64,)), torch.randint(0, 500, (64,))], dim=1)
    depth = torch.randint(0, 40, (64,))
    assert torch.equal(enc(x, depth.clone()), ref(x, depth.clone()))


def test_ast_encoder_leaves_the_callers_depth_untouched():
    enc = egc_amd.ASTNodeEncoder(8, 98, 50, 20)
    x = torch.stack([torch.randint(0, 98, (32,)), torch.randint(0, 50, (32,))], dim=1)
    depth = torch.arange(32) * 2          # half of them beyond max_depth
    before = depth.clone()
    out = enc(x, depth)
    assert torch.equal(depth, before)
    assert torch.equal(out[31], enc.type_encoder.weight[x[31, 0]] + enc.attribute_encoder.weight[x[31, 1]] + enc.depth_encoder.weight[20])


def test_cpu_gradients_and_dropout_follow_torch():
    torch.manual_seed(1)
    enc = egc_amd.AtomEncoder(16)
    ref = _RefAtomEncoder(16)
    ref.load_state_dict(enc.state_dict(), strict=True)
    x = _atom_idx(90, seed=4)
    go = torch.randn(90, 16)
    enc(x).backward(go)
    ref(x).backward(go)
    for a, b in zip(enc.parameters(), ref.parameters()):
        assert torch.equal(a.grad, b.grad)
    drop = egc_amd.AtomEncoder(16, dropout=0.5)
    drop.load_state_dict(enc.state_dict())
    drop.eval()
    assert torch.equal(drop(x), enc(x))                      # eval mode: nothing is dropped
    drop.train()
    out = drop(x)
    kept = out != 0
    assert 0.2 < float(kept.float().mean()) < 0.8
    assert torch.equal(out[kept], (enc(x) * 2.0)[kept])      # 1 / (1 - 0.5)


def test_argument_errors():
    with pytest.raises(ValueError):
        egc_amd.NodeEncoder([], 8)
    with pytest.raises(ValueError):
        egc_amd.NodeEncoder([4, 0], 8)
    with pytest.raises(ValueError):
        egc_amd.NodeEncoder([4, 5], 8, clamp=[3])
    with pytest.raises(ValueError):
        egc_amd.AtomEncoder(16, dropout=1.0)
    with pytest.raises(ValueError):
        egc_amd.Embedding(0, 4)
    with pytest.raises(ValueError):
        egc_amd.ASTNodeEncoder(8, 10, 10, -1)
    enc = egc_amd.AtomEncoder(8)
    with pytest.raises(ValueError, match=r"\[N, 9\]"):
        enc(torch.zeros(5, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        enc(torch.zeros(5, 9, dtype=torch.int32))
    ast = egc_amd.ASTNodeEncoder(8, 10, 10, 5)
    with pytest.raises(ValueError):
        ast(torch.zeros(5, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))


def test_functional_entry_points_refuse_cpu_tensors():
    from egc_amd import functional as F
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.encoder_forward([torch.zeros(4, 8)], torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.encoder_backward(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64), [4])
    assert not F.encoder_supported([torch.zeros(4, 8)], torch.zeros(3, dtype=torch.int64))


def test_limits_are_the_librarys_own():
    """encoder_supported asks egc_encoder_workspace_bytes: the limits of include/egc_hip.h, which the binding reads from it."""
    from egc_amd import _C
    max_tables, max_width = _C.ENCODER_MAX_TABLES, _C.ENCODER_MAX_WIDTH
    assert _C.ENCODER_MAX_TABLE_ROWS == 1 << 20
    lib = _C.load()
    assert lib.egc_encoder_workspace_bytes(1, max_tables, max_tables, 8) > 0
    assert lib.egc_encoder_workspace_bytes(1, max_tables + 1, max_tables + 1, 8) == 0
    assert lib.egc_encoder_workspace_bytes(1, 1, 4, max_width) > 0
    assert lib.egc_encoder_workspace_bytes(1, 1, 4, max_width + 1) == 0
    assert lib.egc_encoder_workspace_bytes(1, 1, (1 << 20) + 1, 8) == 0


def test_workspace_query_and_limits_on_the_host():
    from egc_amd import _C
    lib = _C.load()
    assert lib.egc_encoder_workspace_bytes(0, 9, 173, 296) == 0
    # molhiv batch of 52,771 nodes: 207 chunks x min(173, 9 * 256) partial rows of 296 floats + the chunk map
    chunks = -(-52771 // 256)
    assert chunks == 207
    assert lib.egc_encoder_workspace_bytes(52771, 9, 173, 296) == chunks * 173 * 296 * 4 + chunks * 173 * 4
    assert lib.egc_encoder_workspace_bytes(1000, 3, 10149, 304) == 4 * 768 * 304 * 4 + 4 * 10149 * 4
    assert lib.egc_encoder_workspace_bytes(1000, 17, 100, 64) == 0       # beyond EGC_ENCODER_MAX_TABLES
    assert lib.egc_encoder_workspace_bytes(-1, 1, 10, 64) == 0
