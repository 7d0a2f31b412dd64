"""egc_amd -- the EGC message-passing layer's hot path, native to MI355X (gfx950).

Public surface (mirrors the reference's layer API):
  EfficientGraphConv   drop-in for experiments/layers.py:EfficientGraphConv
  EGConv               drop-in for experiments/optimized_layers.py:EGConv
  REGConv              drop-in for experiments/rmag/models.py:REGConv (relational EGC)
  RGCNConv / REGC      the R-GCN baseline layer of the same file (state-dict compatible; its per-relation mean is one
                       typed-mean launch per node type, forward and backward) and the relational net over both layers
  Mpnn                 drop-in for experiments/layers.py:Mpnn, the baseline MPNN-Sum / -Mean / -Max layer (state-dict compatible):
                       the per-edge message Linear split into two [N, d] projections, aggregated by one gather launch that
                       writes the update's operand; no [E, d] array forward or backward
  GATv2Conv            PyG 2.x GATv2Conv, the attention baseline of the reference's nets (state-dict compatible): lin_l and lin_r as
                       one dense product, the per-destination edge softmax and the weighted gather fused in one launch with
                       an online softmax; the backward recomputes the scores; no [E, .] array forward or backward
  GATConv              PyG GATConv (non-bipartite, no edge features), the GAT baseline of the reference's nets at gat_version=1
                       (state-dict compatible, PyG 2.0 - 2.2 names and the later single lin.weight): xl and the two per-node
                       halves of the additive score as one dense product, the edge softmax and the weighted gather in one
                       launch with no cross-lane work per entry; the backward takes one head sum per row; no [E, .] array
  gat_aggregate / gat_aggregate_lse / gat_aggregate_backward
                       the kernel-level calls under GATConv
  PNAConv              PyG 2.x PNAConv (edge_dim=None, one pre and one post layer), the strongest baseline of the reference's nets
                       (state-dict compatible): the per-edge pre-transform split into two [N, W] projections, every listed
                       aggregator (sum / mean / min / max / var / std) out of one gather launch, the degree scalers moved behind
                       the folded post o lin product and applied by one combine launch; no [E, .] and no [N, S A W] array
  degree_histogram     the in-degree histogram PNAConv's ``deg`` wants, from an edge_index, a SparseTensor or a CSRGraph
  pna_aggregate / pna_aggregate_backward / pna_scale_combine
                       the kernel-level calls under PNAConv
  GCNConv / SAGEConv / GINConv
                       PyG 2.x GCNConv, SAGEConv (mean / sum) and GINConv, the three cheapest baselines of the reference's nets
                       (state-dict compatible), on one neighbour-sum launch: the symmetric normalisation, the mean's division,
                       the self loop / root / (1 + eps) term fused in, forward and backward; no [E, .] array
  neighbor_sum         the kernel-level call under the three: a row-scaled sum of source-scaled neighbour rows plus a
                       multiple of the row's own features (sum / mean / mean_t / sym), differentiable
  FusedEGCBlock        conv -> BatchNorm1d -> ReLU (-> dropout) -> + identity: eval mode in the kernel's store, training
                       mode in two passes each way
  global_mean_pool / global_add_pool / global_max_pool, readout(name)
                       the graph-level readouts of the reference's nets (differentiable segmented mean / sum / max)
  Embedding / AtomEncoder / ASTNodeEncoder, NodeEncoder(table_rows, emb_dim)
                       the node encoders at the head of the reference's batched nets (state-dict compatible): a sum of
                       embedding rows (+ input dropout) in one forward launch and two atomic-free backward launches
  log_softmax / nll_log_softmax / cross_entropy, RowSelection(index, n_rows)
                       the output head and loss of the classification nets on the full-width logits: the row
                       log-softmax (+ arg-max) in one read, and ``F.nll_loss(x[:, :C].log_softmax(-1)[idx], y[idx])`` as
                       one read of the selected rows forward and one read plus one write of the gradient backward
  TokenHead(in_features, num_classes, seq_len), token_head_loss / token_head_argmax
                       the token predictors of the ogbg-code net (state-dict compatible) fused with their loss: the Linear
                       maps, the mean cross-entropy over the positions, the arg-max and the backward without a logits array
  GraphHead(sizes, act, dropout), l1_loss / masked_bce_with_logits
                       the graph-level MLP head of the batched nets (experiments.utils.mlp, state-dict compatible) with
                       the L1 / NaN-masked BCE loss fused into its last launch: one launch per Linear forward (one in all
                       in evaluation), one row pass per Linear and one parameter-gradient launch backward
  SparseTensor         minimal adj_t container (torch_sparse is not required)
  CSRGraph             device CSR + degree statistics + long-row plan
  GraphBatch           a PyG-style batch of small graphs (edge_index + graph offsets) for the tile kernels: the CSR of
                       each tile of whole graphs is built in LDS by the workgroup that aggregates it
  egc_layer_forward    operator-level call into libegc_hip.so
  ops                  the same call as torch.library operators (torch.ops.egc_amd.layer_forward / _train / _backward)
  GraphedStep          a whole training / inference step (graph build included) recorded as one hipGraph
  GraphStore(node_ptr, edge_ptr, edge_index, node_fields, graph_fields)
                       a dataset of small graphs that lives on the device: M graphs back to back, node ids local to their
                       graph, named per-node and per-graph arrays (nothing is copied)
  BatchCollator(store, batch_size, n_pad, e_pad, graph_fill)
                       the input side of a recorded step, in place of PyG's DataLoader + ``batch.to(device)``: owns the static
                       padded buffers of one batch (fields, edge_index, batch, ptr, edge_ptr, n_valid / e_valid / g_valid,
                       counts, graph_mask, inv_g) and fills ALL of them in two launches without host work --
                       ``collate(ids)``, or ``set_epoch(perm)`` + ``next()`` with cursor and permutation read on the device, so
                       that ``next()`` recorded inside a GraphedStep makes one replay the whole iteration; malformed batches
                       are clamped, flagged and named by ``check()``
  Adam(params, lr, betas, eps, weight_decay)
                       drop-in for torch.optim.Adam at the reference's settings (L2 weight decay, no amsgrad; state dicts
                       exchange with torch's): the step of ALL tensors of a parameter group -- parameter, both moments and,
                       with ``step(zero_grad=True)``, the zeroed gradients -- as one launch that records into a GraphedStep;
                       ``lr`` is a device scalar the kernel reads, so a scheduler changes the rate of a recorded step
"""
from .graph import CSRGraph, GraphBatch, SparseTensor, GLOBAL_GRAPH_CACHE  # noqa: F401
from .functional import egc_layer_forward, make_spec, LayerSpec  # noqa: F401
from .layers import EfficientGraphConv  # noqa: F401
from .optimized_layers import EGConv  # noqa: F401
from .relational import REGC, REGConv, RGCNConv  # noqa: F401
from ._mpnn import Mpnn  # noqa: F401
from ._gat import GATConv, GATv2Conv, gat_aggregate, gat_aggregate_backward, gat_aggregate_lse  # noqa: F401
from ._pna import PNAConv, degree_histogram, pna_aggregate, pna_aggregate_backward, pna_scale_combine  # noqa: F401
from ._nbr import GCNConv, GINConv, SAGEConv, neighbor_sum  # noqa: F401
from .fusion import FusedEGCBlock, global_add_pool, global_max_pool, global_mean_pool, readout  # noqa: F401
from .encoders import ASTNodeEncoder, AtomEncoder, Embedding, NodeEncoder  # noqa: F401
from ._softmax import RowSelection, cross_entropy, log_softmax, nll_log_softmax  # noqa: F401
from ._token_head import TokenHead, token_head_argmax, token_head_loss  # noqa: F401
from ._head import GraphHead, l1_loss, masked_bce_with_logits  # noqa: F401
from .hipgraph import GraphedStep  # noqa: F401
from ._collate import EGC_COLLATE_MAX_FIELDS, BatchCollator, GraphStore  # noqa: F401
from .optim import Adam  # noqa: F401
from . import ops  # noqa: F401  (registers torch.ops.egc_amd.*)

__version__ = "0.1.0"
