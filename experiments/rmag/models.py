"""Import-path shim: ``from experiments.rmag.models import REGConv, RGCNConv, REGC`` resolves to the gfx950 drop-ins
(reference experiments/rmag/models.py:32-72, 75-148, 151-212): the relational EGC layer, the R-GCN baseline layer and the
net over both, with the reference's parameter names."""
from egc_amd.relational import EDGE_TYPES, NODE_TYPES, REGC, REGConv, RGCNConv  # noqa: F401
