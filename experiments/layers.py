"""``from experiments.layers import EfficientGraphConv, Mpnn`` -> the gfx950-native drop-ins (egc_amd.layers, egc_amd._mpnn)."""
from egc_amd.layers import EfficientGraphConv, _AggLayer  # noqa: F401
from egc_amd._mpnn import Mpnn  # noqa: F401
