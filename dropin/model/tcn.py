"""`from model.tcn import MustafaNet1DTCN` (reference: model/tcn.py, main.py:19-25) -> r3d_amd.model.tcn."""
from r3d_amd.model.tcn import Chomp1d, TemporalBlock1D, TemporalConvNet1D, MustafaNet1DTCN  # noqa: F401
