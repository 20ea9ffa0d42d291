"""`from loss.spc import SupConLoss` (reference: loss/spc.py, main_nturgbd.py:15) -> r3d_amd.loss.spc."""
from r3d_amd.loss.spc import SupConLoss  # noqa: F401
