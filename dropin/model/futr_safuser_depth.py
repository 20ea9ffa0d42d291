"""`from model.futr_safuser_depth import FUTR` -> r3d_amd.model.futr_safuser_depth."""
from r3d_amd.model.futr_safuser_depth import FUTR, CMFuser  # noqa: F401
