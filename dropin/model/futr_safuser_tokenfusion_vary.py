"""`from model.futr_safuser_tokenfusion_vary import FUTR` -> r3d_amd.model.futr_safuser_tokenfusion_vary."""
from r3d_amd.model.futr_safuser_tokenfusion_vary import FUTR, CMFuser  # noqa: F401
