"""``from model.afft import FUTR`` (the import main_darai.py keeps commented out) -> the HIP-backed AFFT baseline."""
from r3d_amd.model.afft import CMFuser, FUTR  # noqa: F401
