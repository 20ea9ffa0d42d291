"""`from model.cnn import FUTR` (reference: model/cnn.py, main_nturgbd.py:19) -> r3d_amd.model.cnn."""
from r3d_amd.model.cnn import FUTR  # noqa: F401
