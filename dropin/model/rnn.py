"""`from model.rnn import FUTR` (reference: model/rnn.py, main_nturgbd.py:20) -> r3d_amd.model.rnn."""
from r3d_amd.model.rnn import FUTR  # noqa: F401
