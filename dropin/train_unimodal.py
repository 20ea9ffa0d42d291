"""`from train_unimodal import train` (reference: train/train_unimodal.py, main_nturgbd.py:32) -> r3d_amd."""
from r3d_amd.train_unimodal import train, validate, get_last_non_padding_labels, weighted_accuracy  # noqa: F401
