"""`from train_tcn import train` (reference: train/train_tcn.py, main.py:101) -> r3d_amd."""
from r3d_amd.train_tcn import train, validate  # noqa: F401
