"""`from train_unsupervised import train` (reference: train/train_unsupervised.py, main_darai.py:40) -> r3d_amd."""
from r3d_amd.train_unsupervised import (train, validate, get_warmup_factor, get_cluster_intervals,  # noqa: F401
                                        weighted_accuracy, get_last_non_padding_labels)
