"""`from model.futr_unsupervised_temp3 import FUTR` (reference: model/futr_unsupervised_temp3.py, the commented line of main_darai.py:36) -> r3d_amd."""
from r3d_amd.model.futr_unsupervised_temp3 import FUTR  # noqa: F401
