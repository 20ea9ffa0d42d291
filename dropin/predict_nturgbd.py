"""`from predict_nturgbd import predict` (reference: evaluation/predict_nturgbd.py, main_nturgbd.py:40) -> r3d_amd.predict."""
from r3d_amd.predict import predict_nturgbd as predict  # noqa: F401
