from .spc import SupConLoss  # noqa: F401
