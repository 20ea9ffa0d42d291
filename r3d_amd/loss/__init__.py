from .spc import SupConLoss  # noqa: F401
from .temporal import (Runs, label_runs, runs_from_intervals, get_cluster_intervals, temporal_cluster_loss,  # noqa: F401
                       temporal_contrastive_loss, focal_loss, cal_performance_focal)
