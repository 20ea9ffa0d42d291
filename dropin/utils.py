"""`from utils import read_mapping_dict` (reference: utils.py:325-356, main_darai.py:16) -> r3d_amd.utils; the temporal
auxiliary losses of utils.py (:229-321, :394, :493; train/train_unsupervised.py:7) -> r3d_amd.loss.temporal."""
from r3d_amd.utils import read_mapping_dict, normalize_duration, eval_file  # noqa: F401
from r3d_amd.loss.temporal import (temporal_cluster_loss, temporal_contrastive_loss, focal_loss,  # noqa: F401
                                   cal_performance_focal)
