"""Evaluation (eval/trajectory_metrics.py and eval/reconstruction_metrics.py of the reference) without
torchmetrics and pytorch3d."""
from .trajectory_metrics import (AbsoluteTrajectoryError, RelativePoseError, ScaleConsistency,  # noqa: F401
                                 poses_c2w_from_predictions)
from .reconstruction_metrics import (ChamferDistanceMetrics, ICPSolution, iterative_closest_point,  # noqa: F401
                                     nearest_neighbors)
from .point_preparation import (masked_clouds, prepare_data_for_metrics, quantile, quantile_rank,  # noqa: F401
                                search_subsample_factor)
