"""Training-side pieces of the reference's ``training/`` folder on the HIP path."""
from .loss import (MultitaskLoss, check_and_fix_inf_nan, compute_camera_pose_loss, compute_depth_loss,  # noqa: F401
                   compute_relative_pose_loss, per_chunk_regularization_loss, per_frame_regularization_loss)
