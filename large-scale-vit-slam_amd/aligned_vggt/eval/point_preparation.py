"""The middle of the reference's test-mode reconstruction protocol:
``Metrics.prepare_data_for_metrics`` (training/training_metrics.py:219-369),
which turns a sequence's dense outputs into the two clouds ICP receives --
unproject the depth maps, threshold the confidences at a global quantile,
search an image-space subsampling factor that brings the GT cloud under
``max_points_icp``, subsample points and masks bilinearly, compact the selected
pixels in row-major order.

The reference does this on host memory with ``torch.kthvalue``, a homogeneous
point tensor, up to ~18 full-image ``F.interpolate`` calls and boolean
indexing.  Here the data stays on the device and three HIP entry points
(csrc/points.hip) do the work: ``vggt_kth_value_f32`` (the quantile, never read
back), ``vggt_subsample_mask_count`` (one launch and one 8-byte readback per
step of the factor search) and ``vggt_prepare_clouds`` (select, unproject the
selected taps, compact).  There is no CPU path: tensors on the CPU raise
``RuntimeError`` like every other binding.  The ``F.interpolate`` and
``kthvalue`` semantics restated are listed in SPEC_ASSUMPTIONS.md.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import torch

from .. import _native
from ..utils.data import pose_encoding_to_extri
from ..utils.geometry import closed_form_inverse_se3
from ..utils.pose_enc import pose_encoding_to_extri_intri
from .reconstruction_metrics import iterative_closest_point
from .trajectory_metrics import poses_c2w_from_predictions


def quantile_rank(n: int, q: float, interpolation: str = "nearest") -> int:
    """The 1-based rank ``torch_quantile`` (training_metrics.py:663-723) hands to
    ``torch.kthvalue``: ``round(q * (n - 1)) + 1`` with Python's ``round``
    (halves go to the even neighbour), floor / ceil for "lower" / "higher"."""
    try:
        q = float(q)
        assert 0 <= q <= 1
    except Exception:
        raise ValueError(f"Only scalar input 0<=q<=1 is currently supported (got {q})!")
    if n < 1:
        raise ValueError("quantile_rank: empty input")
    inter = {"nearest": round, "lower": math.floor, "higher": math.ceil}.get(interpolation)
    if inter is None:
        raise ValueError(f"Supported interpolations currently are {{'nearest', 'lower', 'higher'}} "
                         f"(got '{interpolation}')!")
    return int(inter(q * (n - 1))) + 1


def quantile(x: torch.Tensor, q: float, interpolation: str = "nearest") -> torch.Tensor:
    """``torch_quantile(x, q)`` over all elements of the fp32 device tensor ``x``:
    a 0-dim device tensor, written by ``vggt_kth_value_f32`` without a host
    synchronisation."""
    if not x.is_cuda:
        raise RuntimeError(f"quantile: tensor on {x.device}; the MI355X hot path runs on HIP devices only")
    return _native.kth_value(x.float(), quantile_rank(x.numel(), q, interpolation))


def search_subsample_factor(count_fn: Callable[[int], int], valid_points: int, max_points: int, H: int,
                            W: int) -> Tuple[int, int]:
    """The subsampling-factor search of training_metrics.py:281-320, decision for
    decision.  ``count_fn(f)`` is the number of valid GT pixels after a bilinear
    subsample to ``(H // f, W // f)``; ``valid_points`` the full-resolution count.
    First guess ``ceil(sqrt(valid / max))``, doubled until the count fits or the
    factor passes ``max(H, W)``, then a binary search between the last failing and
    the first passing factor.  Returns ``(factor, valid_points)``; ``(1,
    valid_points)`` when nothing needs subsampling (the reference does not enter
    the search then).  Raises ``ValueError`` where the reference would ask
    ``F.interpolate`` for an empty output (``H // f == 0`` or ``W // f == 0``)."""
    if not max_points or valid_points <= max_points:
        return 1, valid_points

    def count(f: int) -> int:
        if H // f == 0 or W // f == 0:
            raise ValueError(f"search_subsample_factor: factor {f} gives an empty ({H // f}, {W // f}) grid from "
                             f"({H}, {W}); the reference's F.interpolate fails here")
        return int(count_fn(f))

    factor = math.ceil(math.sqrt(valid_points / max_points))
    last = 0
    while valid_points > max_points:
        if last > 0:
            last = factor
            factor = factor * 2
        else:
            last = factor
        if factor > max(H, W):
            break
        valid_points = count(factor)
    if last != factor:
        while last + 1 < factor:
            mid = (last + factor) // 2
            v = count(mid)
            if v <= max_points:
                factor, valid_points = mid, v
            else:
                last = mid
    if H // factor == 0 or W // factor == 0:
        raise ValueError(f"search_subsample_factor: the search ends at factor {factor}, an empty "
                         f"({H // factor}, {W // factor}) grid from ({H}, {W}); the reference's F.interpolate fails here")
    return factor, valid_points


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def masked_clouds(pred_dict: dict, gt_dict: dict, pred_extr: Optional[torch.Tensor],
                  pred_intr: Optional[torch.Tensor], valid_point_quantile: float = 0.25,
                  max_points_icp: Optional[int] = None):
    """The clouds training_metrics.py:264-355 hands to ICP, padded:
    ``(pred_cloud (B, Np, 3), pred_len (B,), gt_cloud (B, Ng, 3), gt_len (B,),
    factor)`` with ``Np`` / ``Ng`` the largest length in the batch and the
    lengths int64 on the device.

    ``pred_dict``: ``depth`` (B, S, H, W[, 1]) with ``depth_conf`` -- preferred,
    unprojected with ``pred_extr`` (B, S, 3, 4) w2c and ``pred_intr`` (B, S, 3, 3)
    -- or ``world_points`` (B, S, H, W, 3) with ``world_points_conf``.
    ``gt_dict``: ``world_points`` and ``point_masks`` (B, S, H, W) bool.  The
    host sees one 8-byte count per step of the factor search and the 2 B lengths
    that size the outputs; the confidence threshold stays on the device."""
    gt_points = gt_dict["world_points"]
    gt_mask = gt_dict["point_masks"]
    for t in (gt_points, gt_mask):
        if not t.is_cuda:
            raise RuntimeError(f"masked_clouds: tensor on {t.device}; the MI355X hot path runs on HIP devices only")
    B, S, H, W, _ = gt_points.shape
    dev = gt_points.device
    depth = kinv = c2w = point_map = None
    if "depth" in pred_dict:
        depth = _f32(pred_dict["depth"]).reshape(B, S, H, W)
        conf = pred_dict["depth_conf"]
        kinv = _f32(torch.inverse(pred_intr.float().to(dev))).reshape(B, S, 3, 3)
        c2w = closed_form_inverse_se3(pred_extr.float().to(dev).reshape(B * S, 3, 4))[:, :3, :]
        c2w = c2w.reshape(B, S, 3, 4).contiguous()
    else:
        point_map = _f32(pred_dict["world_points"]).reshape(B, S, H, W, 3)
        conf = pred_dict["world_points_conf"]
    if not conf.is_cuda:
        raise RuntimeError(f"masked_clouds: tensor on {conf.device}; the MI355X hot path runs on HIP devices only")
    conf = _f32(conf).reshape(B, S, H, W)
    gt_points = _f32(gt_points)
    gt_mask = gt_mask.detach().bool().contiguous()

    thr = quantile(conf, valid_point_quantile)

    factor = 1
    if max_points_icp:
        count = torch.empty((), device=dev, dtype=torch.int64)
        valid = int(_native.subsample_mask_count(gt_mask, H, W, out=count).item())
        factor, _ = search_subsample_factor(
            lambda f: int(_native.subsample_mask_count(gt_mask, H // f, W // f, out=count).item()), valid,
            max_points_icp, H, W)  # factor 1 (nothing to subsample) is the reference's unsubsampled branch
    Ho, Wo = H // factor, W // factor

    args = (depth, kinv, c2w, point_map, conf, thr, gt_points, gt_mask, Ho, Wo)
    pred_len, gt_len, ws = _native.prepare_clouds(*args, phase=_native.PREPARE_COUNT)
    lens = torch.stack([pred_len, gt_len]).cpu()
    pred_cloud = torch.zeros(B, int(lens[0].max()), 3, device=dev, dtype=torch.float32)
    gt_cloud = torch.zeros(B, int(lens[1].max()), 3, device=dev, dtype=torch.float32)
    _native.prepare_clouds(*args, pred_cloud=pred_cloud, gt_cloud=gt_cloud, pred_len=pred_len, gt_len=gt_len,
                           phase=_native.PREPARE_SCATTER, ws=ws)
    return pred_cloud, pred_len, gt_cloud, gt_len, factor


def prepare_data_for_metrics(pred_dict: dict, gt_dict: dict, valid_point_quantile: float = 0.25,
                             max_points_icp: Optional[int] = None, device=None, poses: bool = True,
                             points: bool = True):
    """``Metrics.prepare_data_for_metrics`` (training_metrics.py:219-369): returns
    ``(pred_poses, gt_poses, pred_points, gt_points)`` -- 4x4 c2w poses
    (B, S, 4, 4) and, per batch element, the ICP-aligned predicted cloud and the
    GT cloud as lists of (N_i, 3) tensors; the halves not asked for (``poses`` /
    ``points``, the reference's "are there trajectory / reconstruction metrics")
    or not available (no ``depth`` or ``world_points`` predicted) are ``None``.
    A 9-wide ``pose_enc`` carries its own intrinsics; a 7-wide one takes the GT
    intrinsics, as the reference does."""
    pose_enc = pred_dict["pose_enc"]
    for t in (pose_enc, gt_dict["extrinsics"]):
        if not t.is_cuda:
            raise RuntimeError(f"prepare_data_for_metrics: tensor on {t.device}; the MI355X hot path runs on HIP "
                               f"devices only")
    points = points and ("world_points" in pred_dict or "depth" in pred_dict)
    image_hw = gt_dict["images"].shape[-2:] if "images" in gt_dict else gt_dict["world_points"].shape[2:4]
    B, S = gt_dict["extrinsics"].shape[:2]
    if pose_enc.shape[-1] == 9:
        pred_extr, pred_intr = pose_encoding_to_extri_intri(pose_enc.float(), image_size_hw=image_hw)
        pred_poses, gt_poses = poses_c2w_from_predictions(pose_enc, gt_dict["extrinsics"], image_hw, device)
    elif pose_enc.shape[-1] == 7:
        pred_extr = pose_encoding_to_extri(pose_enc.float())[:, :, :3, :4]
        pred_intr = gt_dict["intrinsics"]  # the reference uses the GT intrinsics here
        pred_poses = closed_form_inverse_se3(pred_extr.reshape(B * S, 3, 4)).reshape(B, S, 4, 4)
        gt_poses = closed_form_inverse_se3(gt_dict["extrinsics"].float().reshape(B * S, 3, 4)).reshape(B, S, 4, 4)
        if device is not None:
            pred_poses, gt_poses = pred_poses.to(device), gt_poses.to(device)
    else:
        raise ValueError("Unkown pose enc type")
    if not poses:
        pred_poses = gt_poses = None
    if not points:
        return pred_poses, gt_poses, None, None

    pred_cloud, pred_len, gt_cloud, gt_len, _ = masked_clouds(pred_dict, gt_dict, pred_extr, pred_intr,
                                                              valid_point_quantile, max_points_icp)
    sol = iterative_closest_point(pred_cloud, gt_cloud, max_iterations=30, X_lengths=pred_len, Y_lengths=gt_len)
    lens = torch.stack([pred_len, gt_len]).cpu()
    pred_points: List[torch.Tensor] = [sol.Xt[b, : int(lens[0, b])] for b in range(B)]
    gt_points: List[torch.Tensor] = [gt_cloud[b, : int(lens[1, b])] for b in range(B)]
    if device is not None:
        pred_points = [p.to(device) for p in pred_points]
        gt_points = [p.to(device) for p in gt_points]
    return pred_poses, gt_poses, pred_points, gt_points
