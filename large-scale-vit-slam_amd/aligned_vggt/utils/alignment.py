"""Sim(3) / scale alignment utilities (aligned_vggt/utils/alignment.py).

Two kinds of callers:
  * the point-aligned model (pointAligned_wrapped_vggt.py) applies Sim(3)
    transforms to dense point maps / poses every chunk -- the dense part runs
    in the HIP kernel ``vggt_sim3_points`` (device tensors only);
  * GT-based evaluation post-processing (``alignAndConvertOutputs``,
    data.py:108-153): closed-form Umeyama / Horn and the L1/LSE scale
    alignments -- host-side numpy/torch exactly as the reference (small,
    once per sequence), pinned by tests/golden/{alignment_utils,
    scale_alignment}.npz;
  * a training step with ``gt_alignment_type: scale_from_depths`` runs
    ``scale_align_from_depths`` on the step's device tensors, between the model
    and the loss: there the weighted median is the HIP kernel
    ``vggt_depth_scale_l1`` (csrc/gt_align.hip) and nothing visits the host;
  * the five pose-based GT alignments (``scale_from_poses``, ``scale_from_fc_poses``,
    ``per_frame_scale_from_poses``, ``per_chunk_scale_from_poses``,
    ``sim3_from_poses``) take the kernel ``vggt_gt_pose_align`` (csrc/pose.hip)
    when the pose encoding and the GT extrinsics are fp32 tensors on one HIP
    device: the scale / transform stays on the device and nothing synchronises.
    Host tensors, other dtypes and VGGT_GT_ALIGN=torch run the reference's host
    code;
  * ``sim3_from_points`` (``umeyama_alignment_from_points``) takes the kernel
    ``vggt_gt_points_align`` (csrc/gt_points.hip) when its four arguments are
    tensors on one HIP device, fp32 with a bool or uint8 mask: numpy's fp32
    percentile by radix select, the selection compacted in boolean indexing's
    order, and Umeyama's closed form in fp64, with transform and scale left on
    the device.  The reference's ``reshape(3, -1)`` of the (n, 3) selection
    interleaves coordinates (it is not the transpose); the kernel reads the
    compacted rows that way too (``columns="reference"``), and
    ``columns="points"`` is the per-point fit.  Arrays, host tensors, other
    dtypes, mixed placements and VGGT_GT_ALIGN=torch run the reference's numpy
    code.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .geometry import closed_form_inverse_se3
from .pose_enc import extri_intri_to_pose_encoding, pose_encoding_to_extri_intri


def umeyama(x: np.ndarray, y: np.ndarray) -> tuple:
    """alignment.py:6-59: Sim(m) least squares x -> y (3xn each); returns r, t, c."""
    if x.shape != y.shape:
        raise AssertionError("x shape not equal to y shape")
    m, n = x.shape
    mean_x = x.mean(axis=1)
    mean_y = y.mean(axis=1)
    sigma_x = 1.0 / n * (np.linalg.norm(x - mean_x[:, None]) ** 2)
    cov_xy = (y - mean_y[:, None]) @ (x - mean_x[:, None]).T / n
    u, d, v = np.linalg.svd(cov_xy)
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[m - 1, m - 1] = -1
    r = u.dot(s).dot(v)
    c = 1 / sigma_x * np.trace(np.diag(d).dot(s))
    t = mean_y - c * r.dot(mean_x)
    return r, t, c


def methodOfHorn(model: np.ndarray, data: np.ndarray, align_scale: bool = True) -> tuple:
    """alignment.py:61-111 (Horn closed form, evaluate_ate_scale convention)."""
    if model.shape != data.shape:
        raise AssertionError("model shape not equal to data shape")
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    Wm = mz @ dz.T
    U, d, Vh = np.linalg.svd(Wm.T)
    S = np.identity(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    if align_scale:
        rotmodel = rot @ mz
        s = float((dz * rotmodel).sum() / (mz ** 2).sum())
    else:
        s = 1.0
    trans = data.mean(1) - s * rot @ model.mean(1)
    return rot, trans, np.asarray(s)


def scale_lse_solver(x: np.ndarray, y: np.ndarray) -> float:
    """alignment.py:113-129."""
    if x.shape != y.shape:
        raise AssertionError("x shape not equal to y shape")
    return np.abs(np.sum(x * y) / np.sum(x ** 2))


def per_frame_scale_alignment_from_poses(predictions: dict, batch: dict) -> None:
    """alignment.py:131-165 (note: ``alignment_scales`` keeps the last batch
    element's per-frame list, as the reference does)."""
    if _pose_align_kernel_applies(predictions["pose_enc"], batch["extrinsics"]):
        return _per_frame_scale_alignment_from_poses_device(predictions, batch)
    B, S = batch["extrinsics"].shape[:2]
    gt_positions = batch["extrinsics"][..., :3, 3].detach().cpu().numpy()
    pred_positions = predictions["pose_enc"][..., :3].detach().cpu().numpy()
    frame_scales = []
    for b in range(B):
        frame_scales = []
        for s in range(S):
            frame_scale = 1.0 if s == 0 else scale_lse_solver(pred_positions[b, s], gt_positions[b, s])
            predictions["pose_enc"][b, s, :3] *= frame_scale
            frame_scales.append(frame_scale)
            if "depth" in predictions:
                predictions["depth"][b, s] *= frame_scale
            if "world_points" in predictions:
                predictions["world_points"][b, s] *= frame_scale
    predictions["alignment_scales"] = frame_scales


def per_chunk_scale_alignment_from_poses(predictions: dict, batch: dict) -> None:
    """alignment.py:167-204 (chunked lists)."""
    if all(_pose_align_kernel_applies(p, e) for p, e in zip(predictions["pose_enc"], batch["extrinsics"])):
        return _per_chunk_scale_alignment_from_poses_device(predictions, batch)
    C = len(batch["extrinsics"])
    B = batch["extrinsics"][0].shape[0]
    chunk_scales = []
    for c in range(C):
        gt = batch["extrinsics"][c][..., :3, 3].detach().cpu().numpy()
        pred = predictions["pose_enc"][c][..., :3].detach().cpu().numpy()
        scales = []
        for b in range(B):
            sc = scale_lse_solver(pred[b], gt[b])
            predictions["pose_enc"][c][b, :, :3] *= sc
            scales.append(sc)
            if b == B - 1:
                chunk_scales.append(torch.tensor(scales))
            if "depth" in predictions:
                predictions["depth"][c][b, ...] *= sc
            if "world_points" in predictions:
                predictions["world_points"][c][b, ...] *= sc
    predictions["alignment_scales_per_chunk"] = chunk_scales


def scale_alignment_from_poses(predictions: dict, batch: dict, seq_width: int = -1) -> None:
    """alignment.py:206-242."""
    if _pose_align_kernel_applies(predictions["pose_enc"], batch["extrinsics"]):
        return _scale_alignment_from_poses_device(predictions, batch, seq_width)
    B = batch["extrinsics"].shape[0]
    if seq_width == -1:
        seq_width = batch["extrinsics"].shape[1]
    gt = batch["extrinsics"][:, :seq_width, :3, 3].detach().cpu().numpy()
    pred = predictions["pose_enc"][:, :seq_width, :3].detach().cpu().numpy()
    scales = []
    for b in range(B):
        sc = scale_lse_solver(pred[b], gt[b])
        predictions["pose_enc"][b, :, :3] *= sc
        scales.append(sc)
        if "depth" in predictions:
            predictions["depth"][b, ...] *= sc
        if "world_points" in predictions:
            predictions["world_points"][b, ...] *= sc
    predictions["alignment_scales"] = scales


def _pose_align_kernel_applies(pose_enc, extrinsics) -> bool:
    """Pose encoding and GT extrinsics fp32 on one HIP device; VGGT_GT_ALIGN=torch (read
    per call) keeps the host code."""
    if os.environ.get("VGGT_GT_ALIGN", "") == "torch":
        return False
    return (torch.is_tensor(pose_enc) and torch.is_tensor(extrinsics) and pose_enc.is_cuda
            and extrinsics.device == pose_enc.device and pose_enc.dtype == torch.float32
            and extrinsics.dtype == torch.float32)


def _pose_align_launch(pose_enc, extrinsics, mode, seq_width=-1, image_hw=None):
    """vggt_gt_pose_align on detached contiguous views: (scales, transform, pose_enc_out)."""
    from .. import _native
    with torch.no_grad():
        return _native.gt_pose_align(pose_enc.detach().contiguous(), extrinsics.detach()[..., :3, :].contiguous(),
                                     mode, seq_width, image_hw)


def _scale_alignment_from_poses_device(predictions: dict, batch: dict, seq_width: int) -> None:
    """The kernel route of scale_alignment_from_poses: the LSE scale from device memory,
    no host synchronisation; ``alignment_scales`` is a list of 0-dim device tensors."""
    from .. import _native
    S = batch["extrinsics"].shape[1]
    W = -1 if seq_width == -1 else min(int(seq_width), S)  # a slice past the end stops at S
    scales, _, _ = _pose_align_launch(predictions["pose_enc"], batch["extrinsics"], _native.GT_POSE_SCALE, W)
    predictions["pose_enc"][..., :3] *= scales[:, None, None]  # torch's in-place multiply: autograd records it
    if "depth" in predictions:
        _scale_batch_(predictions["depth"], scales)
    if "world_points" in predictions:
        _scale_batch_(predictions["world_points"], scales)
    predictions["alignment_scales"] = list(scales.unbind(0))


def _per_frame_scale_alignment_from_poses_device(predictions: dict, batch: dict) -> None:
    """The kernel route of per_frame_scale_alignment_from_poses; dense tensors are scaled
    as B * S blocks.  ``alignment_scales``: the last batch element's S values, as the
    reference keeps them, here 0-dim device tensors."""
    from .. import _native
    B, S = batch["extrinsics"].shape[:2]
    scales, _, _ = _pose_align_launch(predictions["pose_enc"], batch["extrinsics"], _native.GT_POSE_PER_FRAME)
    predictions["pose_enc"][..., :3] *= scales[:, :, None]
    for key in ("depth", "world_points"):
        if key in predictions:
            t = predictions[key]
            if t.is_contiguous():
                _scale_batch_(t.view(B * S, *t.shape[2:]), scales.view(B * S))
            else:
                t *= scales.view(B, S, *([1] * (t.dim() - 2)))
    predictions["alignment_scales"] = list(scales[-1].unbind(0))


def _per_chunk_scale_alignment_from_poses_device(predictions: dict, batch: dict) -> None:
    """The kernel route of per_chunk_scale_alignment_from_poses: one launch per chunk;
    ``alignment_scales_per_chunk`` is a list of (B,) device tensors."""
    from .. import _native
    chunk_scales = []
    for c in range(len(batch["extrinsics"])):
        scales, _, _ = _pose_align_launch(predictions["pose_enc"][c], batch["extrinsics"][c], _native.GT_POSE_SCALE)
        predictions["pose_enc"][c][..., :3] *= scales[:, None, None]
        if "depth" in predictions:
            _scale_batch_(predictions["depth"][c], scales)
        if "world_points" in predictions:
            _scale_batch_(predictions["world_points"][c], scales)
        chunk_scales.append(scales)
    predictions["alignment_scales_per_chunk"] = chunk_scales


def _gt_align_kernel_applies(d_pred, conf, d_gt, mask) -> bool:
    """All four on the device, fp32 values and a bool mask; VGGT_GT_ALIGN=torch (read
    per call) keeps the torch chain."""
    if os.environ.get("VGGT_GT_ALIGN", "") == "torch":
        return False
    return (all(t.is_cuda for t in (d_pred, conf, d_gt, mask)) and d_pred.dtype == torch.float32
            and conf.dtype == torch.float32 and d_gt.dtype == torch.float32 and mask.dtype == torch.bool)


def _scale_batch_(t: torch.Tensor, scales: torch.Tensor) -> None:
    """t[b] *= scales[b] in place.  The scale is a constant of the graph: a tensor
    autograd tracks takes torch's in-place multiply, which it records; any other
    fp32 tensor with contiguous per-batch blocks takes vggt_scale_f32.  That kernel
    writes through the raw pointer and does not bump the tensor's version counter:
    a tensor without requires_grad that another op saved for its backward would
    change without autograd noticing (the step's outputs here are not saved so)."""
    if ((t.requires_grad and torch.is_grad_enabled()) or t.dtype != torch.float32 or not t[0].is_contiguous()
            or not t.is_cuda):
        t *= scales.view(-1, *([1] * (t.dim() - 1)))
    else:
        from .. import _native
        _native.scale_(t, scales)


def _scale_align_from_depths_device(predictions: dict, batch: dict) -> None:
    """The kernel path (csrc/gt_align.hip): the weighted median by radix select on
    the device, the scale applied from device memory; no host synchronisation."""
    from .. import _native
    d_pred = predictions["depth"]
    B, S, H, W, _ = d_pred.shape
    N = S * H * W
    with torch.no_grad():
        flat = [t.detach().reshape(B, N).contiguous() for t in
                (d_pred, predictions["depth_conf"], batch["depths"], batch["point_masks"])]
        scales, _state = _native.depth_scale_l1(*flat)
    # outside no_grad, as the reference's in-place multiplies (:315-321): autograd sees them
    _scale_batch_(predictions["depth"], scales)
    if "world_points" in predictions:
        _scale_batch_(predictions["world_points"], scales)
    if "pose_enc" in predictions:
        predictions["pose_enc"][..., :3] *= scales[:, None, None]
    predictions["alignment_scales"] = list(scales.unbind(0))


def scale_align_from_depths(predictions: dict, batch: dict) -> None:
    """alignment.py:244-323: per-batch weighted-median (L1-optimal) depth scale.
    Device fp32 tensors take the kernel path (``alignment_scales`` is then a list of
    0-dim device tensors and nothing visits the host); host tensors, other dtypes,
    mixed placements and VGGT_GT_ALIGN=torch take the torch chain."""
    if _gt_align_kernel_applies(predictions["depth"], predictions["depth_conf"], batch["depths"],
                                batch["point_masks"]):
        return _scale_align_from_depths_device(predictions, batch)
    return _scale_align_from_depths_torch(predictions, batch)


@torch.no_grad()
def _scale_align_from_depths_torch(predictions: dict, batch: dict) -> None:
    """The reference's chain of torch ops, on whatever device the tensors are."""
    d_pred, conf, d_gt, mask = predictions["depth"], predictions["depth_conf"], batch["depths"], batch["point_masks"]
    B, S, H, W, _ = d_pred.shape
    N = S * H * W
    x = d_pred.reshape(B, N).float()
    y = d_gt.reshape(B, N).float()
    m = mask.reshape(B, N).float()
    w_conf = conf.reshape(B, N).float()
    sum_valid = m.sum(dim=-1, keepdim=True).clamp_min(1.0)
    mean_depth = (y * m).sum(dim=-1, keepdim=True) / sum_valid
    y_clamped = torch.max(y, 0.1 * mean_depth)
    w = m * w_conf * (1.0 / y_clamped.clamp_min(1e-6))
    sign = torch.sign(x)
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    x_pos, y_pos = x * sign, y * sign
    r = y_pos / x_pos.clamp_min(1e-6)
    w_eff = w * x_pos
    r_sorted, idx = torch.sort(r, dim=-1)
    cumsum = torch.gather(w_eff, -1, idx).cumsum(-1)
    idx_med = torch.searchsorted(cumsum, 0.5 * cumsum[:, -1:], side="left").clamp(max=N - 1)
    scales = torch.gather(r_sorted, -1, idx_med).squeeze(-1)
    scales[scales <= 0] *= -1
    predictions["depth"] *= scales[:, None, None, None, None]
    if "world_points" in predictions:
        predictions["world_points"] *= scales[:, None, None, None, None]
    if "pose_enc" in predictions:
        predictions["pose_enc"][..., :3] *= scales[:, None, None]
    predictions["alignment_scales"] = [scales[b].item() for b in range(B)]


def apply_sim3_alignment_on_point_maps(point_maps: torch.Tensor, alignment_transforms: torch.Tensor,
                                       alignment_scales: torch.Tensor) -> torch.Tensor:
    """alignment.py:491-526 -> (B,S,H,W,3): T[:3,:3] (s p) + T[:3,3].  Device
    tensors go through the HIP kernel; host tensors (evaluation on offloaded
    outputs) through the same arithmetic in torch."""
    if point_maps.dim() == 4:
        point_maps, alignment_transforms, alignment_scales = (point_maps[None], alignment_transforms[None],
                                                              alignment_scales.reshape(1))
    assert point_maps.shape[0] == alignment_transforms.shape[0] == alignment_scales.shape[0], \
        "Inputs must have matching batch dimension"
    B = point_maps.shape[0]
    T = alignment_transforms.float()
    sc = torch.as_tensor(alignment_scales, dtype=torch.float32, device=point_maps.device).reshape(B)
    if point_maps.is_cuda:
        from .. import _native
        return _native.sim3_points(point_maps.float().contiguous(), T, sc)
    p = point_maps.float() * sc.view(B, 1, 1, 1, 1)
    out = p.reshape(B, -1, 3) @ T[:, :3, :3].transpose(-1, -2) + T[:, None, :3, 3]
    return out.view(point_maps.shape)


def apply_sim3_alignment_on_c2w(poses: torch.Tensor, alignment_transform: torch.Tensor,
                                alignment_scales: torch.Tensor) -> torch.Tensor:
    """alignment.py:558-594 (scale the translation -- in place on a 4x4 input,
    as the reference -- then left-multiply T)."""
    if poses.dim() == 3:
        poses, alignment_transform, alignment_scales = poses[None], alignment_transform[None], \
            torch.as_tensor(alignment_scales).reshape(1)
    B, S = poses.shape[:2]
    if poses.shape[-2] != 4:
        poses = torch.nn.functional.pad(poses, (0, 0, 0, 1, 0, 0), mode="constant")
        poses[:, 3, 3] = 1.0  # (sic) reference indexing, alignment.py:585
    sc = torch.as_tensor(alignment_scales, dtype=poses.dtype, device=poses.device).view(B, 1, 1)
    poses[:, :, :3, 3] = poses[:, :, :3, 3] * sc
    return torch.matmul(alignment_transform.to(poses).unsqueeze(1).expand(-1, S, -1, -1), poses)


def apply_sim3_alignment_on_w2c(extr: torch.Tensor, alignment_transform: torch.Tensor,
                                alignment_scales: torch.Tensor) -> torch.Tensor:
    """alignment.py:528-556: w2c -> c2w -> Sim(3) -> w2c (B,S,4,4)."""
    if extr.dim() == 3:
        extr, alignment_transform, alignment_scales = extr[None], alignment_transform[None], \
            torch.as_tensor(alignment_scales).reshape(1)
    B, S = extr.shape[:2]
    poses = closed_form_inverse_se3(extr.reshape(B * S, *extr.shape[-2:])).reshape(B, S, 4, 4)
    poses = apply_sim3_alignment_on_c2w(poses, alignment_transform, alignment_scales)
    return closed_form_inverse_se3(poses.reshape(B * S, 4, 4)).reshape(B, S, 4, 4)


def apply_sim3_alignment(alignment_transforms, alignment_scales, pose_encodings, images_size, points=None,
                         depths=None) -> tuple:
    """alignment.py:449-489.  Transforms and scales may be arrays (the reference's) or
    tensors, which stay where they are when that is the encodings' device."""
    B = alignment_transforms.shape[0]
    dev = pose_encodings.device

    def f32(a):
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=torch.float32)
        return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
    sc = f32(alignment_scales)
    T = f32(alignment_transforms)
    extr, intr = pose_encoding_to_extri_intri(pose_encodings, images_size)
    extr = apply_sim3_alignment_on_w2c(extr, T, sc)
    pose_encodings = extri_intri_to_pose_encoding(extr, intr, images_size)
    if points is not None:
        points = apply_sim3_alignment_on_point_maps(points, T, sc)
    if depths is not None:
        depths *= sc.view(B, 1, 1, 1, 1)
    return pose_encodings, points, depths


def apply_sim3_alignment_on_dict(pred: dict, images_size: tuple, alignment_poses, alignment_scales) -> None:
    """alignment.py:428-447."""
    pe, pts, d = apply_sim3_alignment(alignment_poses, alignment_scales, pred["pose_enc"], images_size,
                                      pred.get("world_points"), pred.get("depth"))
    pred["pose_enc"] = pe
    if "world_points" in pred:
        pred["world_points"] = pts
    if "depth" in pred:
        pred["depth"] = d


def umeyama_alignment_from_poses(predictions: dict, batch: dict, seq_width: int) -> None:
    """alignment.py:325-370: Sim(3) of predicted to GT camera centres."""
    if _pose_align_kernel_applies(predictions["pose_enc"], batch["extrinsics"]):
        return _umeyama_alignment_from_poses_device(predictions, batch, seq_width)
    B = batch["extrinsics"].shape[0]
    gt_poses = closed_form_inverse_se3(batch["extrinsics"][:, :seq_width].reshape(B * seq_width, 3, 4)).reshape(
        B, seq_width, 4, 4).detach().cpu().numpy()
    gt_positions = gt_poses[..., :3, 3]
    pred_extr, _ = pose_encoding_to_extri_intri(predictions["pose_enc"][:, :seq_width], batch["images"].shape[-2:])
    pred_positions = closed_form_inverse_se3(pred_extr.reshape(B * seq_width, 3, 4)).reshape(
        B, seq_width, 4, 4)[..., :3, 3].detach().cpu().numpy()
    transforms, scales = [], []
    for b in range(B):
        r, t, c = umeyama(pred_positions[b].transpose(), gt_positions[b].transpose())
        pose = np.pad(r, ((0, 1), (0, 1)), mode="constant")
        pose[:3, 3] = t
        pose[3, 3] = 1.0
        transforms.append(pose)
        scales.append(c)
    pe, pts, d = apply_sim3_alignment(np.array(transforms), np.array(scales), predictions["pose_enc"],
                                      batch["images"].shape[-2:], predictions.get("world_points"),
                                      predictions.get("depth"))
    predictions["pose_enc"] = pe
    if "world_points" in predictions:
        predictions["world_points"] = pts
    if "depth" in predictions:
        predictions["depth"] = d


def _umeyama_alignment_from_poses_device(predictions: dict, batch: dict, seq_width: int) -> None:
    """The kernel route of umeyama_alignment_from_poses: transform and scale stay on the
    device.  When nothing requires grad the kernel also writes the aligned encoding and
    the dense tensors take vggt_sim3_points / the scale kernel; otherwise
    apply_sim3_alignment's differentiable torch chain runs with the device transform."""
    from .. import _native
    image_hw = batch["images"].shape[-2:]
    tracked = torch.is_grad_enabled() and any(
        predictions[k].requires_grad for k in ("pose_enc", "world_points", "depth") if k in predictions)
    scales, T, enc = _pose_align_launch(predictions["pose_enc"], batch["extrinsics"], _native.GT_POSE_SIM3,
                                        int(seq_width), None if tracked else image_hw)
    if tracked:
        enc, pts, d = apply_sim3_alignment(T, scales, predictions["pose_enc"], image_hw,
                                           predictions.get("world_points"), predictions.get("depth"))
    else:
        pts = d = None
        if "world_points" in predictions:
            pts = apply_sim3_alignment_on_point_maps(predictions["world_points"], T, scales)
        if "depth" in predictions:
            d = predictions["depth"]
            _scale_batch_(d, scales)
    predictions["pose_enc"] = enc
    if "world_points" in predictions:
        predictions["world_points"] = pts
    if "depth" in predictions:
        predictions["depth"] = d


def _points_align_kernel_applies(pred_points, pred_confidence, target_points, target_point_mask) -> bool:
    """All four tensors on one HIP device, fp32 values and a bool or uint8 mask;
    VGGT_GT_ALIGN=torch (read per call) keeps the host code."""
    if os.environ.get("VGGT_GT_ALIGN", "") == "torch":
        return False
    ts = (pred_points, pred_confidence, target_points, target_point_mask)
    if not all(torch.is_tensor(t) for t in ts) or not pred_points.is_cuda:
        return False
    return (all(t.device == pred_points.device for t in ts)
            and all(t.dtype == torch.float32 for t in ts[:3])
            and target_point_mask.dtype in (torch.bool, torch.uint8))


_POINT_COLUMNS = ("reference", "points")


def umeyama_alignment_from_points(pred_points, pred_confidence, target_points, target_point_mask,
                                  confidence_threshold: int, *, columns: str = "reference") -> tuple:
    """alignment.py:372-426 (percentile-thresholded Umeyama on point maps).

    ``columns="reference"`` fits the reference's samples, the ``reshape(3, -1)`` of the
    (n, 3) selection (sic); ``columns="points"`` fits the selected points themselves (the
    transpose), as the reference's docstring describes.

    Four tensors on one HIP device (fp32, bool or uint8 mask) take the kernel
    ``vggt_gt_points_align``: the result is ``(T (B, 4, 4), scales (B,))`` as fp32 device
    tensors with no graph attached (the reference detaches too), and nothing visits the
    host.  A batch element with no selected pixel gives NaN there; the host route raises
    inside LAPACK.  Everything else (arrays, host tensors, other dtypes, mixed placements,
    VGGT_GT_ALIGN=torch) runs the reference's numpy code and returns fp32/fp64 arrays."""
    if columns not in _POINT_COLUMNS:
        raise ValueError(f"columns must be one of {_POINT_COLUMNS}, got {columns!r}")
    if _points_align_kernel_applies(pred_points, pred_confidence, target_points, target_point_mask):
        from .. import _native

        def blocks(t):  # per-batch blocks contiguous, as [:, :seq_width] of a contiguous tensor is
            t = t.detach()
            return t if t[0].is_contiguous() else t.contiguous()
        with torch.no_grad():
            T, scales, _state = _native.gt_points_align(
                blocks(pred_points), blocks(pred_confidence), blocks(target_points), blocks(target_point_mask),
                float(confidence_threshold), _POINT_COLUMNS.index(columns))
        return T, scales

    def np_(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    pred_points, target_points = np_(pred_points), np_(target_points)
    pred_confidence, target_point_mask = np_(pred_confidence), np_(target_point_mask)
    poses, cs = [], []
    for b in range(pred_points.shape[0]):
        thr = np.percentile(pred_confidence[b], confidence_threshold)
        m = (target_point_mask[b] > 0) & (pred_confidence[b] >= thr) & (pred_confidence[b] > 1e-5)
        if columns == "reference":
            r, t, c = umeyama(pred_points[b][m].reshape(3, -1), target_points[b][m].reshape(3, -1))
        else:
            r, t, c = umeyama(pred_points[b][m].T, target_points[b][m].T)
        pose = np.pad(r, ((0, 1), (0, 1)), mode="constant")
        pose[:3, 3] = t
        pose[3, 3] = 1.0
        poses.append(pose)
        cs.append(c)
    return np.array(poses), np.array(cs)
