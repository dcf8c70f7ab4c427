"""The training objective on the HIP path: ``MultitaskLoss`` (reference
training/loss.py, the ``loss._target_`` of train_featureAlignedVGGT_vkitti.yaml).

Same constructor, same ``setupScheduling`` / ``compute_warmup_weight`` /
``forward``, same loss-dict keys and the same order of accumulation into
``objective``: setting ``_target_`` to ``aligned_vggt.training.loss.MultitaskLoss``
is the whole switch.

* The depth term -- the one dense computation of the objective, every pixel of
  every frame -- runs as HIP kernels (csrc/loss.hip) behind one
  ``torch.autograd.Function``.  Nothing is gathered, every branch the reference
  takes on a count (fewer than 100 valid pixels, 1000 or fewer before or after
  the quantile filter) is taken on the device, and the backward recomputes from
  the inputs: no host synchronisation, no dense intermediate kept, usable under
  ``runtime.GraphedStep``.  The gradient goes to ``predictions["depth"]`` only
  (the depth head's confidence is frozen: ``depth_conf.requires_grad`` raises).
* The four small terms (per-frame / per-chunk regularisation, absolute and
  relative camera pose) work on B * S * 9 numbers and stay differentiable torch
  ops on the device, built from ``utils.pose_enc``, ``utils.rotation`` and
  ``utils.geometry``.  The reference's ``valid_frame_mask.sum() == 0`` branches
  are ``torch.where`` on the device; the far offset of the relative pose loss
  is ``torch.randint`` on the host, as the reference draws it (here also when no
  frame is valid, where the reference returns before drawing).
"""
from __future__ import annotations

from math import floor

import torch

from .. import _native as N
from ..utils.geometry import compute_relative_poses
from ..utils.pose_enc import extri_intri_to_pose_encoding, pose_encoding_to_extri_intri
from ..utils.rotation import mat_to_quat


def check_and_fix_inf_nan(input_tensor, loss_name: str = "default", hard_max=100):
    """NaN and +-inf become 0, then the result is clamped to +-``hard_max`` unless
    that is None (VGGT's training helper, SPEC_ASSUMPTIONS.md A20).  Unlike the
    original it does not look at the tensor first (``.any()`` is a host
    synchronisation): the values and the gradients are the same."""
    if not isinstance(input_tensor, torch.Tensor):
        return input_tensor
    out = torch.where(torch.isfinite(input_tensor), input_tensor, torch.zeros_like(input_tensor))
    if hard_max is not None:
        out = torch.clamp(out, min=-hard_max, max=hard_max)
    return out


class MultitaskLoss(torch.nn.Module):
    """Weighted sum of the per-frame / per-chunk regularisation, depth, absolute
    and relative camera pose losses; each argument is that term's config dict
    (``weight``, the ``warmup_*`` keys and the term's own options) or None."""

    def __init__(self, perFrameReg=None, perChunkReg=None, depth=None, cameraPose=None, cameraPoseRel=None, **kwargs):
        super().__init__()
        self.perFrameReg = perFrameReg
        self.perChunkReg = perChunkReg
        self.depth = depth
        self.cameraPose = cameraPose
        self.cameraPoseRel = cameraPoseRel
        # the reference's "exp" warm-up reads this attribute and never sets it
        self.weight_warmup_exp = kwargs.get("weight_warmup_exp")

    def setupScheduling(self, total_steps: int):
        self.total_steps = total_steps

    def compute_warmup_weight(self, loss_type_dict: dict, current_step: int) -> float:
        end_weight = loss_type_dict["weight"]
        warmup_steps = floor(self.total_steps * loss_type_dict["warmup_percent"]) \
            if "warmup_percent" in loss_type_dict else 0.
        start_step = floor(self.total_steps * loss_type_dict["warmup_start_percent"]) \
            if "warmup_start_percent" in loss_type_dict else 0.
        start_weight = loss_type_dict.get("warmup_start_weight", 0.)
        warmup_type = loss_type_dict.get("warmup_type", "exp")

        if warmup_steps <= 0:
            return end_weight
        if start_step > current_step:
            return 0.0
        if (start_step + warmup_steps) < current_step:
            return end_weight

        delta_steps = current_step - start_step
        delta_weights = end_weight - start_weight
        if warmup_type == "exp":
            if self.weight_warmup_exp is None:
                raise ValueError("warmup_type 'exp' needs weight_warmup_exp (a MultitaskLoss keyword argument)")
            warmup_factor = (min(1.0, (float(delta_steps) / float(warmup_steps)))) ** self.weight_warmup_exp
        elif warmup_type == "linear":
            warmup_factor = (min(1.0, (float(delta_steps) / float(warmup_steps))))
        else:
            raise ValueError("Invalid learning rate warmup type")
        return start_weight + delta_weights * warmup_factor

    def forward(self, predictions: dict, batch: dict, current_step: int) -> dict:
        total_loss = 0
        loss_dict = {}

        if "frame_se3_alignment_enc" in predictions and self.perFrameReg is not None:
            d = per_frame_regularization_loss(predictions, **self.perFrameReg)
            total_loss = total_loss + d["loss_per_frame_reg"] * self.compute_warmup_weight(self.perFrameReg, current_step)
            loss_dict.update(d)

        if "chunk_sim3_alignment_enc" in predictions and self.perChunkReg is not None:
            d = per_chunk_regularization_loss(predictions, **self.perChunkReg)
            total_loss = total_loss + d["loss_per_chunk_reg"] * self.compute_warmup_weight(self.perChunkReg, current_step)
            loss_dict.update(d)

        if "depth" in predictions and self.depth is not None:
            d = compute_depth_loss(predictions, batch, **self.depth)
            total_loss = total_loss + d["loss_depth"] * self.compute_warmup_weight(self.depth, current_step)
            loss_dict.update(d)

        if "pose_enc" in predictions and self.cameraPose is not None:
            d = compute_camera_pose_loss(predictions, batch, **self.cameraPose)
            total_loss = total_loss + d["loss_camera"] * self.compute_warmup_weight(self.cameraPose, current_step)
            loss_dict.update(d)

        if "pose_enc" in predictions and self.cameraPoseRel is not None:
            d = compute_relative_pose_loss(predictions, batch, **self.cameraPoseRel)
            total_loss = total_loss + d["loss_camera_rel"] * self.compute_warmup_weight(self.cameraPoseRel, current_step)
            loss_dict.update(d)

        loss_dict["objective"] = total_loss
        return loss_dict


# ------------------------------------------------------------------------------------------- depth (HIP)
class DepthLossFn(torch.autograd.Function):
    """loss_depth of (pred, conf, gt, mask), all (B, S, H, W): vggt_depth_loss_values
    + vggt_depth_loss_reduce forward, vggt_depth_loss_bwd backward.  Saves the
    inputs, the per-frame amax and the 48-byte decision state: nothing dense."""

    @staticmethod
    def forward(ctx, pred, conf, gt, mask, valid_range):
        pred = pred.detach()
        val, amax, n, ws = N.depth_loss_values(pred, conf, gt, mask)
        loss, state = N.depth_loss_reduce(val, n, valid_range, ws)
        ctx.save_for_backward(pred, conf, gt, mask, amax, state)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        pred, conf, gt, mask, amax, state = ctx.saved_tensors
        dpred = N.depth_loss_bwd(pred, conf, gt, mask, amax, state, grad_loss.float().contiguous())
        return dpred, None, None, None, None


def _dense_f32(t: torch.Tensor, shape) -> torch.Tensor:
    t = t.reshape(shape)
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def compute_depth_loss(predictions, batch, valid_range=-1, **kwargs):
    """The reference's compute_depth_loss (log-space L1 weighted by the per-frame
    normalised confidence, quantile-filtered) on the HIP kernels."""
    pred_depth = predictions["depth"]  # (B, S, H, W, 1)
    conf = predictions["depth_conf"]  # (B, S, H, W)
    gt_depth = batch["depths"]
    mask = batch["point_masks"]
    if conf.requires_grad:
        raise NotImplementedError("compute_depth_loss: depth_conf.requires_grad (the depth head is frozen; the "
                                  "gradient goes to predictions['depth'] only)")
    for t in (pred_depth, conf, gt_depth, mask):
        if t.device.type != "cuda":
            raise RuntimeError(f"compute_depth_loss: tensor on {t.device}; the MI355X hot path runs on HIP devices only")
    shape = conf.shape
    if mask.dtype != torch.bool:
        mask = mask != 0
    loss = DepthLossFn.apply(_dense_f32(pred_depth, shape), _dense_f32(conf.detach(), shape),
                             _dense_f32(gt_depth.detach(), shape), mask.reshape(shape), float(valid_range))
    return {"loss_depth": loss}


# ------------------------------------------------------------------------------- the four small terms
def _valid_frames(batch_data) -> torch.Tensor:
    """0-dim bool on the device: some batch element's first frame has more than 100 valid points."""
    return (batch_data["point_masks"][:, 0].sum(dim=[-1, -2]) > 100).any()


def compute_camera_pose_loss(pred_dict: dict, batch_data: dict, loss_type: str = "l1",
                             pose_encoding_type: str = "absT_quaR_FoV", **kwargs):
    pred = pred_dict["pose_enc"]
    image_hw = batch_data["images"].shape[-2:]
    gt = extri_intri_to_pose_encoding(batch_data["extrinsics"], batch_data["intrinsics"], image_hw,
                                      pose_encoding_type=pose_encoding_type)
    if loss_type == "l1":
        loss_T = (pred[..., :3] - gt[..., :3]).abs()
        loss_R = (pred[..., 3:7] - gt[..., 3:7]).abs()
    elif loss_type == "l2":
        loss_T = (pred[..., :3] - gt[..., :3]).norm(dim=-1, keepdim=True)
        loss_R = (pred[..., 3:7] - gt[..., 3:7]).norm(dim=-1)
    else:
        raise ValueError(f"Unknown loss type: {loss_type}")
    loss_T = check_and_fix_inf_nan(loss_T, "loss_T_pose").clamp(max=100).mean()
    loss_R = check_and_fix_inf_nan(loss_R, "loss_R_pose").mean()

    ok = _valid_frames(batch_data)
    zero = (pred * 0).mean()
    loss_T = torch.where(ok, loss_T, zero)
    loss_R = torch.where(ok, loss_R, zero)
    return {"loss_camera": loss_T + loss_R, "loss_T": loss_T, "loss_R": loss_R}


def compute_relative_pose_loss(pred_dict, batch_data, loss_type="l1", pose_encoding_type="absT_quaR_FoV",
                               weight_trans=1.0, weight_rot=1.0, scale_agnostic=False, **kwargs):
    pred_enc = pred_dict["pose_enc"]
    pred_extr, _ = pose_encoding_to_extri_intri(pred_enc, pose_encoding_type=pose_encoding_type,
                                                build_intrinsics=False)
    gt_extr = batch_data["extrinsics"]

    S = gt_extr.shape[1]
    large_offset = torch.randint(int(S / 2), S, (1,)).item()  # a host generator: no device round trip
    gt_rel = torch.cat((compute_relative_poses(gt_extr), compute_relative_poses(gt_extr, large_offset)), dim=1)
    pred_rel = torch.cat((compute_relative_poses(pred_extr), compute_relative_poses(pred_extr, large_offset)), dim=1)

    gt_q, pred_q = mat_to_quat(gt_rel[:, :, :3, :3]), mat_to_quat(pred_rel[:, :, :3, :3])
    gt_t, pred_t = gt_rel[:, :, :3, 3], pred_rel[:, :, :3, 3]
    if scale_agnostic:
        gt_t = gt_t / gt_t.norm(dim=-1, keepdim=True)
        pred_t = pred_t / pred_t.norm(dim=-1, keepdim=True)

    if loss_type == "l1":
        loss_T = (pred_t - gt_t).abs()
        loss_R = (pred_q - gt_q).abs()
    elif loss_type == "l2":
        loss_T = (pred_t - gt_t).norm(dim=-1, keepdim=True)
        loss_R = (pred_q - gt_q).norm(dim=-1)
    else:
        raise ValueError(f"Unknown loss type: {loss_type}")
    loss_T = check_and_fix_inf_nan(loss_T, "loss_T_rel").clamp(max=100).mean()
    loss_R = check_and_fix_inf_nan(loss_R, "loss_R_rel").mean()

    ok = _valid_frames(batch_data)
    zero = (pred_enc * 0).mean()
    loss_T = torch.where(ok, loss_T, zero)
    loss_R = torch.where(ok, loss_R, zero)
    total = torch.where(ok, (weight_trans * loss_T) + (weight_rot * loss_R), zero)
    return {"loss_camera_rel": total, "loss_T_rel": loss_T, "loss_R_rel": loss_R}


def _unit_rotation(rotation: torch.Tensor) -> torch.Tensor:
    return rotation / rotation.norm(dim=-1, keepdim=True).clamp(min=1e-8)


def per_frame_regularization_loss(pred_dict, **kwargs):
    enc = pred_dict["frame_se3_alignment_enc"].reshape(-1, 7)
    rotation = _unit_rotation(enc[..., 3:7])
    loss_t = check_and_fix_inf_nan(enc[..., :3].norm(dim=-1, keepdim=True), "frame_reg_t")
    loss_r = check_and_fix_inf_nan((1 - (rotation[..., -1] ** 2)).abs(), "frame_reg_r")
    return {"loss_per_frame_reg": loss_t.clamp(max=100).mean() + loss_r.mean()}


def per_chunk_regularization_loss(pred_dict, **kwargs):
    enc = pred_dict["chunk_sim3_alignment_enc"]  # (B * num_chunks, 1, 8)
    rotation = _unit_rotation(enc[..., 3:7])
    loss_t = check_and_fix_inf_nan(enc[..., :3].norm(dim=-1, keepdim=True), "chunk_reg_t")
    loss_r = check_and_fix_inf_nan((1 - (rotation[..., -1] ** 2)).abs(), "chunk_reg_r")
    loss = loss_t.clamp(max=100).mean() + loss_r.mean()
    if enc.shape[-1] == 8:
        loss_s = check_and_fix_inf_nan(torch.log(enc[..., 7].clamp_min(1e-6)) ** 2, "chunk_reg_s")
        loss = loss + loss_s.mean()
    return {"loss_per_chunk_reg": loss}
