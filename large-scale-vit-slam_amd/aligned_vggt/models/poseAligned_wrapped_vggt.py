"""Pose-aligned VGGT (aligned_vggt/models/poseAligned_wrapped_vggt.py:16-205) on
MI355X -- the baseline of test_poseAlignedWrappedVGGT_vkitti.yaml.

Same constructor / ``set_config`` / ``forward(images, num_overlap, context,
gt_poses)`` and module names (``aggregator``, ``camera_head``, ``point_head``,
``depth_head``, ``track_head``) as the reference; the module tree is that of the
point-aligned ``VGGT``, so a ``facebook/VGGT-1B`` state dict loads unchanged.

Per chunk: HIP aggregator and HIP camera / depth / point heads, none of which
depends on other chunks (:meth:`VGGT.encode_chunk`); consecutive chunks are then
aligned through their camera poses alone (:func:`align_chunk`, :36-205): every
frame is re-centred on the chunk's first one, with ``gt_poses`` the translations
(and depth / points) are scaled by ``|sum x.y / sum x^2|`` against the GT
translations, and the chunk is moved onto the context by the Markley mean of the
overlap transforms.  Only B x overlap x 9 floats of pose encoding cross from
chunk to chunk.  The pose algebra is ONE launch (``vggt_pose_align``), the dense
part ``vggt_scale_f32`` / ``vggt_sim3_points``: no host round trip per chunk in
any mode, GT included (the reference copies to numpy per chunk, :95-96).
``forward == align_chunk(encode_chunk(.))`` exactly, which is what
``dist.pipeline.apply_sequence_to_model`` needs for its grouped encode.

Where the reference is undefined (SPEC_ASSUMPTIONS.md A24-A28):
  * ``gt_poses`` with S == 1 and a depth or point head: the reference hits a
    NameError (``batch_scales`` is never set); here ValueError before any launch.
  * ``gt_poses`` without a camera head but with a depth or point head: the same
    NameError; ValueError.
  * all predicted translations zero with GT: 0/0, a NaN scale that propagates into
    poses, depth and points -- kept, 1 is not substituted.
  * ``torch.cuda.empty_cache()`` per chunk (:66): not reproduced.
  * the caller's ``gt_poses`` is never mutated (the reference pads into a new
    tensor too).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as N
from ..backbone.aggregator import Aggregator
from ..backbone.camera_head import CameraHead
from ..backbone.dpt_head import DPTHead
from ..backbone.track_head import TrackHead
from ..utils.data import pose_encoding_to_extri
from ..utils.geometry import closed_form_inverse_se3
from ..utils.rotation import mat_to_quat, quat_to_mat

try:
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover
    class PyTorchModelHubMixin:  # type: ignore
        pass

MAX_OVERLAP_HIP = 64  # vggt_pose_align keeps the overlap transforms in LDS


class VGGT(nn.Module, PyTorchModelHubMixin):
    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, enable_camera=True, enable_point=True,
                 enable_depth=True, enable_track=True):
        super().__init__()
        self.intermediate_layer_indices = [4, 11, 17, 23]
        n = len(self.intermediate_layer_indices)
        self.aggregator = Aggregator(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim)
        self.camera_head = CameraHead(dim_in=2 * embed_dim) if enable_camera else None
        self.point_head = DPTHead(dim_in=2 * embed_dim, output_dim=4, activation="inv_log", conf_activation="expp1",
                                  intermediate_layer_idx=range(n)) if enable_point else None
        self.depth_head = DPTHead(dim_in=2 * embed_dim, output_dim=2, activation="exp", conf_activation="expp1",
                                  intermediate_layer_idx=range(n)) if enable_depth else None
        self.track_head = TrackHead(dim_in=2 * embed_dim, patch_size=patch_size) if enable_track else None

    def set_config(self, cfg):
        """poseAligned_wrapped_vggt.py:30-34."""
        self.camera_head = self.camera_head if cfg.enable_camera else None
        self.point_head = self.point_head if cfg.enable_point else None
        self.depth_head = self.depth_head if cfg.enable_depth else None
        self.track_head = self.track_head if cfg.enable_track else None

    @torch.no_grad()
    def forward(self, images: torch.Tensor, num_overlap: int, context: dict = None,
                gt_poses: torch.Tensor = None) -> dict:
        """poseAligned_wrapped_vggt.py:36-205."""
        return self.align_chunk(self.encode_chunk(images), num_overlap, context, gt_poses)

    @torch.no_grad()
    def encode_chunk(self, images: torch.Tensor) -> dict:
        """Everything of the chunk's forward that does not depend on other chunks
        (:62-74, :139-141, :159-161): the aggregator and every enabled head, raw.
        Every tensor has the batch leading, so a grouped encode splits per chunk."""
        toks, psi = self.aggregator(images, keep_layers=self.intermediate_layer_indices)
        enc = {"images": images}
        if self.camera_head is not None:
            enc["pose_enc"] = self.camera_head(toks)[-1]
        if self.depth_head is not None:
            enc["depth"], enc["depth_conf"] = self.depth_head(toks, images=images, patch_start_idx=psi)
        if self.point_head is not None:
            enc["world_points"], enc["world_points_conf"] = self.point_head(toks, images=images, patch_start_idx=psi)
        return enc

    @torch.no_grad()
    def align_chunk(self, enc: dict, num_overlap: int, context: dict = None, gt_poses: torch.Tensor = None) -> dict:
        return align_chunk(enc, num_overlap, context, gt_poses, self.training)


def align_chunk(enc: dict, num_overlap: int, context: Optional[dict] = None, gt_poses: Optional[torch.Tensor] = None,
                training: bool = False) -> dict:
    """poseAligned_wrapped_vggt.py:74-205 on an ``encode_chunk`` result, driven by
    the keys present in ``enc`` (``pose_enc``: camera head, ``depth``: depth head,
    ``world_points``: point head).  Returns a fresh dict whose lists are the
    context's lists with this chunk appended; ``enc["depth"]`` is scaled in place
    with ``gt_poses``, as the reference scales the head's output."""
    images = enc["images"]
    B, S = images.shape[:2]
    has_cam, has_depth, has_pts = "pose_enc" in enc, "depth" in enc, "world_points" in enc
    if gt_poses is not None and (has_depth or has_pts):
        if not has_cam:
            raise ValueError("gt_poses without a camera head: the GT scale of the depth / point maps is that of the "
                             "camera translations (poseAligned_wrapped_vggt.py:84-104)")
        if S == 1:
            raise ValueError("gt_poses with a one-frame chunk: no GT scale is defined for the depth / point maps "
                             "(poseAligned_wrapped_vggt.py:89)")
    pred: dict = {}

    def put(key, value):
        if context is None:
            pred[key] = [value]
        else:
            context.setdefault(key, []).append(value)
            pred[key] = context[key]

    point_transform = scales = None
    if has_cam:
        ctx_pe = context["pose_enc"][-1] if context is not None else None
        aligned, point_transform, scales = align_chunk_poses(enc["pose_enc"], images.shape[-2:], num_overlap, ctx_pe,
                                                             gt_poses)
        put("pose_enc", aligned)
    if has_depth:
        depth = enc["depth"]
        if gt_poses is not None:  # :144-146, in place
            if depth.is_cuda:
                N.scale_(depth, scales)
            else:
                depth.mul_(scales.to(depth).view(B, 1, 1, 1, 1))
        put("depth", depth)
        put("depth_conf", enc["depth_conf"])
    if has_pts:
        pts = enc["world_points"]
        if has_cam:  # :164-187: scale (1 without GT), then the SE(3) of the point transform
            if pts.is_cuda:
                pts = N.sim3_points(pts.contiguous(), point_transform, scales)
            else:
                T = point_transform.to(pts)
                p = pts * scales.to(pts).view(B, 1, 1, 1, 1)
                pts = (p.reshape(B, -1, 3) @ T[:, :3, :3].transpose(-1, -2) + T[:, None, :3, 3]).view(pts.shape)
        put("world_points", pts)
        put("world_points_conf", enc["world_points_conf"])
    if not training:
        put("images", images)
    return pred


def _hip_eligible(*tensors) -> bool:
    return all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)


def align_chunk_poses(pose_enc: torch.Tensor, image_hw, num_overlap: int, ctx_pose_enc: Optional[torch.Tensor] = None,
                      gt_poses: Optional[torch.Tensor] = None, form: Optional[str] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The chunk's pose algebra (:74-130, :171-177): raw camera-head encoding
    (B,S,9), the context's last aligned encoding (B,S_prev,9) or None, GT w2c
    poses (B,S,3,4) or None -> aligned encoding (B,S,9), point transform (B,4,4),
    scales (B,) (ones without GT, and for S == 1).

    ``form``: "hip" (``vggt_pose_align``, one launch), "torch" (the reference's
    operations in the reference's order, in the inputs' dtype, on the inputs'
    device) or None: hip when every input is a contiguous fp32 device tensor,
    ``num_overlap <= 64`` and the chunk is not a one-frame chunk with GT, unless
    VGGT_POSE=device (or host: the same here) asks for torch; read per call."""
    if form is None:
        S = pose_enc.shape[1]
        hip = _hip_eligible(pose_enc, ctx_pose_enc, gt_poses) and num_overlap <= MAX_OVERLAP_HIP \
            and not (gt_poses is not None and S == 1) and os.environ.get("VGGT_POSE", "hip") not in ("device", "host")
        form = "hip" if hip else "torch"
    if form == "hip":
        return N.pose_align(pose_enc, ctx_pose_enc, gt_poses, num_overlap, image_hw, want_point_transform=True)
    if form != "torch":
        raise ValueError(f"align_chunk_poses: unknown form {form!r}")
    return _align_chunk_poses_torch(pose_enc, image_hw, num_overlap, ctx_pose_enc, gt_poses)


def _pad4(e: torch.Tensor) -> torch.Tensor:
    e = F.pad(e, (0, 0, 0, 1, 0, 0, 0, 0), mode="constant")
    e[:, :, 3, 3] = 1.0
    return e


def _extri_to_pose_encoding(extrinsics: torch.Tensor) -> torch.Tensor:
    """utils.data.extri_to_pose_encoding without the final .float()."""
    quat = mat_to_quat(extrinsics[:, :, :3, :3])
    quat = quat / quat.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    return torch.cat([extrinsics[:, :, :3, 3], quat], dim=-1)


def _average_pose_encodings(pose_encodings: torch.Tensor) -> torch.Tensor:
    """utils.geometry.averagePoseEncodings without the final .float() (the 4 x 4
    eigenproblem on the host, as there)."""
    B, n, _ = pose_encodings.shape
    avg_t = pose_encodings[..., :3].mean(dim=1, keepdim=True)
    q = pose_encodings[..., 3:7]
    q = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    w = (torch.ones(B, n, device=q.device, dtype=q.dtype) / n).unsqueeze(-1).unsqueeze(-1)
    M = (w * (q.unsqueeze(-1) * q.unsqueeze(-2))).sum(dim=1)
    _, vec = torch.linalg.eigh(M.cpu())
    v = vec[..., -1].to(M.device)
    v = v / v.norm(dim=-1, keepdim=True)
    return torch.cat([avg_t, v.unsqueeze(1)], dim=-1)


def _align_chunk_poses_torch(pose_enc, image_hw, num_overlap, ctx_pose_enc, gt_poses):
    B, S = pose_enc.shape[:2]
    H, W = int(image_hw[0]), int(image_hw[1])
    # pose_encoding_to_extri_intri (VGGT): the raw quaternion, 2 / |q|^2 form; focal lengths from the FoV
    extr = _pad4(torch.cat([quat_to_mat(pose_enc[..., 3:7]), pose_enc[..., :3, None]], dim=-1))
    fy = (H / 2.0) / torch.tan(pose_enc[..., 7] / 2.0)
    fx = (W / 2.0) / torch.tan(pose_enc[..., 8] / 2.0)
    ident = closed_form_inverse_se3(extr[:, 0])                                  # :79
    point_identity = extr[:, 0].detach().clone()                                 # :80
    extr = extr @ ident.view(B, 1, 4, 4)                                         # :81
    scales = torch.ones(B, device=extr.device, dtype=extr.dtype)
    gt = None
    if gt_poses is not None:
        gt = _pad4(gt_poses.to(extr))                                            # :86-87, a new tensor
        if S > 1:
            centred = gt @ closed_form_inverse_se3(gt[:, 0]).view(B, 1, 4, 4)    # :90-92
            x, y = extr[..., :3, 3], centred[..., :3, 3]
            scales = ((x * y).sum(dim=(1, 2)) / (x * x).sum(dim=(1, 2))).abs()   # scale_lse_solver, on the device
            extr[:, :, :3, 3] *= scales.view(B, 1, 1)                            # :102
    if ctx_pose_enc is not None:
        if gt is not None:
            mean = gt[:, :1]                                                     # :109, not centred
        else:
            ctx_o = pose_encoding_to_extri(ctx_pose_enc[:, -num_overlap:].to(extr))                          # :111
            inv_o = closed_form_inverse_se3(extr[:, :num_overlap].reshape(B * num_overlap, 4, 4)).reshape(
                B, num_overlap, 4, 4)                                                                        # :113
            ct = inv_o @ ctx_o
            if num_overlap > 1:
                mean = pose_encoding_to_extri(_average_pose_encodings(_extri_to_pose_encoding(ct)))          # :118-122
            else:
                mean = ct
    else:
        mean = torch.eye(4, device=extr.device, dtype=extr.dtype).view(1, 1, 4, 4).expand(B, -1, -1, -1)
    aligned_extr = torch.matmul(extr, mean)                                      # :129
    fov_h = 2 * torch.atan((H / 2) / fy)                                         # extri_intri_to_pose_encoding
    fov_w = 2 * torch.atan((W / 2) / fx)
    aligned = torch.cat([aligned_extr[:, :, :3, 3], mat_to_quat(aligned_extr[:, :, :3, :3]), fov_h[..., None],
                         fov_w[..., None]], dim=-1)
    if ctx_pose_enc is not None:                                                 # :171-177
        pt = closed_form_inverse_se3(mean.squeeze(1)) @ point_identity
    else:
        pt = point_identity
    return aligned, pt, scales
