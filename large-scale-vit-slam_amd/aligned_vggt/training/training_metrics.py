"""The metrics module of the reference's test protocol (training/training_metrics.py),
resident on the device: ``metrics._target_: aligned_vggt.training.training_metrics.Metrics``.

``run_model.py``'s ``validation_step`` / ``test_step`` are the model's forward plus one
call of this module: metrics of the step's batch, then -- on rank 0 -- of whole
sequences run chunk by chunk through the model (``apply_sequence_to_model``), GT-aligned,
prepared (``aligned_vggt.eval.prepare_data_for_metrics``: unprojection, confidence
quantile, image-space subsampling, ICP) and scored by the trajectory and reconstruction
metrics' ``plot``.

Differences from the reference, all of them about where the data lives:
  * no hydra, torchmetrics, PyTorch3D or viser: metric entries are ready objects or
    ``_target_`` mappings resolved here (``eval.<...>`` inside ``aligned_vggt.eval``,
    any other dotted path imported as given); ``visualize=True`` raises;
  * ``sequence_outputs="device"`` (the default) keeps every chunk's outputs on the
    device: the driver below runs with ``offload=False``, the merge and the pose-based GT
    alignments run there (csrc/pose.hip) and the first host visit of a value is a
    metric's ``.item()``.  It holds the merged outputs of one sequence in device memory:
    B S (H W (c_depth + c_points) + 9) fp32 values, c_depth = 2 (depth, confidence) and
    c_points = 4 (points, confidence) for the heads that are enabled, and the GT that the
    alignments and the preparation read, 29 bytes a pixel, as the sequence, its chunked
    copy and the merged copy (INTEGRATION.md has the sum).  ``"host"`` is the reference's route: chunk outputs are offloaded as
    they are produced, merged and aligned on the host, and copied back for the
    preparation, which runs on the device in either case.
"""
from __future__ import annotations

import contextlib
import importlib
from math import ceil, floor
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import eval as _eval
from ..dist import pipeline as _pipeline
from ..utils.data import (chunk_outputs_stay_in_place, normalize_camera_extrinsics_and_points_batch,
                          pose_encoding_to_extri)
from ..utils.pose_enc import pose_encoding_to_extri_intri


# what the GT alignments and the preparation read of a sequence's GT (cam_points and ids stay on the host)
_DEVICE_GT_KEYS = ("images", "extrinsics", "intrinsics", "depths", "world_points", "point_masks")


def _instantiate(entry):
    """A metric entry: a ready object, or a mapping with ``_target_`` and keyword
    arguments.  ``eval.<module>.<Class>`` (the reference's configs) resolves inside
    ``aligned_vggt.eval``; any other dotted path is imported as given."""
    if not (hasattr(entry, "keys") and "_target_" in entry):
        return entry
    target = str(entry["_target_"])
    kwargs = {k: entry[k] for k in entry.keys() if not str(k).startswith("_")}
    if target.startswith("eval."):
        target = "aligned_vggt." + target
    module, _, name = target.rpartition(".")
    if not module:
        raise ValueError(f"metric _target_ '{target}' is not a dotted path")
    return getattr(importlib.import_module(module), name)(**kwargs)


class Metrics(torch.nn.Module):
    """Batch and full-sequence metrics (training_metrics.py:20-459).

    Args (the reference's): mode ("train" | "validate" | "test"), overlap, chunk_width,
    gt_alignment_type, full_seq_sample_mode, use_random_sequences,
    max_points_for_icp_batch, max_points_for_icp_full_seq, trajectory_metrics,
    reconstruction_metrics (lists of metric entries), visualize (must be False),
    save_for_visualization.  New: sequence_outputs ("device" | "host", see the module
    docstring)."""

    def __init__(self, mode: str, overlap: int, chunk_width: int, gt_alignment_type: str, full_seq_sample_mode: str,
                 use_random_sequences: bool = True, max_points_for_icp_batch: int = 250000,
                 max_points_for_icp_full_seq: int = 500000, trajectory_metrics: Optional[list] = None,
                 reconstruction_metrics: Optional[list] = None, visualize: bool = False,
                 save_for_visualization: bool = False, sequence_outputs: str = "device", **kwargs):
        super().__init__()
        if visualize:
            raise NotImplementedError("Metrics(visualize=True): the viser viewer is not part of this package; "
                                      "use save_for_visualization=True and view the saved arrays elsewhere")
        if sequence_outputs not in ("device", "host"):
            raise ValueError(f"sequence_outputs must be 'device' or 'host', got {sequence_outputs!r}")
        self.mode = mode
        self.num_overlap = overlap
        self.chunk_width = chunk_width
        self.full_seq_sample_mode = full_seq_sample_mode
        self.gt_alignment_type = gt_alignment_type
        self.use_random_sequences = use_random_sequences
        self.max_points_for_icp_batch = max_points_for_icp_batch
        self.max_points_for_icp_full_seq = max_points_for_icp_full_seq
        self.log_dir = None
        self.visualize = False
        self.save_for_visualization = save_for_visualization
        self.sequence_outputs = sequence_outputs
        self.trajectory_metrics = [_instantiate(m) for m in (trajectory_metrics or [])]
        self.reconstruction_metrics = [_instantiate(m) for m in (reconstruction_metrics or [])]

    def _has_points(self, predictions: dict) -> bool:
        return len(self.reconstruction_metrics) > 0 and ("world_points" in predictions or "depth" in predictions)

    def forward(self, predictions: dict, batch: dict, model: torch.nn.Module, trainer) -> Tuple[dict, dict]:
        """(batch metrics, sequence metrics) of one validation / test step; the sequence
        metrics are computed on the global-zero rank only, the others wait at a barrier."""
        if self.log_dir is None:
            self.log_dir = trainer.logger.log_dir
        batch_metrics, seq_metrics = {}, {}
        if len(self.trajectory_metrics) > 0 or self._has_points(predictions):
            batch_metrics = self.compute_batch_metrics(predictions, batch)
            if trainer.is_global_zero:
                loaders = trainer.test_dataloaders if self.mode == "test" else trainer.val_dataloaders
                datasets = loaders.dataset.base_dataset.datasets
                seq_metrics = self.compute_full_sequence_metrics(datasets, model, predictions["pose_enc"].device)
            trainer.strategy.barrier("Compute sequence metrics")
        return batch_metrics, seq_metrics

    def compute_batch_metrics(self, predictions: dict, batch: dict) -> dict:
        """Metrics of the step's batch: every sequence of the batch updates each metric,
        which is computed and reset; the first sequence is plotted when there is a log
        directory."""
        out: dict = {}
        log_additional_data(predictions, out)
        pred_poses, gt_poses, pred_points, gt_points = self.prepare_data_for_metrics(
            predictions, batch, max_points_icp=self.max_points_for_icp_batch)
        title = f"seq: {batch['seq_name'][0]}"
        prefix = f"{self.log_dir}/batch_" if self.log_dir else None
        with torch.amp.autocast("cuda", enabled=False):
            for metric in self.trajectory_metrics:
                metric = metric.to(gt_poses)
                if hasattr(metric, "update_batch"):
                    metric.update_batch(pred_poses, gt_poses)
                else:
                    for pred, gt in zip(pred_poses, gt_poses):
                        metric.update(pred, gt)
                out.update(metric.compute())
                metric.reset()
                if prefix:
                    metric.plot(pred_poses[0], gt_poses[0], title, prefix)
            if self._has_points(predictions):
                for metric in self.reconstruction_metrics:
                    metric = metric.to(gt_points[0])
                    for pred, gt in zip(pred_points, gt_points):
                        metric.update(pred, gt)
                    out.update(metric.compute())
                    metric.reset()
                    if prefix:
                        metric.plot(pred_points[0], gt_points[0], title, prefix)
        return out

    def compute_full_sequence_metrics(self, datasets: list, model: torch.nn.Module, device: torch.device) -> dict:
        """Metrics of whole sequences (one random one, or all of them): the sequence runs
        through the model chunk by chunk, is GT-aligned and prepared, and every metric's
        ``plot`` gives its numbers.  Keys carry ``seq_metrics/`` or
        ``<dataset>_<sequence>/`` in front."""
        out: dict = {}
        on_device = self.sequence_outputs == "device"
        for seq in gather_sequences(datasets, self.use_random_sequences):
            per_seq: dict = {}
            seq_data = get_sequence_data(*seq)
            for k in (_DEVICE_GT_KEYS if on_device else ("images",)):
                seq_data[k] = seq_data[k].to(device)
            predictions = apply_sequence_to_model(seq_data, model, self.chunk_width, self.num_overlap,
                                                  self.full_seq_sample_mode, self.gt_alignment_type,
                                                  offload=not on_device)
            log_additional_data(predictions, per_seq)
            pred_poses, gt_poses, pred_points, gt_points = self.prepare_data_for_metrics(
                predictions, seq_data, max_points_icp=self.max_points_for_icp_full_seq, device=device)
            title = f"{seq_data['dataset_name']}_seq[{seq_data['seq_name']}]"
            if self.use_random_sequences:
                prefix, image_path = "seq_metrics/", f"{self.log_dir}/seq_"
            else:
                prefix = f"{seq_data['dataset_name']}_{seq_data['seq_name']}/"
                image_path = f"{self.log_dir}/[{seq_data['dataset_name']}_{seq_data['seq_name']}]_"
            if not self.log_dir:
                image_path = None  # nowhere to write: the numbers only
            if self.save_for_visualization and image_path:
                self.save_dict_for_visualization(predictions, seq_data, image_path)
            with torch.amp.autocast("cuda", enabled=False):
                if len(self.trajectory_metrics) > 0:
                    assert pred_poses.shape[0] == 1, "full-sequence metrics take one sequence at a time"
                    for metric in self.trajectory_metrics:
                        per_seq.update(metric.plot(pred_poses[0], gt_poses[0], title, image_path)[0])
                if self._has_points(predictions):
                    assert len(pred_points) == 1, "full-sequence metrics take one sequence at a time"
                    for metric in self.reconstruction_metrics:
                        per_seq.update(metric.plot(pred_points[0], gt_points[0], title, image_path)[0])
            for k, v in per_seq.items():
                out[f"{prefix}{k}"] = v
        return out

    def prepare_data_for_metrics(self, pred_dict: dict, gt_dict: dict, valid_point_quantile: float = 0.25,
                                 max_points_icp: Optional[int] = None, device: Optional[torch.device] = None):
        """(pred_poses, gt_poses, pred_points, gt_points) through
        ``aligned_vggt.eval.prepare_data_for_metrics``, which works on device tensors: what
        it reads and is still on the host (the "host" route's merged outputs) is copied to
        ``device`` first."""
        want_points = self._has_points(pred_dict)
        want_poses = len(self.trajectory_metrics) > 0
        if device is None:
            device = pred_dict["pose_enc"].device
        keys = ["pose_enc", "extrinsics", "intrinsics", "images"]
        if want_points:
            keys += ["depth", "depth_conf", "world_points", "world_points_conf", "point_masks"]

        def on(d):
            return {k: (v.to(device) if k in keys and isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        with torch.amp.autocast("cuda", enabled=False):
            return _eval.prepare_data_for_metrics(on(pred_dict), on(gt_dict), valid_point_quantile, max_points_icp,
                                                  device, poses=want_poses, points=want_points)

    def save_dict_for_visualization(self, predictions: dict, seq_data: dict, save_path: str) -> None:
        """Write ``{save_path}visualization_data.npy`` (predictions, with ``extrinsic`` /
        ``intrinsic`` decoded from the pose encoding) and ``..._gt.npy`` (the GT under the
        same names) for a viewer; ``predictions`` gains the two decoded keys."""
        enc = predictions["pose_enc"]
        if enc.shape[-1] == 9:
            extr, intr = pose_encoding_to_extri_intri(enc, image_size_hw=seq_data["images"].shape[-2:])
        elif enc.shape[-1] == 7:
            extr, intr = pose_encoding_to_extri(enc)[:, :, :3, :4], seq_data["intrinsics"]
        else:
            raise ValueError(f"pose_enc must be 7 or 9 wide, got {enc.shape[-1]}")
        predictions["extrinsic"], predictions["intrinsic"] = extr, intr

        def host(d, keys):
            return {k: d[k].detach().cpu().numpy().squeeze(0) for k in d
                    if k in keys and isinstance(d[k], torch.Tensor)}
        np.save(f"{save_path}visualization_data.npy",
                host(predictions, ("images", "intrinsic", "extrinsic", "world_points", "world_points_conf", "depth",
                                   "depth_conf")))
        gt = host(seq_data, ("images", "intrinsics", "extrinsics", "world_points", "point_masks", "depths"))
        gt["intrinsic"] = gt.pop("intrinsics")
        gt["extrinsic"] = gt.pop("extrinsics")
        gt["world_points_conf"] = gt.pop("point_masks").astype(float)
        gt["depth_conf"] = gt["world_points_conf"]
        gt["depth"] = gt.pop("depths")[..., None]
        np.save(f"{save_path}visualization_data_gt.npy", gt)


def _unit_quats(q: torch.Tensor) -> torch.Tensor:
    return q / q.norm(dim=-1, keepdim=True).clamp(min=1e-8)


def _offdiag_cosine(tokens: torch.Tensor) -> float:
    """Mean cosine similarity between different tokens of (B, N, D)."""
    B, N = tokens.shape[:2]
    n = F.normalize(tokens, p=2, dim=-1, eps=1e-8)
    sim = torch.bmm(n, n.transpose(1, 2)) * (1.0 - torch.eye(N, device=n.device).unsqueeze(0))
    return (sim.sum() / (B * N * (N - 1))).item()


def log_additional_data(pred_dict: dict, log_dict: dict) -> None:
    """training_metrics.py:462-524: averages of what the alignment left in the
    predictions -- GT alignment scales, the per-frame SE(3) and per-chunk Sim(3)
    encodings, the memory tokens' mutual similarity -- written into ``log_dict``;
    ``memory_tokens`` is removed from ``pred_dict``.  The scales may be floats (host
    route) or device tensors (kernel route)."""
    if "alignment_scales_per_chunk" in pred_dict:
        log_dict["avg_per_chunk_alignment_scale"] = torch.stack(pred_dict["alignment_scales_per_chunk"],
                                                                dim=1).mean().item()
    if "alignment_scales" in pred_dict:
        sc = pred_dict["alignment_scales"]
        t = torch.stack(list(sc)) if len(sc) and all(isinstance(s, torch.Tensor) for s in sc) else torch.tensor(sc)
        log_dict["avg_alignment_scale"] = t.mean().item()
    if "frame_se3_alignment_enc" in pred_dict:
        enc = pred_dict["frame_se3_alignment_enc"]
        log_dict["avg_per_frame_trans_norm"] = enc[:, :, :3].norm(dim=-1).mean().item()
        q = _unit_quats(enc[:, :, 3:7])
        log_dict["avg_per_frame_quat_magnitude"] = (2.0 * torch.sqrt(torch.clamp(1 - q[:, :, -1] ** 2,
                                                                                 min=0.0))).mean().item()
    if "chunk_sim3_alignment_enc" in pred_dict:
        enc = pred_dict["chunk_sim3_alignment_enc"]
        log_dict["avg_per_chunk_trans_norm"] = enc[..., :3].norm(dim=-1).mean().item()
        q = _unit_quats(enc[..., 3:7])
        # (sic) the reference indexes the second axis here, not the quaternion's w
        log_dict["avg_per_chunk_quat_magnitude"] = (2.0 * torch.sqrt(torch.clamp(1 - q[:, -1] ** 2,
                                                                                 min=0.0))).mean().item()
        if enc.shape[-1] == 8:
            log_dict["avg_per_chunk_scale"] = enc[..., 7].mean().item()
    if "memory_tokens" in pred_dict:
        first, last = pred_dict["memory_tokens"][0].cpu(), pred_dict["memory_tokens"][-1].cpu()
        log_dict["avg_memory_token_similarity"] = _offdiag_cosine(last)
        log_dict["avg_memory_token_similarity_first"] = _offdiag_cosine(first)
        pred_dict.pop("memory_tokens", None)


def gather_sequences(datasets: list, use_random_sequences: bool) -> list:
    """training_metrics.py:527-560: ``(dataset, index, name, number of frames)`` of one
    random sequence of one random dataset (numpy's global generator, dataset first), or
    of every sequence of every dataset in order."""
    def entry(ds, j):
        return ds, j, ds.get_seq_name(j), ds.seq_frame_num[j]
    if use_random_sequences:
        ds = datasets[np.random.randint(0, len(datasets))]
        return [entry(ds, np.random.randint(0, ds.sequence_list_len))]
    return [entry(ds, j) for ds in datasets for j in range(ds.sequence_list_len)]


def get_sequence_data(dataset, seq_index: int, seq_name: str, seq_num_frames: int) -> dict:
    """training_metrics.py:562-614: all frames of one sequence as host tensors with a
    leading batch axis of 1 -- images (1, S, 3, H, W) in [0, 1], GT extrinsics, points
    and depths expressed in the first camera's frame (not rescaled)."""
    raw = dataset.get_data(seq_index, -1, None, np.arange(seq_num_frames))

    def f32(key):
        return torch.from_numpy(np.stack(raw[key]).astype(np.float32))
    images = f32("images").contiguous().permute(0, 3, 1, 2).to(torch.get_default_dtype()).div(255)
    point_masks = torch.from_numpy(np.stack(raw["point_masks"]))
    with torch.amp.autocast("cuda", enabled=False):
        extrinsics, cam_points, world_points, depths = normalize_camera_extrinsics_and_points_batch(
            extrinsics=f32("extrinsics").unsqueeze(0), cam_points=f32("cam_points").unsqueeze(0),
            world_points=f32("world_points").unsqueeze(0), depths=f32("depths").unsqueeze(0),
            point_masks=point_masks.unsqueeze(0), scale_by_points=False)
    return {"dataset_name": dataset.__class__.__name__, "seq_name": seq_name,
            "ids": torch.from_numpy(raw["ids"]).unsqueeze(0), "images": images.unsqueeze(0), "depths": depths,
            "extrinsics": extrinsics, "intrinsics": f32("intrinsics").unsqueeze(0), "cam_points": cam_points,
            "world_points": world_points, "point_masks": point_masks.unsqueeze(0)}


def apply_sequence_to_model(batch: dict, model, chunk_width, num_overlap, sample_mode: str = "chunk_overlap",
                            alignment_type: Optional[str] = None, offload: bool = True) -> dict:
    """training_metrics.py:616-659, where the reference defines it: the sequence driver
    ``aligned_vggt.dist.pipeline.apply_sequence_to_model`` (chunk loop, grouped encodes,
    GT alignment, merge into overlap-free tensors; ``batch`` gains the merged GT).

    ``offload=True`` (the default) is that driver as it stands: older chunk outputs go to
    pinned host memory as they are produced, the merge and the alignment run on the host.
    ``offload=False`` runs the same driver inside ``utils.data.chunk_outputs_stay_in_place()``,
    which turns its host copies into no-ops: every chunk's outputs stay where the model
    left them and the merge and the GT alignment run on the device (with the GT tensors of
    ``batch`` there too, the pose-based alignments never visit the host)."""
    with contextlib.nullcontext() if offload else chunk_outputs_stay_in_place():
        return _pipeline.apply_sequence_to_model(batch, model, chunk_width, num_overlap, sample_mode, alignment_type)


def torch_quantile(input: torch.Tensor, q, dim: Optional[int] = None, keepdim: bool = False, *,
                   interpolation: str = "nearest", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One scalar quantile by ``torch.kthvalue`` (no 2^24-element limit), with the
    signature the reference keeps at training_metrics.py:663-732: ``q`` in [0, 1],
    ``interpolation`` "nearest" | "lower" | "higher", ``out`` must be None.  The
    preparation itself uses ``aligned_vggt.eval.quantile`` (a radix select on the device)."""
    try:
        q = float(q)
        ok = 0 <= q <= 1
    except Exception:
        ok = False
    if not ok:
        raise ValueError(f"torch_quantile: q must be one number in [0, 1], got {q!r}")
    rounders = {"nearest": round, "lower": floor, "higher": ceil}
    if interpolation not in rounders:
        raise ValueError(f"torch_quantile: interpolation must be one of {sorted(rounders)}, got {interpolation!r}")
    if out is not None:
        raise ValueError("torch_quantile: out= is not supported")
    flat = dim is None
    if flat:
        dim = 0
        input = input.reshape((-1,) + (1,) * (input.ndim - 1))
    k = rounders[interpolation](q * (input.shape[dim] - 1)) + 1
    res = torch.kthvalue(input, k, dim, keepdim=True)[0]
    if keepdim:
        return res
    return res.squeeze() if flat else res.squeeze(dim)
