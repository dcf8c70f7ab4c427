"""Generate tests/golden/multitask_loss.npz from the reference's own training/loss.py
(run where the reference checkout exists; the fixture is data only).

training/loss.py imports the ``vggt`` package at module level, which is not
available, so -- as gen_golden.py does -- the file is parsed with ``ast`` and only
its class and function definitions are executed.  What the missing imports would
have provided is supplied here:

  * ``check_and_fix_inf_nan``: the helper of aligned_vggt/training/loss.py
    (SPEC_ASSUMPTIONS.md A20).  Every input below is finite and every loss value
    is below 100, so the fixture does not depend on that assumption;
  * ``mat_to_quat`` / ``pose_encoding_to_extri_intri``: this repository's utils
    (pinned against VGGT's by the existing fixtures);
  * ``extri_intri_to_pose_encoding``: the same arithmetic without the final
    ``.float()``, so that the fixture is fp64 throughout;
  * ``compute_relative_poses``: extracted from the reference's own
    aligned_vggt/utils/geometry.py.

Everything runs on the CPU in fp64 (default dtype fp64, so the reference's
``torch.eye`` is fp64 too) on inputs that are exactly representable in fp32.
Cases (valid_range = 0.98 unless said): the four branches of the depth term --
n = 91 (skipped), n = 1006 (quantile taken, m <= 1000: unfiltered), n = 1036
(m = 1014: filtered), 2 x 3 x 14 x 37 with n = 2797 (filtered) -- and
valid_range = -1.

Usage:  python tests/golden/gen_loss.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import ast
import json
import os
import sys
from dataclasses import dataclass
from math import ceil, floor

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "large-scale-vit-slam_amd"))

CASES = [  # tag, (B, S, H, W), n, valid_range
    ("skipped", (1, 2, 14, 37), 91, 0.98),
    ("unfiltered", (1, 2, 14, 37), 1006, 0.98),
    ("filtered", (1, 2, 14, 37), 1036, 0.98),
    ("filtered_b2", (2, 3, 14, 37), 2797, 0.98),
    ("no_range", (2, 3, 14, 37), 2797, -1),
]
TOTAL_STEPS, CURRENT_STEP, SEED = 100, 20, 1234


def config(valid_range):
    return {"perFrameReg": {"weight": 0.1},
            "perChunkReg": {"weight": 0.05, "warmup_percent": 0.5, "warmup_type": "linear"},
            "depth": {"weight": 1.0, "valid_range": valid_range},
            "cameraPose": {"weight": 2.0, "loss_type": "l1"},
            "cameraPoseRel": {"weight": 0.5, "loss_type": "l1", "weight_trans": 1.0, "weight_rot": 2.0}}


def _definitions(path, names=None):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and (names is None or n.name in names)]
    return ast.Module(body=keep, type_ignores=[])


def reference_loss(ref):
    from aligned_vggt.training.loss import check_and_fix_inf_nan
    from aligned_vggt.utils.pose_enc import pose_encoding_to_extri_intri
    from aligned_vggt.utils.rotation import mat_to_quat

    def extri_intri_to_pose_encoding(extrinsics, intrinsics, image_size_hw=None, pose_encoding_type="absT_quaR_FoV"):
        H, W = image_size_hw
        fov_h = 2 * torch.atan((H / 2) / intrinsics[..., 1, 1])
        fov_w = 2 * torch.atan((W / 2) / intrinsics[..., 0, 0])
        return torch.cat([extrinsics[:, :, :3, 3], mat_to_quat(extrinsics[:, :, :3, :3]), fov_h[..., None],
                          fov_w[..., None]], dim=-1)

    geo = {"torch": torch, "__name__": "golden_extract"}
    exec(compile(_definitions(os.path.join(ref, "aligned_vggt/utils/geometry.py"), ["compute_relative_poses"]),
                 "geometry.py", "exec"), geo)
    g = {"torch": torch, "dataclass": dataclass, "ceil": ceil, "floor": floor, "__name__": "golden_extract",
         "check_and_fix_inf_nan": check_and_fix_inf_nan, "mat_to_quat": mat_to_quat,
         "extri_intri_to_pose_encoding": extri_intri_to_pose_encoding,
         "pose_encoding_to_extri_intri": pose_encoding_to_extri_intri,
         "compute_relative_poses": geo["compute_relative_poses"]}
    exec(compile(_definitions(os.path.join(ref, "training/loss.py")), "training/loss.py", "exec"), g)
    return g["MultitaskLoss"]


def _rotations(g, *lead):
    q = torch.randn(*lead, 4, generator=g, dtype=torch.float32).double()
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(*lead, 3, 3)


def inputs(ci, shape, n):
    """Seeded inputs, every one an fp32 value (stored as fp32, used as fp64)."""
    from aligned_vggt.utils.rotation import mat_to_quat
    B, S, H, W = shape
    g = torch.Generator().manual_seed(100 + ci)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    depth = 0.5 + 4.0 * torch.rand(B, S, H, W, 1, generator=g, dtype=torch.float32)
    gt = (depth[..., 0] * torch.exp(0.4 * r(B, S, H, W))).float()
    conf = 1.0 + torch.exp(r(B, S, H, W))
    mask = torch.zeros(B * S * H * W, dtype=torch.bool)
    mask[torch.randperm(B * S * H * W, generator=g)[:n]] = True
    extr = torch.cat([_rotations(g, B, S), r(B, S, 3, 1).double()], -1).float()
    intr = torch.zeros(B, S, 3, 3, dtype=torch.float32)
    intr[..., 0, 0] = 40.0 + 5.0 * torch.rand(B, S, generator=g, dtype=torch.float32)
    intr[..., 1, 1] = 30.0 + 5.0 * torch.rand(B, S, generator=g, dtype=torch.float32)
    intr[..., 0, 2], intr[..., 1, 2], intr[..., 2, 2] = W / 2, H / 2, 1.0
    e = extr.double()
    fov = torch.stack([2 * torch.atan((H / 2) / intr[..., 1, 1].double()),
                       2 * torch.atan((W / 2) / intr[..., 0, 0].double())], -1)
    pose = (torch.cat([e[..., :3, 3], mat_to_quat(e[..., :3, :3]), fov], -1) + 0.05 * r(B, S, 9).double()).float()
    frame = 0.1 * r(B, S - 1, 7)
    frame[..., 6] += 1.0
    chunk = 0.1 * r(B, 1, 8)
    chunk[..., 6] += 1.0
    chunk[..., 7] += 1.0
    return {"depth": depth, "depth_conf": conf, "pose_enc": pose, "frame_se3_alignment_enc": frame,
            "chunk_sim3_alignment_enc": chunk, "depths": gt, "point_masks": mask.view(B, S, H, W),
            "extrinsics": extr, "intrinsics": intr}


PRED_KEYS = ("depth", "depth_conf", "pose_enc", "frame_se3_alignment_enc", "chunk_sim3_alignment_enc")
GRAD_KEYS = ("depth", "pose_enc", "frame_se3_alignment_enc", "chunk_sim3_alignment_enc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (training/loss.py, aligned_vggt/utils)")
    a = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    MultitaskLoss = reference_loss(a.ref)
    out = {"cases": np.array(json.dumps([{"tag": t, "shape": s, "n": n, "valid_range": v, "config": config(v)}
                                         for t, s, n, v in CASES])),
           "total_steps": np.array(TOTAL_STEPS), "current_step": np.array(CURRENT_STEP), "seed": np.array(SEED)}
    for ci, (tag, shape, n, vr) in enumerate(CASES):
        x = inputs(ci, shape, n)
        B, S, H, W = shape
        assert int(x["point_masks"].sum()) == n
        pred = {k: x[k].double().requires_grad_(k in GRAD_KEYS) for k in PRED_KEYS}
        batch = {"depths": x["depths"].double(), "point_masks": x["point_masks"], "extrinsics": x["extrinsics"].double(),
                 "intrinsics": x["intrinsics"].double(), "images": torch.zeros(B, S, 3, H, W)}
        loss = MultitaskLoss(**config(vr))
        loss.setupScheduling(TOTAL_STEPS)
        torch.manual_seed(SEED)
        offset = int(torch.randint(int(S / 2), S, (1,)).item())  # what the forward below draws
        torch.manual_seed(SEED)
        d = loss(pred, batch, CURRENT_STEP)
        d["objective"].backward()
        for k, v in x.items():
            assert v.dtype in (torch.float32, torch.bool), (k, v.dtype)
            out[f"{tag}.in.{k}"] = v.numpy()
        out[f"{tag}.large_offset"] = np.array(offset)
        for k, v in d.items():
            assert torch.isfinite(v).all() and v.abs().max() < 100
            out[f"{tag}.loss.{k}"] = v.detach().numpy()
        for k in GRAD_KEYS:
            grad = pred[k].grad
            out[f"{tag}.grad.{k}"] = (torch.zeros_like(pred[k]) if grad is None else grad).numpy()
        print(tag, {k: float(v) for k, v in d.items()})
    np.savez_compressed(os.path.join(HERE, "multitask_loss.npz"), **out)
    print("wrote multitask_loss.npz", os.path.getsize(os.path.join(HERE, "multitask_loss.npz")), "bytes")


if __name__ == "__main__":
    main()
