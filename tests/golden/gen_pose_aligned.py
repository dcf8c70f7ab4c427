"""Generate tests/golden/ref_pose_aligned.npz from the reference's OWN
aligned_vggt/models/poseAligned_wrapped_vggt.py (run where the reference checkout
exists; the fixture is data only).

As gen_golden.py does for the feature-aligned model, the test-only ``vggt`` shim
(tests/golden/vggt_shim.py) stands in for the absent VGGT package: the stub
aggregator / camera / DPT heads return what ``_Feed`` holds, and the reference's
forward -- re-centring, GT scale through numpy, Markley mean over the overlap,
point transform, context bookkeeping -- runs unchanged over whole chunk sequences,
in fp32 on the CPU.

What is fed: one smooth global w2c trajectory per run; every chunk sees it through
its own rigid transform plus a little noise, with unnormalised quaternions
(|q| in 0.7 .. 1.4), so the overlap transforms of a chunk agree up to the noise
and no rotation is near 180 degrees.  GT poses are the same trajectory with
translations 2.5 x as large.  Dense maps are 6 x 8; images are not stored
(``images_of`` below is restated by the test).

Runs: (a) B = 2, three chunks of 4, ov = 2, all heads; (b) ov = 1; (c) a shorter
tail chunk; (d) GT poses on every chunk; (e) camera + depth only; (f) camera +
points only; (g) training=True (no ``images`` key).

Usage:  python tests/golden/gen_pose_aligned.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HW = (6, 8)

RUNS = [  # tag, B, chunk lengths, ov, gt, (camera, depth, point), training
    ("a", 2, (4, 4, 4), 2, False, (True, True, True), False),
    ("b", 1, (4, 4, 4), 1, False, (True, True, True), False),
    ("c", 1, (4, 4, 3), 2, False, (True, True, True), False),
    ("d", 2, (4, 4, 4), 2, True, (True, True, True), False),
    ("e", 1, (4, 4, 4), 2, False, (True, True, False), False),
    ("f", 1, (4, 4, 4), 2, False, (True, False, True), False),
    ("g", 1, (4, 4, 4), 2, False, (True, True, True), True),
]


def images_of(B, S):
    n = B * S * 3 * HW[0] * HW[1]
    return ((torch.arange(n) % 7).float() / 7.0).view(B, S, 3, *HW)


def _axis_angle(axis, angle):
    a = axis / axis.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _quat(R):
    """Unit xyzw quaternion of a rotation (the CPU oracle's mat_to_quat, fp64)."""
    from oracle import vggt_oracle as O
    q = O.mat_to_quat(R.view(1, 3, 3))[0].double()
    return q / q.norm()


def feeds(run_index, B, lengths, ov):
    """Per chunk: what the stub heads return (fp32) and the GT poses (B,S,3,4)."""
    g = torch.Generator().manual_seed(500 + run_index)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    starts = [0]
    for n in lengths[:-1]:
        starts.append(starts[-1] + n - ov)
    total = starts[-1] + lengths[-1]
    glob = torch.zeros(B, total, 4, 4, dtype=torch.float64)
    for b in range(B):
        axis, base = r(3), r(3)
        for f in range(total):
            glob[b, f, :3, :3] = _axis_angle(axis + 0.1 * r(3), 0.2 + 0.07 * f) @ _axis_angle(base, 0.3)
            glob[b, f, :3, 3] = 0.4 * f * torch.tensor([1.0, 0.2, -0.3], dtype=torch.float64) + 0.1 * r(3) + 0.5
            glob[b, f, 3, 3] = 1.0
    out = []
    H, W = HW
    for ci, (s0, S) in enumerate(zip(starts, lengths)):
        pose = torch.zeros(B, S, 9, dtype=torch.float64)
        for b in range(B):
            C = torch.eye(4, dtype=torch.float64)
            C[:3, :3] = _axis_angle(r(3), 0.5 + 0.2 * ci)
            C[:3, 3] = r(3)
            for f in range(S):
                P = torch.eye(4, dtype=torch.float64)
                P[:3, :3] = _axis_angle(r(3), 0.01)
                P[:3, 3] = 0.01 * r(3)
                E = glob[b, s0 + f] @ C @ P
                pose[b, f, :3] = E[:3, 3]
                pose[b, f, 3:7] = _quat(E[:3, :3]) * (0.7 + 0.7 * float(torch.rand(1, generator=g, dtype=torch.float64)))
        pose[..., 7:] = 0.3 + 1.2 * torch.rand(B, S, 2, generator=g, dtype=torch.float64)
        gt = glob[:, s0:s0 + S, :3, :].clone()
        gt[..., 3] *= 2.5
        out.append({"pose_enc": pose.float(),
                    "depth": (0.5 + 4.0 * torch.rand(B, S, H, W, 1, generator=g, dtype=torch.float64)).float(),
                    "depth_conf": (1.0 + torch.exp(r(B, S, H, W))).float(),
                    "points": (2.0 * r(B, S, H, W, 3)).float(),
                    "points_conf": (1.0 + torch.exp(r(B, S, H, W))).float(),
                    "gt": gt.float()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (aligned_vggt/models, aligned_vggt/utils)")
    a = ap.parse_args()
    for p in (ROOT, HERE, a.ref):  # the reference's aligned_vggt first
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    import vggt_shim as shim
    shim.install()
    from aligned_vggt.models.poseAligned_wrapped_vggt import VGGT  # the reference's module
    assert os.path.abspath(sys.modules[VGGT.__module__].__file__).startswith(os.path.abspath(a.ref))
    out = {"runs": np.array(json.dumps([{"tag": t, "B": B, "lengths": list(L), "ov": ov, "gt": gt, "heads": list(h),
                                         "training": tr} for t, B, L, ov, gt, h, tr in RUNS])),
           "hw": np.array(HW)}
    for ri, (tag, B, lengths, ov, use_gt, heads, training) in enumerate(RUNS):
        m = VGGT(enable_camera=heads[0], enable_depth=heads[1], enable_point=heads[2], enable_track=False)
        m.train(training)
        ctx = None
        fed = feeds(ri, B, lengths, ov)
        for ci, feed in enumerate(fed):
            shim._Feed.tokens = [torch.zeros(1)] * 4
            for k in ("pose_enc", "depth", "depth_conf", "points", "points_conf"):
                setattr(shim._Feed, k, feed[k])
            gt = feed["gt"].clone() if use_gt else None
            with torch.no_grad():
                new = m(images_of(B, lengths[ci]), ov, ctx, gt_poses=gt)
            assert ctx is None or all(new[k] is ctx[k] for k in new)
            if gt is not None:
                assert torch.equal(gt, feed["gt"])  # the reference pads into a new tensor
            ctx = new
            p = f"{tag}.{ci}."
            out[p + "in.pose_enc"] = feed["pose_enc"].numpy()
            if heads[1]:
                out[p + "in.depth"], out[p + "in.depth_conf"] = feed["depth"].numpy(), feed["depth_conf"].numpy()
            if heads[2]:
                out[p + "in.points"], out[p + "in.points_conf"] = feed["points"].numpy(), feed["points_conf"].numpy()
            if use_gt:
                out[p + "in.gt"] = feed["gt"].numpy()
        out[f"{tag}.keys"] = np.array(json.dumps(sorted(ctx.keys())))
        for k, v in ctx.items():
            assert len(v) == len(lengths), (tag, k)
            if k == "images":
                for ci, t in enumerate(v):
                    assert torch.equal(t, images_of(B, lengths[ci]))
                continue
            for ci, t in enumerate(v):
                assert t.dtype == torch.float32 and torch.isfinite(t).all(), (tag, k, ci)
                out[f"{tag}.{ci}.out.{k}"] = t.numpy()
        print(tag, sorted(ctx.keys()), [tuple(t.shape) for t in ctx["pose_enc"]])
    path = os.path.join(HERE, "ref_pose_aligned.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_pose_aligned.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
