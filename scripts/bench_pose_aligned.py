#!/usr/bin/env python3
"""Speed of the pose-aligned VGGT's per-chunk alignment (models.poseAligned_wrapped_vggt.align_chunk) at the shipped
configuration's shape -- B = 1, chunks of 75 frames of 154 x 518, overlap 30, camera and depth heads
(test_poseAlignedWrappedVGGT_vkitti.yaml) -- on one GPU:

    hip         the default: vggt_pose_align (one launch), vggt_scale_f32 for the depth with GT
    torch       VGGT_POSE=device: the reference's operations as torch ops on the device (the 4 x 4 eigenproblem of
                the Markley mean on the host, as utils.geometry.averagePoseEncodings)
    reference   the reference's composition restated with its host round trip: the translations copied to numpy,
                scale_lse_solver per batch element, the translations and the depth scaled per batch element
                (poseAligned_wrapped_vggt.py:95-104, :144-146); with GT only

each with a context and no GT (the Markley path) and with a context and GT (``chunk_gt``).  Device events around
whole calls (the host work between the launches included); ``--rounds`` rounds alternate the sides in one process,
every round is listed and the median reported.  A call with GT scales the depth in place: the GT translations are
the predicted ones plus 0.1 % noise, so the scale stays near 1 and the depth does not drift away.  ``--forward``
adds the whole per-chunk forward (aggregator, camera and depth heads, alignment) of a synthetic-weight model, hip
against torch.  ``--compose`` times vggt_pose_compose (the feature-aligned model's composition, one launch) alone
instead, through the C ABI into preallocated outputs, with a context (the Markley mean over the overlap) and without.
Prints one JSON line per measurement.

    python scripts/bench_pose_aligned.py [--frames 75] [--overlap 30] [--rounds 3] [--seconds 1.5] [--forward]
    python scripts/bench_pose_aligned.py --compose
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT, os.path.join(ROOT, "scripts")]

from bench_loss import event_ms, median  # noqa: E402

H, W = 154, 518


def make_chunk(PA, B, S, ov, dev, seed=0):
    """Raw head outputs of one chunk, the previous chunk's aligned encoding (its last ov frames consistent with this
    chunk's first ov up to a little noise) and GT poses whose centred translations are the predicted ones."""
    from aligned_vggt.utils.data import pose_encoding_to_extri
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * (0.7 + 0.6 * torch.rand(B, S, 1, generator=g))
    pose = torch.cat([torch.randn(B, S, 3, generator=g), q, 0.4 + torch.rand(B, S, 2, generator=g)], -1)
    first, _, _ = PA.align_chunk_poses(pose.double(), (H, W), ov, form="torch")  # re-centred, fp64
    extr = pose_encoding_to_extri(first)
    move = pose_encoding_to_extri(torch.tensor([0.3, -0.2, 0.5, 0.1, 0.2, -0.1, 0.9], dtype=torch.float64).view(1, 1, 7))
    prev = PA._extri_to_pose_encoding(extr @ move)
    prev = torch.cat([prev + 1e-3 * torch.randn(prev.shape, generator=g).double(), first[..., 7:]], -1).float()
    prev = torch.roll(prev, S - ov, dims=1)  # the previous chunk's last ov frames are this chunk's first ov
    gt = extr[:, :, :3, :].clone()
    gt[..., 3] *= 1.0 + 1e-3 * torch.randn(B, S, 3, generator=g).double()
    enc = {"images": torch.zeros(1, device=dev).expand(B, S, 3, H, W), "pose_enc": pose.to(dev),
           "depth": (0.5 + 79.5 * torch.rand(B, S, H, W, 1, generator=g)).to(dev),
           "depth_conf": (1.0 + torch.rand(B, S, H, W, generator=g)).to(dev)}
    return enc, prev.to(dev).contiguous(), gt.float().to(dev).contiguous()


def reference_align(enc, ov, ctx_pe, gt_poses):
    """The reference's per-chunk composition with GT, restated with this package's helpers, host round trip included."""
    import torch.nn.functional as F
    from aligned_vggt.utils.alignment import scale_lse_solver
    from aligned_vggt.utils.geometry import closed_form_inverse_se3
    from aligned_vggt.utils.pose_enc import extri_intri_to_pose_encoding, pose_encoding_to_extri_intri
    B, S = enc["pose_enc"].shape[:2]
    extr, intr = pose_encoding_to_extri_intri(enc["pose_enc"], image_size_hw=(H, W))
    extr = F.pad(extr, (0, 0, 0, 1, 0, 0, 0, 0))
    extr[:, :, 3, 3] = 1.0
    extr = extr @ closed_form_inverse_se3(extr[:, 0]).view(B, 1, 4, 4)
    gt = F.pad(gt_poses, (0, 0, 0, 1, 0, 0, 0, 0))
    gt[:, :, 3, 3] = 1.0
    centred = gt @ closed_form_inverse_se3(gt[:, 0]).view(B, 1, 4, 4)
    gt_pos, pred_pos = centred[..., :3, 3].cpu().numpy(), extr[..., :3, 3].cpu().numpy()
    depth = enc["depth"]
    for b in range(B):
        s = scale_lse_solver(pred_pos[b], gt_pos[b])
        extr[b, :, :3, 3] *= s
        depth[b, ...] *= s
    aligned = torch.matmul(extr, gt[:, :1])
    return extri_intri_to_pose_encoding(aligned, intr, image_size_hw=(H, W)), depth


def rounds_of(sides, rounds, win):
    """{name: fn} -> {name: [ms per round]}, the sides alternating within every round."""
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(event_ms(fn, win))
    return ms


def report(what, ms, against="hip"):
    rec = {"what": what}
    for k, v in ms.items():
        rec[k + "_ms_rounds"] = [round(t, 4) for t in v]
        rec[k + "_ms"] = round(median(v), 4)
    for k, v in ms.items():
        if k != against:
            rec[f"{against}_faster_than_{k}_in_every_round"] = all(a < b for a, b in zip(ms[against], v))
            rec[f"{k}_over_{against}"] = round(median(v) / median(ms[against]), 2)
    print(json.dumps(rec), flush=True)


def compose_only(enc, prev, B, S, ov, dev, rounds, win):
    """vggt_pose_compose alone: device events around the one call, every round listed."""
    from aligned_vggt import _native as N
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B, S, 4, generator=g)
    frame = torch.cat([0.1 * torch.randn(B, S, 3, generator=g), q / q.norm(dim=-1, keepdim=True)], -1)
    chunk = torch.cat([frame[:, 0], 1.0 + 0.1 * torch.rand(B, 1, generator=g)], -1).to(dev).contiguous()
    frame = frame[:, 1:].to(dev).contiguous()
    cam = enc["pose_enc"].contiguous()
    out, pt = torch.empty(B, S, 9, device=dev), torch.empty(B, 4, 4, device=dev)
    L, p = N.lib(), N._p

    def call(ctx):
        def run():
            rc = L.vggt_pose_compose(p(chunk), p(frame), p(cam), p(ctx), ctx.shape[1] if ctx is not None else 0, None,
                                     B, S, ov, H, W, p(out), p(pt), N._stream())
            assert rc == 0, rc
        return run

    for name, ctx in (("context", prev), ("no context", None)):
        call(ctx)()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        ms = rounds_of({"hip": call(ctx)}, rounds, win)
        print(json.dumps({"what": f"vggt_pose_compose B={B} S={S} ov={ov} {name}",
                          "hip_us_rounds": [round(1e3 * t, 2) for t in ms["hip"]],
                          "hip_us": round(1e3 * median(ms["hip"]), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=75)
    ap.add_argument("--overlap", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side, over all rounds")
    ap.add_argument("--forward", action="store_true", help="also time the whole per-chunk forward")
    ap.add_argument("--compose", action="store_true", help="time vggt_pose_compose alone, and nothing else")
    args = ap.parse_args()
    from aligned_vggt.models import poseAligned_wrapped_vggt as PA
    dev = torch.device("cuda:0")
    B, S, ov = 1, args.frames, args.overlap
    enc, prev, gt = make_chunk(PA, B, S, ov, dev)
    win = args.seconds * 1e3 / args.rounds
    if args.compose:
        return compose_only(enc, prev, B, S, ov, dev, args.rounds, win)
    knob = os.environ.get("VGGT_POSE")

    def align(mode, use_gt):
        def call():
            os.environ["VGGT_POSE"] = mode
            ctx = {"pose_enc": [prev], "depth": [enc["depth"]], "depth_conf": [enc["depth_conf"]], "images": [enc["images"]]}
            return PA.align_chunk(dict(enc), ov, ctx, gt if use_gt else None, False)
        return call

    try:
        for use_gt in (False, True):
            sides = {"hip": align("hip", use_gt), "torch": align("device", use_gt)}
            if use_gt:
                sides["reference"] = lambda: reference_align(enc, ov, prev, gt)
            a, b = sides["hip"]()["pose_enc"][-1], sides["torch"]()["pose_enc"][-1]
            err = float((a[..., :3] - b[..., :3]).norm() / b[..., :3].norm())
            report(f"align_chunk B={B} S={S} ov={ov} {H}x{W} {'context + GT' if use_gt else 'context'} "
                   f"(hip vs torch translation rel {err:.1e})", rounds_of(sides, args.rounds, win))
        if args.forward:
            from aligned_vggt.utils.synthetic import condition_pose_outputs_, synthetic_images, synthetic_init_
            model = PA.VGGT(enable_point=False, enable_track=False)
            synthetic_init_(model, seed=0)
            condition_pose_outputs_(model)
            model = model.to(dev).eval()
            x = synthetic_images(B, S, H, W, seed=1234, device="cpu").to(dev)
            ctx0 = model(x, ov)

            def forward(mode):
                def call():
                    os.environ["VGGT_POSE"] = mode
                    return model(x, ov, {k: list(v) for k, v in ctx0.items()})
                return call

            report(f"forward B={B} S={S} ov={ov} {H}x{W} camera + depth, second chunk",
                   rounds_of({"hip": forward("hip"), "torch": forward("device")}, args.rounds, 2 * win))
    finally:
        if knob is None:
            os.environ.pop("VGGT_POSE", None)
        else:
            os.environ["VGGT_POSE"] = knob


if __name__ == "__main__":
    main()
