#!/usr/bin/env python3
"""Speed of the GT depth-scale alignment of a training step (utils.alignment.scale_align_from_depths): the kernel
path (csrc/gt_align.hip: vggt_depth_scale_l1, then vggt_scale_f32) against the VGGT_GT_ALIGN=torch path (the
reference's chain of torch ops: sort with int64 indices, two gathers, cumsum, searchsorted, one .item() per batch
element) on the same GPU.

Shapes: 2 x 16 x 518 x 518 (two training chunks) and 1 x 512 x 154 x 518 (the long sequence).  Inputs are seeded and
synthetic, as scripts/bench_loss.py's: depths in 0.5-80 m, GT within a factor exp(N(0, 0.3)), confidences
1 + exp(N(0, 1)), GT masks 70 % set.  Device events around whole calls (host readbacks included, as a caller sees
them); ``--rounds`` rounds alternate the two sides in one process and the median round is reported, with every round
listed; a second figure ("cold") rewrites 512 MiB before every call, outside the timed window, so that the inputs
come from HBM and not from the 256 MiB last-level cache.  The peak device memory each side allocates beyond the
step's own tensors is reported too.  A call scales depth in place, so the depth drifts by the (near 1) scale from
call to call; the selected ratio drifts with it and the work per call does not change.  Prints one JSON line per
shape.

    python scripts/bench_gt_alignment.py [--shape 2 16 518 518] [--rounds 3] [--seconds 1.5] [--no-baseline]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT, os.path.join(ROOT, "scripts")]

from bench_loss import event_ms, median  # noqa: E402

SHAPES = ([2, 16, 518, 518], [1, 512, 154, 518])


def make_inputs(shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    depth = 0.5 + 79.5 * torch.rand(shape, generator=g)
    gt = depth * torch.exp(0.3 * torch.randn(shape, generator=g))
    conf = 1.0 + torch.exp(torch.randn(shape, generator=g))
    mask = torch.rand(shape, generator=g) < 0.7
    B, S = shape[:2]
    pred = {"depth": depth[..., None].to(dev), "depth_conf": conf.to(dev),
            "pose_enc": torch.randn(B, S, 9, generator=g).to(dev)}
    return pred, {"depths": gt.to(dev), "point_masks": mask.to(dev)}


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench(shape, rounds, seconds, baseline):
    from aligned_vggt.utils import alignment as A
    dev = torch.device("cuda:0")
    pred, batch = make_inputs(tuple(shape), dev)
    depth0 = pred["depth"].clone()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    win = seconds * 1e3 / rounds

    def side(knob):
        def call():
            os.environ["VGGT_GT_ALIGN"] = knob
            A.scale_align_from_depths(pred, batch)
        return call

    ours, base = side("kernel"), side("torch")

    def first(fn):
        pred["depth"].copy_(depth0)
        fn()
        return [float(s) for s in pred["alignment_scales"]]

    rec = {"shape": shape, "scales": first(ours), "extra_mib": peak_extra_mib(ours)}
    if baseline:
        rec["torch_scales"] = first(base)
        rec["torch_extra_mib"] = peak_extra_mib(base)
    t_ours, t_base, c_ours, c_base = [], [], [], []
    for _ in range(rounds):
        t_ours.append(event_ms(ours, win))
        c_ours.append(event_ms(ours, win / 4, flush))
        if baseline:
            t_base.append(event_ms(base, win))
            c_base.append(event_ms(base, win / 4, flush))
    rec.update(ms_rounds=[round(t, 4) for t in t_ours], ms=median(t_ours), cold_ms_rounds=[round(t, 4) for t in c_ours],
               cold_ms=median(c_ours))
    if baseline:
        rec.update(torch_ms_rounds=[round(t, 4) for t in t_base], torch_ms=median(t_base),
                   torch_cold_ms_rounds=[round(t, 4) for t in c_base], torch_cold_ms=median(c_base),
                   speedup=median(t_base) / median(t_ours), cold_speedup=median(c_base) / median(c_ours),
                   faster_in_every_round=all(o < b for o, b in zip(t_ours + c_ours, t_base + c_base)))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=4, type=int, default=None, help="one shape instead of the two documented ones")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side and sweep, over all rounds")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    knob = os.environ.get("VGGT_GT_ALIGN")
    try:
        for shape in ([args.shape] if args.shape else SHAPES):
            bench(shape, args.rounds, args.seconds, not args.no_baseline)
            torch.cuda.empty_cache()
    finally:
        if knob is None:
            os.environ.pop("VGGT_GT_ALIGN", None)
        else:
            os.environ["VGGT_GT_ALIGN"] = knob


if __name__ == "__main__":
    main()
