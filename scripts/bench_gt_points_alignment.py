#!/usr/bin/env python3
"""Speed of the GT alignment sim3_from_points of a merged sequence (utils.data.alignAndConvertOutputs with
"sim3_from_points"): the kernel route (csrc/gt_points.hip: vggt_gt_points_align, then vggt_sim3_points and the pose
chain from device memory) against VGGT_GT_ALIGN=torch (the reference's host code: four .cpu() copies of the first
seq_width frames, numpy's percentile, boolean selection and SVD, and the result copied back) on the same GPU.

Shapes: 1 x 16 x 154 x 518 and 2 x 16 x 518 x 518 with both dense heads, seq_width = 16.  Inputs are seeded and
synthetic: predicted points N(0, (3, 2, 1)), GT a similarity of them plus noise, confidences 1 + exp(N(0, 1)), GT
masks 70 % set.  Every call gets the outputs as one-chunk lists, as the sequence driver hands them over (the merge is
then a copy, the same on both sides).  Wall clock between device synchronisations around whole calls; ``--rounds``
rounds alternate the two sides in one process and the median round is reported, with every round listed.  Prints
one JSON line per shape.

    python scripts/bench_gt_points_alignment.py [--shape 1 16 154 518] [--rounds 3] [--calls 5] [--no-baseline]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT, os.path.join(ROOT, "scripts")]

SHAPES = ([1, 16, 154, 518], [2, 16, 518, 518])


def make_inputs(shape, dev, seed=0):
    B, S, H, W = shape
    g = torch.Generator().manual_seed(seed)
    wp = torch.randn(B, S, H, W, 3, generator=g) * torch.tensor([3.0, 2.0, 1.0])
    R0 = torch.tensor([[0.7648, -0.6442, 0.0], [0.6442, 0.7648, 0.0], [0.0, 0.0, 1.0]])
    gt = 1.4 * wp @ R0.T + torch.tensor([0.5, -1.0, 2.0]) + 0.05 * torch.randn(B, S, H, W, 3, generator=g)
    q = torch.randn(B, S, 4, generator=g)
    enc = torch.cat([torch.randn(B, S, 3, generator=g), q / q.norm(dim=-1, keepdim=True),
                     0.8 + 0.5 * torch.rand(B, S, 2, generator=g)], -1)
    pred = {"pose_enc": enc, "world_points": wp, "world_points_conf": 1.0 + torch.exp(torch.randn(B, S, H, W, generator=g)),
            "depth": 0.5 + 79.5 * torch.rand(B, S, H, W, 1, generator=g),
            "depth_conf": 1.0 + torch.rand(B, S, H, W, generator=g)}
    batch = {"images": torch.zeros(B, S, 3, H, W), "world_points": gt, "point_masks": torch.rand(B, S, H, W, generator=g) < 0.7,
             "extrinsics": torch.eye(4)[:3].expand(B, S, 3, 4).contiguous()}
    return {k: v.to(dev) for k, v in pred.items()}, {k: v.to(dev) for k, v in batch.items()}


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def median(v):
    s = sorted(v)
    return round(s[len(s) // 2], 4)


def bench(shape, rounds, calls, baseline):
    from aligned_vggt.utils.data import alignAndConvertOutputs
    dev = torch.device("cuda:0")
    pred, batch = make_inputs(tuple(shape), dev)
    last = {}

    def side(knob):
        def call():
            os.environ["VGGT_GT_ALIGN"] = knob
            p = {k: [v] for k, v in pred.items()}
            cb = {k: [v] for k, v in batch.items()}
            alignAndConvertOutputs(p, {}, cb, "sim3_from_points", shape[1], 0)
            last[knob] = p
        return call

    ours, base = side("kernel"), side("torch")
    ours()
    rec = {"shape": shape, "pixels_per_element": shape[1] * shape[2] * shape[3]}
    if baseline:
        base()
        a, b = last["kernel"]["world_points"], last["torch"]["world_points"]
        rec["max_abs_diff_vs_torch"] = float((a - b).abs().max())
    t_ours, t_base = [], []
    for _ in range(rounds):
        t_ours.append(wall_ms(ours, calls))
        if baseline:
            t_base.append(wall_ms(base, calls))
    rec.update(ms_rounds=[round(t, 4) for t in t_ours], ms=median(t_ours))
    if baseline:
        rec.update(torch_ms_rounds=[round(t, 4) for t in t_base], torch_ms=median(t_base),
                   speedup=round(median(t_base) / median(t_ours), 2),
                   faster_in_every_round=all(o < b for o, b in zip(t_ours, t_base)))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=4, type=int, default=None, help="one shape instead of the two documented ones")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="calls per side and round")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    knob = os.environ.get("VGGT_GT_ALIGN")
    try:
        for shape in ([args.shape] if args.shape else SHAPES):
            bench(shape, args.rounds, args.calls, not args.no_baseline)
            torch.cuda.empty_cache()
    finally:
        if knob is None:
            os.environ.pop("VGGT_GT_ALIGN", None)
        else:
            os.environ["VGGT_GT_ALIGN"] = knob


if __name__ == "__main__":
    main()
