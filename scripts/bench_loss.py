#!/usr/bin/env python3
"""Speed of the depth term of MultitaskLoss, forward plus backward (training.loss.compute_depth_loss:
vggt_depth_loss_values, vggt_depth_loss_reduce, vggt_depth_loss_bwd), against the same protocol composed from
torch ops on the same GPU (what the reference's compute_depth_loss / filter_by_quantile do: boolean-index gathers,
per-frame amax, logs, clamp, torch.kthvalue, compare, gather, scrub, mean, and autograd backwards through them).

Shape: 1 x 16 x 518 x 518 (one training chunk), valid_range = 0.98.  Inputs are seeded and synthetic: depths in
0.5-80 m, GT within a factor exp(N(0, 0.3)), confidences 1 + exp(N(0, 1)), GT masks 70 % set.  Device events
around whole forward + backward calls (host readbacks included, as a caller sees them); ``--rounds`` rounds
alternate the two sides in one process and the median round is reported, with every round listed; a second figure
("cold") rewrites 512 MiB before every call, outside the timed window, so that the inputs come from HBM and not
from the 256 MiB last-level cache.  The forward alone (no autograd) is timed as well.  Prints one JSON line.

    python scripts/bench_loss.py [--shape 1 16 518 518] [--rounds 3] [--seconds 1.5] [--no-baseline]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT]


def make_inputs(shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    depth = 0.5 + 79.5 * torch.rand(shape, generator=g)
    gt = depth * torch.exp(0.3 * torch.randn(shape, generator=g))
    conf = 1.0 + torch.exp(torch.randn(shape, generator=g))
    mask = torch.rand(shape, generator=g) < 0.7
    pred = {"depth": depth[..., None].to(dev).requires_grad_(True), "depth_conf": conf.to(dev)}
    return pred, {"depths": gt.to(dev), "point_masks": mask.to(dev)}


# ---------------------------------------------------------------- the torch composition (the reference's steps)
def _fix(t, hard_max=100):
    if torch.isnan(t).any() or torch.isinf(t).any():
        t = torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    return t if hard_max is None else t.clamp(min=-hard_max, max=hard_max)


def torch_depth_loss(pred, batch, valid_range, min_elements=1000, hard_max=100):
    depth, conf = pred["depth"], pred["depth_conf"]
    gt = _fix(batch["depths"], None)[..., None]
    mask = batch["point_masks"].clone()
    if mask.sum() < 100:
        return (0.0 * depth).mean()
    conf = conf / conf.amax(dim=(2, 3), keepdim=True).clamp_min(1e-8)
    loss = (torch.log(depth[mask].clamp_min(1e-8)) - torch.log(gt[mask].clamp_min(1e-8))).abs().squeeze(-1) * conf[mask]
    if valid_range > 0 and loss.numel() > min_elements:
        loss = loss.clamp(max=hard_max)
        k = round(valid_range * (loss.numel() - 1)) + 1
        thr = min(torch.kthvalue(loss.detach().reshape(-1), k).values, hard_max)
        keep = loss < thr
        if keep.sum() > min_elements:
            loss = loss[keep]
    return _fix(loss).mean()


def event_ms(fn, min_ms, flush=None):
    """ms per call over at least `min_ms` of timed work: device events around each call (the host work between
    its launches included).  With `flush`, a buffer larger than the 256 MiB last-level cache is rewritten before
    every call, outside the timed window, so the call finds its inputs in HBM as after a model's forward pass."""
    total, calls = 0.0, 0
    while total < min_ms or calls == 0:
        if flush is not None:
            flush.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        calls += 1
    return total / calls


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=4, type=int, default=[1, 16, 518, 518])
    ap.add_argument("--valid-range", type=float, default=0.98)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side and sweep, over all rounds")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()

    from aligned_vggt.training.loss import compute_depth_loss
    dev = torch.device("cuda:0")
    pred, batch = make_inputs(tuple(args.shape), dev)
    vr = args.valid_range
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    win = args.seconds * 1e3 / args.rounds

    def run(fwd):
        pred["depth"].grad = None
        loss = fwd()
        loss.backward()
        return loss

    fwd_ours = lambda: compute_depth_loss(pred, batch, valid_range=vr)["loss_depth"]  # noqa: E731
    fwd_base = lambda: torch_depth_loss(pred, batch, vr)  # noqa: E731
    ours, base = (lambda: run(fwd_ours)), (lambda: run(fwd_base))
    rec = {"shape": args.shape, "valid_range": vr, "loss": float(ours().detach())}
    g_ours = pred["depth"].grad.clone()
    if not args.no_baseline:
        rec["torch_loss"] = float(base().detach())
        rec["max_abs_grad_diff_vs_torch"] = float((pred["depth"].grad - g_ours).abs().max())
    t_ours, t_base, c_ours, c_base, f_ours, f_base = [], [], [], [], [], []
    for _ in range(args.rounds):
        t_ours.append(event_ms(ours, win))
        c_ours.append(event_ms(ours, win / 4, flush))
        with torch.no_grad():
            f_ours.append(event_ms(fwd_ours, win / 4))
        if not args.no_baseline:
            t_base.append(event_ms(base, win))
            c_base.append(event_ms(base, win / 4, flush))
            with torch.no_grad():
                f_base.append(event_ms(fwd_base, win / 4))
    rec.update(ms_rounds=[round(t, 4) for t in t_ours], ms=median(t_ours), cold_ms_rounds=[round(t, 4) for t in c_ours],
               cold_ms=median(c_ours), forward_ms=median(f_ours))
    if not args.no_baseline:
        rec.update(torch_ms_rounds=[round(t, 4) for t in t_base], torch_ms=median(t_base),
                   torch_cold_ms_rounds=[round(t, 4) for t in c_base], torch_cold_ms=median(c_base),
                   torch_forward_ms=median(f_base), speedup=median(t_base) / median(t_ours),
                   cold_speedup=median(c_base) / median(c_ours),
                   faster_in_every_round=all(o < b for o, b in zip(t_ours + c_ours, t_base + c_base)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
