#!/usr/bin/env python3
"""Speed of the point-cloud preparation before ICP (eval.masked_clouds: vggt_kth_value_f32,
vggt_subsample_mask_count, vggt_prepare_clouds) against the same protocol composed from torch ops on the
same GPU (unproject_depth_map_to_point_map, torch.kthvalue, F.interpolate, boolean indexing: what
training_metrics.py:264-355 does, on the device instead of the host).

Shapes: 1 x 512 x 154 x 518 with max_points_icp = 500000 (a full sequence) and 1 x 16 x 518 x 518 with 250000
(a batch item).  Inputs are seeded and synthetic: depths in 1-80 m, confidences 1 + exp(N(0, 1)), GT masks 70 %
set, cameras on a circle.  Device events around whole calls (host readbacks included, as a caller sees them);
``--rounds`` rounds alternate the two sides in one process and the median round is reported, with every round
listed; a second figure ("cold") rewrites 512 MiB before every call, outside the timed window, so that the
inputs come from HBM and not from the 256 MiB last-level cache.  Each side's stages -- quantile, factor search,
final pass -- are timed the same way in a second sweep.  Prints one JSON line per shape and a markdown table.

    python scripts/bench_prepare_points.py [--shapes full item] [--rounds 3] [--seconds 1.5] [--no-baseline]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT]

SHAPES = {"full": ((1, 512, 154, 518), 500_000), "item": ((1, 16, 518, 518), 250_000)}


def make_inputs(shape, dev, seed=0):
    from aligned_vggt.utils.geometry import unproject_depth_map_to_point_map
    B, S, H, W = shape
    g = torch.Generator().manual_seed(seed)
    depth = (1.0 + 79.0 * torch.rand(shape, generator=g)).to(dev)
    conf = (1.0 + torch.exp(torch.randn(shape, generator=g))).to(dev)
    mask = (torch.rand(shape, generator=g) < 0.7).to(dev)
    ang = torch.linspace(0, 6.28, S).repeat(B, 1)
    R = torch.zeros(B, S, 3, 3)
    R[..., 0, 0], R[..., 0, 2], R[..., 2, 0], R[..., 2, 2], R[..., 1, 1] = ang.cos(), ang.sin(), -ang.sin(), ang.cos(), 1
    extr = torch.cat([R, 5.0 * torch.randn(B, S, 3, 1, generator=g)], -1).to(dev)
    intr = torch.zeros(B, S, 3, 3)
    intr[..., 0, 0] = intr[..., 1, 1] = 0.9 * W
    intr[..., 0, 2], intr[..., 1, 2], intr[..., 2, 2] = W / 2, H / 2, 1.0
    intr = intr.to(dev)
    gt_depth = (depth * (1.0 + 0.01 * torch.randn(shape, generator=g).to(dev)))[..., None]
    gt_points = unproject_depth_map_to_point_map(gt_depth, extr, intr).contiguous()
    pred = {"depth": depth[..., None], "depth_conf": conf}
    gt = {"world_points": gt_points, "point_masks": mask}
    return pred, gt, extr, intr


# ---------------------------------------------------------------- the torch composition, stage by stage
def torch_quantile_stage(conf, q):
    from aligned_vggt.eval import quantile_rank
    return torch.kthvalue(conf.reshape(-1), quantile_rank(conf.numel(), q)).values


def torch_search_stage(mask, max_points):
    from aligned_vggt.eval import search_subsample_factor
    B, S, H, W = mask.shape
    pre = mask.reshape(B * S, 1, H, W).float()

    def count(f):
        sub = F.interpolate(pre, size=(H // f, W // f), mode="bilinear", align_corners=False)
        return (sub > 0.5).sum().item()
    return search_subsample_factor(count, mask.sum().item(), max_points, H, W)[0]


def torch_final_stage(pred, gt, extr, intr, thr, f):
    from aligned_vggt.utils.geometry import unproject_depth_map_to_point_map
    B, S, H, W = gt["point_masks"].shape
    points = unproject_depth_map_to_point_map(pred["depth"], extr, intr)
    pmask = pred["depth_conf"] > thr
    gmask = gt["point_masks"]
    gpts = gt["world_points"]
    if f > 1:
        size = (H // f, W // f)

        def sub(x, c):
            y = F.interpolate(x.reshape(B, S, H, W, c).permute(0, 1, 4, 2, 3).reshape(B * S, c, H, W).float(), size=size,
                              mode="bilinear", align_corners=False)
            return y.view(B, S, c, *size).permute(0, 1, 3, 4, 2)
        points, gpts = sub(points, 3), sub(gpts, 3)
        pmask, gmask = sub(pmask, 1).squeeze(-1) > 0.5, sub(gmask, 1).squeeze(-1) > 0.5
    pc = [points[b][torch.logical_and(pmask[b], gmask[b])] for b in range(B)]
    gc = [gpts[b][gmask[b]] for b in range(B)]
    return pc, gc


def torch_protocol(pred, gt, extr, intr, q, max_points):
    thr = torch_quantile_stage(pred["depth_conf"], q)
    f = torch_search_stage(gt["point_masks"], max_points)
    return torch_final_stage(pred, gt, extr, intr, thr, f) + (f,)


# ---------------------------------------------------------------- the kernel path, stage by stage
def ours_search_stage(mask, max_points):
    from aligned_vggt import _native
    from aligned_vggt.eval import search_subsample_factor
    B, S, H, W = mask.shape
    count = torch.empty((), device=mask.device, dtype=torch.int64)
    valid = int(_native.subsample_mask_count(mask, H, W, out=count).item())
    return search_subsample_factor(lambda f: int(_native.subsample_mask_count(mask, H // f, W // f, out=count).item()),
                                   valid, max_points, H, W)[0]


def ours_final_stage(pred, gt, extr, intr, thr, f):
    from aligned_vggt import _native
    from aligned_vggt.utils.geometry import closed_form_inverse_se3
    B, S, H, W = gt["point_masks"].shape
    kinv = torch.inverse(intr).contiguous()
    c2w = closed_form_inverse_se3(extr.reshape(B * S, 3, 4))[:, :3, :].reshape(B, S, 3, 4).contiguous()
    args = (pred["depth"].reshape(B, S, H, W), kinv, c2w, None, pred["depth_conf"], thr, gt["world_points"],
            gt["point_masks"], H // f, W // f)
    pl, gl, ws = _native.prepare_clouds(*args, phase=_native.PREPARE_COUNT)
    lens = torch.stack([pl, gl]).cpu()
    pc = torch.zeros(B, int(lens[0].max()), 3, device=thr.device)
    gc = torch.zeros(B, int(lens[1].max()), 3, device=thr.device)
    _native.prepare_clouds(*args, pred_cloud=pc, gt_cloud=gc, pred_len=pl, gt_len=gl, phase=_native.PREPARE_SCATTER,
                           ws=ws)
    return pc, gc


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
    ap.add_argument("--shapes", nargs="+", default=["full", "item"], choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side, shape and sweep, over all rounds")
    ap.add_argument("--quantile", type=float, default=0.25)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()

    from aligned_vggt.eval import masked_clouds, quantile
    dev = torch.device("cuda:0")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    win = args.seconds * 1e3 / args.rounds
    rows = []
    for name in args.shapes:
        shape, max_points = SHAPES[name]
        pred, gt, extr, intr = make_inputs(shape, dev)
        q = args.quantile
        ours = lambda: masked_clouds(pred, gt, extr, intr, q, max_points)  # noqa: E731
        base = lambda: torch_protocol(pred, gt, extr, intr, q, max_points)  # noqa: E731
        pc, pl, gc, gl, f = ours()  # warm-up
        rec = {"shape": list(shape), "max_points_icp": max_points, "factor": f, "pred_len": pl.tolist(),
               "gt_len": gl.tolist()}
        if not args.no_baseline:
            tpc, tgc, tf = base()
            rec["torch_factor"] = tf
            rec["torch_lens_equal"] = [int(t.shape[0]) for t in tpc] == pl.tolist() and \
                [int(t.shape[0]) for t in tgc] == gl.tolist()
            if rec["torch_lens_equal"]:
                rec["max_abs_diff_vs_torch"] = max(
                    max(float((tpc[b] - pc[b, :tpc[b].shape[0]]).abs().max()) for b in range(shape[0])),
                    max(float((tgc[b] - gc[b, :tgc[b].shape[0]]).abs().max()) for b in range(shape[0])))
            del tpc, tgc
        t_ours, t_base, c_ours, c_base = [], [], [], []
        for _ in range(args.rounds):
            t_ours.append(event_ms(ours, win))
            c_ours.append(event_ms(ours, win / 4, flush))
            if not args.no_baseline:
                t_base.append(event_ms(base, win))
                c_base.append(event_ms(base, win / 4, flush))
        rec["ms_rounds"] = [round(t, 3) for t in t_ours]
        rec["ms"] = median(t_ours)
        rec["cold_ms_rounds"] = [round(t, 3) for t in c_ours]
        rec["cold_ms"] = median(c_ours)
        # stages
        thr = quantile(pred["depth_conf"], q)
        st = {"quantile": [], "search": [], "final": []}
        sb = {"quantile": [], "search": [], "final": []}
        for _ in range(args.rounds):
            st["quantile"].append(event_ms(lambda: quantile(pred["depth_conf"], q), win / 4))
            st["search"].append(event_ms(lambda: ours_search_stage(gt["point_masks"], max_points), win / 4))
            st["final"].append(event_ms(lambda: ours_final_stage(pred, gt, extr, intr, thr, f), win / 4))
            if not args.no_baseline:
                sb["quantile"].append(event_ms(lambda: torch_quantile_stage(pred["depth_conf"], q), win / 4))
                sb["search"].append(event_ms(lambda: torch_search_stage(gt["point_masks"], max_points), win / 4))
                sb["final"].append(event_ms(lambda: torch_final_stage(pred, gt, extr, intr, thr, f), win / 4))
        rec["stage_ms"] = {k: round(median(v), 3) for k, v in st.items()}
        if not args.no_baseline:
            rec["torch_ms_rounds"] = [round(t, 3) for t in t_base]
            rec["torch_ms"] = median(t_base)
            rec["torch_cold_ms_rounds"] = [round(t, 3) for t in c_base]
            rec["torch_cold_ms"] = median(c_base)
            rec["cold_speedup"] = rec["torch_cold_ms"] / rec["cold_ms"]
            rec["speedup"] = rec["torch_ms"] / rec["ms"]
            rec["faster_in_every_round"] = all(o < b for o, b in zip(t_ours + c_ours, t_base + c_base))
            rec["torch_stage_ms"] = {k: round(median(v), 3) for k, v in sb.items()}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        del pred, gt
        torch.cuda.empty_cache()
    print("\n| shape | factor | kernels ms (rounds) | torch ms (rounds) | ratio | cold: kernels / torch ms | "
          "quantile ms | search ms | final ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        s, ts = r["stage_ms"], r.get("torch_stage_ms", {})
        pair = lambda k: f"{s[k]:.2f} / {ts[k]:.2f}" if ts else f"{s[k]:.2f}"  # noqa: E731
        print(f"| {' x '.join(map(str, r['shape']))} | {r['factor']} | {r['ms']:.2f} ({r['ms_rounds']}) | "
              f"{r.get('torch_ms', float('nan')):.2f} ({r.get('torch_ms_rounds', [])}) | "
              f"{r.get('speedup', float('nan')):.1f}x | {r['cold_ms']:.2f} / {r.get('torch_cold_ms', float('nan')):.2f} | "
              f"{pair('quantile')} | {pair('search')} | {pair('final')} |")


if __name__ == "__main__":
    main()
