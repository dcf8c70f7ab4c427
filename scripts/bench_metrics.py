#!/usr/bin/env python3
"""What the metrics module costs after the model's forward, host route against device route on one GPU.

(a) ``sequence``: the post-forward part of a 1 x 512 x 154 x 518 sequence -- 43 chunks (width 16, overlap 4) of
    synthetic device outputs (pose encoding, depth + confidence, points + confidence) replayed by a stand-in model
    through ``apply_sequence_to_model(..., "scale_from_poses")``, then ``Metrics.prepare_data_for_metrics`` (at most
    500,000 points: unprojection, quantile, subsampling, ICP), ``ChamferDistanceMetrics.plot`` and the ATE / RPE
    ``plot``.  Host route: ``offload=True`` with the GT on the host (today's default: every chunk copied to pinned
    host memory, merged and aligned there, then copied back for the preparation).  Device route: ``offload=False``
    with the GT on the device.  Wall clock between two device synchronisations.
(b) ``step``: ``alignAndConvertOutputs(..., "scale_from_poses")`` on the device outputs of a 2 x 16 x 518 x 518
    step (pose encoding, depth, points), the kernel route against VGGT_GT_ALIGN=torch; device events around whole
    calls, and the host synchronisations of one call of each (``torch.cuda.set_sync_debug_mode("warn")``).
(c) ``updates``: one ``update`` of AbsoluteTrajectoryError and of RelativePoseError with S = 512 device poses,
    state on the host (the default) against state on the device.

Every figure comes from ``--rounds`` rounds that alternate the two sides in one process; the median round is
reported with every round listed.  Prints one JSON line per measurement.

    python scripts/bench_metrics.py [--only sequence,step,updates] [--rounds 3] [--seconds 1.5] [--frames 512]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "large-scale-vit-slam_amd"), ROOT, os.path.join(ROOT, "scripts")]

from bench_loss import event_ms, median  # noqa: E402

DEV = torch.device("cuda:0")


def synthetic_sequence(S, H, W, seed=0):
    """Per-frame predictions and GT of one sequence on the device: a walk whose predicted translations are
    0.5 x the GT's plus noise, depths in 0.5-80 m with GT within exp(N(0, 0.1)), masks 70 % set."""
    from aligned_vggt.utils.geometry import unproject_depth_map_to_point_map
    from aligned_vggt.utils.pose_enc import pose_encoding_to_extri_intri
    g = torch.Generator().manual_seed(seed)
    yaw = torch.cumsum(0.02 * torch.randn(S, generator=g), 0)
    quat = torch.stack([torch.zeros(S), torch.sin(yaw / 2), torch.zeros(S), torch.cos(yaw / 2)], -1)
    t = torch.cumsum(0.3 * torch.rand(S, 3, generator=g), 0)
    t[0] = 0.0
    fov = torch.tensor([0.6, 1.6]).expand(S, 2)
    gt_enc = torch.cat([t, quat, fov], -1)[None]
    extr, intr = pose_encoding_to_extri_intri(gt_enc, (H, W))
    pose = torch.cat([0.5 * t + 0.01 * torch.randn(S, 3, generator=g), quat, fov], -1)[None].to(DEV)
    gt_depth = (0.5 + 79.5 * torch.rand(1, S, H, W, generator=g)).to(DEV)
    depth = gt_depth * torch.exp(0.1 * torch.randn(1, S, H, W, generator=g).to(DEV))
    conf = 1.0 + torch.exp(torch.randn(1, S, H, W, generator=g)).to(DEV)
    extr, intr = extr.to(DEV), intr.to(DEV)
    world = torch.cat([unproject_depth_map_to_point_map(gt_depth[:, a:a + 32, ..., None], extr[:, a:a + 32],
                                                        intr[:, a:a + 32]) for a in range(0, S, 32)], 1)
    pred = {"pose_enc": pose, "depth": depth[..., None].contiguous(), "depth_conf": conf,
            "world_points": world * 0.5, "world_points_conf": conf.clone()}
    gt = {"extrinsics": extr, "intrinsics": intr, "depths": gt_depth, "world_points": world,
          "point_masks": (torch.rand(1, S, H, W, generator=g) < 0.7).to(DEV),
          "images": torch.zeros(1, S, 3, H, W, device=DEV)}
    return pred, gt


class Replay:
    """The chunk protocol over stored per-frame outputs: chunk i's outputs are fresh device copies of its
    frames, appended to the context's lists as the models do."""

    def __init__(self, pred, indices):
        self.pred, self.indices, self.i = pred, indices, 0

    def __call__(self, images, num_overlap, context=None, gt_poses=None):
        ids = self.indices[self.i]
        self.i = (self.i + 1) % len(self.indices)
        out = {k: v[:, ids].clone() for k, v in self.pred.items()}
        if context is None:
            return {k: [v] for k, v in out.items()}
        for k, v in out.items():
            context[k].append(v)
        return context


def bench_sequence(rounds, frames):
    from aligned_vggt.training.training_metrics import Metrics
    from aligned_vggt.utils.data import generate_chunks
    H, W, width, ov = 154, 518, 16, 4
    pred, gt = synthetic_sequence(frames, H, W)
    indices = generate_chunks(frames, "chunk_overlap", width, ov)
    gt_host = {k: (v if k == "images" else v.cpu()) for k, v in gt.items()}
    metrics = Metrics(mode="test", overlap=[ov], chunk_width=[width], gt_alignment_type="scale_from_poses",
                      full_seq_sample_mode="chunk_overlap", use_random_sequences=False,
                      trajectory_metrics=[{"_target_": "eval.trajectory_metrics.AbsoluteTrajectoryError"},
                                          {"_target_": "eval.trajectory_metrics.RelativePoseError"}],
                      reconstruction_metrics=[{"_target_": "eval.reconstruction_metrics.ChamferDistanceMetrics"}])

    def route(on_device):
        return _sequence_route(metrics, pred, gt, gt_host, indices, width, ov, on_device)
    rec = {"bench": "sequence", "shape": [1, frames, H, W], "chunks": len(indices), "rounds": []}
    route(True)  # warm: library, allocator, pinned pool
    route(False)
    for _ in range(rounds):
        h, hv, hs = route(False)
        d, dv, ds = route(True)
        rec["rounds"].append({"host": {k: round(v * 1e3, 1) for k, v in h.items()},
                              "device": {k: round(v * 1e3, 1) for k, v in d.items()}})
    rec["host_ms"] = median([r["host"]["total"] for r in rec["rounds"]])
    rec["device_ms"] = median([r["device"]["total"] for r in rec["rounds"]])
    rec["speedup"] = rec["host_ms"] / rec["device_ms"]
    rec["device_faster_in_every_round"] = all(r["device"]["total"] < r["host"]["total"] for r in rec["rounds"])
    rec["values"] = {"host": hv, "device": dv, "host_scale": hs, "device_scale": ds}
    rec["chunk_outputs_mib"] = round(sum(v[:, i].numel() * v.element_size() for v in pred.values() for i in indices)
                                     / 2 ** 20, 1)
    print(json.dumps(rec), flush=True)


def _sequence_route(metrics, pred, gt, gt_host, indices, width, ov, on_device):
    """One pass of measurement (a): (stage seconds, metric values, alignment scales)."""
    from aligned_vggt.training.training_metrics import apply_sequence_to_model
    batch = dict(gt if on_device else gt_host)
    stages = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = apply_sequence_to_model(batch, Replay(pred, indices), [width], [ov], "chunk_overlap", "scale_from_poses",
                                  offload=not on_device)
    torch.cuda.synchronize()
    stages["drive_merge_align"] = time.perf_counter() - t0
    t1 = time.perf_counter()
    pp, gp, ppts, gpts = metrics.prepare_data_for_metrics(out, batch, max_points_icp=500000, device=DEV)
    torch.cuda.synchronize()
    stages["prepare_icp"] = time.perf_counter() - t1
    t2 = time.perf_counter()
    res = {}
    for m in metrics.trajectory_metrics:
        res.update(m.plot(pp[0], gp[0], "bench", None)[0])
    for m in metrics.reconstruction_metrics:
        res.update(m.plot(ppts[0], gpts[0], "bench", None)[0])
    torch.cuda.synchronize()
    stages["metric_plots"] = time.perf_counter() - t2
    stages["total"] = time.perf_counter() - t0
    return stages, {k: float(v) for k, v in res.items()}, [float(s) for s in out["alignment_scales"]]


def count_syncs(fn):
    """Host synchronisations torch reports for one call (a prototype detector: a lower bound)."""
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


def bench_step(rounds, seconds):
    from aligned_vggt.utils.data import alignAndConvertOutputs
    B, S, H, W = 2, 16, 518, 518
    g = torch.Generator().manual_seed(1)
    pose = torch.randn(B, S, 9, generator=g).to(DEV)
    extr = torch.randn(B, S, 3, 4, generator=g)
    extr[..., 3] = 1.3 * pose[..., :3].cpu() * (1 + 0.1 * torch.randn(B, S, 3, generator=g))
    extr = extr.to(DEV)
    depth = (0.5 + 79.5 * torch.rand(B, S, H, W, 1, generator=g)).to(DEV)
    points = torch.randn(B, S, H, W, 3, generator=g).to(DEV)

    def side(knob):
        def call():
            os.environ["VGGT_GT_ALIGN"] = knob
            p = {"pose_enc": [pose], "depth": [depth], "world_points": [points]}
            alignAndConvertOutputs(p, {}, {"extrinsics": [extr]}, "scale_from_poses", S, 0)
            return p
        return call

    ours, base = side("kernel"), side("torch")
    rec = {"bench": "step", "shape": [B, S, H, W], "scales": [float(s) for s in ours()["alignment_scales"]],
           "torch_scales": [float(s) for s in base()["alignment_scales"]],
           "host_syncs": count_syncs(ours), "torch_host_syncs": count_syncs(base)}
    win = seconds * 1e3 / rounds
    t_ours, t_base = [], []
    for _ in range(rounds):
        t_ours.append(event_ms(ours, win))
        t_base.append(event_ms(base, win))
    rec.update(ms_rounds=[round(t, 4) for t in t_ours], ms=median(t_ours), torch_ms_rounds=[round(t, 4) for t in t_base],
               torch_ms=median(t_base), speedup=median(t_base) / median(t_ours),
               faster_in_every_round=all(o < b for o, b in zip(t_ours, t_base)))
    print(json.dumps(rec), flush=True)


def bench_updates(rounds, seconds):
    from aligned_vggt.eval import AbsoluteTrajectoryError, RelativePoseError
    S = 512
    g = torch.Generator().manual_seed(2)

    def poses():
        q = torch.randn(S, 4, generator=g)
        from aligned_vggt.utils.rotation import quat_to_mat
        M = torch.eye(4).repeat(S, 1, 1)
        M[:, :3, :3] = quat_to_mat(q)
        M[:, :3, 3] = torch.cumsum(0.3 * torch.randn(S, 3, generator=g), 0)
        return M.to(DEV)
    pred, gt = poses(), poses()

    def side(device_state):
        ms = [AbsoluteTrajectoryError(), RelativePoseError()]
        if device_state:
            ms = [m.to(DEV) for m in ms]

        def call():
            for m in ms:
                m.update(pred, gt)
                m.reset()
        return call

    dev_side, host_side = side(True), side(False)
    rec = {"bench": "updates", "S": S, "host_syncs": count_syncs(dev_side), "host_state_host_syncs": count_syncs(host_side)}
    win = seconds * 1e3 / rounds
    t_dev, t_host = [], []
    for _ in range(rounds):
        t_dev.append(event_ms(dev_side, win))
        t_host.append(event_ms(host_side, win))
    rec.update(ms_rounds=[round(t, 4) for t in t_dev], ms=median(t_dev), host_state_ms_rounds=[round(t, 4) for t in t_host],
               host_state_ms=median(t_host), speedup=median(t_host) / median(t_dev),
               faster_in_every_round=all(o < b for o, b in zip(t_dev, t_host)))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="sequence,step,updates")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side of (b) and (c), over all rounds")
    ap.add_argument("--frames", type=int, default=512, help="frames of the sequence of (a)")
    args = ap.parse_args()
    knob = os.environ.get("VGGT_GT_ALIGN")
    try:
        for name in args.only.split(","):
            if name == "sequence":
                os.environ.pop("VGGT_GT_ALIGN", None)
                bench_sequence(args.rounds, args.frames)
            elif name == "step":
                bench_step(args.rounds, args.seconds)
            elif name == "updates":
                bench_updates(args.rounds, args.seconds)
            else:
                raise SystemExit(f"unknown measurement {name!r}")
            torch.cuda.empty_cache()
    finally:
        if knob is None:
            os.environ.pop("VGGT_GT_ALIGN", None)
        else:
            os.environ["VGGT_GT_ALIGN"] = knob


if __name__ == "__main__":
    main()
