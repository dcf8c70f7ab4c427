#!/usr/bin/env python3
"""Key-split tail of the global attention launch, alone and batched: attn_fwd
(16 heads, D 64, nq = nk = 21,984) as B = 1 (1,376 units) and as B = 2 in one
launch (2,752 units), with the per-element plan (VGGT_TUNE_ATTN_TAIL_SPLIT 0)
against unsplit (-1).  The arms alternate inside every round; HIP events over
back-to-back launches.  Prints one line per (round, B, knob) and one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-vit-slam_amd"))

import torch  # noqa: E402

from aligned_vggt import _native as N  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, D, NQ = 16, 64, 21984
    C = H * D
    reps = int(os.environ.get("REPS", "10"))
    rounds = int(os.environ.get("ROUNDS", "3"))
    batches = [int(x) for x in os.environ.get("BATCHES", "1,2").split(",")]
    bmax = max(batches)
    q = (torch.randn(bmax * NQ, C, device=dev) * 0.5).bfloat16()
    k = (torch.randn(bmax * NQ, C, device=dev) * 0.5).bfloat16()
    v = (torch.randn(bmax * NQ, C, device=dev) * 0.5).bfloat16()
    o = torch.empty(bmax * NQ, C, device=dev, dtype=torch.bfloat16)

    def launch(b):
        N.attention(q, k, v, o, b, H, NQ, NQ, D, NQ, NQ, NQ)

    t_end = time.time() + 2.0
    while time.time() < t_end:
        launch(1)
        torch.cuda.synchronize()
    res = {}
    for r in range(rounds):
        for b in batches:
            for knob in (-1, 0):
                prev = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
                try:
                    launch(b)  # (the first split launch allocates the workspace)
                    torch.cuda.synchronize()
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        launch(b)
                    e1.record()
                    e1.synchronize()
                finally:
                    N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev)
                ms = e0.elapsed_time(e1) / reps
                key = "B%d_%s" % (b, "split" if knob == 0 else "unsplit")
                res.setdefault(key, []).append(round(ms, 4))
                print("round", r, key, "ms %.4f" % ms, "TF/s %.1f" % (4.0 * b * NQ * NQ * D * H / ms / 1e9), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
