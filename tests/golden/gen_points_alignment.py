"""Generate tests/golden/points_alignment.npz from the reference's own
``umeyama_alignment_from_points`` and ``umeyama`` (aligned_vggt/utils/alignment.py:372-426, :6-59),
pulled out of the reference file by gen_golden.extract (run where the reference checkout exists).

Six small seeded inputs (the reference's umeyama carries a per-point Python loop): (B, S, H, W) =
(1, 1, 1, 5), (1, 2, 7, 9) and (2, 3, 5, 11); kept counts n with n mod 3 = 0, 1 and 2 (asserted
below); one input whose confidences tie at the threshold; one with q = 90.  Data only: inputs and the
reference's outputs.

Each case's seed is the first from its starting value at which the fp32 model of tests/edge_rules.py
(_umeyama_torch in fp32 against its fp64 form, on the case's own samples, in both column layouts) is off
by at least 3 fp32 roundings on the transform rows and on the scale: the CPU tests hold the code to 2 x
that model's error, and a model that happens to be exact would decide them (the rule of
edge_rules._svd_centres).  The choice reads the model alone, never the code under test.
Usage:  python tests/golden/gen_points_alignment.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np

from gen_golden import extract

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from edge_rules import F32, F64, U, _row_err  # noqa: E402
from points_alignment_rules import solve_batch  # noqa: E402

# name: (B, S, H, W), q, first seed tried, tied confidences, masked fraction
CASES = {
    "tiny": ((1, 1, 1, 5), 50.0, 1, False, 0.0),
    "mid": ((1, 2, 7, 9), 50.0, 2, False, 0.2),
    "batch": ((2, 3, 5, 11), 50.0, 3, False, 0.3),
    "ties": ((1, 2, 7, 9), 50.0, 4, True, 0.1),
    "q90": ((1, 2, 7, 9), 90.0, 5, False, 0.0),
    "mid2": ((1, 2, 7, 9), 37.5, 6, False, 0.25),
}


def inputs(shape, seed, ties, masked):
    B = shape[0]
    g = np.random.default_rng(seed)
    pred = (g.standard_normal(shape + (3,)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)
    c, s = np.cos(0.7), np.sin(0.7)
    R0 = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    gt = (1.4 * pred.astype(np.float64) @ R0.T + np.array([0.5, -1.0, 2.0])
          + 0.05 * g.standard_normal(shape + (3,))).astype(np.float32)
    conf = (1.0 + g.random(shape) * 4.0).astype(np.float32)
    if ties:  # five levels: dozens of values equal the percentile
        conf = (1.0 + np.floor(g.random(shape) * 5.0)).astype(np.float32)
    mask = g.random(shape) >= masked
    assert B == pred.shape[0]
    return pred, conf, gt, mask


def model_is_inexact(pred, conf, gt, mask, q):
    for columns in ("reference", "points"):
        T64, c64, n, _ = solve_batch(pred, conf, gt, mask, q, columns, F64)
        T32, c32, _, _ = solve_batch(pred, conf, gt, mask, q, columns, F32)
        B = len(n)
        if min(n) < 3:
            return False
        if float(_row_err(T32[:, :3], T64[:, :3]).max()) < 3 * U:
            return False
        if float(_row_err(c32.reshape(B, 1), c64.reshape(B, 1)).max()) < 3 * U:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    fns = extract(a.ref, "aligned_vggt/utils/alignment.py", ["umeyama", "umeyama_alignment_from_points"])
    out, mods = {}, set()
    for name, (shape, q, seed, ties, masked) in CASES.items():
        while True:
            pred, conf, gt, mask = inputs(shape, seed, ties, masked)
            if model_is_inexact(pred, conf, gt, mask, q):
                break
            seed += 10
        T, sc = fns["umeyama_alignment_from_points"](pred, conf, gt, mask, q)
        n = []
        for b in range(shape[0]):
            thr = np.percentile(conf[b], q)
            keep = (mask[b] > 0) & (conf[b] >= thr) & (conf[b] > 1e-5)
            n.append(int(keep.sum()))
            mods.add(n[-1] % 3)
            if ties:
                assert int((conf[b] == thr).sum()) > 10, "no ties at the threshold"
        for k, v in (("pred", pred), ("conf", conf), ("gt", gt), ("mask", mask), ("q", np.float64(q)),
                     ("T", np.asarray(T)), ("scale", np.asarray(sc)), ("n", np.asarray(n, dtype=np.int64))):
            out[f"{name}.{k}"] = v
        print(name, shape, "seed", seed, "q", q, "n", n, "scale", np.asarray(sc))
    assert mods == {0, 1, 2}, mods
    np.savez_compressed(os.path.join(HERE, "points_alignment.npz"), **out)
    print("wrote points_alignment.npz", os.path.getsize(os.path.join(HERE, "points_alignment.npz")), "bytes")


if __name__ == "__main__":
    main()
