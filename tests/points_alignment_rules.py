"""Helpers shared by test_points_alignment.py and test_gpu_points_alignment.py: numpy's fp32 percentile
restated operation by operation, the selection and the two column layouts of
umeyama_alignment_from_points, and the fp64 / fp32 solves they are compared with.  A plain module: no
tests, no fixtures."""
import os

import numpy as np
import torch

from edge_rules import _row_err, _umeyama_torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_alignment.npz")
CASES = ("tiny", "mid", "batch", "ties", "q90", "mid2")
f32 = np.float32


def percentile32(v, q):
    """np.percentile(v, q) of a float32 vector and a Python-float q, every operation rounded to fp32 on
    its own: (thr, a, c) with a and c the two order statistics."""
    v = np.asarray(v, dtype=f32).reshape(-1)
    P = v.size
    s = np.sort(v)
    h = f32(f32(P - 1) * f32(f32(q) / f32(100.0)))
    fl = np.floor(h)
    lo = min(int(fl), P - 1)
    g = f32(h - fl)
    hi = min(lo + 1, P - 1)
    a, c = s[lo], s[hi]
    d = f32(c - a)
    thr = f32(a + f32(d * g))
    if g >= f32(0.5):
        thr = f32(c - f32(d * f32(f32(1.0) - g)))
    if np.isnan(v).any():
        thr = f32(np.nan)
    return thr, a, c


def select(conf, mask, q):
    """The kept pixels of one batch element (flat boolean, row-major) and numpy's threshold."""
    conf = np.asarray(conf, dtype=f32).reshape(-1)
    thr = np.percentile(conf, float(q))  # a Python float: numpy then stays in fp32
    assert thr.dtype == f32
    keep = (np.asarray(mask).reshape(-1) > 0) & (conf >= thr) & (conf > 1e-5)
    return keep, thr


def samples(rows, columns):
    """(n, 3) selected rows -> the (n, 3) samples the fit sees."""
    rows = np.ascontiguousarray(rows)
    return rows.reshape(3, -1).T if columns == "reference" else rows


def solve(pred, conf, gt, mask, q, columns, dt):
    """One batch element: (T (4, 4), c) in `dt` arithmetic with LAPACK's SVD, n and thr."""
    keep, thr = select(conf, mask, q)
    X = samples(np.asarray(pred, dtype=f32).reshape(-1, 3)[keep], columns)
    Y = samples(np.asarray(gt, dtype=f32).reshape(-1, 3)[keep], columns)
    R, t, c = _umeyama_torch(torch.from_numpy(X.copy()), torch.from_numpy(Y.copy()), dt)
    T = torch.eye(4, dtype=dt)
    T[:3, :3], T[:3, 3] = R, t
    return T, c.reshape(1), int(keep.sum()), thr


def solve_batch(pred, conf, gt, mask, q, columns, dt):
    out = [solve(pred[b], conf[b], gt[b], mask[b], q, columns, dt) for b in range(pred.shape[0])]
    return torch.stack([o[0] for o in out]), torch.cat([o[1] for o in out]), [o[2] for o in out], [o[3] for o in out]


def host_rule(errs, name, got, want, model, ref):
    """A host result against the values it should reproduce: its worst row error against `want` is at
    most 2 x the fp32 model's worst row error against its own fp64 form."""
    eg, em = float(_row_err(got.double(), want.double()).max()), float(_row_err(model, ref).max())
    print(f"host {name}: got {eg:.3e} model {em:.3e}")
    if not eg <= 2 * em:
        errs.append(f"{name}: {eg:.3e} > 2 x model {em:.3e}")


def load_case(z, name):
    return {k: z[f"{name}.{k}"] for k in ("pred", "conf", "gt", "mask", "q", "T", "scale", "n")}
