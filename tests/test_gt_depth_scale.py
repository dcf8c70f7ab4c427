"""The definition that csrc/gt_align.hip implements (include/vggt_mi355x.h, "GT scale alignment"), as a numpy
oracle, pinned to the restatement of the reference's scale_align_from_depths before any kernel runs.

The oracle: the fsum mean, the reference's per-pixel fp32 arithmetic (:281-295), integer weights
q = rint(ldexp(w_eff, e)) with ldexp(wmax, e) in (2^35, 2^36], a stable sort of the ratio keys and an int64
cumulative sum searched for the first index at which twice the sum reaches the total.  tests/test_gpu_gt_depth_scale.py
holds the kernel to it bit for bit."""
import math

import numpy as np
import pytest
import torch

from aligned_vggt.utils import alignment as A

F = np.float32


def bits(v) -> int:
    return int(np.asarray(v, dtype=F).reshape(1).view(np.uint32)[0])


# ------------------------------------------------------------------------------------------------- the oracle
def keys_of(r: np.ndarray) -> np.ndarray:
    """vggt_kth_value_f32's order as uint32: -inf < finite < +inf < NaN, -0 == +0."""
    b = np.ascontiguousarray(r, dtype=F).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[b == np.uint32(0x80000000)] = np.uint32(0x80000000)
    k[(b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = np.uint32(0xffffffff)
    return k


def unkey(k: int) -> np.float32:
    k = int(k)
    if k == 0xffffffff:
        return np.array([0x7fc00000], dtype=np.uint32).view(F)[0]
    b = (k & 0x7fffffff) if (k & 0x80000000) else (~k & 0xffffffff)
    return np.array([b], dtype=np.uint32).view(F)[0]


def fsum_mean(y: np.ndarray, m: np.ndarray) -> np.float32:
    """(float)(sum(y * m) / max(cnt, 1)) with the sum exact."""
    cnt = int(m.astype(bool).sum())
    with np.errstate(all="ignore"):
        prod = (y.astype(F) * m.astype(bool).astype(F)).astype(np.float64)
    return F(math.fsum(prod.tolist()) / max(cnt, 1))


def terms(x, conf, y, m, mean):
    """(r, w_eff) per pixel, every operation rounded to fp32 on its own; np.maximum keeps a NaN, as torch.max."""
    x, conf, y = (np.ascontiguousarray(a, dtype=F) for a in (x, conf, y))
    with np.errstate(all="ignore"):
        min_depth = F(0.1) * F(mean)
        w = (m.astype(bool).astype(F) * conf) * (F(1.0) / np.maximum(np.maximum(y, min_depth), F(1e-6)))
        sign = np.where(x < 0, F(-1.0), F(1.0)).astype(F)
        x_pos = x * sign
        r = (y * sign) / np.maximum(x_pos, F(1e-6))
        w_eff = w * x_pos
    assert r.dtype == F and w_eff.dtype == F
    return r, w_eff


def valid_weights(w_eff: np.ndarray) -> np.ndarray:
    """A weight that is NaN, +-inf or negative counts as 0."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(w_eff) & ~(w_eff < 0)
    return np.where(ok, w_eff, F(0.0)).astype(F)


def quantise(w_eff: np.ndarray):
    """(q int64, e, wmax): q = rint(ldexp(w_eff, e)), ldexp(wmax, e) in (2^35, 2^36]; e = 0 when wmax == 0."""
    wv = valid_weights(w_eff)
    wmax = F(wv.max())
    if wmax == 0:
        e = 0
    else:
        fr, k = math.frexp(float(wmax))
        e = 36 - k + (1 if fr == 0.5 else 0)
        assert 2.0 ** 35 < math.ldexp(float(wmax), e) <= 2.0 ** 36
    q = np.rint(np.ldexp(wv.astype(np.float64), e)).astype(np.int64)
    return q, e, wmax


def oracle(x, conf, y, m, mean=None) -> dict:
    """One batch element (1-D arrays).  `mean`: the fp32 mean to use (default: the fsum mean)."""
    x, conf, y, m = (np.asarray(a).reshape(-1) for a in (x, conf, y, m))
    if mean is None:
        mean = fsum_mean(y, m)
    r, w_eff = terms(x, conf, y, m, mean)
    q, e, wmax = quantise(w_eff)
    keys = keys_of(r)
    order = np.argsort(keys, kind="stable")
    cum = np.cumsum(q[order], dtype=np.int64)
    total = int(cum[-1])
    i = int(np.searchsorted(2 * cum, total, side="left"))  # the first index with 2 cum >= total; total 0: index 0
    key = int(keys[order][i])
    rs = unkey(key)
    scale = -rs if rs <= 0 else rs
    return {"scale": F(scale), "r": rs, "key": key, "e": e, "total": total, "wmax": wmax, "mean": F(mean),
            "cnt": int(m.astype(bool).sum()), "below": int(q[keys < key].sum()), "through": int(q[keys <= key].sum()),
            "q": q, "keys": keys, "w_eff": w_eff, "ratios": r}


# ------------------------------------------------------------------------------------------------- inputs
def seeded_inputs(shape, seed):
    """scripts/bench_loss.py's synthetic step: depths 0.5-80, GT within exp(N(0, 0.3)), confidences
    1 + exp(N(0, 1)), masks 70 % set.  (depth, conf, gt, mask) as torch CPU tensors of `shape`."""
    g = torch.Generator().manual_seed(seed)
    depth = 0.5 + 79.5 * torch.rand(shape, generator=g)
    gt = depth * torch.exp(0.3 * torch.randn(shape, generator=g))
    conf = 1.0 + torch.exp(torch.randn(shape, generator=g))
    mask = torch.rand(shape, generator=g) < 0.7
    return depth, conf, gt, mask


def predictions_of(depth, conf, seed):
    """A predictions dict around (B, S, H, W) depth and conf: world points and a pose encoding to scale."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, S = depth.shape[:2]
    return {"depth": depth[..., None].clone(), "depth_conf": conf.clone(),
            "world_points": torch.randn(*depth.shape, 3, generator=g),
            "pose_enc": torch.randn(B, S, 9, generator=g)}


SHAPE = (2, 2, 37, 53)
SEEDS = (0, 1, 2, 3, 4, 5)


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_is_the_cpu_restatement_bitwise(seed):
    depth, conf, gt, mask = seeded_inputs(SHAPE, seed)
    pred = predictions_of(depth, conf, seed)
    A.scale_align_from_depths(pred, {"depths": gt, "point_masks": mask})
    B = SHAPE[0]
    for b in range(B):
        o = oracle(depth[b].numpy(), conf[b].numpy(), gt[b].numpy(), mask[b].numpy())
        assert bits(pred["alignment_scales"][b]) == bits(o["scale"]), (seed, b, pred["alignment_scales"][b], o["scale"])
        np.testing.assert_array_equal(pred["depth"][b, ..., 0].numpy(), depth[b].numpy() * o["scale"])


def test_oracle_decisions():
    one = np.ones(2, dtype=F)
    # weights {1, 1} at r = {1, 2}: twice the first cumulative sum reaches the total, the left one is taken
    o = oracle(one, np.array([1, 2], dtype=F), np.array([1, 2], dtype=F), np.array([True, True]))
    assert o["w_eff"].tolist() == [1.0, 1.0] and o["scale"] == 1.0 and o["through"] * 2 == o["total"] and o["below"] == 0
    assert o["e"] == 36 and o["q"].tolist() == [2 ** 36, 2 ** 36]
    # a total of 0 selects the smallest ratio; a negative one comes back negated
    o = oracle(np.array([2, -4], dtype=F), one, np.array([1, 1], dtype=F), np.array([False, False]))
    assert o["total"] == 0 and o["e"] == 0 and o["r"] == F(-0.25) and o["scale"] == F(0.25)
    # NaN, inf and negative weights count as 0
    assert valid_weights(np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 2.0], dtype=F)).tolist() == [0, 0, 0, 0, 0, 2.0]
    # the order of the keys
    v = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], dtype=F)
    k = keys_of(v)
    assert k[3] == k[4] and list(np.argsort(k, kind="stable")) == [6, 5, 3, 4, 2, 1, 0]
    assert all(bits(unkey(k[i])) == bits(v[i]) for i in (1, 2, 3, 5, 6))


def test_entry_point_refuses_bad_arguments():
    """vggt_depth_scale_l1 answers from its argument checks, before any launch: no GPU call is made here and the
    pointers are never read."""
    import ctypes
    import os
    from aligned_vggt import _native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built")
    L = N.lib()
    assert L.vggt_depth_scale_ws_bytes(0, 10) == 0 and L.vggt_depth_scale_ws_bytes(1, 0) == 0
    assert L.vggt_depth_scale_ws_bytes(1, 10 ** 8 + 1) == 0
    need = L.vggt_depth_scale_ws_bytes(2, 1000)
    assert need > L.vggt_depth_scale_ws_bytes(1, 1000) > 0 and need == L.vggt_depth_scale_ws_bytes(2, 10 ** 8)
    p = ctypes.c_void_p(1 << 20)

    def call(B, n, ws=p, ws_bytes=need, bstride=None):
        return L.vggt_depth_scale_l1(p, p, p, p, B, n, n if bstride is None else bstride, p, p, ws, ws_bytes, None)

    assert call(0, 1000) == N.VGGT_ERR_SHAPE and call(2, 0) == N.VGGT_ERR_SHAPE and call(2, -5) == N.VGGT_ERR_SHAPE
    assert call(2, 1000, ws=ctypes.c_void_p((1 << 20) + 8)) == N.VGGT_ERR_SHAPE   # a misaligned ws
    assert call(2, 1000, ws_bytes=need - 1) == N.VGGT_ERR_SHAPE and call(2, 1000, ws=None) == N.VGGT_ERR_SHAPE
    assert call(2, 1000, bstride=999) == N.VGGT_ERR_SHAPE                        # overlapping elements
    assert call(1, 10 ** 8 + 1) == N.VGGT_ERR_UNSUPPORTED
    odd = ctypes.c_void_p((1 << 20) + 2)
    assert L.vggt_depth_scale_l1(odd, p, p, p, 2, 1000, 1000, p, p, p, need, None) == N.VGGT_ERR_ALIGN
    assert L.vggt_depth_scale_l1(p, p, p, p, 2, 1000, 1000, p, ctypes.c_void_p((1 << 20) + 4), p, need,
                                 None) == N.VGGT_ERR_ALIGN                       # state_out off an 8-byte boundary


def test_cpu_path_is_the_torch_chain(monkeypatch):
    """Host tensors never reach the kernel path, whatever the knob says."""
    depth, conf, gt, mask = seeded_inputs(SHAPE, 0)
    outs = []
    for knob in (None, "torch"):
        if knob is None:
            monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
        else:
            monkeypatch.setenv("VGGT_GT_ALIGN", knob)
        pred = predictions_of(depth, conf, 0)
        A.scale_align_from_depths(pred, {"depths": gt, "point_masks": mask})
        assert all(isinstance(s, float) for s in pred["alignment_scales"])
        outs.append(pred)
    for k in ("depth", "world_points", "pose_enc"):
        assert torch.equal(outs[0][k], outs[1][k])
