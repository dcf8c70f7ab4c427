"""The pose-aligned VGGT's per-chunk alignment (aligned_vggt.models.poseAligned_wrapped_vggt
.align_chunk, torch form on host tensors) against the reference's OWN forward over whole
chunk sequences (tests/golden/ref_pose_aligned.npz, written by tests/golden/gen_pose_aligned.py
from the reference's poseAligned_wrapped_vggt.py on the test-only vggt shim).  CPU only.

The bars are those tests/test_ref_alignment_golden.py applies to the feature-aligned
composition for the same quantities (TOL f32 = 2e-6): translations, rotations (quaternions up
to sign), depth and points at 10 x TOL, FoV at TOL; pass-through confidences bit for bit."""
import json

import pytest
import torch

from aligned_vggt.models import poseAligned_wrapped_vggt as PA

TOL = 2e-6


def _t(a):
    return torch.from_numpy(a.copy())


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _quat_rot_err(a, b):
    return float((1.0 - (a[..., 3:7] * b[..., 3:7]).sum(-1).abs()).abs().max())


def _images(B, S, hw):
    n = B * S * 3 * hw[0] * hw[1]
    return ((torch.arange(n) % 7).float() / 7.0).view(B, S, 3, *hw)


def _enc(g, run, ci, hw):
    p = f"{run['tag']}.{ci}."
    pose = _t(g[p + "in.pose_enc"])
    enc = {"images": _images(pose.shape[0], pose.shape[1], hw), "pose_enc": pose}
    if run["heads"][1]:
        enc["depth"], enc["depth_conf"] = _t(g[p + "in.depth"]), _t(g[p + "in.depth_conf"])
    if run["heads"][2]:
        enc["world_points"], enc["world_points_conf"] = _t(g[p + "in.points"]), _t(g[p + "in.points_conf"])
    return enc, (_t(g[p + "in.gt"]) if run["gt"] else None)


@pytest.fixture(scope="module")
def fixture():
    from conftest import load_golden
    g = load_golden("ref_pose_aligned")
    return g, json.loads(str(g["runs"])), tuple(int(v) for v in g["hw"])


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f", "g"])
def test_align_chunk_matches_reference(fixture, tag):
    g, runs, hw = fixture
    run, = [r for r in runs if r["tag"] == tag]
    ctx = None
    for ci in range(len(run["lengths"])):
        enc, gt = _enc(g, run, ci, hw)
        gt_before = None if gt is None else gt.clone()
        new = PA.align_chunk(enc, run["ov"], ctx, gt, run["training"])
        if gt is not None:
            assert torch.equal(gt, gt_before), "the caller's gt_poses was modified"
        assert new is not ctx and new is not enc
        if ctx is not None:
            assert all(new[k] is ctx[k] for k in new), "the lists are the context's"
        ctx = new
    assert sorted(ctx.keys()) == json.loads(str(g[f"{tag}.keys"]))
    assert ("images" in ctx) == (not run["training"])
    worst = {}
    for k, v in ctx.items():
        assert isinstance(v, list) and len(v) == len(run["lengths"]), k
        for ci, got in enumerate(v):
            if k == "images":
                assert torch.equal(got, _images(run["B"], run["lengths"][ci], hw))
                continue
            ref = _t(g[f"{tag}.{ci}.out.{k}"])
            assert got.shape == ref.shape and got.dtype == torch.float32, (k, ci)
            if k == "pose_enc":
                e = {"translation": _rel(got[..., :3], ref[..., :3]) / 10, "rotation": _quat_rot_err(got, ref) / 10,
                     "fov": _rel(got[..., 7:], ref[..., 7:])}
            elif k.endswith("_conf"):
                assert torch.equal(got, ref), (k, ci)
                continue
            else:
                e = {k: _rel(got, ref) / 10}
            for name, val in e.items():
                worst[name] = max(worst.get(name, 0.0), val)
    print(tag, "worst error / its bar:", {k: round(v / TOL, 4) for k, v in worst.items()})
    assert max(worst.values()) < TOL, (tag, worst)


def _small(B=1, S=1, depth=True, points=False, cam=True):
    g = torch.Generator().manual_seed(3)
    enc = {"images": torch.zeros(B, S, 3, 6, 8)}
    if cam:
        enc["pose_enc"] = torch.cat([torch.randn(B, S, 7, generator=g), 0.5 + torch.rand(B, S, 2, generator=g)], -1)
    if depth:
        enc["depth"], enc["depth_conf"] = torch.rand(B, S, 6, 8, 1, generator=g), torch.ones(B, S, 6, 8)
    if points:
        enc["world_points"], enc["world_points_conf"] = torch.randn(B, S, 6, 8, 3, generator=g), torch.ones(B, S, 6, 8)
    gt = torch.cat([torch.eye(3).expand(B, S, 3, 3), torch.randn(B, S, 3, 1, generator=g)], -1)
    return enc, gt


@pytest.mark.parametrize("depth,points", [(True, False), (False, True)])
def test_gt_with_one_frame_and_a_dense_head_raises(depth, points):
    enc, gt = _small(S=1, depth=depth, points=points)
    before = {k: v.clone() for k, v in enc.items()}
    with pytest.raises(ValueError, match="one-frame"):
        PA.align_chunk(enc, 1, None, gt, False)
    assert all(torch.equal(enc[k], before[k]) for k in enc)


@pytest.mark.parametrize("depth,points", [(True, False), (False, True)])
def test_gt_without_camera_head_raises(depth, points):
    enc, gt = _small(S=3, depth=depth, points=points, cam=False)
    with pytest.raises(ValueError, match="camera head"):
        PA.align_chunk(enc, 1, None, gt, False)


def test_gt_with_one_frame_camera_only_follows_reference():
    """The reference defines this case (:84-109): no scale, and with a context the mean is the
    GT pose."""
    enc, gt = _small(S=1, depth=False)
    first = PA.align_chunk(enc, 1, None, gt, False)
    plain = PA.align_chunk(_small(S=1, depth=False)[0], 1, None, None, False)
    assert torch.equal(first["pose_enc"][0], plain["pose_enc"][0])
    _, _, scales = PA.align_chunk_poses(enc["pose_enc"], (6, 8), 1, first["pose_enc"][0], gt)
    assert torch.equal(scales, torch.ones(1))


def test_zero_translations_with_gt_give_nan():
    enc, gt = _small(S=3, depth=True, points=True)
    enc["pose_enc"][..., :3] = 0.0
    out = PA.align_chunk(enc, 1, None, gt, False)
    pe = out["pose_enc"][0]
    # the 4 x 4 product carries the NaN translation into the rotation (NaN * 0), so x, y, z are NaN too
    assert torch.isnan(pe[..., :6]).all() and torch.isfinite(pe[..., 6:]).all()
    assert torch.isnan(out["depth"][0]).all() and torch.isnan(out["world_points"][0]).all()


def test_torch_form_is_dtype_generic():
    g = torch.Generator().manual_seed(5)
    B, S, ov = 2, 5, 3
    pe = torch.cat([torch.randn(B, S, 7, generator=g), 0.5 + torch.rand(B, S, 2, generator=g)], -1)
    ctx = torch.cat([torch.randn(B, 4, 7, generator=g), 0.5 + torch.rand(B, 4, 2, generator=g)], -1)
    gt = torch.cat([torch.eye(3).expand(B, S, 3, 3), torch.randn(B, S, 3, 1, generator=g)], -1)
    for c, t in ((None, None), (ctx, None), (ctx, gt), (None, gt)):
        d = lambda x: None if x is None else x.double()  # noqa: E731
        a64, p64, s64 = PA.align_chunk_poses(d(pe), (6, 8), ov, d(c), d(t), form="torch")
        a32, p32, s32 = PA.align_chunk_poses(pe, (6, 8), ov, c, t, form="torch")
        assert a64.dtype == p64.dtype == s64.dtype == torch.float64
        assert a32.dtype == p32.dtype == s32.dtype == torch.float32
        assert a32.shape == (B, S, 9) and p32.shape == (B, 4, 4) and s32.shape == (B,)
        assert _rel(a32[..., :3], a64[..., :3]) < 1e-5 and _rel(p32, p64) < 1e-5 and _rel(s32, s64) < 1e-5
        if t is None:
            assert torch.equal(s32, torch.ones(B))
