"""csrc/pose.hip vggt_pose_align and the pose-aligned VGGT built on it
(aligned_vggt/models/poseAligned_wrapped_vggt.py), in the style of test_gpu_geometry_edges.py
section 5 (the shared helpers live in edge_rules.py).

Kernel edges.  Reference: align_chunk_poses' torch form in fp64; model: the same form in fp32 on
the host; _model_rule (kernel worst row <= 2 x the model's worst row, both against fp64)
separately for translation, rotation (the quaternions as 3 x 3 matrices, so their sign is free),
FoV, point transform and scale.  The entry point is called through the C ABI: outputs sit between
sentinel guards, inputs one element into a NaN-filled buffer, every call is made twice and must
repeat bit for bit.  S = 1, 2, 63, 64, 65, 130 (second and third trip of the 64-lane frame loop),
S_prev != S, ov = 1, 2, S, 64, B = 1 and 3, the four modes (first chunk, context, context + GT,
GT without a context).  Overlap contexts are built so that the overlap transforms agree up to
2 degrees (a Markley mean of unrelated rotations has no eigen-gap and no meaningful answer).
Quaternions: every mat_to_quat candidate and the w < 0 flip (asserted from the fp64 matrices),
unnormalised camera quaternions throughout, overlap transforms 0.2 degrees from a half turn
(quaternions of both signs: the mean must not move), identical overlap transforms.  GT scale:
negative correlation (the absolute value decides), all-zero predicted translations (NaN in the
kernel and in the model, asserted on its own).  Error returns write nothing.

No synchronisation: align_chunk on device tensors under set_sync_debug_mode("error").

Model: a 4-block VGGT at 42 x 56; forward == align_chunk(encode_chunk(.)) bit for bit, the new
code checked against the torch forms applied to the model's own raw head outputs (which keeps the
encoder's bf16 spread out of the comparison).  Sequence: apply_sequence_to_model with its grouped
encode against VGGT_ENCODE_GROUP=1."""
import ctypes
import math

import pytest
import torch

from edge_rules import (ERR_SHAPE, F32, F64, NAN, OK, SENT, _done, _eq_bits, _figures, _gen, _guarded, _guards_ok,
                        _model_rule)

pytestmark = pytest.mark.gpu

DEV = "cuda"
HW = (154, 518)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def PA():
    from aligned_vggt.models import poseAligned_wrapped_vggt
    return poseAligned_wrapped_vggt


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ inputs
def _rq(g, *shape):
    q = torch.randn(*shape, 4, generator=g)
    return q / q.norm(dim=-1, keepdim=True)


def _cam(g, B, S):
    """Raw camera-head encodings: unnormalised quaternions (|q| in 0.6 .. 1.5), FoV in 0.2 .. 2.6."""
    return torch.cat([torch.randn(B, S, 3, generator=g), _rq(g, B, S) * (0.6 + 0.9 * torch.rand(B, S, 1, generator=g)),
                      0.2 + 2.4 * torch.rand(B, S, 2, generator=g)], -1)


def _axis_angle(axis, deg):
    from aligned_vggt.utils.rotation import quat_to_mat
    a = torch.as_tensor(axis, dtype=F64)
    a = a / a.norm()
    h = math.radians(deg) / 2
    return quat_to_mat(torch.cat([a * math.sin(h), torch.tensor([math.cos(h)], dtype=F64)]))


def _recentred64(PA, cam):
    from aligned_vggt.utils.geometry import closed_form_inverse_se3
    from aligned_vggt.utils.rotation import quat_to_mat
    c = cam.double()
    extr = PA._pad4(torch.cat([quat_to_mat(c[..., 3:7]), c[..., :3, None]], -1))
    return extr @ closed_form_inverse_se3(extr[:, 0]).view(c.shape[0], 1, 4, 4)


def _ctx(PA, g, cam, S_prev, ov, mean_deg=75.0, spread_deg=2.0):
    """A context whose last ov encodings are extr[k] @ mean @ P_k, P_k a rotation of at most
    spread_deg (the first one exactly spread_deg) and a 0.05 translation: the overlap transforms
    inv(extr[k]) @ ctx[k] = mean @ P_k agree up to P_k."""
    B = cam.shape[0]
    extr = _recentred64(PA, cam)
    ctx = torch.cat([torch.randn(B, S_prev, 3, generator=g), _rq(g, B, S_prev), torch.rand(B, S_prev, 2, generator=g)], -1)
    for b in range(B):
        mean = torch.eye(4, dtype=F64)
        mean[:3, :3] = _axis_angle([0.3 + b, -0.5, 0.8], mean_deg)
        mean[:3, 3] = torch.randn(3, generator=g, dtype=F64)
        for k in range(ov):
            P = torch.eye(4, dtype=F64)
            if spread_deg > 0:
                ang = spread_deg * (2 * float(torch.rand(1, generator=g)) - 1) if k else spread_deg
                P[:3, :3] = _axis_angle(torch.randn(3, generator=g, dtype=F64).tolist(), ang)
                P[:3, 3] = 0.05 * torch.randn(3, generator=g, dtype=F64)
            ctx[b, S_prev - ov + k, :7] = PA._extri_to_pose_encoding((extr[b, k] @ mean @ P).view(1, 1, 4, 4))[0, 0].float()
    return ctx


def _gt(g, B, S):
    """GT w2c poses (B,S,3,4): random rotations, translations of a few units."""
    from aligned_vggt.utils.rotation import quat_to_mat
    return torch.cat([quat_to_mat(_rq(g, B, S)), 2.0 * torch.randn(B, S, 3, 1, generator=g)], -1).contiguous()


def _inputs(PA, g, B, S, S_prev, mode, ov):
    cam = _cam(g, B, S)
    ctx = _ctx(PA, g, cam, S_prev, ov) if mode in ("ctx", "ctx_gt") else None
    gt = _gt(g, B, S) if mode in ("gt", "ctx_gt") else None
    return cam, ctx, gt


# ------------------------------------------------------------------ the call
def _offset(t):
    """A device copy of t that starts one element into a NaN-filled buffer."""
    if t is None:
        return None, None
    flat = t.to(F32).contiguous().reshape(-1)
    buf = torch.full((flat.numel() + 2,), NAN, dtype=F32)
    buf[1:-1] = flat
    d = buf.to(DEV)
    return d, ctypes.c_void_p(d.data_ptr() + 4)


class Call:
    """One vggt_pose_align call on host tensors; outputs between guards."""

    def __init__(self, N, cam, ctx, gt, ov, hw=HW, S_prev=None, null=(), B=None, S=None):
        self.B, self.S = cam.shape[:2] if B is None else (B, S)
        B, S = cam.shape[:2]
        keep = [_offset(cam), _offset(ctx), _offset(gt)]
        self.bufs = {"out": _guarded((B, S, 9), F32), "pt": _guarded((B, 4, 4), F32), "scales": _guarded((B,), F32)}
        p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in self.bufs.items()}
        p["cam"] = keep[0][1]
        for n in null:
            p[n] = None
        sp = (ctx.shape[1] if ctx is not None else 0) if S_prev is None else S_prev
        self.rc = N.lib().vggt_pose_align(p["cam"], keep[1][1], sp, keep[2][1], self.B, self.S, int(ov), int(hw[0]),
                                          int(hw[1]), p["out"], p["pt"], p["scales"], _stream())
        torch.cuda.synchronize()
        self.out, self.pt, self.scales = (self.bufs[k][1].cpu() for k in ("out", "pt", "scales"))

    def guards_ok(self):
        return all(_guards_ok(buf, view.numel()) for buf, view in self.bufs.values())

    def untouched(self, names=("out", "pt", "scales")):
        return self.guards_ok() and all(bool((self.bufs[k][1] == SENT).all()) for k in names)


def _run(N, errs, tag, cam, ctx, gt, ov):
    """The call, twice: return code, guards, bitwise repeatability."""
    a, b = Call(N, cam, ctx, gt, ov), Call(N, cam, ctx, gt, ov)
    assert a.rc == OK and b.rc == OK, (tag, a.rc, b.rc)
    if not (a.guards_ok() and b.guards_ok()):
        errs.append(f"{tag}: guards around the outputs overwritten")
    for name, x, y in (("encoding", a.out, b.out), ("point transform", a.pt, b.pt), ("scales", a.scales, b.scales)):
        if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            errs.append(f"{tag}: {name} differs between two calls")
    return a


def _rotm(q):
    from aligned_vggt.utils.rotation import quat_to_mat
    return quat_to_mat(q.double()).reshape(-1, 9)


def _check(PA, errs, tag, got, gpt, gsc, cam, ctx, gt, ov, ftag, hw=HW):
    """_model_rule per quantity; returns the fp64 reference (encoding, point transform, scales)."""
    d = lambda t: None if t is None else t.double()  # noqa: E731
    B, S = cam.shape[:2]
    ref, rpt, rsc = PA.align_chunk_poses(d(cam), hw, ov, d(ctx), d(gt), form="torch")
    mod, mpt, msc = PA.align_chunk_poses(cam, hw, ov, ctx, gt, form="torch")
    assert mod.dtype == F32 and ref.dtype == F64
    _model_rule(errs, f"{tag} translation", got[..., :3].reshape(-1, 3), mod[..., :3].reshape(-1, 3),
                ref[..., :3].reshape(-1, 3), ftag + " translation")
    _model_rule(errs, f"{tag} rotation", _rotm(got[..., 3:7]), _rotm(mod[..., 3:7]), _rotm(ref[..., 3:7]),
                ftag + " rotation")
    _model_rule(errs, f"{tag} fov", got[..., 7:].reshape(-1, 2), mod[..., 7:].reshape(-1, 2), ref[..., 7:].reshape(-1, 2),
                ftag + " fov")
    _model_rule(errs, f"{tag} point transform", gpt.reshape(B * 4, 4), mpt.reshape(B * 4, 4), rpt.reshape(B * 4, 4),
                ftag + " point transform")
    _eq_bits(errs, f"{tag} point transform row 3", gpt.view(B, 4, 4)[:, 3], torch.tensor([0.0, 0, 0, 1]).expand(B, 4))
    _model_rule(errs, f"{tag} scale", gsc.view(B, 1), msc.view(B, 1), rsc.view(B, 1), ftag + " scale")
    if gt is None and not torch.equal(gsc, torch.ones(B)):
        errs.append(f"{tag}: scales without GT are not ones")
    return ref, rpt, rsc


# ================================================================== 1. frames, overlaps, modes
@pytest.mark.parametrize("S,mode,ov,B", [(1, "first", 1, 3), (1, "ctx", 1, 1), (2, "ctx", 2, 3), (2, "gt", 1, 3),
                                         (2, "ctx_gt", 1, 1), (63, "ctx", 2, 3), (64, "ctx", 64, 1), (65, "ctx", 64, 3),
                                         (65, "gt", 1, 3), (130, "ctx", 1, 3), (130, "ctx_gt", 2, 1), (130, "gt", 1, 3),
                                         (130, "first", 1, 1)])
def test_pose_align_frames(N, PA, S, mode, ov, B):
    errs = []
    S_prev = max(ov, 3) + 1
    S_prev += S_prev == S
    g = _gen(50, S, ov, B, len(mode))
    cam, ctx, gt = _inputs(PA, g, B, S, S_prev, mode, ov)
    c = _run(N, errs, f"S={S} {mode}", cam, ctx, gt, ov)
    _check(PA, errs, f"S={S} {mode} ov={ov} B={B}", c.out, c.pt, c.scales, cam, ctx, gt, ov, "pose_align")
    nul = Call(N, cam, ctx, gt, ov, null=("pt",))  # point_transform NULL
    assert nul.rc == OK
    _eq_bits(errs, "point_transform NULL: the encoding", nul.out, c.out)
    _eq_bits(errs, "point_transform NULL: the scales", nul.scales, c.scales)
    if not nul.untouched(("pt",)):
        errs.append("point_transform NULL: the unused buffer was written")
    if B > 1:  # every element is its own B = 1 run
        for b in range(B):
            one = Call(N, cam[b:b + 1], None if ctx is None else ctx[b:b + 1], None if gt is None else gt[b:b + 1], ov)
            assert one.rc == OK
            _eq_bits(errs, f"element {b} alone: encoding", one.out[0], c.out[b])
            _eq_bits(errs, f"element {b} alone: point transform", one.pt[0], c.pt[b])
            _eq_bits(errs, f"element {b} alone: scale", one.scales, c.scales[b:b + 1])
    _done(errs, (f"S={S} B={B} {mode}", {"frame_loop_trips": -(-S // 64), "ov": ov, "S_prev": S_prev}))


# ================================================================== 2. quaternions
def _branches(R):
    """mat_to_quat's candidate (argmax of q_abs) and the w < 0 flip per rotation, from fp64 matrices."""
    m = R.reshape(-1, 3, 3)
    d = torch.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                     1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], -1)
    b = d.clamp_min(0).sqrt().argmax(-1)
    wc = torch.stack([d[:, 0], m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]], -1)
    return b, wc.gather(1, b[:, None])[:, 0] < 0


def test_pose_align_quaternion_branches(N, PA):
    errs = []
    B, S = 3, 130
    cam, _, _ = _inputs(PA, _gen(51), B, S, 2, "first", 1)
    c = _run(N, errs, "branches", cam, None, None, 1)
    _check(PA, errs, "branches", c.out, c.pt, c.scales, cam, None, None, 1, "pose_align")
    br, flip = _branches(_recentred64(PA, cam)[..., :3, :3])  # first chunk: aligned = the re-centred extrinsics
    hist = [int((br == k).sum()) for k in range(4)]
    print("branch histogram", hist, "w < 0 flips", int(flip.sum()))
    if min(hist) == 0 or int(flip.sum()) == 0:
        errs.append(f"a mat_to_quat branch is not reached: {hist}, flips {int(flip.sum())}")
    if bool((c.out[..., 6] < 0).any()):
        errs.append("an output quaternion has w < 0")
    norms = cam[..., 3:7].norm(dim=-1)
    assert float(norms.min()) < 0.7 and float(norms.max()) > 1.4  # the camera quaternions are unnormalised
    _done(errs, ("branches", hist, "flips", int(flip.sum())))


def _overlap_quats(PA, cam, ctx, ov):
    """The overlap transforms' unit quaternions in fp64 and the eigenvalues of their Markley matrix."""
    from aligned_vggt.utils.data import pose_encoding_to_extri
    from aligned_vggt.utils.geometry import closed_form_inverse_se3
    B = cam.shape[0]
    extr = _recentred64(PA, cam)
    ct = closed_form_inverse_se3(extr[:, :ov].reshape(B * ov, 4, 4)).reshape(B, ov, 4, 4) \
        @ pose_encoding_to_extri(ctx.double()[:, -ov:])
    q = PA._extri_to_pose_encoding(ct)[..., 3:7]
    M = (q.unsqueeze(-1) * q.unsqueeze(-2)).sum(dim=1) / ov
    return q, torch.linalg.eigvalsh(M)


@pytest.mark.parametrize("ov", [2, 7, 64])
@pytest.mark.parametrize("mean_deg", [75.0, 179.8])
def test_pose_align_markley(N, PA, ov, mean_deg):
    """Overlap transforms within 2 degrees of a generic mean, and of one 0.2 degrees from a half turn, where
    mat_to_quat hands out quaternions of both signs: q q^T does not see the sign, the mean must not move."""
    errs = []
    B, S, S_prev = 2, max(ov, 3), ov + 1
    g = _gen(52, ov, int(mean_deg))
    cam = _cam(g, B, S)
    ctx = _ctx(PA, g, cam, S_prev, ov, mean_deg)
    c = _run(N, errs, "markley", cam, ctx, None, ov)
    tag = f"Markley ov={ov} mean {mean_deg}"
    _check(PA, errs, tag, c.out, c.pt, c.scales, cam, ctx, None, ov, "markley")
    q, eig = _overlap_quats(PA, cam, ctx, ov)
    gap = float((eig[:, 3] - eig[:, 2]).min())
    signs = (q * q[:, :1]).sum(-1) < 0  # quaternions opposite to the first one
    assert gap >= 0.9, f"eigen-gap {gap}"
    if mean_deg > 179:  # the inputs reach the case: at every ov a quaternion opposite to the first one
        assert bool(signs.any()), f"{tag}: no overlap quaternion has the opposite sign"
    _done(errs, (tag, {"eigen_gap": gap, "opposite_sign_quaternions": int(signs.sum())}))


def test_pose_align_identical_overlap(N, PA):
    errs = []
    B, S, S_prev, ov = 2, 6, 7, 5
    g = _gen(53)
    cam = _cam(g, B, S)
    ctx = _ctx(PA, g, cam, S_prev, ov, spread_deg=0.0)
    c = _run(N, errs, "identical", cam, ctx, None, ov)
    _check(PA, errs, "identical overlap transforms", c.out, c.pt, c.scales, cam, ctx, None, ov, "markley")
    _, eig = _overlap_quats(PA, cam, ctx, ov)
    assert float(eig[:, 2].abs().max()) < 1e-6  # rank one up to the fp32 rounding of the context
    _done(errs, ("identical", {"second_eigenvalue": float(eig[:, 2].abs().max())}))


# ================================================================== 3. GT scale
def test_pose_align_negative_correlation(N, PA):
    """GT translations that run against the predicted ones: sum x.y < 0, the scale is its absolute value."""
    errs = []
    B, S = 3, 65
    g = _gen(54)
    cam = _cam(g, B, S)
    x = _recentred64(PA, cam)[..., :3, 3]
    gt = torch.cat([torch.eye(3).expand(B, S, 3, 3), (-2.0 * x + 0.05 * torch.randn(B, S, 3, generator=g).double()
                                                       + torch.tensor([1.0, -2.0, 0.5], dtype=F64))[..., None].float()],
                   -1).contiguous()
    y = gt.double()[..., 3] - gt.double()[:, :1, :, 3]
    quot = (x * y).sum(dim=(1, 2)) / (x * x).sum(dim=(1, 2))
    assert bool((quot < -1.5).all()), quot
    for ctx in (None, _ctx(PA, g, cam, 4, 2)):
        mode = "gt" if ctx is None else "ctx_gt"
        c = _run(N, errs, mode, cam, ctx, gt, 2)
        _, _, rsc = _check(PA, errs, f"negative correlation {mode}", c.out, c.pt, c.scales, cam, ctx, gt, 2, "gt scale")
        if not bool((c.scales > 1.5).all()) or float((rsc + quot).abs().max()) > 1e-6:
            errs.append(f"{mode}: scales {c.scales.tolist()} are not |{quot.tolist()}|")
    _done(errs, ("negative correlation", quot.tolist()))


def test_pose_align_zero_translations_nan(N, PA):
    """All predicted translations zero with GT: 0 / 0, a NaN scale in the kernel and in the model, carried
    into the translations (and, through the reference's 4 x 4 product, into the quaternion's x, y, z)."""
    B, S = 2, 65
    g = _gen(55)
    cam = _cam(g, B, S)
    cam[..., :3] = 0.0
    gt = _gt(g, B, S)
    a, b = Call(N, cam, None, gt, 1), Call(N, cam, None, gt, 1)
    assert a.rc == OK and a.guards_ok()
    mod, mpt, msc = PA.align_chunk_poses(cam, HW, 1, None, gt, form="torch")
    assert bool(torch.isnan(a.scales).all()) and bool(torch.isnan(msc).all())
    assert bool(torch.isnan(a.out[..., :3]).all()) and bool(torch.isnan(mod[..., :3]).all())
    assert torch.equal(torch.isnan(a.out), torch.isnan(mod))
    assert torch.equal(a.out[..., 7:], b.out[..., 7:]) and bool(torch.isfinite(a.out[..., 6:]).all())
    assert torch.equal(torch.isnan(a.out), torch.isnan(b.out))
    assert bool(torch.isfinite(a.pt).all()) and torch.equal(a.pt, b.pt)


# ================================================================== 4. error returns
def test_pose_align_error_returns(N, PA):
    errs = []
    g = _gen(56)
    cam, ctx, _ = _inputs(PA, g, 1, 3, 4, "ctx", 1)
    gt = _gt(g, 1, 3)
    big, bigctx, _ = _inputs(PA, g, 1, 66, 66, "ctx", 1)
    cases = [("overlap 65", Call(N, big, bigctx, None, 65)),
             ("overlap 0", Call(N, cam, ctx, None, 0)),
             ("overlap above S", Call(N, cam, ctx, None, 4)),
             ("overlap above S_prev", Call(N, cam, ctx, None, 3, S_prev=2)),
             ("S = 1 with GT", Call(N, cam[:, :1], None, gt[:, :1], 1)),
             ("S = 1 with GT and a context", Call(N, cam[:, :1], ctx, gt[:, :1], 1)),
             ("cam NULL", Call(N, cam, ctx, None, 1, null=("cam",))),
             ("aligned_pose_enc NULL", Call(N, cam, ctx, None, 1, null=("out",))),
             ("scales NULL", Call(N, cam, ctx, None, 1, null=("scales",))),
             ("B = 0", Call(N, cam, ctx, None, 1, B=0, S=3)),
             ("S = 0", Call(N, cam, ctx, None, 1, B=1, S=0)),
             ("H = 0", Call(N, cam, ctx, None, 1, hw=(0, 518))),
             ("W < 0", Call(N, cam, ctx, None, 1, hw=(154, -2)))]
    for name, c in cases:
        if c.rc != ERR_SHAPE or not c.untouched():
            errs.append(f"{name}: returned {c.rc} or wrote its outputs")
    # with GT the overlap is neither read nor checked
    ok = Call(N, cam, ctx, gt, 99)
    if ok.rc != OK or not ok.guards_ok():
        errs.append(f"overlap 99 with GT: returned {ok.rc}")
    _done(errs)


def test_overlap_65_falls_back_to_torch_form(N, PA, monkeypatch):
    monkeypatch.delenv("VGGT_POSE", raising=False)
    g = _gen(57)
    S = S_prev = 66
    cam = _cam(g, 2, S)
    ctx = _ctx(PA, g, cam, S_prev, 65)
    got = PA.align_chunk_poses(cam.to(DEV), HW, 65, ctx.to(DEV))
    want = PA.align_chunk_poses(cam.to(DEV), HW, 65, ctx.to(DEV), form="torch")
    for a, b in zip(got, want):
        assert a.is_cuda and torch.equal(a, b)
    with pytest.raises(RuntimeError, match=r"\(code -1\)"):
        PA.align_chunk_poses(cam.to(DEV), HW, 65, ctx.to(DEV), form="hip")
    # and the knob: VGGT_POSE=device takes the torch form at an overlap the kernel accepts
    monkeypatch.setenv("VGGT_POSE", "device")
    dev = PA.align_chunk_poses(cam.to(DEV), HW, 3, ctx.to(DEV))
    tor = PA.align_chunk_poses(cam.to(DEV), HW, 3, ctx.to(DEV), form="torch")
    assert all(torch.equal(a, b) for a, b in zip(dev, tor))


# ================================================================== 5. no synchronisation
def _dev_enc(g, B, S, h=6, w=8):
    return {"images": torch.zeros(B, S, 3, h, w, device=DEV), "pose_enc": _cam(g, B, S).to(DEV),
            "depth": torch.rand(B, S, h, w, 1, generator=g).to(DEV), "depth_conf": torch.ones(B, S, h, w, device=DEV),
            "world_points": torch.randn(B, S, h, w, 3, generator=g).to(DEV),
            "world_points_conf": torch.ones(B, S, h, w, device=DEV)}


def test_align_chunk_does_not_synchronise(N, PA, monkeypatch):
    monkeypatch.delenv("VGGT_POSE", raising=False)
    B, S, ov = 2, 5, 2

    def sequence(guard):
        g = _gen(58)
        outs = []
        for use_gt in (False, True):  # first chunk, context | GT without a context, context + GT
            encs = [_dev_enc(g, B, S), _dev_enc(g, B, S)]
            gts = [_gt(g, B, S).to(DEV) if use_gt else None for _ in encs]
            torch.cuda.synchronize()
            before = torch.cuda.get_sync_debug_mode()
            if guard:
                torch.cuda.set_sync_debug_mode("error")
            try:
                ctx = None
                for enc, gt in zip(encs, gts):
                    ctx = PA.align_chunk(enc, ov, ctx, gt, False)
            finally:
                torch.cuda.set_sync_debug_mode(before)
            outs.append(ctx)
        return outs

    warm = sequence(False)  # the library is loaded, the allocator is warm
    got = sequence(True)
    for a, b in zip(warm, got):
        for k in ("pose_enc", "depth", "world_points"):
            assert len(b[k]) == 2 and all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


# ================================================================== 6. the model
@pytest.fixture(scope="module")
def model(PA):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt.backbone.aggregator import Aggregator
    from aligned_vggt.utils.synthetic import condition_pose_outputs_, synthetic_init_
    m = PA.VGGT(enable_track=False)
    m.aggregator = Aggregator(depth=4, dino_depth=1)
    m.intermediate_layer_indices = [0, 1, 2, 3]
    synthetic_init_(m, seed=7)
    condition_pose_outputs_(m)
    return m.cuda().eval()


def test_pose_aligned_state_dict_names(model):
    sd = model.state_dict()
    for k in ("aggregator.camera_token", "point_head.scratch.output_conv2.2.weight", "depth_head.projects.0.weight",
              "camera_head.trunk.0.attn.qkv.weight"):
        assert k in sd, k


@pytest.mark.parametrize("B,ov,use_gt", [(1, 1, False), (1, 2, False), (1, 2, True), (2, 1, True)])
def test_model_two_chunks(N, PA, model, monkeypatch, B, ov, use_gt):
    from aligned_vggt.utils.synthetic import synthetic_images
    monkeypatch.delenv("VGGT_POSE", raising=False)
    errs = []
    S, H, W = 3, 42, 56
    imgs = torch.cat([synthetic_images(1, 2 * S - ov, H, W, seed=30 + b) for b in range(B)], 0).cuda()
    chunks = [list(range(0, S)), list(range(S - ov, 2 * S - ov))]
    g = _gen(60, B, ov)
    gts = [_gt(g, B, S).cuda() if use_gt else None for _ in chunks]
    fwd = ctx = None
    for ci, ids in enumerate(chunks):
        x = imgs[:, ids].contiguous()
        gt_before = None if gts[ci] is None else gts[ci].clone()
        fwd = model(x, ov, fwd, gt_poses=gts[ci])
        enc = model.encode_chunk(x)
        raw = {k: v.clone() for k, v in enc.items()}
        ctx_pe = ctx["pose_enc"][-1] if ctx is not None else None
        new = model.align_chunk(enc, ov, ctx, gt_poses=gts[ci])
        assert ctx is None or all(new[k] is ctx[k] for k in new)
        ctx = new
        if use_gt:
            assert torch.equal(gts[ci], gt_before)
        tag = f"chunk {ci}"
        # pose algebra: the kernel against the torch forms on the model's own raw camera-head output
        hw = (H, W)
        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        pe, pt, sc = PA.align_chunk_poses(raw["pose_enc"], hw, ov, ctx_pe, gts[ci], form="hip")
        _eq_bits(errs, f"{tag} pose_enc is the kernel's", ctx["pose_enc"][ci].cpu(), pe.cpu())
        _check(PA, errs, tag, pe.cpu(), pt.cpu(), sc.cpu(), cpu(raw["pose_enc"]), cpu(ctx_pe), cpu(gts[ci]), ov, "model",
               hw)
        # depth: one IEEE multiply by the scale (none without GT)
        want = raw["depth"] * sc.view(B, 1, 1, 1, 1) if use_gt else raw["depth"]
        _eq_bits(errs, f"{tag} depth", ctx["depth"][ci].cpu(), want.cpu())
        _eq_bits(errs, f"{tag} depth_conf", ctx["depth_conf"][ci].cpu(), raw["depth_conf"].cpu())
        # points: T (s p) + t, fp64 and fp32 on the host from the kernel's own transform and scale
        p64 = raw["world_points"].cpu().double() * sc.cpu().double().view(B, 1, 1, 1, 1)
        T64 = pt.cpu().double()
        r64 = (p64.reshape(B, -1, 3) @ T64[:, :3, :3].transpose(-1, -2) + T64[:, None, :3, 3]).reshape(-1, 3)
        p32 = raw["world_points"].cpu() * sc.cpu().view(B, 1, 1, 1, 1)
        T32 = pt.cpu()
        m32 = (p32.reshape(B, -1, 3) @ T32[:, :3, :3].transpose(-1, -2) + T32[:, None, :3, 3]).reshape(-1, 3)
        _model_rule(errs, f"{tag} world_points", ctx["world_points"][ci].cpu().reshape(-1, 3), m32, r64, "model points")
        assert ctx["world_points"][ci].shape == (B, S, H, W, 3) and ctx["depth"][ci].shape == (B, S, H, W, 1)
    torch.cuda.synchronize()
    assert sorted(fwd.keys()) == sorted(ctx.keys()) == ["depth", "depth_conf", "images", "pose_enc", "world_points",
                                                         "world_points_conf"]
    for k in fwd:
        assert len(fwd[k]) == len(ctx[k]) == 2
        for ci in range(2):
            _eq_bits(errs, f"forward vs align_chunk(encode_chunk) {k}[{ci}]", fwd[k][ci].cpu(), ctx[k][ci].cpu())
    _done(errs)


def _synthetic_w2c(n):
    yaw = torch.linspace(0, 0.6, n)
    c2w = torch.eye(4).repeat(n, 1, 1)
    c2w[:, 0, 0], c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 2, 2] = yaw.cos(), yaw.sin(), -yaw.sin(), yaw.cos()
    c2w[:, :3, 3] = torch.cumsum(torch.stack([yaw.sin(), torch.zeros(n), yaw.cos()], -1), 0)
    return torch.linalg.inv(c2w)[:, :3, :][None].contiguous()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("mode,n,w,ov", [("chunk_overlap", 7, 3, 1), ("chunk_gt", 9, 3, 0)])
def test_sequence_grouped_encode_matches(N, model, monkeypatch, mode, n, w, ov):
    """Three chunks through apply_sequence_to_model: the grouped encode (default: the three equal chunks as
    one batch) against one chunk at a time, by the rule of test_pipeline_grouped_encode_matches."""
    from aligned_vggt.dist.pipeline import apply_sequence_to_model
    from aligned_vggt.utils.data import generate_chunks
    from aligned_vggt.utils.synthetic import synthetic_images
    monkeypatch.delenv("VGGT_POSE", raising=False)
    H, W = 42, 56
    assert len(generate_chunks(n, mode, w, ov)) == 3
    imgs, extr = synthetic_images(1, n, H, W, seed=41), _synthetic_w2c(n)
    outs = {}
    for group in (None, "1"):
        if group is None:
            monkeypatch.delenv("VGGT_ENCODE_GROUP", raising=False)
        else:
            monkeypatch.setenv("VGGT_ENCODE_GROUP", group)
        batch = {"images": imgs.cuda(), "extrinsics": extr.cuda()}
        outs[group] = apply_sequence_to_model(batch, model, [w], [ov], mode, "scale_from_poses")
    merged = n
    for k, shape in (("pose_enc", (1, merged, 9)), ("depth", (1, merged, H, W, 1)), ("world_points", (1, merged, H, W, 3)),
                     ("depth_conf", (1, merged, H, W)), ("world_points_conf", (1, merged, H, W))):
        assert outs[None][k].shape == outs["1"][k].shape == shape, (k, outs[None][k].shape)
        assert bool(torch.isfinite(outs[None][k]).all()), k
        e = _rel(outs[None][k], outs["1"][k])
        print(mode, k, "grouped vs per chunk", e)
        assert e < 1e-5, (mode, k, e)


def test_figures():
    """Not a check: prints the figures the tests above gathered (DESIGN.md tabulates them)."""
    _figures("")
