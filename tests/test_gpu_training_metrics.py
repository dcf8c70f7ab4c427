"""The metrics module on the GPU: the two kernels of csrc/pose.hip (vggt_gt_pose_align,
vggt_trajectory_errors) against fp64 on the host, the Python routes built on them, the absence
of host synchronisations, and Metrics.forward end to end on both sequence_outputs routes.

Bounds (tests/edge_rules.py: u = 2^-24, a bound is derived from the documented arithmetic).
Both kernels compute in fp64 from the fp32 inputs and round each output to fp32 once, so every
bound is  u |ref|  (the one rounding)  +  E64  (what the fp64 evaluation and the host's own fp64
reference may differ by).

  scale quotients   a / d with a, d fp64 sums of n products of fp32 pairs (exact in fp64): each sum is
                    within n 2^-53 sum|terms| whatever the order, so E64 = 4 n 2^-53 (1 + sum|x y| /
                    |sum x y|) |ref|  (kernel and reference, numerator and denominator).
  SIM3              the fp64 Umeyama takes the SVD of the 3x3 covariance C from Jacobi on C^T C, which
                    squares C's condition number: the singular vectors carry c 2^-53 k(C)^2 with c of
                    order 10^2 (three sweeps of 3 rotations, the products that follow).  The test clouds
                    have axis spreads 3 : 2 : 1 with a Sim(3) (or mirrored Sim(3)) image, k(C) <= 2^5 for
                    every seed used, so E64 = 2^-30 (1/64 of u) times the magnitude of the output: 1 for
                    R, |mean_y| + c |mean_x| for t, c for the scale.
  pose_enc_out      an fp32 chain, as the reference's (w2c -> c2w, x c, T ., -> w2c, mat_to_quat), checked
                    against its fp64 restatement fed with the kernel's own (already checked) fp32 transform
                    and scale.  A rotation entry from a quaternion takes ~10 roundings on values <= 3
                    (30 u); it enters the result twice (the first inverse, the product with T), each of
                    the four 3-term products adds gamma_3, the scale and the sums ~4 u: below 128 u of
                    M = |Ra^T| (|Rt| c |R^T| |t| + |tt|), the product of absolute values, per
                    translation component.  mat_to_quat divides differences of entries carrying <= 100 u
                    by 2 q_max >= 2 and takes one square root of an argument >= 1: 512 u absolute.  The
                    FoV pair is an fp64 round trip rounded once: u |ref| + 2^-40.
  ate_vec           the fp32 difference itself (fp64 difference of two fp32 values, rounded once): bitwise.
  ate_norm, scale_factor
                    u |ref| + 8 2^-53 (sum of absolute terms).
  rpe_trans         err = inv(inv(g_i) g_j) inv(p_i) p_j: three adjugate inverses and three products in
                    fp64.  An inverse is within c 2^-53 k(A) |A^-1| of the exact one, and the errors pass
                    through the products, so the entries of err carry E64 = 256 2^-53 k(g_i) k(g_rel)
                    k(p_i) max(1, |err|_max); the condition numbers are taken from the inputs in fp64.
  rpe_rot           acos((tr - 1) / 2) with the trace carrying 3 E64: the fp64 term is the larger of
                    |acos(c +- 1.5 E64) - acos(c)| (clamped), which is 1.5 E64 / sqrt(1 - c^2) away from
                    +-1 and sqrt(3 E64) at c = 1 (pred == gt) -- the conditioning term near 0.

Routes.  The host functions take their scale from numpy fp32 sums of n = 3 S <= 30 products: within
gamma_n (1 + sum|x y| / |sum x y|) <= 2^-17 of the kernel's; "agree" is rtol 2^-16 on every scaled
tensor.  Host SIM3 is an fp32 LAPACK SVD of a 3x3 with k <= 2^5 followed by the same fp32 chain: 2^-12
relative to each tensor's largest magnitude.

End to end.  GT translations are exactly twice the predicted ones, so the LSE scale is 2.0 in any
arithmetic and both routes feed identical bits to the same kernels: every value is compared bitwise.
With noisy GT the routes' scales differ by the host's fp32 summation error ds <= 2^-17 (above), every
aligned translation by ds |p|: the trajectory values are compared under 4 ds max|p| (scale_var: every
factor g.p / p.p moves by ds f, their variance by 2 ds max f^2; 8 ds max f^2 with f^2 <= 1.5).
"""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from edge_rules import (ERR_UNSUPPORTED, U, _centre_poses, _done, _eq_bits, _raises, _svd_centres, _svd_pair_check,
                        _within)

pytestmark = pytest.mark.gpu

F64 = torch.float64
DEV = "cuda:0"
E30 = 2.0 ** -30


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _rot64(q):
    """quat_to_mat (xyzw, 2 / |q|^2 scaling) in fp64."""
    from aligned_vggt.utils.rotation import quat_to_mat
    return quat_to_mat(q.double())


def _poses(B, S, width, g, mirror=False, sim=(1.7, (0.4, -1.0, 2.0))):
    """(pose_enc (B,S,width), gt_extr (B,S,3,4)) fp32: predicted centres x spread 3 : 2 : 1, GT
    centres s R0 (M) x + t0 + noise with M = diag(1, 1, -1) when mirrored."""
    x = torch.randn(B, S, 3, generator=g, dtype=F64) * torch.tensor([3.0, 2.0, 1.0], dtype=F64)
    q = torch.randn(B, S, 4, generator=g, dtype=F64)
    q = q / q.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(B, S, 1, generator=g, dtype=F64))
    q = q.float()
    R = _rot64(q)
    t = -(R @ x[..., None])[..., 0]
    enc = torch.cat([t.float(), q, 0.8 + 0.5 * torch.rand(B, S, 2, generator=g)], -1)[..., :width].contiguous()
    R0 = _rot64(torch.tensor([0.3, -0.2, 0.5, 0.8]))
    xm = x * torch.tensor([1.0, 1.0, -1.0], dtype=F64) if mirror else x
    y = sim[0] * xm @ R0.T + torch.tensor(sim[1], dtype=F64) + 0.05 * torch.randn(B, S, 3, generator=g, dtype=F64)
    Rg = _rot64(torch.randn(B, S, 4, generator=g))
    tg = -(Rg @ y[..., None])[..., 0]
    return enc, torch.cat([Rg, tg[..., None]], -1).float().contiguous()


def _quotient(x, y):
    """|sum x y / sum x x| over the last two axes in fp64, and the bound's condition term."""
    x, y = x.double(), y.double()
    a, d = (x * y).sum((-1, -2)), (x * x).sum((-1, -2))
    ref = (a / d).abs()
    kappa = 1.0 + (x * y).abs().sum((-1, -2)) / a.abs().clamp_min(1e-300)
    n = x.shape[-1] * x.shape[-2]
    return ref, ref * (U + 4 * n * 2.0 ** -53 * kappa)


# ------------------------------------------------------------------------------------------------- vggt_gt_pose_align
@pytest.mark.parametrize("width", [7, 9])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 130])
def test_pose_scale_modes_vs_fp64(N, S, B, width):
    errs = []
    enc, extr = _poses(B, S, width, _gen(1, S, B, width))
    e, x = enc.to(DEV), extr.to(DEV)
    for W in sorted({-1, S // 2 + 1}):
        Wn = S if W == -1 else W
        sc, T, out = N.gt_pose_align(e, x, N.GT_POSE_SCALE, W)
        assert sc.shape == (B,) and T is None and out is None
        ref, bound = _quotient(enc[:, :Wn, :3], extr[:, :Wn, :3, 3])
        w = _within(errs, f"scale W={W}", sc.cpu(), ref, bound)
        print(f"scale S={S} W={W}: worst {w:.3f} of the bound")
    sc, _, _ = N.gt_pose_align(e, x, N.GT_POSE_PER_FRAME)
    assert sc.shape == (B, S)
    got = sc.cpu()
    _eq_bits(errs, "frame 0", got[:, 0], torch.ones(B))
    if S > 1:
        ref, bound = _quotient(enc[:, 1:, None, :3], extr[:, 1:, None, :3, 3])
        _within(errs, "per frame", got[:, 1:], ref, bound)
    _done(errs)


def test_pose_scale_zero_denominator_is_nan(N):
    enc, extr = _poses(2, 5, 9, _gen(2))
    enc[0, :, :3] = 0.0   # sum x x = 0 for batch element 0
    enc[1, 2, :3] = 0.0   # and for one frame of element 1
    e, x = enc.to(DEV), extr.to(DEV)
    sc = N.gt_pose_align(e, x, N.GT_POSE_SCALE)[0].cpu()
    assert math.isnan(sc[0]) and math.isfinite(sc[1])
    pf = N.gt_pose_align(e, x, N.GT_POSE_PER_FRAME)[0].cpu()
    assert pf[0, 0] == 1.0 and torch.isnan(pf[0, 1:]).all()
    assert math.isnan(pf[1, 2]) and torch.isfinite(pf[1, [0, 1, 3, 4]]).all()


def _umeyama64(enc, extr, W):
    """(R (B,3,3), t (B,3), c (B,), magnitude of t's terms) of the repository's numpy umeyama in fp64 on
    the centres -R^T t taken in fp64 from the fp32 inputs."""
    from aligned_vggt.utils import alignment as A
    R = _rot64(enc[:, :W, 3:7])
    x = -(R.transpose(-1, -2) @ enc[:, :W, :3].double()[..., None])[..., 0]
    Rg = extr[:, :W, :, :3].double()
    y = -(Rg.transpose(-1, -2) @ extr[:, :W, :, 3].double()[..., None])[..., 0]
    out = [A.umeyama(x[b].numpy().T, y[b].numpy().T) for b in range(enc.shape[0])]
    Rr = torch.tensor(np.stack([o[0] for o in out]))
    tr = torch.tensor(np.stack([o[1] for o in out]))
    cr = torch.tensor(np.array([o[2] for o in out]))
    mag = y.mean(1).abs() + cr[:, None] * x.mean(1).abs().sum(-1, keepdim=True)
    return Rr, tr, cr, mag


def _aligned_enc64(enc, T, c, hw):
    """apply_sim3_alignment restated in fp64 on the fp32 transform and scale; also the magnitude M of
    the translation's terms (product of absolute values)."""
    from aligned_vggt.utils.rotation import mat_to_quat
    R = _rot64(enc[..., 3:7])
    t = enc[..., :3].double()
    Rp = R.transpose(-1, -2)
    tp = -(Rp @ t[..., None])[..., 0] * c.double()[:, None, None]
    Rt, tt = T[:, None, :3, :3].double(), T[:, None, :3, 3].double()
    Ra = Rt @ Rp
    ta = (Rt @ tp[..., None])[..., 0] + tt
    Rw = Ra.transpose(-1, -2)
    tw = -(Rw @ ta[..., None])[..., 0]
    M = (Rw.abs() @ ((Rt.abs() @ (c.double()[:, None, None, None] * (Rp.abs() @ t.abs()[..., None])))
                     + tt.abs()[..., None]))[..., 0]
    H, Wd = hw
    fov = enc[..., 7:9].double()
    size = torch.tensor([H / 2.0, Wd / 2.0], dtype=F64)
    fov = 2 * torch.atan(size / (size / torch.tan(fov / 2)))
    return tw, mat_to_quat(Rw), fov, M


@pytest.mark.parametrize("mirror", [False, True], ids=["proper", "reflection"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [63, 64, 65, 130])
def test_pose_sim3_vs_fp64(N, S, B, mirror):
    """SIM3 needs W >= 3 centres, so S in {1, 2} run the two scale modes only (above)."""
    errs = []
    enc, extr = _poses(B, S, 9, _gen(3, S, B, mirror), mirror=mirror)
    hw = (28, 42)
    for W in (-1, S // 2 + 1, 3):
        Wn = S if W == -1 else W
        e = enc.to(DEV)
        sc, T, out = N.gt_pose_align(e, extr.to(DEV), N.GT_POSE_SIM3, W, hw)
        Rr, tr, cr, mag = _umeyama64(enc, extr, Wn)
        if mirror:  # the branch is taken: a proper rotation although the clouds are mirror images
            assert (torch.linalg.det(Rr) > 0.99).all()
        Th = T.cpu()
        _eq_bits(errs, "last row", Th[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4).contiguous())
        if Wn > 3:  # three centres span a plane: the rank-2 covariance is outside the k(C) the bound assumes
            _within(errs, f"R W={W}", Th[:, :3, :3], Rr, U * Rr.abs() + E30)
            _within(errs, f"t W={W}", Th[:, :3, 3], tr, U * tr.abs() + E30 * mag)
            _within(errs, f"c W={W}", sc.cpu(), cr, cr * (U + E30))
        else:
            torch.testing.assert_close(Th[:, :3, :3].double(), Rr, rtol=0, atol=1e-5)
            torch.testing.assert_close(sc.cpu().double(), cr, rtol=1e-5, atol=0)
        tw, qw, fov, M = _aligned_enc64(enc, Th, sc.cpu(), hw)
        got = out.cpu()
        assert got.shape == (B, S, 9)
        _within(errs, f"enc t W={W}", got[..., :3], tw, 128 * U * M)
        sign = torch.where((got[..., 3:7].double() * qw).sum(-1, keepdim=True) < 0, -1.0, 1.0)
        _within(errs, f"enc q W={W}", got[..., 3:7], sign * qw, torch.full_like(qw, 512 * U))
        _within(errs, f"enc fov W={W}", got[..., 7:], fov, U * fov.abs() + 2.0 ** -40)
        # in place: pose_enc_out may be pose_enc
        alias = enc.to(DEV)
        sc2, T2, out2 = N.gt_pose_align(alias, extr.to(DEV), N.GT_POSE_SIM3, W, hw, pose_enc_out=alias)
        assert out2.data_ptr() == alias.data_ptr()
        _eq_bits(errs, f"alias enc W={W}", alias.cpu(), got)
        _eq_bits(errs, f"alias T W={W}", T2.cpu(), Th)
        _eq_bits(errs, f"alias c W={W}", sc2.cpu(), sc.cpu())
    _done(errs)


@pytest.mark.parametrize("kind", ["general", "line"])
def test_pose_sim3_shares_its_svd_with_the_point_alignment(N, kind):
    """umeyama3's half of the pair that csrc/small_eig.h serves (the other half, on the same centres:
    test_gpu_geometry_edges.py::test_solve_shares_its_svd_with_the_pose_alignment): the centres as poses with
    identity rotations, Sim(3) mode."""
    errs = []
    enc, extr = _centre_poses(*_svd_centres(kind))
    sc, T, _ = N.gt_pose_align(enc.to(DEV), extr.to(DEV), N.GT_POSE_SIM3)
    Th = T.cpu()[0]
    _svd_pair_check(errs, "gt_pose_align", kind, Th[:3, :3].contiguous(), Th[:3, 3].contiguous(), sc.cpu()[0])
    _done(errs)


def test_pose_sim3_refuses_seven_wide(N):
    enc, extr = _poses(1, 8, 7, _gen(4))
    _raises(ERR_UNSUPPORTED, N.gt_pose_align, enc.to(DEV), extr.to(DEV), N.GT_POSE_SIM3, -1, (28, 42))


# ------------------------------------------------------------------------------------------------- vggt_trajectory_errors
def _c2w(B, S, g, rigid=True, spread=2.0):
    q = torch.randn(B, S, 4, generator=g)
    M = torch.eye(4).repeat(B, S, 1, 1)
    M[..., :3, :3] = _rot64(q).float()
    M[..., :3, 3] = spread * torch.randn(B, S, 3, generator=g)
    if not rigid:  # sheared, scaled and with a projective last row: only the general inverse is right
        M[..., :3, :3] = M[..., :3, :3] @ (torch.eye(3) + 0.3 * torch.randn(B, S, 3, 3, generator=g))
        M[..., 3, :3] = 0.05 * torch.randn(B, S, 3, generator=g)
        M[..., 3, 3] = 1.0 + 0.2 * torch.rand(B, S, generator=g)
    return M.contiguous()


def _check_errors(errs, tag, out, pred, gt, delta):
    p, g = pred.double(), gt.double()
    B, S = pred.shape[:2]
    pt, gt_ = p[..., :3, 3], g[..., :3, 3]
    if "ate_vec" in out:
        _eq_bits(errs, f"{tag} ate_vec", out["ate_vec"].cpu(), (pt - gt_).float())
        ref = (pt - gt_).norm(dim=-1)
        _within(errs, f"{tag} ate_norm", out["ate_norm"].cpu(), ref, ref * (U + 8 * 2.0 ** -53))
    if "scale_factor" in out:
        assert out["scale_factor"].shape == (B, S - 1)
        den = (pt[:, 1:] ** 2).sum(-1).clamp_min(float(np.float32(1e-8)))
        ref = (gt_[:, 1:] * pt[:, 1:]).sum(-1) / den
        bound = U * ref.abs() + 8 * 2.0 ** -53 * ((gt_[:, 1:] * pt[:, 1:]).abs().sum(-1) / den + ref.abs())
        _within(errs, f"{tag} scale_factor", out["scale_factor"].cpu(), ref, bound)
    if "rpe_trans" in out:
        n = max(S - delta, 0)
        assert out["rpe_trans"].shape == (B, n) and out["rpe_rot"].shape == (B, n)
        if n == 0:
            return
        inv = torch.linalg.inv
        p_rel, g_rel = inv(p[:, :-delta]) @ p[:, delta:], inv(g[:, :-delta]) @ g[:, delta:]
        err = inv(g_rel) @ p_rel
        cond = torch.linalg.cond
        E64 = 256 * 2.0 ** -53 * cond(g[:, :-delta]) * cond(g_rel) * cond(p[:, :-delta]) \
            * err.abs().amax((-1, -2)).clamp_min(1.0)
        ref_t = err[..., :3, 3].norm(dim=-1)
        wt = _within(errs, f"{tag} rpe_trans", out["rpe_trans"].cpu(), ref_t, U * ref_t + 2 * E64)
        c = ((err[..., 0, 0] + err[..., 1, 1] + err[..., 2, 2] - 1) / 2)
        ac = lambda v: torch.acos(v.clamp(-1.0, 1.0))  # noqa: E731
        ref_r = ac(c)
        e_r = torch.maximum((ac(c + 1.5 * E64) - ref_r).abs(), (ac(c - 1.5 * E64) - ref_r).abs())
        wr = _within(errs, f"{tag} rpe_rot", out["rpe_rot"].cpu(), ref_r, U * ref_r + e_r)
        print(f"{tag}: rpe_trans {wt:.3f}, rpe_rot {wr:.3f} of the bound")


@pytest.mark.parametrize("delta", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 65, 257])
def test_trajectory_errors_vs_fp64(N, S, delta):
    """S = delta (nothing written to the RPE outputs) and S = delta + 1 (one pair) are in the grid:
    (1, 1), (2, 1), (3, 3), (4, 3)."""
    errs = []
    for B in (1, 3):
        g = _gen(5, S, delta, B)
        pred, gt = _c2w(B, S, g), _c2w(B, S, g)
        out = N.trajectory_errors(pred.to(DEV), gt.to(DEV), delta)
        assert set(out) == {"ate_vec", "ate_norm", "rpe_trans", "rpe_rot", "scale_factor"}
        _check_errors(errs, f"S={S} B={B}", out, pred, gt, delta)
    _done(errs)


def test_trajectory_errors_pred_equals_gt(N):
    errs = []
    pred = _c2w(2, 65, _gen(6))
    out = N.trajectory_errors(pred.to(DEV), pred.clone().to(DEV), 1)
    assert torch.count_nonzero(out["ate_vec"]) == 0 and torch.count_nonzero(out["ate_norm"]) == 0
    _check_errors(errs, "equal", out, pred, pred, 1)
    assert float(out["rpe_rot"].max()) < 1e-6 and float(out["rpe_trans"].max()) < 1e-12
    torch.testing.assert_close(out["scale_factor"].cpu(), torch.ones(2, 64), rtol=2 * U, atol=0)
    _done(errs)


def test_trajectory_errors_general_inverse(N):
    """Non-rigid but invertible poses: the rigid closed form [R^T | -R^T t] would be far off."""
    from aligned_vggt.utils.geometry import closed_form_inverse_se3
    errs = []
    g = _gen(7)
    pred, gt = _c2w(2, 9, g, rigid=False, spread=1.0), _c2w(2, 9, g, rigid=False, spread=1.0)
    out = N.trajectory_errors(pred.to(DEV), gt.to(DEV), 2)
    _check_errors(errs, "non-rigid", out, pred, gt, 2)
    rigid = closed_form_inverse_se3(pred[0, :-2].double()) @ pred[0, 2:].double()
    exact = torch.linalg.inv(pred[0, :-2].double()) @ pred[0, 2:].double()
    assert float((rigid - exact).abs().max()) > 1e-2  # the test can tell the two inverses apart
    _done(errs)


def test_trajectory_errors_null_outputs(N):
    errs = []
    g = _gen(8)
    pred, gt = _c2w(2, 6, g), _c2w(2, 6, g)
    full = N.trajectory_errors(pred.to(DEV), gt.to(DEV), 1)
    for want in ({"ate": True}, {"rpe": True}, {"scale": True}, {}):
        kw = {"ate": False, "rpe": False, "scale": False, **want}
        part = N.trajectory_errors(pred.to(DEV), gt.to(DEV), 1, **kw)
        keys = {"ate": {"ate_vec", "ate_norm"}, "rpe": {"rpe_trans", "rpe_rot"}, "scale": {"scale_factor"}}
        assert set(part) == set().union(*(keys[k] for k in want))
        for k, v in part.items():
            _eq_bits(errs, k, v.cpu(), full[k].cpu())
    _done(errs)


# ------------------------------------------------------------------------------------------------- routes
def _step(B=2, S=7, H=6, W=9, seed=0, sim3=False):
    g = _gen(9, seed)
    enc, extr = _poses(B, S, 9, g)
    if not sim3:  # a scale to find: GT translations 1.3 x the predicted ones, 10 % noise
        extr[..., :3, 3] = 1.3 * enc[..., :3] * (1 + 0.1 * torch.randn(B, S, 3, generator=g))
    pred = {"pose_enc": enc, "depth": 0.5 + torch.rand(B, S, H, W, 1, generator=g),
            "world_points": torch.randn(B, S, H, W, 3, generator=g)}
    return pred, {"extrinsics": extr, "images": torch.zeros(B, S, 3, H, W)}


def _to_dev(d):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _chunked(pred, batch, cuts=((0, 4), (4, 7))):
    p = {k: [v[:, a:b].clone() for a, b in cuts] for k, v in pred.items()}
    return p, {"extrinsics": [batch["extrinsics"][:, a:b].clone() for a, b in cuts]}


def _run_type(kind, pred, batch):
    from aligned_vggt.utils import alignment as A
    if kind == "scale_from_poses":
        A.scale_alignment_from_poses(pred, batch)
    elif kind == "scale_from_fc_poses":
        A.scale_alignment_from_poses(pred, batch, 4)
    elif kind == "per_frame_scale_from_poses":
        A.per_frame_scale_alignment_from_poses(pred, batch)
    elif kind == "sim3_from_poses":
        A.umeyama_alignment_from_poses(pred, batch, 7)
    return pred


KINDS = ["scale_from_poses", "scale_from_fc_poses", "per_frame_scale_from_poses", "sim3_from_poses"]


@pytest.mark.parametrize("kind", KINDS + ["per_chunk_scale_from_poses"])
def test_alignment_types_on_device_agree_with_host(N, kind, monkeypatch):
    from aligned_vggt.utils import alignment as A
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    pred, batch = _step(sim3=kind == "sim3_from_poses")
    if kind == "per_chunk_scale_from_poses":
        ref, ref_b = _chunked(pred, batch)
        A.per_chunk_scale_alignment_from_poses(ref, ref_b)
        got, got_b = _chunked(pred, batch)
        got, got_b = {k: [t.to(DEV) for t in v] for k, v in got.items()}, {"extrinsics": [t.to(DEV) for t in got_b["extrinsics"]]}
        A.per_chunk_scale_alignment_from_poses(got, got_b)
        sc = got["alignment_scales_per_chunk"]
        assert len(sc) == 2 and all(s.is_cuda and s.shape == (2,) and s.dtype == torch.float32 for s in sc)
        for a, b in zip(sc, ref["alignment_scales_per_chunk"]):
            torch.testing.assert_close(a.cpu(), b.float(), rtol=2.0 ** -16, atol=0)
        for k in ("pose_enc", "depth", "world_points"):
            for a, b in zip(got[k], ref[k]):
                torch.testing.assert_close(a.cpu(), b, rtol=2.0 ** -16, atol=0)
        return
    ref = _run_type(kind, copy.deepcopy(pred), batch)
    got = _run_type(kind, _to_dev(copy.deepcopy(pred)), _to_dev(batch))
    assert all(got[k].is_cuda for k in ("pose_enc", "depth", "world_points"))
    if kind == "sim3_from_poses":
        assert "alignment_scales" not in got
        for k in ("pose_enc", "depth", "world_points"):
            torch.testing.assert_close(got[k].cpu(), ref[k], rtol=0, atol=2.0 ** -12 * float(ref[k].abs().max()))
        return
    sc = got["alignment_scales"]
    assert len(sc) == (7 if kind.startswith("per_frame") else 2)
    assert all(isinstance(s, torch.Tensor) and s.is_cuda and s.dim() == 0 for s in sc)
    torch.testing.assert_close(torch.stack(sc).cpu(), torch.tensor([float(v) for v in ref["alignment_scales"]]),
                               rtol=2.0 ** -16, atol=0)
    for k in ("pose_enc", "depth", "world_points"):
        torch.testing.assert_close(got[k].cpu(), ref[k], rtol=2.0 ** -16, atol=0)


def test_sim3_route_with_a_graph_matches_the_fused_route(N, monkeypatch):
    """A tensor that requires grad sends SIM3 through apply_sim3_alignment with the device transform;
    the values agree with the fused kernel route (two fp32 chains of the same transform, each within
    128 u M of the exact one with M <= 2 max|value|: 2^-14 of the largest magnitude)."""
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    pred, batch = _step(sim3=True)
    fused = _run_type("sim3_from_poses", _to_dev(copy.deepcopy(pred)), _to_dev(batch))
    p = _to_dev(copy.deepcopy(pred))
    leaf = p["pose_enc"].clone().requires_grad_(True)
    p["pose_enc"] = leaf * 1.0
    got = _run_type("sim3_from_poses", p, _to_dev(batch))
    assert got["pose_enc"].requires_grad
    got["pose_enc"][..., :3].sum().backward()
    assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all())
    for k in ("pose_enc", "depth", "world_points"):
        torch.testing.assert_close(got[k].detach(), fused[k], rtol=0, atol=2.0 ** -14 * float(fused[k].abs().max()))


@pytest.mark.parametrize("kind", KINDS[:3])
def test_knob_runs_the_host_chain_bitwise(N, kind, monkeypatch):
    """VGGT_GT_ALIGN=torch on device tensors: the scale comes from the host's numpy sums and one fp32
    multiply per element applies it, so the result has the bits of the same call on host copies."""
    pred, batch = _step()
    want = _run_type(kind, copy.deepcopy(pred), batch)
    monkeypatch.setenv("VGGT_GT_ALIGN", "torch")
    got = _run_type(kind, _to_dev(copy.deepcopy(pred)), _to_dev(batch))
    assert not isinstance(got["alignment_scales"][0], torch.Tensor)
    assert [float(a) for a in got["alignment_scales"]] == [float(b) for b in want["alignment_scales"]]
    for k in ("pose_enc", "depth", "world_points"):
        assert torch.equal(got[k].cpu(), want[k]), k


def test_knob_sends_per_chunk_and_sim3_to_the_host_code(N, monkeypatch):
    """The other two entry points read the knob too: under VGGT_GT_ALIGN=torch neither launches
    vggt_gt_pose_align, the per-chunk scales are the host code's CPU tensors with the bits of the
    same call on host copies, and SIM3 is the host chain on the device tensors."""
    from aligned_vggt.utils import alignment as A
    pred, batch = _step()
    want, want_b = _chunked(pred, batch)
    A.per_chunk_scale_alignment_from_poses(want, want_b)
    sim_pred, sim_batch = _step(sim3=True)
    sim_want = _run_type("sim3_from_poses", copy.deepcopy(sim_pred), sim_batch)

    def refuse(*a, **k):
        raise AssertionError("vggt_gt_pose_align launched under VGGT_GT_ALIGN=torch")
    monkeypatch.setenv("VGGT_GT_ALIGN", "torch")
    monkeypatch.setattr(N, "gt_pose_align", refuse)
    got, got_b = _chunked(pred, batch)
    got = {k: [t.to(DEV) for t in v] for k, v in got.items()}
    A.per_chunk_scale_alignment_from_poses(got, {"extrinsics": [t.to(DEV) for t in got_b["extrinsics"]]})
    for a, b in zip(got["alignment_scales_per_chunk"], want["alignment_scales_per_chunk"]):
        assert not a.is_cuda and torch.equal(a, b)
    for k in ("pose_enc", "depth", "world_points"):
        for a, b in zip(got[k], want[k]):
            assert a.is_cuda and torch.equal(a.cpu(), b), k
    sim_got = _run_type("sim3_from_poses", _to_dev(copy.deepcopy(sim_pred)), _to_dev(sim_batch))
    for k in ("pose_enc", "depth", "world_points"):  # the same fp32 chain, torch on the device against torch on the host
        assert sim_got[k].is_cuda
        torch.testing.assert_close(sim_got[k].cpu(), sim_want[k], rtol=0, atol=2.0 ** -14 * float(sim_want[k].abs().max()))


def test_pose_enc_with_a_graph_keeps_its_gradient(N, monkeypatch):
    from aligned_vggt.utils import alignment as A
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    pred, batch = _step()
    p = _to_dev(copy.deepcopy(pred))
    leaf = p["pose_enc"].clone().requires_grad_(True)
    p["pose_enc"] = leaf * 1.0
    A.scale_alignment_from_poses(p, _to_dev(batch))
    scale = torch.stack(p["alignment_scales"])
    assert not scale.requires_grad and p["pose_enc"].requires_grad
    g = torch.randn(p["pose_enc"].shape, generator=_gen(10)).to(DEV)
    (p["pose_enc"] * g).sum().backward()
    want = g.clone()
    want[..., :3] *= scale.view(-1, 1, 1)
    assert torch.equal(leaf.grad, want)  # d pose_enc[..., :3] = scale d out, the rest passes through


# ------------------------------------------------------------------------------------------------- no synchronisation
class _no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        self.before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.before)


def test_align_and_convert_outputs_does_not_synchronise(N, monkeypatch):
    from aligned_vggt.utils.data import alignAndConvertOutputs
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    pred, batch = _step()
    cuts = ((0, 4), (2, 6), (4, 7))  # chunk 4, overlap 2

    def run(dev, guard):
        p, cb = _chunked(pred, batch, cuts)
        p = {k: [t.to(dev) for t in v] for k, v in p.items()}
        cb = {k: [t.to(dev) for t in v] for k, v in cb.items()}
        merged = {}
        if guard:
            with _no_sync():
                alignAndConvertOutputs(p, merged, cb, "scale_from_poses", 4, 2)
        else:
            alignAndConvertOutputs(p, merged, cb, "scale_from_poses", 4, 2)
        return p, merged
    run(DEV, False)  # the library is loaded, the allocator is warm
    got, merged = run(DEV, True)
    ref, _ = run("cpu", False)
    assert got["pose_enc"].shape == (2, 7, 9) and merged["extrinsics"].shape == (2, 7, 3, 4)
    for k in ("pose_enc", "depth", "world_points"):
        torch.testing.assert_close(got[k].cpu(), ref[k], rtol=2.0 ** -16, atol=0)


def test_device_state_update_batch_does_not_synchronise(N):
    from aligned_vggt.eval import AbsoluteTrajectoryError, RelativePoseError, ScaleConsistency
    g = _gen(11)
    pred, gt = _c2w(3, 9, g), _c2w(3, 9, g)
    pd, gd = pred.to(DEV), gt.to(DEV)
    dev_m = [AbsoluteTrajectoryError(detailed=True).to(DEV), RelativePoseError(delta=2, detailed=True).to(gd),
             ScaleConsistency().to(DEV)]
    for m in dev_m:
        m.update_batch(pd, gd)  # warm
        m.reset()
        assert all(getattr(m, n).is_cuda for n in m._state)
    with _no_sync():
        for m in dev_m:
            m.update_batch(pd, gd)
            m.update(pd[0], gd[0])
    host_m = [AbsoluteTrajectoryError(detailed=True), RelativePoseError(delta=2, detailed=True), ScaleConsistency()]
    for m in host_m:
        m.update_batch(pred, gt)
        m.update(pred[0], gt[0])
    for a, b in zip(dev_m, host_m):
        ra, rb = a.compute(), b.compute()
        assert list(ra) == list(rb)
        for k in ra:  # the host chain is fp32 throughout: a loose agreement, the kernel is held to fp64 above
            np.testing.assert_allclose(np.asarray(torch.as_tensor(ra[k]).cpu(), dtype=np.float64),
                                       np.asarray(torch.as_tensor(rb[k]), dtype=np.float64), rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("rmse", [True, False], ids=["rmse", "mean"])
def test_chamfer_plot_writes_its_two_files(N, tmp_path, rmse):
    from aligned_vggt.eval import ChamferDistanceMetrics
    g = _gen(13)
    pred, gt = torch.randn(50, 3, generator=g).to(DEV), torch.randn(60, 3, generator=g).to(DEV)
    metric = ChamferDistanceMetrics(rmse=rmse).to(gt)
    prefix = str(tmp_path / "seq_")
    d, path = metric.plot(pred, gt, "title", prefix)
    metric.update(pred, gt)
    assert metric.pred_to_gt.is_cuda and metric.pred_to_gt.shape == (50,) and metric.gt_to_pred.shape == (60,)
    want = metric.compute()  # the same kernels on the same clouds
    assert list(d) == list(want) and path == prefix + "rec_chamfer_distribution.png"
    for k in d:
        assert isinstance(d[k], torch.Tensor if rmse else float) and float(d[k]) == float(want[k]) > 0.0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["seq_rec_chamfer_distribution.npy",
                                                          "seq_rec_chamfer_distribution.png"]
    assert (tmp_path / "seq_rec_chamfer_distribution.png").stat().st_size > 0
    data = np.load(prefix + "rec_chamfer_distribution.npy", allow_pickle=True).item()
    assert set(data) == {"dists_pred_to_gt", "dists_gt_to_pred", "chamfer", "acc", "comp"}
    assert data["dists_pred_to_gt"].shape == (50,) and data["dists_gt_to_pred"].shape == (60,)
    assert np.array_equal(data["dists_pred_to_gt"], metric.pred_to_gt.cpu().numpy())
    values = list(d.values())
    for k, v in zip(("chamfer", "acc", "comp"), values):
        assert isinstance(data[k], np.ndarray) and data[k].shape == () and float(data[k]) == float(v)
    metric.plot(pred, gt)  # no outpath: nothing more is written
    assert len(list(tmp_path.iterdir())) == 2


# ------------------------------------------------------------------------------------------------- end to end
H, W = 28, 42


class _StubModel(torch.nn.Module):
    """A device model with the chunk protocol: per frame, the translation is the image's pixel (0, 0),
    the quaternion comes from pixel (0, 1); depth and confidence from the image planes."""

    def forward(self, images, num_overlap, context=None, gt_poses=None):
        B, S = images.shape[:2]
        t = images[:, :, :, 0, 0]
        q = torch.cat([0.3 * images[:, :, :, 0, 1] - 0.15, torch.ones(B, S, 1, device=images.device)], -1)
        fov = torch.tensor([0.9, 1.2], device=images.device).expand(B, S, 2)
        out = {"pose_enc": torch.cat([t, q, fov], -1), "depth": (1.0 + images[:, :, 0])[..., None],
               "depth_conf": 1.0 + images[:, :, 1]}
        if context is None:
            return {k: [v] for k, v in out.items()}
        for k, v in out.items():
            context[k].append(v)
        return context


def _frames(S, seed, noise=0.0):
    """Per-frame uint8 images and GT with extrinsic translations exactly (noise = 0) twice what the stub
    predicts; frame 0 is the identity, so the first-camera normalisation changes no bit."""
    r = np.random.RandomState(seed)
    images = r.randint(0, 256, (S, H, W, 3)).astype(np.uint8)
    images[1:, 0, 0] = r.randint(64, 256, (S - 1, 3))  # translations away from the origin
    images[0, 0, 0] = 0
    t_pred = torch.from_numpy(images[:, 0, 0].astype(np.float32)).div(255)
    extr = torch.zeros(S, 3, 4)
    q = torch.randn(S, 4, generator=_gen(12, seed))
    q[0] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    extr[:, :, :3] = _rot64(q).float()
    extr[:, :, 3] = 2.0 * t_pred
    if noise:
        extr[1:, :, 3] += noise * torch.from_numpy(r.randn(S - 1, 3).astype(np.float32))
    world = torch.from_numpy(r.randn(S, H, W, 3).astype(np.float32)) + torch.tensor([0.0, 0.0, 3.0])
    return {"images": images, "extrinsics": extr.numpy(), "world_points": world.numpy(),
            "cam_points": world.numpy().copy(), "depths": (1.0 + r.rand(S, H, W)).astype(np.float32),
            "intrinsics": np.tile(np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], np.float32), (S, 1, 1)),
            "point_masks": r.rand(S, H, W) < 0.85}


class _Dataset:
    def __init__(self, S, seed, noise=0.0):
        self.data = _frames(S, seed, noise)
        self.seq_frame_num, self.sequence_list_len = [S], 1

    def get_seq_name(self, i):
        return "walk"

    def get_data(self, seq_index, img_per_seq, seq_name, ids):
        d = {k: [v[i] for i in ids] for k, v in self.data.items()}
        d["ids"] = np.asarray(ids)
        return d


def _batch(B, S, seed, noise=0.0):
    """A (B, S) batch as the datamodule hands it over, on the device."""
    from aligned_vggt.training.training_metrics import get_sequence_data
    seqs = [get_sequence_data(_Dataset(S, seed + b, noise), 0, "walk", S) for b in range(B)]
    out = {k: torch.cat([s[k] for s in seqs], 0).to(DEV) for k in seqs[0] if isinstance(seqs[0][k], torch.Tensor)}
    out["seq_name"] = ["walk"] * B
    return out


class _GroupedStub(_StubModel):
    """The same outputs through the encode_chunk / align_chunk split, which makes the driver encode
    consecutive equal-length chunks in one call."""

    def __init__(self):
        super().__init__()
        self.encoded = []  # batch sizes of the encode calls

    def encode_chunk(self, images):
        self.encoded.append(images.shape[0])
        return {k: v[0] for k, v in _StubModel.forward(self, images, 0).items()}

    def align_chunk(self, enc, num_overlap, context=None, gt_poses=None):
        if context is None:
            return {k: [v] for k, v in enc.items()}
        for k, v in enc.items():
            context[k].append(v)
        return context


@pytest.mark.parametrize("stub", [_StubModel, _GroupedStub], ids=["per_chunk", "grouped_encode"])
def test_driver_without_offload_is_bitwise_the_offloading_one(N, monkeypatch, stub):
    from aligned_vggt.dist import pipeline
    from aligned_vggt.training.training_metrics import apply_sequence_to_model
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    monkeypatch.delenv("VGGT_ENCODE_GROUP", raising=False)
    model = stub().to(DEV)
    res = {}
    for offload in (True, False):
        batch = _batch(2, 7, 30)
        if offload:  # the reference's route: GT on the host, where the merged outputs end up
            batch = {k: (v.cpu() if isinstance(v, torch.Tensor) and k != "images" else v) for k, v in batch.items()}
        res[offload] = apply_sequence_to_model(batch, model, [4], [2], "chunk_overlap", "scale_from_poses",
                                               offload=offload), batch
    (host, hb), (dev, db) = res[True], res[False]
    if stub is _GroupedStub:  # both drivers encoded chunks 0 and 1 (4 frames each) together, the tail alone
        assert model.encoded == [4, 2, 4, 2]
    # the default is the sequence driver itself, with its own signature
    got = pipeline.apply_sequence_to_model(_batch(2, 7, 30), stub().to(DEV), [4], [2], "chunk_overlap", "scale_from_poses")
    assert not got["depth"].is_cuda and torch.equal(got["depth"], host["depth"])
    assert dev["pose_enc"].is_cuda and dev["depth"].is_cuda and not host["depth"].is_cuda
    assert dev["pose_enc"].shape == (2, 7, 9) and dev["depth"].shape == (2, 7, H, W, 1)
    assert [float(s) for s in dev["alignment_scales"]] == [2.0, 2.0] == [float(s) for s in host["alignment_scales"]]
    for k in ("pose_enc", "depth", "depth_conf"):
        assert torch.equal(dev[k].cpu(), host[k].cpu()), k
    for k in ("extrinsics", "world_points", "point_masks", "depths"):
        assert torch.equal(db[k].cpu(), hb[k].cpu()), k


def _trainer(datasets):
    loader = SimpleNamespace(dataset=SimpleNamespace(base_dataset=SimpleNamespace(datasets=datasets)))
    return SimpleNamespace(logger=SimpleNamespace(log_dir=None), is_global_zero=True, test_dataloaders=loader,
                           val_dataloaders=None, strategy=SimpleNamespace(barrier=lambda name: None))


def _forward(route, datasets, batch, trajectory, reconstruction, cap):
    from aligned_vggt.training.training_metrics import Metrics
    m = Metrics(mode="test", overlap=[2], chunk_width=[4], gt_alignment_type="scale_from_poses",
                full_seq_sample_mode="chunk_overlap", use_random_sequences=False, max_points_for_icp_batch=cap,
                max_points_for_icp_full_seq=cap, trajectory_metrics=trajectory, reconstruction_metrics=reconstruction,
                sequence_outputs=route)
    model = _StubModel().to(DEV)
    with torch.no_grad():
        step = model(batch["images"], 2)
    step = {k: v[0] for k, v in step.items()}
    return m(step, dict(batch), model, _trainer(datasets))


TRAJ = [{"_target_": "eval.trajectory_metrics.AbsoluteTrajectoryError"},
        {"_target_": "eval.trajectory_metrics.RelativePoseError"},
        {"_target_": "eval.trajectory_metrics.ScaleConsistency"}]


def _f(v):
    return float(v) if not isinstance(v, (list, tuple)) else [float(x) for x in v]


def test_metrics_forward_device_route_equals_host_route(N, monkeypatch):
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    datasets = [_Dataset(7, 40)]
    batch = _batch(2, 4, 50)
    rec = [{"_target_": "eval.reconstruction_metrics.ChamferDistanceMetrics"}]
    cap = 2000  # 7 x 28 x 42 x 0.85 valid GT points: the subsample search runs
    out = {r: _forward(r, datasets, batch, TRAJ, rec, cap) for r in ("device", "host")}
    (bd, sd), (bh, sh) = out["device"], out["host"]
    want = {"ate_rmse", "rpe_trans_rmse", "rpe_rot_rmse", "scale_var", "chamfer_distance_rmse", "accuracy_rmse",
            "completion_rmse"}
    assert set(bd) == set(bh) == want
    assert set(sd) == set(sh) == {f"_Dataset_walk/{k}" for k in want | {"avg_alignment_scale"}}
    assert sd["_Dataset_walk/avg_alignment_scale"] == sh["_Dataset_walk/avg_alignment_scale"] == 2.0
    for k in sd:  # identical bits into the same kernels
        assert _f(sd[k]) == _f(sh[k]) and math.isfinite(_f(sd[k])), (k, sd[k], sh[k])
    for k in bd:  # the batch part does not depend on the route
        assert _f(bd[k]) == _f(bh[k]), k


def test_metrics_forward_noisy_gt_trajectory_values(N, monkeypatch):
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    datasets = [_Dataset(7, 41, noise=0.05)]
    batch = _batch(2, 4, 51, noise=0.05)
    out = {r: _forward(r, datasets, batch, TRAJ, None, None) for r in ("device", "host")}
    (_, sd), (_, sh) = out["device"], out["host"]
    assert set(sd) == set(sh) and len(sd) == 5
    ds = 2.0 ** -17
    pmax = 2.0 * 1.0 * 1.1  # translations are pixel values in [0, 1], scaled by ~2
    for k in sd:
        bound = 8 * ds * 1.5 if k.endswith("scale_var") else 4 * ds * pmax  # factors within 1 +- 0.2
        print(k, _f(sd[k]), _f(sh[k]), bound)
        assert abs(_f(sd[k]) - _f(sh[k])) <= bound, (k, sd[k], sh[k], bound)
