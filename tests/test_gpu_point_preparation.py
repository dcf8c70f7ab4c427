"""GPU checks of the point-cloud preparation before ICP (csrc/points.hip, eval/point_preparation.py):
vggt_kth_value_f32 against CPU torch.kthvalue, vggt_subsample_mask_count and the selection of
vggt_prepare_clouds against CPU F.interpolate (exact), the point values against an fp64 evaluation of the
documented formulas, and prepare_data_for_metrics end to end."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ k-th value
KTH_SIZES = [1, 2, 3, 255, 256, 257, 1023, 4099, 65537, 4_194_307]
NAN = float("nan")


def _ranks(n):
    from aligned_vggt.eval import quantile_rank
    return sorted({1, n, quantile_rank(n, 0.25), quantile_rank(n, 0.5)})


def _kth_inputs(pattern, n, k, g):
    """The arrays of one pattern for rank k (most patterns do not depend on k)."""
    if pattern == "all_equal":
        return [np.full(n, 1.25, np.float32)]
    if pattern == "two_values":  # the boundary between the two values at k - 1, k and k + 1
        out = []
        for m in sorted({min(max(k + d, 0), n) for d in (-2, -1, 0, 1)}):  # m smaller values: boundary after rank m
            x = np.full(n, 3.5, np.float32)
            x[:m] = -2.25
            out.append(g.permutation(x))
        return out
    if pattern == "last_bit":  # neighbours one mantissa bit apart
        return [(np.float32(1.5).view(np.int32) + g.integers(0, 4, n).astype(np.int32)).view(np.float32)]
    if pattern == "signs_zeros_denormals":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 3e-39, -3e-39, 1.17549435e-38, -1.17549435e-38,
                         1.0, -1.0, 2.5e-3, -7.0], np.float32)
        return [pool[g.integers(0, len(pool), n)]]
    if pattern == "infinities":
        x = g.standard_normal(n).astype(np.float32)
        x[g.random(n) < 0.2] = np.inf
        x[g.random(n) < 0.2] = -np.inf
        return [x]
    if pattern == "nans_last":
        x = g.standard_normal(n).astype(np.float32)
        x[g.integers(0, n, min(3, n - 1) if n > 1 else 0)] = NAN  # a few: the top ranks are NaN
        return [x]
    if pattern == "confidences":
        return [(1.0 + np.exp(g.standard_normal(n))).astype(np.float32)]
    raise AssertionError(pattern)


KTH_PATTERNS = ["all_equal", "two_values", "last_bit", "signs_zeros_denormals", "infinities", "nans_last",
                "confidences"]


@pytest.mark.parametrize("pattern", KTH_PATTERNS)
@pytest.mark.parametrize("n", KTH_SIZES)
def test_kth_value_matches_torch_kthvalue(N, n, pattern):
    g = np.random.default_rng(1000 + n + 7 * KTH_PATTERNS.index(pattern))
    for k in _ranks(n):
        for x in _kth_inputs(pattern, n, k, g):
            xc = torch.from_numpy(x)
            want = torch.kthvalue(xc, k).values.numpy()
            xg = xc.cuda()
            got = N.kth_value(xg, k).cpu().numpy()
            again = N.kth_value(xg, k).cpu().numpy()
            assert _bits(got) == _bits(again), (n, k, pattern)  # two runs, bitwise
            if np.isnan(want):
                assert np.isnan(got), (n, k, pattern, got)
            else:
                assert got == want, (n, k, pattern, got, want)  # equal as values (-0 == +0)
                if want != 0:
                    assert _bits(got) == _bits(want), (n, k, pattern, got, want)


def test_kth_value_lands_on_a_zero_before_a_nan_tail(N):
    """n = 257 (one workgroup plus one element): 100 negatives, 60 zeros of both signs, 57 positives, 40 NaN.  The
    ranks 101 .. 160 land on a zero whatever its sign (-0 == +0 in torch.kthvalue's order, here on the same device
    tensor), and the select returns it as +0; the ranks next to them and the NaN tail are torch's bit for bit."""
    g = np.random.default_rng(257)
    zeros = np.where(np.arange(60) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    x = np.concatenate([-1.0 - g.random(100), zeros, 1e-40 + g.random(57), np.full(40, NAN)]).astype(np.float32)
    xg = torch.from_numpy(g.permutation(x)).cuda()
    assert xg.numel() == 257
    for k in (100, 101, 130, 160, 161, 217, 218, 257):
        want = torch.kthvalue(xg, k).values.cpu().numpy()
        got = N.kth_value(xg, k).cpu().numpy()
        if k > 217:
            assert np.isnan(want) and np.isnan(got), (k, got, want)
        elif 101 <= k <= 160:
            assert want == 0 and _bits(got) == 0, (k, got, want)
        else:
            assert _bits(got) == _bits(want), (k, got, want)


def test_kth_value_rejects_bad_ranks_and_cpu(N):
    x = torch.arange(5, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        N.kth_value(x, 1)
    for k in (0, 6, -1):
        with pytest.raises(ValueError):
            N.kth_value(x.cuda(), k)


def test_quantile_is_torch_quantile_nearest(N):
    from aligned_vggt.eval import quantile, quantile_rank
    g = torch.Generator().manual_seed(5)
    conf = 1.0 + torch.exp(torch.randn(2, 3, 37, 70, generator=g))
    for q in (0.0, 0.25, 0.5, 1.0):
        want = torch.kthvalue(conf.reshape(-1), quantile_rank(conf.numel(), q)).values
        got = quantile(conf.cuda(), q)
        assert got.is_cuda and got.dim() == 0
        assert _bits(got.cpu().numpy()) == _bits(want.numpy())
    with pytest.raises(RuntimeError, match="HIP devices only"):
        quantile(conf, 0.25)


# ------------------------------------------------------------------ bilinear subsample, restated in numpy
def _axis(n_in, n_out):
    """The documented per-axis arithmetic in fp32.  The source coordinate is one fused multiply-add: the fp64
    product of the fp32 scale with dst + 0.5 and the subtraction of 0.5 are both exact (35 significant bits), so
    rounding the fp64 result to fp32 is that single rounding."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float64)
    src = (np.float64(scale) * (dst + 0.5) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def _bilinear(x, Ho, Wo, dtype=np.float32):
    """x: (..., H, W) -> (..., Ho, Wo) by the documented arithmetic, every product and sum rounded to `dtype`
    (float32: the kernel's own arithmetic; float64: the reference, on the same fp32 weights).  (H, W) -> (H, W) is
    a pass through."""
    H, W = x.shape[-2:]
    if (Ho, Wo) == (H, W):
        return x.astype(dtype)
    h0, h1, lh0, lh1 = _axis(H, Ho)
    w0, w1, lw0, lw1 = _axis(W, Wo)
    lh0, lh1 = lh0.astype(dtype)[:, None], lh1.astype(dtype)[:, None]
    lw0, lw1 = lw0.astype(dtype), lw1.astype(dtype)
    x = x.astype(dtype)
    a, b = x[..., h0[:, None], w0], x[..., h0[:, None], w1]
    c, d = x[..., h1[:, None], w0], x[..., h1[:, None], w1]
    with np.errstate(invalid="ignore"):
        return lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d)


SHAPES = [(2, 3, 11, 23), (2, 4, 37, 70), (2, 5, 154, 518)]
FACTORS = [1, 2, 3, 4, 5, 11]
MASK_KINDS = ["bernoulli", "blocks"]


@functools.lru_cache(maxsize=None)
def _mask(shape, kind):
    g = torch.Generator().manual_seed(17 + SHAPES.index(shape) + 100 * MASK_KINDS.index(kind))
    if kind == "bernoulli":
        return torch.rand(shape, generator=g) < 0.7
    B, S, H, W = shape  # 4 x 6 blocks switched on with probability 0.6, and a frame-wide hole
    blocks = torch.rand(B, S, (H + 3) // 4, (W + 5) // 6, generator=g) < 0.6
    m = blocks.repeat_interleave(4, 2).repeat_interleave(6, 3)[:, :, :H, :W].clone()
    m[:, S // 2] = False
    return m


@functools.lru_cache(maxsize=None)
def _conf(shape):
    g = torch.Generator().manual_seed(29 + SHAPES.index(shape))
    conf = 1.0 + torch.exp(torch.randn(shape, generator=g))
    conf[1] = 0.5 * torch.rand(shape[1:], generator=g)  # batch element 1: nothing above the threshold
    return conf


def _thr(shape):
    """The 0.25 quantile of batch element 0's confidences: above all of batch element 1's."""
    c = _conf(shape)[0].reshape(-1)
    return torch.kthvalue(c, round(0.25 * (c.numel() - 1)) + 1).values


@functools.lru_cache(maxsize=None)
def _oracle_masks(shape, kind, f):
    """(GT mask, predicted-and-GT mask) at factor f from CPU F.interpolate, (B, S, Ho, Wo) bool numpy; asserts
    the precondition that the numpy restatement of the documented arithmetic takes every decision the same way."""
    B, S, H, W = shape
    Ho, Wo = H // f, W // f
    gt_full = _mask(shape, kind)
    pm_full = _conf(shape) > _thr(shape)
    out = []
    for full in (gt_full, pm_full):
        if f == 1:
            out.append(full.numpy().copy())
            continue
        sub = F.interpolate(full.reshape(B * S, 1, H, W).float(), size=(Ho, Wo), mode="bilinear",
                            align_corners=False).reshape(B, S, Ho, Wo)
        want = (sub > 0.5).numpy()
        mine = _bilinear(full.numpy().astype(np.float32), Ho, Wo) > np.float32(0.5)
        assert int((mine != want).sum()) == 0, "the restated arithmetic disagrees with F.interpolate: pick another seed"
        out.append(want)
    return out[0], out[0] & out[1]


def _cases():
    return [(s, f) for s in SHAPES for f in FACTORS if s[2] // f >= 1 and s[3] // f >= 1]


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("shape,f", _cases())
def test_mask_count_is_exact(N, shape, f, kind):
    B, S, H, W = shape
    gt, _ = _oracle_masks(shape, kind, f)
    got = N.subsample_mask_count(_mask(shape, kind).cuda(), H // f, W // f)
    assert got.dtype == torch.int64 and got.is_cuda
    assert int(got) == int(gt.sum())


def test_even_factors_meet_exact_ties():
    """The strict > is tested: at even factors on even sizes the four weights are 1/4 each and two set taps give
    exactly 0.5, which must not count."""
    shape = SHAPES[2]
    B, S, H, W = shape
    sub = _bilinear(_mask(shape, "bernoulli").numpy().astype(np.float32), H // 2, W // 2)
    assert int((sub == np.float32(0.5)).sum()) > 1000


def _index_points(shape):
    """A point map whose x is the pixel's flat index in its batch element (exact in fp32), y the image, z the row."""
    B, S, H, W = shape
    assert S * H * W < 2 ** 24
    idx = torch.arange(S * H * W, dtype=torch.float32).reshape(1, S, H, W).expand(B, S, H, W)
    s = torch.arange(S, dtype=torch.float32).reshape(1, S, 1, 1).expand(B, S, H, W)
    r = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1).expand(B, S, H, W)
    return torch.stack([idx, s, r], -1).contiguous()


def _run_clouds(N, shape, f, kind, rows_per_workgroup, gt_points, point_map=None, depth=None, kinv=None, c2w=None):
    B, S, H, W = shape
    dev = "cuda"
    args = dict(depth=None if depth is None else depth.to(dev), kinv=None if kinv is None else kinv.to(dev),
                c2w=None if c2w is None else c2w.to(dev), point_map=None if point_map is None else point_map.to(dev),
                conf=_conf(shape).to(dev), thr=_thr(shape).to(dev), gt_points=gt_points.to(dev),
                gt_mask=_mask(shape, kind).to(dev), Ho=H // f, Wo=W // f, rows_per_workgroup=rows_per_workgroup)
    pred_len, gt_len, ws = N.prepare_clouds(**args, phase=N.PREPARE_COUNT)
    pl, gl = pred_len.cpu().numpy(), gt_len.cpu().numpy()
    pred = torch.full((B, int(pl.max()) + 1, 3), -7.0, device=dev)  # one guard row past the longest cloud
    gtc = torch.full((B, int(gl.max()) + 1, 3), -7.0, device=dev)
    N.prepare_clouds(**args, pred_cloud=pred, gt_cloud=gtc, pred_len=pred_len, gt_len=gt_len, ws=ws,
                     phase=N.PREPARE_SCATTER)
    return pred.cpu().numpy(), pl, gtc.cpu().numpy(), gl


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("shape,f", _cases())
def test_selection_lengths_and_order_are_exact(N, shape, f, kind):
    """Lengths exact against F.interpolate; every selected pixel exact and in row-major order, shown by a point map
    that carries the pixel's flat index; bitwise the same for rows_per_workgroup 0, 1 and 7 (7 does not divide a
    batch element's rows, so the last workgroup of every batch element is cut short)."""
    B, S, H, W = shape
    Ho, Wo = H // f, W // f
    gt_m, pred_m = _oracle_masks(shape, kind, f)
    pts = _index_points(shape)
    want = np.moveaxis(_bilinear(np.moveaxis(pts.numpy(), -1, 2), Ho, Wo), 2, -1)  # (B, S, Ho, Wo, 3), fp32 steps
    assert pred_m[1].sum() == 0 and pred_m[0].sum() > 0  # a batch element without predicted points, one with
    first = None
    for rpw in (0, 1, 7):
        pred, pl, gtc, gl = _run_clouds(N, shape, f, kind, rpw, gt_points=pts, point_map=pts)
        assert list(gl) == [int(gt_m[b].sum()) for b in range(B)]
        assert list(pl) == [int(pred_m[b].sum()) for b in range(B)]
        if first is None:
            first = (pred, gtc)
            for b in range(B):
                for cloud, n, m in ((gtc, gl[b], gt_m[b]), (pred, pl[b], pred_m[b])):
                    got = cloud[b, :n]
                    exp = want[b][m]  # boolean indexing: row-major (S, Ho, Wo)
                    # the kernel's products and sums are fp32 steps in this order, so the restatement is bitwise
                    assert np.array_equal(_bits(got), _bits(exp)), (b, f)
                    if f == 1:  # pass through: the flat indices themselves
                        assert np.array_equal(got[:, 0], np.flatnonzero(m.reshape(-1)).astype(np.float32))
                    assert np.all(np.diff(got[:, 0]) > 0)
                    assert np.all(cloud[b, n:] == -7.0)  # nothing written past the length
        else:
            assert np.array_equal(_bits(pred), _bits(first[0])) and np.array_equal(_bits(gtc), _bits(first[1]))


# ------------------------------------------------------------------ point values against fp64
def _cameras(B, S, H, W, seed):
    """Cameras hundreds of metres from the origin looking along random directions; depths 1-80 m."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(B, S, 3, 3)
    t = (torch.rand(B, S, 3, generator=g) - 0.5) * 1200.0
    c2w = torch.cat([R, t[..., None]], -1).contiguous()
    K = torch.zeros(B, S, 3, 3)
    K[..., 0, 0] = 0.9 * W + 20 * torch.rand(B, S, generator=g)
    K[..., 1, 1] = 0.9 * W + 20 * torch.rand(B, S, generator=g)
    K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = W / 2, H / 2, 1.0
    K[..., 0, 1] = 0.01  # a little skew: no entry of the inverse's first two rows is trivially zero
    depth = 1.0 + 79.0 * torch.rand(B, S, H, W, generator=g)
    return depth, torch.inverse(K).contiguous(), c2w


def _unproject64(depth, kinv, c2w):
    """Per pixel, in fp64 on the fp32 inputs: world = R (Kinv (u, v, 1) * d) + t and the sum of the absolute
    values of every term that enters each coordinate."""
    B, S, H, W = depth.shape
    d, K, M = depth.numpy().astype(np.float64), kinv.numpy().astype(np.float64), c2w.numpy().astype(np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack([u, v, np.ones_like(u)], -1)  # (H, W, 3)
    ray = np.einsum("bsjk,hwk->bshwj", K, pix)
    aray = np.einsum("bsjk,hwk->bshwj", np.abs(K), np.abs(pix))
    cam, acam = ray * d[..., None], aray * np.abs(d)[..., None]
    R, t = M[..., :3], M[..., 3]
    world = np.einsum("bsij,bshwj->bshwi", R, cam) + t[:, :, None, None, :]
    aworld = np.einsum("bsij,bshwj->bshwi", np.abs(R), acam) + np.abs(t)[:, :, None, None, :]
    return world, aworld


@pytest.mark.parametrize("source", ["depth", "point_map"])
@pytest.mark.parametrize("shape,f", [(SHAPES[0], 1), (SHAPES[0], 2), (SHAPES[1], 3), (SHAPES[1], 4), (SHAPES[1], 1),
                                     (SHAPES[2], 5), (SHAPES[2], 11)])
def test_point_values_against_fp64(N, shape, f, source):
    """Every coordinate of both clouds within c * u * sum |w_i| |term_i| of the fp64 value of the same formulas on
    the same fp32 inputs and fp32 weights, u = 2^-24.  c counts the roundings on the longest path from an input to
    the coordinate: the bilinear combination l0h * (l0w * a + l1w * b) + l1h * (...) is product, sum, product, sum
    = 4; an unprojected tap adds the 3-term dot Kinv (u, v, 1) (product, sum, sum = 3), the scale by the depth (1),
    the 3-term dot with R (3) and the sum with t (1) = 8.  A pass through (f = 1) has no bilinear roundings."""
    B, S, H, W = shape
    Ho, Wo = H // f, W // f
    kind = "bernoulli"
    gt_m, pred_m = _oracle_masks(shape, kind, f)
    depth, kinv, c2w = _cameras(B, S, H, W, seed=41 + f)
    world, aworld = _unproject64(depth, kinv, c2w)
    g = torch.Generator().manual_seed(43)
    gt_points = (torch.from_numpy(world).float() + 0.05 * torch.randn(B, S, H, W, 3, generator=g)).contiguous()
    if source == "depth":
        pred, pl, gtc, gl = _run_clouds(N, shape, f, kind, 0, gt_points, depth=depth, kinv=kinv, c2w=c2w)
        p_val, p_abs, c_pred = world, aworld, 8
    else:
        pmap = torch.from_numpy(world).float().contiguous()
        pred, pl, gtc, gl = _run_clouds(N, shape, f, kind, 0, gt_points, point_map=pmap)
        p_val = pmap.numpy().astype(np.float64)
        p_abs, c_pred = np.abs(p_val), 0
    g_val = gt_points.numpy().astype(np.float64)
    c_bil = 0 if f == 1 else 4

    def sub(x):  # (B, S, H, W, 3) fp64 -> (B, S, Ho, Wo, 3) fp64 with the fp32 weights
        return np.moveaxis(_bilinear(np.moveaxis(x, -1, 2), Ho, Wo, np.float64), 2, -1)

    worst = {}
    for name, cloud, lens, mask, val, mag, c in (("gt", gtc, gl, gt_m, g_val, np.abs(g_val), c_bil),
                                                 ("pred", pred, pl, pred_m, p_val, p_abs, c_bil + c_pred)):
        want, bar = sub(val), c * U * sub(mag)  # the weights are >= 0: sub(|.|) is sum |w_i| |term_i|
        for b in range(B):
            assert lens[b] == mask[b].sum()
            got = cloud[b, :lens[b]].astype(np.float64)
            assert np.all(np.isfinite(got))
            err = np.abs(got - want[b][mask[b]])
            lim = bar[b][mask[b]]
            if c == 0:
                assert np.all(err == 0), name
                continue
            ratio = float((err / lim).max()) if err.size else 0.0
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert np.all(err <= lim), (name, b, ratio)
    print(f"point values {source} {shape} f={f}: worst error / bar = "
          f"{', '.join(f'{k} {v:.3f}' for k, v in worst.items()) or 'exact'} (c = {c_bil} bilinear + {c_pred} tap)")


def test_pass_through_keeps_non_finite_neighbours_out(N):
    """Ho == H, Wo == W: no interpolation arithmetic, so a NaN or inf next to a selected pixel cannot enter through a
    zero weight (the reference's unsubsampled branch)."""
    shape = SHAPES[0]
    B, S, H, W = shape
    m = _mask(shape, "bernoulli")
    pts = _index_points(shape).clone()
    pts[~m] = NAN
    pts[:, :, 0, 0][~m[:, :, 0, 0]] = float("inf")
    pred, pl, gtc, gl = _run_clouds(N, shape, 1, "bernoulli", 0, gt_points=pts, point_map=pts)
    for b in range(B):
        assert np.all(np.isfinite(gtc[b, :gl[b]])) and np.all(np.isfinite(pred[b, :pl[b]]))


def test_single_call_equals_two_phases_and_caps_drop_rows(N):
    """VGGT_PREPARE_ALL with caps known in advance writes what COUNT then SCATTER write; with caps below the
    lengths the lengths stay the full counts, the first cap rows are the same and nothing is written past a cap."""
    shape, f = SHAPES[1], 3
    B, S, H, W = shape
    pts = _index_points(shape)
    pred, pl, gtc, gl = _run_clouds(N, shape, f, "bernoulli", 0, gt_points=pts, point_map=pts)
    dev = "cuda"
    args = dict(depth=None, kinv=None, c2w=None, point_map=pts.to(dev), conf=_conf(shape).to(dev),
                thr=_thr(shape).to(dev), gt_points=pts.to(dev), gt_mask=_mask(shape, "bernoulli").to(dev), Ho=H // f,
                Wo=W // f)
    for cap_p, cap_g in ((pred.shape[1], gtc.shape[1]), (int(pl.max()) // 2, int(gl.min()) // 3)):
        # one guard row past each cap, in the next batch element's first row or past the end of the allocation
        p1 = torch.full((B * cap_p + 1, 3), -7.0, device=dev)
        g1 = torch.full((B * cap_g + 1, 3), -7.0, device=dev)
        pl1, gl1, _ = N.prepare_clouds(**args, pred_cloud=p1[:B * cap_p].view(B, cap_p, 3),
                                       gt_cloud=g1[:B * cap_g].view(B, cap_g, 3), phase=N.PREPARE_ALL)
        assert np.array_equal(pl1.cpu().numpy(), pl) and np.array_equal(gl1.cpu().numpy(), gl)
        p1, g1 = p1.cpu().numpy(), g1.cpu().numpy()
        assert np.all(p1[-1] == -7.0) and np.all(g1[-1] == -7.0)
        for b in range(B):
            for one, two, cap, n in ((p1, pred, cap_p, pl[b]), (g1, gtc, cap_g, gl[b])):
                rows = one[b * cap:(b + 1) * cap]
                k = min(cap, n)
                assert np.array_equal(_bits(rows[:k]), _bits(two[b, :k]))
                assert np.all(rows[k:] == -7.0)


def test_prepare_clouds_rejects_cpu_tensors(N):
    shape = SHAPES[0]
    pts = _index_points(shape)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        N.prepare_clouds(None, None, None, pts, _conf(shape), _thr(shape), pts, _mask(shape, "bernoulli"), 11, 23)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        N.subsample_mask_count(_mask(shape, "bernoulli"), 11, 23)
    for Ho, Wo in ((12, 23), (11, 24), (0, 23)):  # an output grid larger than the input, or empty: VGGT_ERR_SHAPE
        with pytest.raises(RuntimeError, match="shape"):
            N.subsample_mask_count(_mask(shape, "bernoulli").cuda(), Ho, Wo)


# ------------------------------------------------------------------ prepare_data_for_metrics
def _scene(seed=3, B=2, S=4, H=37, W=70):
    from aligned_vggt.utils.geometry import unproject_depth_map_to_point_map
    from aligned_vggt.utils.pose_enc import extri_intri_to_pose_encoding
    g = torch.Generator().manual_seed(seed)
    ang = 0.1 * torch.randn(B, S, generator=g)
    R = torch.zeros(B, S, 3, 3)
    R[..., 0, 0], R[..., 0, 2], R[..., 2, 0], R[..., 2, 2], R[..., 1, 1] = ang.cos(), ang.sin(), -ang.sin(), ang.cos(), 1
    extr = torch.cat([R, 0.3 * torch.randn(B, S, 3, 1, generator=g)], -1)
    intr = torch.zeros(B, S, 3, 3)
    intr[..., 0, 0] = intr[..., 1, 1] = 60.0
    intr[..., 0, 2], intr[..., 1, 2], intr[..., 2, 2] = W / 2, H / 2, 1.0
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gt_depth = (4.0 + torch.sin(xx / 9.0) + torch.cos(yy / 5.0)).expand(B, S, H, W) + 0.1 * torch.rand(B, S, H, W, generator=g)
    gt = {"extrinsics": extr, "intrinsics": intr, "images": torch.zeros(B, S, 3, H, W),
          "world_points": unproject_depth_map_to_point_map(gt_depth[..., None], extr, intr).contiguous(),
          "point_masks": torch.rand(B, S, H, W, generator=g) < 0.8}
    pose_enc = extri_intri_to_pose_encoding(extr, intr, (H, W))
    pose_enc[..., :3] += 0.02 * torch.randn(B, S, 3, generator=g)
    pred = {"pose_enc": pose_enc, "depth": (gt_depth * (1 + 0.02 * torch.randn(B, S, H, W, generator=g)))[..., None],
            "depth_conf": 1.0 + torch.exp(torch.randn(B, S, H, W, generator=g))}
    return pred, gt


def test_prepare_data_for_metrics(N, monkeypatch):
    from aligned_vggt.eval import (iterative_closest_point, masked_clouds, point_preparation,
                                   poses_c2w_from_predictions, prepare_data_for_metrics)
    from aligned_vggt.utils.pose_enc import pose_encoding_to_extri_intri
    pred_cpu, gt_cpu = _scene()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        prepare_data_for_metrics(pred_cpu, gt_cpu, max_points_icp=1500)
    pred = {k: v.cuda() for k, v in pred_cpu.items()}
    gt = {k: v.cuda() for k, v in gt_cpu.items()}
    B, S, H, W = gt["point_masks"].shape
    assert int(gt["point_masks"].sum()) > 1500  # the factor search runs

    seen = {}

    def spy(X, Y, **kw):
        seen.update(X=X.clone(), Y=Y.clone(), kw=kw)
        return iterative_closest_point(X, Y, **kw)
    monkeypatch.setattr(point_preparation, "iterative_closest_point", spy)
    pred_poses, gt_poses, pred_points, gt_points = prepare_data_for_metrics(pred, gt, max_points_icp=1500)

    # the clouds entering ICP are masked_clouds', bitwise
    extr, intr = pose_encoding_to_extri_intri(pred["pose_enc"].float(), image_size_hw=(H, W))
    pc, pl, gc, gl, factor = masked_clouds(pred, gt, extr, intr, 0.25, 1500)
    assert factor >= 2 and int(gl.sum()) <= 1500
    assert torch.equal(seen["X"].view(torch.int32), pc.view(torch.int32))
    assert torch.equal(seen["Y"].view(torch.int32), gc.view(torch.int32))
    assert seen["kw"]["max_iterations"] == 30
    assert torch.equal(seen["kw"]["X_lengths"], pl) and torch.equal(seen["kw"]["Y_lengths"], gl)
    # the lists are iterative_closest_point's on those clouds, bitwise
    sol = iterative_closest_point(pc, gc, max_iterations=30, X_lengths=pl, Y_lengths=gl)
    assert len(pred_points) == len(gt_points) == B
    for b in range(B):
        assert pred_points[b].shape == (int(pl[b]), 3) and gt_points[b].shape == (int(gl[b]), 3)
        assert torch.equal(pred_points[b].view(torch.int32), sol.Xt[b, :int(pl[b])].contiguous().view(torch.int32))
        assert torch.equal(gt_points[b].view(torch.int32), gc[b, :int(gl[b])].contiguous().view(torch.int32))
        assert bool(torch.isfinite(pred_points[b]).all()) and bool(torch.isfinite(gt_points[b]).all())
        assert int(pl[b]) > 0
    # the pose pair
    want_pred, want_gt = poses_c2w_from_predictions(pred["pose_enc"], gt["extrinsics"], (H, W))
    assert torch.equal(pred_poses, want_pred) and torch.equal(gt_poses, want_gt)
    assert bool(torch.isfinite(pred_poses).all()) and bool(torch.isfinite(gt_poses).all())
    # halves switched off; the 7-wide encoding takes the GT intrinsics
    assert prepare_data_for_metrics(pred, gt, max_points_icp=1500, points=False)[2:] == (None, None)
    pred7 = dict(pred, pose_enc=pred["pose_enc"][..., :7].contiguous())
    p7, g7, pts7, gts7 = prepare_data_for_metrics(pred7, gt, max_points_icp=1500, poses=False)
    assert p7 is None and g7 is None and len(pts7) == B and all(bool(torch.isfinite(p).all()) for p in pts7)
