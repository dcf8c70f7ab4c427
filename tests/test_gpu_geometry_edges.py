"""csrc/align.hip (vggt_irls_sim3, vggt_sim3_points, vggt_scale_f32) and csrc/pose.hip
(vggt_pose_compose) at their degenerate inputs, decision boundaries, grid caps and strides, per
element against fp64 (the style of test_gpu_norm_edges.py; the shared helpers live in edge_rules.py).

Inputs come from a seeded host generator; every reference is fp64, computed from the fp32 values
actually passed.  The entry points are called through the C ABI, so strides, misaligned bases,
NULL operands and error codes are the test's to choose.  Strided operands sit in `Blocks`: inputs
NaN between the batch elements, outputs a sentinel that must be intact bit for bit afterwards.
`_reach_*` restate the host dispatch and are printed with the figures.  u = 2^-24.

Entry point, paths reached, rule:
  vggt_irls_sim3, one weighted solve (max_iters = 0, conf_dst NULL, factor <= 0: the weights are
        the fp32 numbers passed).  Reference: the weighted Umeyama closed form in fp64 with LAPACK's
        SVD.  The kernel reduces in fp64, solves in fp64 and rounds each output once, so an output
        is the fp32 rounding of a number that differs from the reference by fp64 rounding times the
        conditioning of the solve, far below u for every cloud here.  Bound per element: one fp32
        ulp at the magnitude of the row, 2 u for R (|R_ij| <= 1), 2 u |t|_inf for t, 2 u s for s;
        t = mu_y - s R mu_x cancels, and an fp64 error e in s R shows as e |mu_x| in t, which
        2 u |t|_inf does not cover when t is small (the identity map has t = 0): t gets the
        conditioning term u |s (R mu_x)_i| on top.  Clouds: generic, mirrored (d = -1; det R = +1
        and s = (sv0 + sv1 - sv2) / var_x asserted), coplanar, the cube (Sg^T Sg = s^2 I exactly:
        Jacobi exits with V = I), identity, offset by (1e4, -2e4, 3e4), anisotropic with the
        covariance's singular values at 1 : 1e-3 : 1e-6 (extents 1 : 0.03 : 1e-3; the solve
        diagonalises Sg^T Sg, so its R follows an fp64 SVD only to 2^-53 (sv0 / sv1)^2, and a needle
        with EXTENTS 1 : 1e-3 : 1e-6 is 1.5e-5 off in a host restatement: the header states that
        limit), three points; n = 3, 255, 256, 257, 65 537 (second trip of the 256 x 256 pass grid).
        Rank 1 (37 collinear points, two points): the rotation about the line is free, so
        properties are asserted.  R is the fp32 rounding (|dR_ij| <= u) of an orthogonal matrix:
        |R R^T - I|_ij <= u (|R_i|_1 + |R_j|_1) + u^2 <= 2 sqrt(3) u < 4 u, |det R - 1| <=
        u sum |cofactor| = u sum |R_ij| <= 3 sqrt(3) u < 6 u.  R v0 = u0 for the top singular pair
        of the fp64 covariance: |dR v0|_i <= u |v0|_1 <= sqrt(3) u < 2 u.  s against fp64, 2 u s.
        The weighted RMS residual of the least-squares solution is at most that of the exact map,
        whose residual is the data's rounding: rho = sqrt(3) u (s max|x| + max|y|); the outputs'
        own rounding adds, per point, u s |x|_1 (R) + 2 u s |R x|_inf (s) + the bound of t.
        One point (var_x = 0): all outputs NaN, as for a total weight below 1e-6.
        Batch: B = 4, strides above 3 n / n with NaN gaps, outputs between guards; a generic, a
        mirrored, a weightless (NaN outputs) and one with NaN / inf coordinates at weight 0; every
        element bitwise its own B = 1 run; a second call on the dirty workspace bitwise the first.
  vggt_irls_sim3, the threshold (factor 0.5, max_iters = 0).  Borderline points carry a dst 50
        units off, so one wrong keep / drop moves t by 50 w_i / W, orders above the bound.
        Reference: the fp64 solve on the reference's mask, comb >= fl(0.5 median) with
        torch.median's lower middle; comb is exact in fp32 (raw values, or cs = cd multiples of
        1/4 whose product and root are exact).  Bound: that of the single solve.
  vggt_irls_sim3, iterations.  The fp64 restatement decides how many re-weightings each (tol,
        max_iters) must run; the test first asserts from it alone that the iterates to be told
        apart differ by >= 1e-3 in t and that no delta lies within 1.5 x of the tol used.  Rule:
        per output, the kernel's worst element within 2 x the fp32 CPU oracle's worst element
        (both against fp64) plus one fp32 ulp of the output's magnitude (the kernel's one rounding).
  vggt_sim3_points   fl(s p) is one rounding; then three products and three sums, contracted or
        not: |got - ref| <= gamma_4 (sum_j |r_ij| |fl(s p_j)| + |t_i|) with ref in fp64 from
        fl(s p).  n = 1, 255, 257, 524 291 (second trip of the 2048-block cap); scale NULL;
        strides with sentinels; in place bitwise out of place.
  vggt_scale_f32     bit for bit (one IEEE multiply on the vector and on the scalar path).
  vggt_pose_compose  reference: compose_poses restated in fp64; model: compose_poses itself in
        fp32 on the CPU; _model_rule per frame for translation, quaternion, FoV and the point
        transform.  The first run of this file measured the FoV columns at up to 4.5 x the model
        (tanf, atanf and two divisions on the device against a correctly rounded host libm; a
        frame whose model error is 0 fails at any kernel error); the kernel now takes the FoV round
        trip in fp64 and rounds once.  S = 1, 64, 65, 130 (second and third trip of the 64-lane frame loop), every
        mat_to_quat branch, the w < 0 flip, the 4-way tie and the three 180-degree rotations
        (exact inputs), Markley means of 2 / 7 / 64 transforms within 2 degrees of a generic mean
        and of one 0.2 degrees from 180 degrees (quaternions of both signs), eigen-gap >= 0.9.
  error returns      host side, nothing launched, outputs keep their sentinels.
DESIGN.md (Geometry edge tests) tabulates what was measured."""
import ctypes
import math

import pytest
import torch

from edge_rules import (ERR_ALIGN, ERR_SHAPE, F32, F64, NAN, OK, SENT, U, _bits, _done, _eq_bits, _fig, _figures, _gam,
                        _gen, _model_rule, _svd_centres, _svd_pair_check, _within)

pytestmark = pytest.mark.gpu

from oracle import alignment_oracle as AO  # noqa: E402
from oracle import vggt_oracle as O  # noqa: E402

DEV = "cuda"
INF = float("inf")


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    torch.cuda.synchronize()


class Blocks:
    """B blocks of fp32 at a batch stride `bs` inside a buffer filled with `fill`, `guard` elements
    before the first and after the last, `off` more elements before the first (a misaligned base)."""

    def __init__(self, blocks, bs=None, fill=NAN, guard=64, off=0):
        self.B, self.per = len(blocks), blocks[0].numel()
        self.bs = self.per if bs is None else bs
        self.base = guard + off
        self.host = torch.full((self.base + (self.B - 1) * self.bs + self.per + guard,), fill, dtype=F32)
        for b, x in enumerate(blocks):
            self.host[self.base + b * self.bs:self.base + b * self.bs + self.per] = x.reshape(-1).to(F32)
        self.dev = self.host.to(DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + 4 * self.base)

    def get(self):
        h = self.dev.cpu()
        return [h[self.base + b * self.bs:self.base + b * self.bs + self.per].clone() for b in range(self.B)]

    def intact(self):
        a, b = _bits(self.dev.cpu()).clone(), _bits(self.host).clone()
        for k in range(self.B):
            a[self.base + k * self.bs:self.base + k * self.bs + self.per] = 0
            b[self.base + k * self.bs:self.base + k * self.bs + self.per] = 0
        return torch.equal(a, b)


def _out(B, per, bs=None):
    return Blocks([torch.full((per,), SENT)] * B, bs, fill=SENT)


def _ws(N, B, fill=0xA5):
    nb = int(N.lib().vggt_irls_workspace_bytes(B))
    return torch.full(((nb + 15) // 16 * 16 + 16,), fill, dtype=torch.uint8, device=DEV), nb


def _irls(N, errs, tag, src, dst, cs, cd=None, factor=0.0, delta=0.1, iters=0, tol=0.0, gap=False, ws=None):
    """vggt_irls_sim3 on lists of B host clouds -> R [B,3,3], t [B,3], s [B] on the host."""
    B, n = len(src), src[0].shape[0]
    g = (5, 7, 3, 2) if gap else (0, 0, 0, 0)
    S_, D_ = Blocks(src, 3 * n + g[0]), Blocks(dst, 3 * n + g[1])
    C_ = Blocks(cs, n + g[2])
    Cd = Blocks(cd, n + g[3]) if cd is not None else None
    Ro, to, so = _out(B, 9), _out(B, 3), _out(B, 1)
    if ws is None:
        ws = _ws(N, B)
    rc = N.lib().vggt_irls_sim3(S_.ptr, S_.bs, D_.ptr, D_.bs, C_.ptr, C_.bs, Cd.ptr if Cd else None, Cd.bs if Cd else 0,
                                B, n, float(factor), float(delta), int(iters), float(tol), Ro.ptr, to.ptr, so.ptr,
                                ctypes.c_void_p(ws[0].data_ptr()), ws[1], _stream())
    _sync()
    if rc != OK:
        errs.append(f"{tag}: vggt_irls_sim3 returned {rc}")
    if not (Ro.intact() and to.intact() and so.intact()):
        errs.append(f"{tag}: guard around R / t / s overwritten")
    return torch.stack(Ro.get()).view(B, 3, 3), torch.stack(to.get()), torch.stack(so.get()).view(B)


# ------------------------------------------------------------------ the dispatch, restated
def _reach_pass(n):
    return {"n": n, "threads": 256 * 256, "trips": -(-n // (256 * 256))}


def _reach_hist(n):
    blocks = min(-(-n // 256), 1024)
    return {"n": n, "hist_blocks": blocks, "trips": -(-n // (blocks * 256))}


def _reach_points(n):
    blocks = min(-(-n // 256), 2048)
    return {"n": n, "blocks": blocks, "trips": -(-n // (blocks * 256))}


def _reach_scale(n, bs, ptr):
    blocks = min((n // 4 + 255) // 256 + 1, 2048)
    vec = bs % 4 == 0 and ptr % 16 == 0
    n4 = n // 4 if vec else 0
    return {"n": n, "path": "vector" if vec else "scalar", "blocks": blocks, "vector_trips": -(-n4 // (blocks * 256)),
            "tail": n - 4 * n4}


# ------------------------------------------------------------------ fp64 references
def _rot(g):
    """A rotation uniform over SO(3), fp64."""
    q = torch.randn(4, generator=g, dtype=F64)
    return O.quat_to_mat(q / q.norm())


def _um64(src, dst, w):
    """weighted_umeyama_sim3 in fp64 on fp32 inputs, with the pieces the bounds need."""
    x, y, w = src.double(), dst.double(), w.double()
    W = w.sum()
    mux, muy = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    xc, yc = x - mux, y - muy
    Sg = (w[:, None] * yc).T @ xc / W
    Uu, sv, Vh = torch.linalg.svd(Sg)
    d = 1.0 if float(torch.det(Uu @ Vh)) > 0 else -1.0
    D = torch.diag(torch.tensor([1.0, 1.0, d], dtype=F64))
    R = Uu @ D @ Vh
    varx = (w * (xc ** 2).sum(1)).sum() / W
    s = (sv[0] + sv[1] + d * sv[2]) / varx
    return {"R": R, "t": muy - s * (R @ mux), "s": s, "mux": mux, "U": Uu, "V": Vh.T, "sv": sv, "d": d, "Sg": Sg,
            "varx": varx}


def _solve_bounds(r):
    bR = torch.full((3, 3), 2 * U, dtype=F64)
    bt = 2 * U * r["t"].abs().max() + U * (r["s"] * (r["R"] @ r["mux"])).abs()
    bs = (2 * U * r["s"].abs()).reshape(1)
    return bR, bt, bs


def _solve_check(errs, tag, got, r, ftag):
    """One batch element of a single solve against the fp64 reference `r`; returns the worst ratio."""
    R, t, s = got
    bR, bt, bs = _solve_bounds(r)
    w = max(_within(errs, f"{tag} R", R, r["R"], bR), _within(errs, f"{tag} t", t, r["t"], bt),
            _within(errs, f"{tag} s", s.reshape(1), r["s"].reshape(1), bs))
    print(f"solve {tag}: worst error / bound {w:.3f}")
    _fig(("solve", ftag), w)
    return w


def _proper(errs, tag, R, ftag):
    """R (fp32) is the rounding of a proper rotation: |R R^T - I| <= 4 u, |det R - 1| <= 6 u."""
    R = R.double()
    o = float((R @ R.T - torch.eye(3, dtype=F64)).abs().max())
    d = abs(float(torch.det(R)) - 1.0)
    print(f"rotation {tag}: |R R^T - I| {o:.3e} ({o / (4 * U):.2f} of 4 u)  "
          f"|det R - 1| {d:.3e} ({d / (6 * U):.2f} of 6 u)")
    _fig(("orth", ftag), max(o / (4 * U), d / (6 * U)) if math.isfinite(o) and math.isfinite(d) else math.inf)
    if not (o <= 4 * U and d <= 6 * U):
        errs.append(f"{tag}: not a rotation: |R R^T - I| = {o:.3e}, det R = {float(torch.det(R)):.6f}")


def _all_nan(errs, tag, got):
    for name, v in zip("Rts", got):
        if not bool(torch.isnan(v).all()):
            errs.append(f"{tag}: {name} is not all NaN: {v.reshape(-1).tolist()}")


# ================================================================== 1. one weighted solve
def _cloud(g, n, kind):
    """src, dst [n, 3] and weights [n] fp32: dst = s R0 src + t0 (+ noise), built in fp64."""
    scale = 0.7 if kind in ("mirror", "coplanar", "offset") else 1.3
    R0, t0 = _rot(g), torch.tensor([0.5, -1.0, 2.0], dtype=F64)
    src = torch.randn(n, 3, generator=g, dtype=F64) * 2 + torch.tensor([0.3, -0.2, 6.0], dtype=F64)
    noise = 0.01
    if kind in ("coplanar", "coplanar_noise"):
        src[:, 2] = 0.0
        noise = 0.01 if kind == "coplanar_noise" else 0.0
    elif kind == "offset":
        src = src + torch.tensor([1e4, -2e4, 3e4], dtype=F64)
    elif kind == "aniso":
        ext = torch.tensor([1.0, 1e-3, 1e-6], dtype=F64).sqrt()  # the covariance's singular values are 1 : 1e-3 : 1e-6
        src = (torch.randn(n, 3, generator=g, dtype=F64) * ext) @ _rot(g).T
        noise = 0.0
    elif kind == "line":
        d = torch.tensor([0.48, -0.6, 0.64], dtype=F64)
        src = torch.tensor([0.3, -0.2, 6.0], dtype=F64) + torch.randn(n, 1, generator=g, dtype=F64) * 2 * d
        noise = 0.0
    src = src.float().double()  # the fp32 cloud; dst is the exact map of it, rounded
    base = src * torch.tensor([-1.0, 1.0, 1.0], dtype=F64) if kind == "mirror" else src
    dst = scale * base @ R0.T + t0 + noise * torch.randn(n, 3, generator=g, dtype=F64)
    if kind == "identity":
        dst = src.clone()
    w = 0.1 + torch.rand(n, generator=g)
    return src.float(), dst.float(), w.float()


def _cube():
    """The 8 vertices, equal weights, dst = 1.25 R src + t with R the 3-4-5 rotation about z: every
    number is exact in fp32, Sg = 1.25 R and Sg^T Sg = 1.5625 I exactly."""
    src = torch.tensor([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    sR = torch.tensor([[0.75, -1.0, 0.0], [1.0, 0.75, 0.0], [0.0, 0.0, 1.25]])
    return src, src @ sR.T + torch.tensor([0.5, -1.0, 2.0]), torch.ones(8)


SOLVE_CASES = [("generic", 37), ("mirror", 37), ("coplanar", 37), ("coplanar_noise", 37), ("cube", 8), ("identity", 37),
               ("offset", 37), ("aniso", 37), ("generic", 3), ("generic", 255), ("generic", 256), ("generic", 257),
               ("mirror", 65537)]


def test_solve_clouds(N):
    errs, reach = [], []
    for kind, n in SOLVE_CASES:
        g = _gen(1, n, len(kind))
        src, dst, w = _cube() if kind == "cube" else _cloud(g, n, kind)
        r = _um64(src, dst, w)
        tag = f"{kind} n={n}"
        R, t, s = _irls(N, errs, tag, [src], [dst], [w])
        _solve_check(errs, tag, (R[0], t[0], s[0]), r, "clouds")
        _proper(errs, tag, R[0], "clouds")
        reach.append((tag, _reach_pass(n), "d", r["d"], "sv", [float(v) for v in r["sv"]]))
        if kind == "mirror":
            if r["d"] != -1.0:
                errs.append(f"{tag}: the reference did not take d = -1")
            s_ref = (r["sv"][0] + r["sv"][1] - r["sv"][2]) / r["varx"]
            if abs(float(s[0]) - float(s_ref)) > 2 * U * float(s_ref):
                errs.append(f"{tag}: s {float(s[0])!r} is not (sv0 + sv1 - sv2) / var_x = {float(s_ref)!r}")
        if kind == "cube":
            A = r["Sg"].T @ r["Sg"]
            off = float((A - torch.diag(torch.diag(A))).abs().max())
            reach.append(("cube: off-diagonal of Sg^T Sg", off, "diagonal", torch.diag(A).tolist()))
            if off != 0.0 or len(set(torch.diag(A).tolist())) != 1:
                errs.append("cube: Sg^T Sg is not a multiple of I on the host; the case does not reach V = I")
    assert any(rc[1]["trips"] == 2 for rc in reach if isinstance(rc[1], dict))
    _done(errs, *reach)


@pytest.mark.parametrize("kind,n", [("line", 37), ("line", 2)])
def test_solve_rank_one(N, kind, n):
    """Collinear points and two points.  Before irls_solve completed U[:, 1] orthogonally, this
    measured |R R^T - I| = 2.3e-2, det R = 0.99904 (37 collinear points) and |R R^T - I| = 0.85,
    det R = 0.273 (two points) on the MI355X; s, R v0 and the residual were right."""
    errs = []
    src, dst, w = _cloud(_gen(2, n), n, kind)
    r = _um64(src, dst, w)
    tag = f"{kind} n={n}"
    R, t, s = _irls(N, errs, tag, [src], [dst], [w])
    R, t, s = R[0], t[0], s[0]
    print(f"rank one {tag}: sv {[float(v) for v in r['sv']]} R {R.reshape(-1).tolist()} t {t.tolist()} s {float(s)}")
    assert float(r["sv"][1]) <= 1e-12 * float(r["sv"][0]), "the cloud is not rank one"
    _proper(errs, tag, R, "rank1")
    bs = 2 * U * r["s"].abs().reshape(1)
    ws_ = _within(errs, f"{tag} s", s.reshape(1), r["s"].reshape(1), bs)
    u0, v0 = r["U"][:, 0], r["V"][:, 0]
    wd = _within(errs, f"{tag} R v0 = u0", (R.double() @ v0).float(), u0, torch.full((3,), 2 * U, dtype=F64))
    x, y, wt = src.double(), dst.double(), w.double()
    Rd, sd, td = R.double(), float(s), t.double()
    res = sd * x @ Rd.T + td - y
    rms = float(((wt * (res ** 2).sum(1)).sum() / wt.sum()).sqrt())
    sr = float(r["s"])
    rho = math.sqrt(3) * U * (sr * float(x.abs().max()) + float(y.abs().max()))
    bt = float((2 * U * r["t"].abs().max() + U * (r["s"] * (r["R"] @ r["mux"])).abs()).max())
    rnd = float((U * sr * x.abs().sum(1) + 2 * U * sr * (x @ Rd.T).abs().max(1).values).max()) + bt
    print(f"rank one {tag}: s {ws_:.3f}  R v0 {wd:.3f}  rms residual {rms:.3e} of {rho + rnd:.3e}")
    _fig(("rank1", "s / Rv0 / residual"), max(ws_, wd, rms / (rho + rnd) if math.isfinite(rms) else math.inf))
    if not rms <= rho + rnd:
        errs.append(f"{tag}: weighted RMS residual {rms:.3e} > {rho + rnd:.3e}")
    _done(errs, (tag, _reach_pass(n)))


@pytest.mark.parametrize("kind", ["general", "line"])
def test_solve_shares_its_svd_with_the_pose_alignment(N, kind):
    """irls_solve's half of the pair that csrc/small_eig.h serves (the other half, on the same centres:
    test_gpu_training_metrics.py::test_pose_sim3_shares_its_svd_with_the_point_alignment).  Unit weights, conf_dst
    NULL, max_iters = 0: one solve.  The sums feeding the two solvers are reduced differently, so each is held to
    the fp64 solve, not to the other."""
    errs = []
    x, y = _svd_centres(kind)
    R, t, s = _irls(N, errs, f"svd pair {kind}", [x], [y], [torch.ones(x.shape[0])])
    _svd_pair_check(errs, "irls_sim3", kind, R[0], t[0], s[0])
    _done(errs)


def test_solve_one_point(N):
    """var_x = 0: no rotation or scale is defined (the reference divides 0 by 0).  The entry returns
    NaN in every output, as for a total weight below 1e-6 (include/vggt_mi355x.h)."""
    errs = []
    src, dst, w = _cloud(_gen(3), 1, "generic")
    _all_nan(errs, "n=1", _irls(N, errs, "n=1", [src], [dst], [w]))
    src, dst, w = _cloud(_gen(4), 5, "generic")
    w[1:] = 0.0  # five points, all the weight on one
    _all_nan(errs, "one weighted point of 5", _irls(N, errs, "n=5", [src], [dst], [w]))
    _done(errs, ("n=1", _reach_pass(1)))


def test_solve_batch_strides(N):
    errs = []
    n = 37
    g = _gen(5)
    el = [_cloud(g, n, "generic"), _cloud(g, n, "mirror"), _cloud(g, n, "generic"), _cloud(g, n, "generic")]
    el[2] = (el[2][0], el[2][1], torch.full((n,), 1e-9))  # total weight 3.7e-8 < 1e-6
    src3, dst3, w3 = el[3]
    w3[::5] = 0.0
    for k, i in enumerate(range(0, n, 5)):
        src3[i, k % 3] = (NAN, INF, -INF)[k % 3]
        dst3[i, (k + 1) % 3] = (INF, NAN, -INF)[k % 3]
    src, dst, w = [e[0] for e in el], [e[1] for e in el], [e[2] for e in el]
    ws = _ws(N, 4)
    got = _irls(N, errs, "B=4", src, dst, w, gap=True, ws=ws)
    again = _irls(N, errs, "B=4 again", src, dst, w, gap=True, ws=ws)  # the workspace as the first call left it
    for name, a, b in zip("Rts", got, again):
        _eq_bits(errs, f"second call on the same workspace {name}", b, a)
    for b in range(4):
        alone = _irls(N, errs, f"element {b} alone", [src[b]], [dst[b]], [w[b]])
        for name, a, c in zip("Rts", got, alone):
            _eq_bits(errs, f"element {b} {name} in the batch vs alone", a[b].reshape(-1), c[0].reshape(-1))
    _all_nan(errs, "weightless element", [v[2] for v in got])
    keep = w3 > 0
    for b, r in ((0, _um64(src[0], dst[0], w[0])), (1, _um64(src[1], dst[1], w[1])),
                 (3, _um64(src3[keep], dst3[keep], w3[keep]))):
        _solve_check(errs, f"batch element {b}", (got[0][b], got[1][b], got[2][b]), r, "batch")
    _done(errs, ("B=4 strides", {"src_bs": 3 * n + 5, "dst_bs": 3 * n + 7, "cs_bs": n + 3},
                 "zero-weight points with NaN / inf", int((~keep).sum())))


# ================================================================== 2. the confidence threshold
def _f(bits):
    return torch.tensor(bits, dtype=torch.int32).view(F32)


def _prev(x):
    """The fp32 number one ulp below x > 0."""
    return float((torch.tensor(x, dtype=F32).view(torch.int32) - 1).view(F32))


def _conf_case(name, n, g):
    """-> conf [n] fp32 and the indices of the borderline points.  The lower median is m; low
    values sit around 0.5 m, fillers between, the upper half above."""
    half = (n - 1) // 2
    exact = name.endswith("exact")  # multiples of 1/4, usable as cs = cd
    m = 4.0
    if name.startswith("ties"):
        low = [2.0, 1.75, 2.0, 2.75]
        below = [3.0] * (half - len(low) - n // 5)
        mid = [m] * (n // 5 + 1 + n // 5)
    elif name == "low_byte":
        m = float(_f(0x40000080))
        low = [0.5 * m, _prev(0.5 * m), 0.5 * m]
        below = [float(_f(0x40000000 + (k % 0x80))) for k in range(half - len(low))]
        mid = [m]
    elif name == "top_byte":
        m = 2.0
        low = [1.0, 0.5, _prev(1.0)]
        below = [1.0 + 0.5 * (k % 2) for k in range(half - len(low))]
        mid = [m]
    elif name == "denormal":
        m = float(_f(0x00000100))
        low = [0.5 * m, _prev(0.5 * m), 0.0, float(_f(0x00000001))]
        below = [float(_f(0x00000081 + k)) for k in range(half - len(low))]
        mid = [m]
    elif name == "zeros":
        m = 0.0
        low, below, mid = [], [0.0] * half, [0.0]
    else:
        low = [2.0, 1.75, 2.75, 1.0, 0.25] if exact else [2.0, _prev(2.0), 2.75, 2.0]
        below = [3.0 + 0.25 * (k % 3) for k in range(half - len(low))]
        mid = [m]
    vals = low + below + mid
    if name == "low_byte":
        above = [float(_f(0x40000081 + (k % 0x7f))) for k in range(n - len(vals))]
    elif name == "top_byte":
        above = [float(_f(0x41000000 + 0x01000000 * (k % 3))) for k in range(n - len(vals))]
    elif name == "denormal":
        above = [1.0 + 0.25 * (k % 5) for k in range(n - len(vals))]
    elif name == "zeros":
        above = [0.25 * (1 + k % 3) for k in range(n - len(vals))]
    else:
        above = [6.0 + 0.25 * (k % 7) for k in range(n - len(vals))]
    vals = torch.tensor(vals + above, dtype=F32)
    assert vals.numel() == n
    perm = torch.randperm(n, generator=g)
    conf = torch.empty(n)
    conf[perm] = vals
    border = perm[:len(low)] if low else perm[half + 1:half + 4]  # zeros: three small positive ones
    return conf, border


def _thr_check(N, errs, tag, src, dst, conf, both, ftag):
    if both:
        comb = torch.sqrt(conf * conf)
        assert torch.equal(comb, conf), "sqrt(c * c) is not exact for these confidences"
    med = torch.median(conf)
    thr = torch.tensor(0.5, dtype=F32) * med
    mask = conf >= thr
    r = _um64(src[mask], dst[mask], conf[mask])
    R, t, s = _irls(N, errs, tag, [src], [dst], [conf], [conf] if both else None, factor=0.5)
    _solve_check(errs, tag, (R[0], t[0], s[0]), r, ftag)
    return {"median": float(med), "thr": float(thr), "kept": int(mask.sum()), "at_thr": int((conf == thr).sum())}


THR_CASES = [("plain", 37), ("plain", 38), ("plain_exact", 37), ("plain_exact", 38), ("ties", 37), ("ties_exact", 38),
             ("low_byte", 37), ("top_byte", 37), ("denormal", 37), ("zeros", 37), ("zeros", 38)]


def test_threshold_decisions(N):
    errs, reach = [], []
    for name, n in THR_CASES:
        g = _gen(6, n, len(name))
        src, dst, _ = _cloud(g, n, "generic")
        conf, border = _conf_case(name, n, g)
        for k, i in enumerate(border.tolist()):
            dst[i, k % 3] += 50.0
        info = _thr_check(N, errs, f"{name} n={n}", src, dst, conf, name.endswith("exact"), "threshold")
        reach.append((f"{name} n={n}", info, _reach_hist(n)))
        if name != "zeros" and not (info["at_thr"] >= 1 and 0 < info["kept"] < n):
            errs.append(f"{name} n={n}: the case has no point exactly at the threshold, or drops none")
        if name == "zeros" and not (info["median"] == 0.0 and info["kept"] == n):
            errs.append(f"{name} n={n}: the median is not 0")
    _done(errs, *reach)


def test_threshold_second_grid_trip(N):
    """n = 262 401: irls_hist's 1024 blocks x 256 threads take a second trip."""
    errs = []
    n = 262144 + 257
    g = _gen(7)
    src, dst, _ = _cloud(g, n, "generic")
    conf = torch.randint(1, 65, (n,), generator=g).float() / 4
    med = float(torch.median(conf))
    border = ((conf == 0.5 * med) | (conf == 0.5 * med - 0.25)).nonzero().reshape(-1)[:400]
    dst[border, 0] += 50.0
    info = _thr_check(N, errs, f"n={n}", src, dst, conf, False, "threshold")
    rh = _reach_hist(n)
    assert rh["trips"] == 2 and info["at_thr"] > 0 and border.numel() == 400
    _done(errs, (f"n={n}", info, rh, _reach_pass(n)))


def test_threshold_masked_nan(N):
    """NaN / inf coordinates at dropped points: the reference's boolean mask never reads them.
    Before irls_pass1 / irls_pass2 skipped points of weight 0, 0 * NaN made every output NaN."""
    errs, reach = [], []
    for both in (False, True):
        n = 37
        g = _gen(8, both)
        src, dst, _ = _cloud(g, n, "generic")
        conf, _ = _conf_case("plain_exact", n, g)
        drop = (conf < 0.5 * torch.median(conf)).nonzero().reshape(-1).tolist()
        finite = _irls(N, errs, "finite", [src], [dst], [conf], [conf] if both else None, factor=0.5, iters=2)
        for k, i in enumerate(drop):
            src[i, k % 3] = (NAN, INF, -INF)[k % 3]
            dst[i, (k + 2) % 3] = (INF, NAN, NAN)[k % 3]
        info = _thr_check(N, errs, f"masked NaN conf_dst={both}", src, dst, conf, both, "masked")
        masked = _irls(N, errs, "masked", [src], [dst], [conf], [conf] if both else None, factor=0.5, iters=2)
        for name, a, b in zip("Rts", masked, finite):  # what a dropped point holds changes no bit, IRLS passes included
            _eq_bits(errs, f"conf_dst={both} {name}: NaN against finite coordinates at the dropped points", a, b)
        reach.append((f"conf_dst={both}", info, "dropped points with NaN / inf", len(drop)))
        assert len(drop) >= 2
    _done(errs, *reach)


def test_threshold_nan_negative_confidence(N):
    """Outside the reference's domain; the header's contract: such a point never carries weight and
    orders above every non-negative value in the median (the select orders bit patterns); a NaN
    median drops everything (NaN outputs)."""
    errs = []
    n = 37
    g = _gen(9)
    src, dst, _ = _cloud(g, n, "generic")
    conf = 1.0 + torch.randint(0, 12, (n,), generator=g).float() / 4
    conf[3], conf[11], conf[20] = NAN, NAN, NAN
    conf[5], conf[30] = -2.0, -0.5
    dst[5, 0] += 50.0
    dst[30, 1] += 50.0
    order = torch.sort(conf.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).values
    m = int(order[(n - 1) // 2])  # the lower median of the bit patterns, as unsigned numbers
    med = float(_f(m - 2 ** 32 if m >= 2 ** 31 else m))
    thr = torch.tensor(0.5, dtype=F32) * torch.tensor(med, dtype=F32)
    mask = (conf >= thr) & (conf >= 0)
    assert math.isfinite(med) and med > 0 and int(mask.sum()) < n - 5
    R, t, s = _irls(N, errs, "NaN / negative", [src], [dst], [conf], None, factor=0.5)
    ref = _um64(src[mask], dst[mask], conf[mask])
    _solve_check(errs, "NaN / negative confidences", (R[0], t[0], s[0]), ref, "nanconf")
    conf2 = conf.clone()
    conf2[:20] = NAN
    _all_nan(errs, "NaN median", _irls(N, errs, "NaN median", [src], [dst], [conf2], None, factor=0.5))
    _done(errs, ("NaN / negative", {"median": med, "kept": int(mask.sum())}))


# ================================================================== 3. IRLS iterations
def _irls_cloud(seed, n=301, frac=0.1, out=4.0):
    g = torch.Generator().manual_seed(seed)
    src = 2 * torch.randn(n, 3, generator=g) + torch.tensor([0.0, 0.0, 6.0])
    c, s_ = math.cos(0.4), math.sin(0.4)
    Ry = torch.tensor([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], dtype=F32)
    dst = 1.3 * src @ Ry.T + torch.tensor([0.5, -1.0, 2.0]) + 0.01 * torch.randn(n, 3, generator=g)
    bad = torch.rand(n, generator=g) < frac
    dst[bad] += out * torch.randn(int(bad.sum()), 3, generator=g)
    cs = 1 + 3 * torch.rand(n, generator=g)
    cd = 1 + 3 * torch.rand(n, generator=g)
    return src, dst, cs, cd


def _irls64(src, dst, cs, cd, max_iters, tol, factor=0.5, delta=0.1, dt=F64):
    """irls_sim3_umeyama restated: -> the iterates [(R, t, s)] and the deltas of each re-weighting.
    The mask comes from the fp32 combined confidence, as the kernel and the reference see it."""
    comb32 = torch.sqrt(cs * cd)
    mask = comb32 >= factor * torch.median(comb32)
    x, y, c = src[mask].to(dt), dst[mask].to(dt), torch.sqrt(cs.to(dt) * cd.to(dt))[mask]
    its = [AO.weighted_umeyama_sim3(x, y, c.clone())]
    deltas = []
    for _ in range(max_iters):
        R, t, s = its[-1]
        res = torch.linalg.norm(s * (x @ R.T) + t - y, dim=1)
        rw = torch.where(res <= delta, torch.ones_like(res), delta / res.clamp_min(1e-12))
        its.append(AO.weighted_umeyama_sim3(x, y, c * rw))
        d = (float((its[-1][0] - R).norm()), float((its[-1][1] - t).norm()), float((its[-1][2] - s).abs()))
        deltas.append(d)
        if all(v < tol for v in d):
            break
    return its, deltas


def _iter_rule(errs, tag, got, ref, model, ftag):
    """Per output: the kernel's worst element <= 2 x the fp32 oracle's worst element (both against
    fp64) + one fp32 ulp of the output's magnitude."""
    for name, a, r, m in zip("Rts", got, ref, model):
        r = r.double().reshape(-1)
        k = float((a.double().reshape(-1) - r).abs().max())
        mo = float((m.double().reshape(-1) - r).abs().max())
        bound = 2 * mo + 2 * U * float(r.abs().max())
        print(f"irls {tag} {name}: kernel {k:.3e} model {mo:.3e} bound {bound:.3e} ratio {k / bound:.3f}")
        _fig(("irls", ftag, name), k / bound if math.isfinite(k) else math.inf)
        if not k <= bound:
            errs.append(f"{tag} {name}: kernel {k:.3e} > 2 x model {mo:.3e} + ulp = {bound:.3e}")


# The issue's recipe with two seeds: one cloud cannot serve both tol cases, since tol = 0.2 must stop
# with every first delta below 0.2 / 1.5 = 0.133 and tol = 0.1 must go on with |dt| above 0.15.
# Reference deltas (R, t, s) of the first two re-weightings: seed 14: (0.041, 0.102, 0.002),
# (0.0013, 0.0022, 0.0000); seed 3: (0.040, 0.176, 0.023), (0.0007, 0.0034, 0.0003).
IRLS_SEED_STOP, IRLS_SEED_GO = 14, 3


def _margin(errs, tag, deltas, tol):
    for it, d in enumerate(deltas):
        for v in d:
            if tol / 1.5 < v < tol * 1.5:
                errs.append(f"{tag}: reference delta {v:.4f} of iteration {it + 1} is within 1.5 x of tol {tol}")


def test_irls_iteration_counts(N):
    """tol = 0: exactly max_iters re-weightings.  tol = 0.2: stop after the first (all three deltas
    below).  tol = 0.1: |dt| alone is above tol after the first, so a second one must run."""
    errs, reach = [], []
    cl = _irls_cloud(IRLS_SEED_GO)
    its, deltas = _irls64(*cl, 3, 0.0)
    reach.append(("reference deltas (R, t, s) per iteration", deltas))
    for k in (0, 1):
        dt = float((its[k + 1][1] - its[k][1]).norm())
        if dt < 1e-3:
            errs.append(f"iterates {k} and {k + 1} differ by {dt:.2e} < 1e-3 in t: the test cannot tell them apart")
    for k in (0, 1, 2):
        mod, _ = _irls64(*cl, k, 0.0, dt=F32)
        got = _irls(N, errs, f"max_iters={k}", [cl[0]], [cl[1]], [cl[2]], [cl[3]], factor=0.5, iters=k, tol=0.0)
        _iter_rule(errs, f"tol=0 max_iters={k}", [v[0] for v in got], its[k], mod[-1], "counts")
    for tol, seed, want in ((0.2, IRLS_SEED_STOP, 1), (0.1, IRLS_SEED_GO, 2)):
        cl = _irls_cloud(seed)
        its, deltas = _irls64(*cl, 20, tol)
        _margin(errs, f"tol={tol}", deltas, tol)
        more, _ = _irls64(*cl, want + 1, 0.0)
        for k in range(want + 1 if want == 1 else want):
            dt = float((more[k + 1][1] - more[k][1]).norm())
            if dt < 1e-3:
                errs.append(f"tol={tol}: iterates {k} and {k + 1} differ by {dt:.2e} < 1e-3 in t")
        reach.append((f"tol={tol} seed {seed}", "reference re-weightings", len(deltas), deltas))
        if len(deltas) != want:
            errs.append(f"tol={tol}: the reference runs {len(deltas)} re-weightings, the case needs {want}")
        if want == 2 and not (deltas[0][1] > tol and deltas[0][0] < tol and deltas[0][2] < tol):
            errs.append(f"tol={tol}: the first deltas {deltas[0]} do not have |dt| alone above tol")
        mod, _ = _irls64(*cl, len(deltas), 0.0, dt=F32)
        got = _irls(N, errs, f"tol={tol}", [cl[0]], [cl[1]], [cl[2]], [cl[3]], factor=0.5, iters=20, tol=tol)
        _iter_rule(errs, f"tol={tol}", [v[0] for v in got], its[-1], mod[-1], "counts")
    _done(errs, *reach)


def test_irls_default_arguments(N):
    """tol = 1e-9, 20 iterations: no fp32 iterate converges at that tol; all 20 run."""
    errs = []
    cl = _irls_cloud(IRLS_SEED_GO)
    ref = AO.irls_sim3_umeyama(*(v.double() for v in cl))
    model = AO.irls_sim3_umeyama(*cl)
    got = _irls(N, errs, "defaults", [cl[0]], [cl[1]], [cl[2]], [cl[3]], factor=0.5, iters=20, tol=1e-9)
    _iter_rule(errs, "defaults", [v[0] for v in got], ref, model, "defaults")
    _done(errs, ("defaults", _reach_hist(301), _reach_pass(301)))


def test_irls_batch_stops_apart(N):
    """Three elements under one tol that stop after different numbers of re-weightings: a finished
    element's state and outputs must stay as they are while the others run on."""
    errs = []
    tol = 0.1
    cls = [_irls_cloud(11, frac=0.0), _irls_cloud(IRLS_SEED_GO), _irls_cloud(13, frac=0.3, out=30.0)]
    counts = [len(_irls64(*c, 20, tol)[1]) for c in cls]
    assert len(set(counts)) == 3, f"the reference stops at {counts}: the elements do not stop apart"
    got = _irls(N, errs, "B=3", *[[c[k] for c in cls] for k in range(4)], factor=0.5, iters=20, tol=tol, gap=True)
    for b, c in enumerate(cls):
        alone = _irls(N, errs, f"element {b}", [c[0]], [c[1]], [c[2]], [c[3]], factor=0.5, iters=20, tol=tol)
        for name, a, o in zip("Rts", got, alone):
            _eq_bits(errs, f"element {b} {name} in the batch vs alone", a[b].reshape(-1), o[0].reshape(-1))
        its, _ = _irls64(*c, 20, tol)
        mod, _ = _irls64(*c, counts[b], 0.0, dt=F32)
        _iter_rule(errs, f"batch element {b}", [v[b] for v in got], its[-1], mod[-1], "batch")
    _done(errs, ("re-weightings per element (reference)", counts))


# ================================================================== 4. sim3_points, scale_f32
def _points_call(N, P, n, T, sc, Oo):
    rc = N.lib().vggt_sim3_points(P.ptr, P.bs, P.B, n, ctypes.c_void_p(T.data_ptr()),
                                  ctypes.c_void_p(sc.data_ptr()) if sc is not None else None, Oo.ptr, Oo.bs, _stream())
    _sync()
    return rc


@pytest.mark.parametrize("n,B,scaled,gap", [(1, 2, True, 4), (255, 2, False, 6), (257, 3, True, 5),
                                            (524288 + 3, 1, True, 0)])
def test_sim3_points(N, n, B, scaled, gap):
    errs = []
    g = _gen(20, n, B)
    pts = [torch.randn(n, 3, generator=g) * 3 + torch.tensor([0.0, 1.0, 5.0]) for _ in range(B)]
    T = torch.zeros(B, 4, 4)
    for b in range(B):
        T[b, :3, :3] = _rot(g).float()
        T[b, :3, 3] = torch.randn(3, generator=g) * 2
        T[b, 3, 3] = 1.0
    sc = (0.5 + torch.rand(B, generator=g)) if scaled else None
    Td, scd = T.to(DEV), sc.to(DEV) if scaled else None
    P = Blocks(pts, 3 * n + gap)
    inplace = Blocks(pts, 3 * n + gap, fill=SENT)
    if n < 10 ** 5:
        Oo = _out(B, 3 * n, 3 * n + gap + 1)
        assert _points_call(N, P, n, Td, scd, Oo) == OK
        if not Oo.intact():
            errs.append("out of place: sentinels overwritten")
        got = Oo.get()
    assert _points_call(N, inplace, n, Td, scd, inplace) == OK
    if not inplace.intact():
        errs.append("in place: sentinels between the batch elements overwritten")
    if n < 10 ** 5:
        for b in range(B):
            _eq_bits(errs, f"in place vs out of place, element {b}", inplace.get()[b], got[b])
    else:
        got = inplace.get()
    worst = 0.0
    for b in range(B):
        sp = (pts[b] * sc[b]) if scaled else pts[b]  # one fp32 rounding
        R, t = T[b, :3, :3].double(), T[b, :3, 3].double()
        ref = sp.double() @ R.T + t
        bound = _gam(4) * (sp.double().abs() @ R.abs().T + t.abs())
        worst = max(worst, _within(errs, f"element {b}", got[b].view(n, 3), ref, bound))
    print(f"sim3_points n={n}: worst error / bound {worst:.3f}")
    _fig(("points", "gamma_4"), worst)
    rp = _reach_points(n)
    assert n < 10 ** 5 or rp["trips"] == 2
    _done(errs, (f"n={n} B={B} scale={'yes' if scaled else 'NULL'}", rp))


@pytest.mark.parametrize("n,bs_extra,off", [(1, 3, 0), (3, 1, 0), (4, 4, 0), (5, 3, 0), (1027, 5, 0), (2097152 + 5, 3, 0),
                                            (5, 1, 0), (1027, 2, 0), (1027, 5, 1), (4, 0, 3)])
def test_scale_f32(N, n, bs_extra, off):
    """bs_extra makes bs = n + bs_extra; `off` floats move the base off 16-byte alignment."""
    errs = []
    B = 1 if n > 10 ** 6 else 3
    g = _gen(21, n, bs_extra, off)
    x = [torch.randn(n, generator=g) for _ in range(B)]
    sc = torch.tensor([-0.5, 0.0, 1.0][:B]) if B == 3 else torch.tensor([-0.5])
    X = Blocks(x, n + bs_extra, fill=SENT, off=off)
    rs = _reach_scale(n, X.bs, X.dev.data_ptr() + 4 * X.base)
    scd = sc.to(DEV)
    rc = N.lib().vggt_scale_f32(X.ptr, X.bs, B, n, ctypes.c_void_p(scd.data_ptr()), _stream())
    _sync()
    assert rc == OK
    if not X.intact():
        errs.append("guards / gaps around the blocks overwritten")
    for b in range(B):
        _eq_bits(errs, f"element {b} scale {float(sc[b])}", X.get()[b], x[b] * sc[b])
    _fig(("scale", rs["path"]), 1.0)
    _done(errs, (f"n={n} bs={X.bs} base offset {off}", rs))


def test_scale_f32_paths_reached():
    """The parametrisation above reaches both paths and the second vector trip (host arithmetic)."""
    r = [_reach_scale(n, n + e, 256 + 4 * o) for n, e, o in [(2097157, 3, 0), (5, 1, 0), (1027, 5, 1), (1027, 5, 0)]]
    assert r[0]["path"] == "vector" and r[0]["vector_trips"] == 2
    assert r[1]["path"] == "scalar" and r[2]["path"] == "scalar" and r[3]["path"] == "vector" and r[3]["tail"] == 3


# ================================================================== 5. pose_compose
def _extri_to_enc64(extr):
    quat = O.mat_to_quat(extr[:, :, :3, :3])
    quat = quat / quat.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    return torch.cat([extr[:, :, :3, 3], quat], dim=-1)


def _markley64(enc):
    B, n, _ = enc.shape
    t = enc[..., :3].mean(dim=1, keepdim=True)
    q = enc[..., 3:7]
    q = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    M = (q.unsqueeze(-1) * q.unsqueeze(-2)).sum(dim=1) / n
    val, vec = torch.linalg.eigh(M)
    v = vec[..., -1]
    return torch.cat([t, (v / v.norm(dim=-1, keepdim=True)).unsqueeze(1)], dim=-1), val


def _extr64(cam, scale, hw):
    B = cam.shape[0]
    extr, intr = O.pose_encoding_to_extri_intri(cam, hw)
    extr = torch.nn.functional.pad(extr, (0, 0, 0, 1, 0, 0, 0, 0))
    extr[:, :, 3, 3] = 1.0
    ident = O.closed_form_inverse_se3(extr[:, 0])
    pt_ident = extr[:, 0].clone()
    extr = extr @ ident.view(B, 1, 4, 4)
    extr[:, :, :3, 3] *= scale.view(B, 1, 1)
    return extr, intr, pt_ident


def _compose64(cs, fs, cam, ctx, gt, ov, hw):
    """oracle.vggt_oracle.compose_poses in fp64 throughout (the oracle's pose-encoding helpers end
    in .float(), as the reference's do) -> encoding [B,S,9], point transform [B,4,4], the composed
    matrices [B,S,4,4] and the eigenvalues of the Markley matrix (or None)."""
    cs, fs, cam = cs.double(), fs.double(), cam.double()
    B, S = cam.shape[:2]
    H, W = hw
    chunk = O.pose_encoding_to_extri(cs.view(B, 1, 8)[..., :7])
    pf = torch.cat([chunk, O.pose_encoding_to_extri(fs) @ chunk], dim=1) if S > 1 else chunk
    extr, intr, pt_ident = _extr64(cam, cs.view(B, 8)[:, 7], hw)
    eig = None
    if ctx is not None:
        if gt is not None:
            mean = gt.double().reshape(B, 1, 4, 4)
        else:
            ctx_o = O.pose_encoding_to_extri(ctx.double()[:, -ov:, :7])
            ct = O.closed_form_inverse_se3(extr[:, :ov].reshape(B * ov, 4, 4)).reshape(B, ov, 4, 4) @ ctx_o
            if ov > 1:
                enc, eig = _markley64(_extri_to_enc64(ct))
                mean = O.pose_encoding_to_extri(enc)
            else:
                mean = ct
    else:
        mean = torch.eye(4, dtype=F64).view(1, 1, 4, 4).expand(B, -1, -1, -1)
    pf = pf @ mean
    al = extr @ pf
    fov_h = 2 * torch.atan((H / 2) / intr[..., 1, 1])
    fov_w = 2 * torch.atan((W / 2) / intr[..., 0, 0])
    enc = torch.cat([al[:, :, :3, 3], O.mat_to_quat(al[:, :, :3, :3]), fov_h[..., None], fov_w[..., None]], dim=-1)
    tr = O.closed_form_inverse_se3(pf[:, 0]) @ pt_ident if ctx is not None else pt_ident
    return enc, tr, al, eig


def _branches(al):
    """mat_to_quat's candidate (argmax of q_abs) and the w < 0 flip per composed rotation, fp64."""
    m = al[..., :3, :3].reshape(-1, 3, 3)
    d = torch.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                     1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], -1)
    b = d.clamp_min(0).sqrt().argmax(-1)
    wc = torch.stack([d[:, 0], m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]], -1)
    return b, wc.gather(1, b[:, None])[:, 0] < 0


def _rq(g, *shape):
    q = torch.randn(*shape, 4, generator=g)
    return q / q.norm(dim=-1, keepdim=True)


def _pose_call(N, cs, fs, cam, ctx, gt, ov, hw, want_pt=True, S_prev=None):
    B, S = cam.shape[:2]
    d = lambda t: None if t is None else t.to(F32).contiguous().to(DEV)  # noqa: E731
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a = [d(cs), d(fs) if fs is not None and fs.numel() else None, d(cam), d(ctx), d(gt)]
    out, pt = _out(1, B * S * 9), _out(1, B * 16)
    rc = N.lib().vggt_pose_compose(p(a[0]), p(a[1]), p(a[2]), p(a[3]),
                                   (ctx.shape[1] if ctx is not None else 0) if S_prev is None else S_prev, p(a[4]), B, S,
                                   int(ov), int(hw[0]), int(hw[1]), out.ptr, pt.ptr if want_pt else None, _stream())
    _sync()
    return rc, out, pt


def _pose_check(errs, tag, got, gpt, cs, fs, cam, ctx, gt, ov, hw, ftag):
    B, S = cam.shape[:2]
    ref, rpt, al, eig = _compose64(cs, fs, cam, ctx, gt, ov, hw)
    mod, mpt = O.compose_poses(cs.view(B, 1, 8), fs, cam, ctx, gt, ov, hw)
    got, mod = got.view(B, S, 9), mod.view(B, S, 9)
    _model_rule(errs, f"{tag} translation", got[..., :3].reshape(-1, 3), mod[..., :3].reshape(-1, 3),
                ref[..., :3].reshape(-1, 3), ftag + " translation")
    qr = ref[..., 3:7].reshape(-1, 4)
    qg, qm = got[..., 3:7].reshape(-1, 4).clone(), mod[..., 3:7].reshape(-1, 4).clone()
    al_m = torch.where(((qm.double() * qr).sum(-1, keepdim=True) < 0), -qm, qm)
    bound = 2 * float((al_m.double() - qr).norm(dim=-1).max())
    free = qr[:, 3].abs() <= bound  # w = 0 within the bound: q and -q are the same answer
    for q in (qg, qm):
        flip = free & ((q.double() * qr).sum(-1) < 0)
        q[flip] = -q[flip]
    _model_rule(errs, f"{tag} quaternion", qg, qm, qr, ftag + " quaternion")
    _model_rule(errs, f"{tag} fov", got[..., 7:].reshape(-1, 2), mod[..., 7:].reshape(-1, 2), ref[..., 7:].reshape(-1, 2),
                ftag + " fov")
    if gpt is not None:
        _model_rule(errs, f"{tag} point transform", gpt.view(B * 4, 4), mpt.reshape(B * 4, 4), rpt.reshape(B * 4, 4),
                    ftag + " point transform")
        _eq_bits(errs, f"{tag} point transform row 3", gpt.view(B, 4, 4)[:, 3], torch.tensor([0.0, 0, 0, 1]).expand(B, 4))
    return al, eig, int(free.sum())


def _pose_inputs(g, B, S, S_prev, first):
    cs = torch.cat([torch.randn(B, 3, generator=g), _rq(g, B), 0.5 + torch.rand(B, 1, generator=g)], -1)
    fs = torch.cat([torch.randn(B, S - 1, 3, generator=g), _rq(g, B, S - 1) * 1.3], -1)
    cam = torch.cat([torch.randn(B, S, 3, generator=g), _rq(g, B, S) * 0.9,
                     0.2 + 2.4 * torch.rand(B, S, 2, generator=g)], -1)
    ctx = None if first else torch.cat([torch.randn(B, S_prev, 3, generator=g), _rq(g, B, S_prev),
                                        torch.rand(B, S_prev, 2, generator=g)], -1)
    return cs, fs, cam, ctx


HW = (154, 518)


@pytest.mark.parametrize("S,mode,ov", [(1, "first", 1), (1, "ctx", 1), (64, "ctx", 2), (65, "ctx", 1), (65, "first", 1),
                                       (130, "ctx", 3), (5, "gt", 1)])
def test_pose_compose_frames(N, S, mode, ov):
    errs = []
    B, S_prev = 3, max(ov, 2) + 1
    g = _gen(30, S, ov, len(mode))
    cs, fs, cam, ctx = _pose_inputs(g, B, S, S_prev, mode == "first")
    cam[1, S // 2, 7] = 0.0  # fov = 0 must give exactly 0
    gt = O.pose_encoding_to_extri(torch.cat([torch.randn(B, 1, 3, generator=g), _rq(g, B, 1)], -1))[:, 0] if mode == "gt" else None
    rc, out, pt = _pose_call(N, cs, fs, cam, ctx, gt, ov, HW)
    assert rc == OK
    if not (out.intact() and pt.intact()):
        errs.append("guards around the outputs overwritten")
    got, gpt = out.get()[0], pt.get()[0]
    _pose_check(errs, f"S={S} {mode} ov={ov}", got, gpt, cs, fs, cam, ctx, gt, ov, HW, "pose")
    if float(got.view(B, S, 9)[1, S // 2, 7]) != 0.0:
        errs.append(f"fov = 0 gave {float(got.view(B, S, 9)[1, S // 2, 7])!r}")
    rc, out2, pt2 = _pose_call(N, cs, fs, cam, ctx, gt, ov, HW, want_pt=False)  # point_transform NULL
    assert rc == OK
    _eq_bits(errs, "point_transform NULL: the encoding", out2.get()[0], got)
    if not pt2.intact() or not torch.equal(pt2.get()[0], torch.full((B * 16,), SENT)):
        errs.append("point_transform NULL: the unused buffer was written")
    if mode == "gt":  # without a context the mean is I, gt_first or not
        rc, a, _ = _pose_call(N, cs, fs, cam, None, gt, ov, HW)
        rc2, b_, _ = _pose_call(N, cs, fs, cam, None, None, ov, HW)
        assert rc == OK and rc2 == OK
        _eq_bits(errs, "gt_first without a context vs the first chunk", a.get()[0], b_.get()[0])
        _pose_check(errs, f"S={S} gt without ctx", a.get()[0], None, cs, fs, cam, None, gt, ov, HW, "pose")
    _done(errs, (f"S={S} B={B} {mode}", {"frame_loop_trips": -(-S // 64), "ov": ov}))


def test_pose_compose_quaternion_branches(N):
    """Element 0 composes nothing (identity chunk, frames and first camera), so its rotations are
    the exact matrices of the camera quaternions: the 4-way tie and the three half turns.  The
    others pass random rotations through a generic chain."""
    errs = []
    B, S = 3, 130
    g = _gen(31)
    cs, fs, cam, _ = _pose_inputs(g, B, S, 2, True)
    cs[0, :7] = torch.tensor([0.0, 0, 0, 0, 0, 0, 1])
    fs[0, :, 3:] = torch.tensor([0.0, 0, 0, 1])
    cam[0, 0, :7] = torch.tensor([0.0, 0, 0, 0, 0, 0, 1])
    special = [[1.0, 1, 1, 1], [1.0, 0, 0, 0], [0.0, 1, 0, 0], [0.0, 0, 1, 0]]
    for k, q in enumerate(special):
        cam[0, 1 + k, 3:7] = torch.tensor(q)
    rc, out, pt = _pose_call(N, cs, fs, cam, None, None, 1, HW)
    assert rc == OK
    al, _, free = _pose_check(errs, "branches", out.get()[0], pt.get()[0], cs, fs, cam, None, None, 1, HW, "pose")
    br, flip = _branches(al)
    hist = [int((br == k).sum()) for k in range(4)]
    sp = al[0, 1:5, :3, :3]
    tie = torch.equal(sp[0], torch.tensor([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=F64))
    half = [torch.equal(sp[1 + k], torch.diag(torch.tensor([1.0 if j == k else -1.0 for j in range(3)], dtype=F64)))
            for k in range(3)]
    print("branch histogram", hist, "w < 0 flips", int(flip.sum()), "w = 0 within the bound", free)
    if min(hist) == 0 or int(flip.sum()) == 0:
        errs.append(f"a mat_to_quat branch is not reached: {hist}, flips {int(flip.sum())}")
    if not (tie and all(half)) or free < 3:
        errs.append(f"the exact rotations are not exact: tie {tie}, half turns {half}, w = 0 rows {free}")
    want = torch.tensor([[0.5, 0.5, 0.5, 0.5]])
    _eq_bits(errs, "120 degrees about (1, 1, 1)", out.get()[0].view(B, S, 9)[0, 1:2, 3:7], want)
    _done(errs, ("branches", hist, "flips", int(flip.sum())))


def _axis_angle(axis, deg):
    a = torch.tensor(axis, dtype=F64)
    a = a / a.norm()
    h = math.radians(deg) / 2
    return O.quat_to_mat(torch.cat([a * math.sin(h), torch.tensor([math.cos(h)], dtype=F64)]))


@pytest.mark.parametrize("ov", [2, 7, 64])
@pytest.mark.parametrize("mean_deg", [75.0, 179.8])
def test_pose_compose_markley(N, ov, mean_deg):
    errs = []
    B, S, S_prev = 2, max(ov, 3), ov + 1
    g = _gen(32, ov, int(mean_deg))
    cs, fs, cam, ctx = _pose_inputs(g, B, S, S_prev, False)
    extr, _, _ = _extr64(cam.double(), cs.double()[:, 7], HW)
    mean = torch.eye(4, dtype=F64).repeat(B, 1, 1)
    for b in range(B):
        mean[b, :3, :3] = _axis_angle([0.3 + b, -0.5, 0.8], mean_deg)
        mean[b, :3, 3] = torch.randn(3, generator=g, dtype=F64)
    for b in range(B):
        for k in range(ov):
            P = torch.eye(4, dtype=F64)
            ang = 2.0 * (2 * float(torch.rand(1, generator=g)) - 1) if k else 2.0
            P[:3, :3] = _axis_angle(torch.randn(3, generator=g, dtype=F64).tolist(), ang)
            P[:3, 3] = 0.05 * torch.randn(3, generator=g, dtype=F64)
            ctx[b, S_prev - ov + k, :7] = _extri_to_enc64((extr[b, k] @ mean[b] @ P).view(1, 1, 4, 4))[0, 0].float()
    rc, out, pt = _pose_call(N, cs, fs, cam, ctx, None, ov, HW)
    assert rc == OK
    tag = f"Markley ov={ov} mean {mean_deg}"
    _, eig, _ = _pose_check(errs, tag, out.get()[0], pt.get()[0], cs, fs, cam, ctx, None, ov, HW, "markley")
    gap = float((eig[:, 3] - eig[:, 2]).min())
    ref_ct = _extri_to_enc64(O.closed_form_inverse_se3(extr[:, :ov].reshape(B * ov, 4, 4)).reshape(B, ov, 4, 4)
                             @ O.pose_encoding_to_extri(ctx.double()[:, -ov:, :7]))
    signs = (ref_ct[..., 3:7] * ref_ct[:, :1, 3:7]).sum(-1) < 0  # quaternions opposite to the first one
    assert gap >= 0.9, f"eigen-gap {gap}"
    if mean_deg > 179 and ov >= 7 and not bool(signs.any()):
        errs.append("no overlap quaternion has the opposite sign: the case does not need Markley")
    _done(errs, (tag, {"eigen_gap": gap, "opposite_sign_quaternions": int(signs.sum())}))


# ================================================================== 6. error returns
def test_error_returns(N):
    errs = []
    L = N.lib()
    n = 8
    src, dst, w = _cloud(_gen(40), n, "generic")
    S_, D_, C_ = Blocks([src]), Blocks([dst]), Blocks([w])
    Ro, to, so = _out(1, 9), _out(1, 3), _out(1, 1)
    ws, nb = _ws(N, 1)
    wp = ws.data_ptr()

    def irls(B=1, n_=n, iters=0, wsp=wp, nbytes=nb):
        return L.vggt_irls_sim3(S_.ptr, 3 * n, D_.ptr, 3 * n, C_.ptr, n, None, 0, B, n_, 0.0, 0.1, iters, 0.0, Ro.ptr,
                                to.ptr, so.ptr, ctypes.c_void_p(wsp), nbytes, _stream())

    for name, rc, want in (("B=0", irls(B=0), ERR_SHAPE), ("B=-1", irls(B=-1), ERR_SHAPE), ("n=0", irls(n_=0), ERR_SHAPE),
                           ("n=-1", irls(n_=-1), ERR_SHAPE), ("max_iters=-1", irls(iters=-1), ERR_SHAPE),
                           ("workspace one byte short", irls(nbytes=nb - 1), ERR_ALIGN),
                           ("workspace 8 bytes off", irls(wsp=wp + 8), ERR_ALIGN)):
        if rc != want:
            errs.append(f"irls {name}: returned {rc}, want {want}")
    B, S = 1, 3
    cs, fs, cam, ctx = _pose_inputs(_gen(41), B, S, 4, False)
    for name, kw, fs_ in (("overlap 0", dict(ov=0), fs), ("overlap above S", dict(ov=4), fs),
                          ("overlap above S_prev", dict(ov=3, S_prev=2), fs), ("S > 1 without frame_se3", dict(ov=1), None),
                          ("H = 0", dict(ov=1, hw=(0, 518)), fs), ("H < 0", dict(ov=1, hw=(-2, 518)), fs)):
        rc, out, pt = _pose_call(N, cs, fs_, cam, ctx, None, kw["ov"], kw.get("hw", HW), S_prev=kw.get("S_prev"))
        if rc != ERR_SHAPE or not (out.intact() and pt.intact()) or float(out.get()[0][0]) != SENT:
            errs.append(f"pose_compose {name}: returned {rc} or wrote its outputs")
    cs, fs, cam, ctx = _pose_inputs(_gen(42), 1, 66, 66, False)
    rc, out, pt = _pose_call(N, cs, fs, cam, ctx, None, 65, HW)
    if rc != ERR_SHAPE or float(out.get()[0][0]) != SENT:
        errs.append(f"pose_compose overlap 65: returned {rc}")
    P = Blocks([torch.randn(4, 3)], fill=SENT)
    T = torch.eye(4).view(1, 4, 4).to(DEV)
    one = torch.ones(1, device=DEV)
    for name, B_, n_, want in (("B=0", 0, 4, ERR_SHAPE), ("B=-1", -1, 4, ERR_SHAPE), ("n=-1", 1, -1, ERR_SHAPE), ("n=0", 1, 0, OK)):
        Oo = _out(1, 12)
        rc = L.vggt_sim3_points(P.ptr, 12, B_, n_, ctypes.c_void_p(T.data_ptr()), None, Oo.ptr, 12, _stream())
        X = _out(1, 12)
        rc2 = L.vggt_scale_f32(X.ptr, 12, B_, n_, ctypes.c_void_p(one.data_ptr()), _stream())
        _sync()
        if rc != want or rc2 != want:
            errs.append(f"sim3_points / scale_f32 {name}: returned {rc} / {rc2}, want {want}")
        if float(Oo.get()[0][0]) != SENT or float(X.get()[0][0]) != SENT or not (Oo.intact() and X.intact()):
            errs.append(f"sim3_points / scale_f32 {name}: wrote something")
    _sync()
    for o in (Ro, to, so):
        if not o.intact() or float(o.get()[0][0]) != SENT:
            errs.append("irls error paths wrote an output")
    _done(errs)


def test_figures():
    """Not a check: prints the figures the tests above gathered (DESIGN.md tabulates them)."""
    _figures("")
