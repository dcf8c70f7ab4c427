"""Helpers shared by the fp64 edge files (test_gpu_norm_edges.py, test_gpu_small_edges.py): the
boxes, bit comparisons and comparison rules of test_gpu_train_edges.py, whose docstring derives
them.  A plain module: no tests, no fixtures.

  Box          a host tensor inside a larger buffer: inputs NaN around the window, outputs a sentinel
               that must be intact bit for bit afterwards
  _eq_bits     bit for bit (the exact and the one-operation rules)
  _within      |got - ref| <= bound per element, returns the worst error / bound
  _interval    odtype(s - E) <= got <= odtype(s + E), returns the worst |got - s| / (E + half an
               output ulp for bf16)
  _model_rule  the kernel's worst row (||got - ref64||_2 over the RMS row norm of ref64) must be
               <= 2 x that of the documented fp32 arithmetic restated in plain torch on the host
  _svd_centres, _centre_poses, _svd_pair_check
               one 3x3 Umeyama problem for the two kernels that share csrc/small_eig.h's SVD
               (test_gpu_geometry_edges.py, test_gpu_training_metrics.py)
u = 2^-24, gamma_n = n u / (1 - n u)."""
import math

import pytest
import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SENT = 7.0
U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=F32))
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4


def _gam(n):
    return n * U / (1 - n * U)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _dtn(dt):
    return "bf16" if dt == BF else "f32"


def _bits(x):
    if x.dtype in (torch.int16, torch.int32):
        return x.contiguous()
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


class Box:
    """A 2-D host tensor inside a larger buffer filled with `fill`: `rows` extra rows before /
    after, `cols` extra columns left / right (multiples of 8 elements, so the window keeps its
    16-B alignment)."""

    def __init__(self, x, fill, rows=(2, 3), cols=(8, 16)):
        M, C = x.shape
        self.host = torch.full((M + rows[0] + rows[1], C + cols[0] + cols[1]), fill, dtype=x.dtype)
        self.win = (rows[0], rows[0] + M, cols[0], cols[0] + C)
        self.host[rows[0]:rows[0] + M, cols[0]:cols[0] + C] = x
        self.dev = self.host.cuda()

    @property
    def v(self):
        r0, r1, c0, c1 = self.win
        return self.dev[r0:r1, c0:c1]

    def got(self):
        return self.v.cpu()

    def intact(self, keep=None):
        """Everything outside the window (or, with `keep`, outside that boolean mask over the
        whole buffer of elements the kernel may write) holds its original bits."""
        a, b = _bits(self.dev.cpu()).clone(), _bits(self.host).clone()
        if keep is None:
            r0, r1, c0, c1 = self.win
            a[r0:r1, c0:c1] = 0
            b[r0:r1, c0:c1] = 0
        else:
            a[keep] = 0
            b[keep] = 0
        return torch.equal(a, b)


def _first(bad, *vals):
    idx = bad.nonzero()[:4].tolist()
    return "%d of %d, first %s" % (int(bad.sum()), bad.numel(),
                                   [(tuple(i),) + tuple(float(v[tuple(i)]) for v in vals) for i in idx])


def _eq_bits(errs, name, got, ref):
    if got.dtype != ref.dtype or got.shape != ref.shape:
        errs.append(f"{name}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}")
        return
    bad = _bits(got) != _bits(ref)
    if bool(bad.any()):
        errs.append(f"{name} not bitwise: " + _first(bad, got, ref))


def _interval(errs, name, got, s, E):
    lo, hi = (s - E).to(got.dtype), (s + E).to(got.dtype)
    bad = ~torch.isfinite(got) | (got < lo) | (got > hi)
    if bool(bad.any()):
        errs.append(f"{name} outside its interval: " + _first(bad, got, lo, hi))
    Eo = E + _half_ulp(s, got.dtype)  # the printed ratio counts a bf16 output's own rounding
    w = ((got.double() - s).abs() / Eo.clamp_min(1e-300))[E > 0]
    return float(w.max()) if w.numel() else 0.0


def _within(errs, name, got, ref, bound):
    err = (got.double() - ref).abs()
    bad = ~torch.isfinite(got) | (err > bound)
    if bool(bad.any()):
        errs.append(f"{name} beyond its bound: " + _first(bad, got, ref, bound))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def _half_ulp(ref, dt):
    """Half a unit in the last place of `dt` at |ref| (fp64 tensor); 0 for fp32 outputs, whose
    rounding is inside the derived bounds."""
    if dt != BF:
        return torch.zeros_like(ref)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))).clamp_min(-126)
    return torch.pow(2.0, e - 8)


def _row_err(t, ref):
    """Per row (last dim) ||t - ref||_2 over the RMS row norm of ref."""
    rn = ref.norm(dim=-1)
    rms = float(rn.pow(2).mean().sqrt())
    return (t.double() - ref).norm(dim=-1) / (rms if rms > 0 else 1.0)


FIG = {}


def _fig(key, value):
    FIG[key] = max(FIG.get(key, 0.0), value) if isinstance(value, float) else value


def _model_rule(errs, name, got, model, ref, tag):
    """The kernel's worst row must be within 2 x the fp32 model's worst row; prints kernel, model
    and ratio, and keeps the worst ratio per `tag` in FIG."""
    if not bool(torch.isfinite(got.float()).all()):
        errs.append(f"{name}: non-finite output")
        return
    eg, em = _row_err(got, ref), _row_err(model, ref)
    wg, wm = float(eg.max()), float(em.max())
    ratio = wg / wm if wm > 0 else (0.0 if wg == 0 else math.inf)
    print(f"model {name}: kernel {wg:.3e} model {wm:.3e} ratio {ratio:.2f}")
    old = FIG.get(("model", tag), (0.0, 0.0, -1.0))
    if ratio >= old[2]:
        FIG[("model", tag)] = (wg, wm, ratio)
    if wg > 2 * wm:
        i = int(eg.reshape(-1).argmax())
        errs.append(f"{name}: kernel worst row {wg:.3e} > 2 x model {wm:.3e} (row {i} of {tuple(eg.shape)})")


def _done(errs, *reach):
    for r in reach:
        print("reach", r)
    assert not errs, "\n".join(errs[:40])


def _raises(code, fn, *a, **k):
    with pytest.raises(RuntimeError, match=r"\(code %d\)" % code):
        fn(*a, **k)


def _figures(prefix):
    """Print the figures gathered so far whose tag starts with `prefix` (the last test of a file)."""
    for k in sorted(FIG, key=str):
        if str(k[-1]).startswith(prefix) or str(k[0]).startswith(prefix):
            print("figure", k, FIG[k])


# ------------------------------------------------------------------ one 3x3 problem for the two users of the shared SVD
def _umeyama_torch(x, y, dt):
    """Umeyama's closed form with unit weights on centres x -> y [n, 3] in `dt` arithmetic with LAPACK's SVD
    (fp64: the reference, fp32: the model): R, t, c."""
    x, y = x.to(dt), y.to(dt)
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    Uu, sv, Vh = torch.linalg.svd(yc.T @ xc / x.shape[0])
    D = torch.tensor([1.0, 1.0, -1.0 if float(torch.det(Uu @ Vh)) < 0 else 1.0], dtype=dt)
    R = Uu @ torch.diag(D) @ Vh
    c = (sv * D).sum() / (xc ** 2).sum(1).mean()
    return R, my - c * (R @ mx), c


def _svd_centres(kind):
    """Camera centres x -> y (fp32 [S, 3]) that vggt_irls_sim3 takes as a point cloud with unit weights and
    vggt_gt_pose_align as poses (_centre_poses), so that both solve the same 3x3 problem.
      general  S = 5 in general position (spreads 3 : 2 : 1), y = 1.7 R0 x + t0 + noise.  The seed is chosen from the
               host alone: the fp32 model's error is at least 3 x one fp32 rounding of the fp64 result on R, t and c,
               so the 2 x model rule is not decided by a model that happens to be exact.
      line     S = 3 collinear (rank 1), every number exact in fp32: y = 2 R0 x + t0 with R0 a quarter turn about z."""
    if kind == "line":
        x = torch.tensor([0.5, -0.25, 6.0]) + torch.tensor([[-1.5], [0.25], [2.0]]) * torch.tensor([1.0, -2.0, 2.0])
        R0 = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        return x, 2.0 * x @ R0.T + torch.tensor([0.5, -1.0, 2.0])
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(5, 3, generator=g, dtype=F64) * torch.tensor([3.0, 2.0, 1.0], dtype=F64)).float()
    i, j, k, r = (torch.tensor([0.3, -0.2, 0.5, 0.8], dtype=F64) / math.sqrt(1.02)).tolist()
    R0 = torch.tensor([[1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r)],
                       [2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r)],
                       [2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)]], dtype=F64)
    y = 1.7 * x.double() @ R0.T + torch.tensor([0.4, -1.0, 2.0], dtype=F64) + 0.05 * torch.randn(5, 3, generator=g, dtype=F64)
    return x, y.float()


def _centre_poses(x, y):
    """(pose_enc (1, S, 9), gt_extr (1, S, 3, 4)) whose camera centres -R^T t are exactly x and y: identity rotations
    (the quaternion (0, 0, 0, 1) gives R = I exactly), t = -centre."""
    S = x.shape[0]
    enc = torch.cat([-x, torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]).expand(S, 6)], -1)
    extr = torch.cat([torch.eye(3).expand(S, 3, 3), -y[..., None]], -1)
    return enc[None].contiguous(), extr[None].contiguous()


def _svd_pair_check(errs, who, kind, R, t, c):
    """One user's R [3, 3], t [3], c [] (host fp32) on _svd_centres(kind).  general: _model_rule against the one fp64
    solve.  line: the rotation about the line is free, so R is a proper rotation (det = 1 and R^T R = I within 1e-6:
    the fp32 rounding of an orthogonal matrix moves them by at most 6 u and 4 u) that maps the line onto the line
    (R d = R0 d within 1e-6: the rounding of R moves R d by at most sqrt(3) u), and c = 2 within 2 u c."""
    x, y = _svd_centres(kind)
    if kind == "general":
        Rr, tr, cr = _umeyama_torch(x, y, F64)
        Rm, tm, cm = _umeyama_torch(x, y, F32)
        _model_rule(errs, f"{who} R", R, Rm, Rr, "svd_pair")
        _model_rule(errs, f"{who} t", t.reshape(1, 3), tm.reshape(1, 3), tr.reshape(1, 3), "svd_pair")
        _model_rule(errs, f"{who} c", c.reshape(1, 1), cm.reshape(1, 1), cr.reshape(1, 1), "svd_pair")
        return
    Rd = R.double()
    d = torch.tensor([1.0, -2.0, 2.0], dtype=F64) / 3.0
    figures = {"det": (abs(float(torch.det(Rd)) - 1.0), 1e-6),
               "RtR": (float((Rd.T @ Rd - torch.eye(3, dtype=F64)).abs().max()), 1e-6),
               "line": (float((Rd @ d - torch.tensor([2.0, 1.0, 2.0], dtype=F64) / 3.0).abs().max()), 1e-6),
               "c": (abs(float(c) - 2.0), 4 * U)}
    print(f"svd pair {who} {kind}: {figures}")
    for name, (v, bound) in figures.items():
        if not v <= bound:
            errs.append(f"{who} {kind}: {name} {v:.3e} > {bound:.3e}")


# ------------------------------------------------------------------ dense outputs between sentinel guards
def _guarded(shape, dt, fill=SENT, guard=64):
    n = math.prod(shape)
    buf = torch.full((n + 2 * guard,), fill, dtype=dt, device="cuda")
    return buf, buf[guard:guard + n].view(*shape)


def _guards_ok(buf, n, fill=SENT, guard=64):
    h = buf.cpu()
    ref = torch.full((guard,), fill, dtype=buf.dtype)
    return torch.equal(_bits(h[:guard]), _bits(ref)) and torch.equal(_bits(h[guard + n:]), _bits(ref))


# ------------------------------------------------------------------ per-head norm + RoPE on the host
TAB = 11
POS = {1: [-3, 4, TAB + 5], 2: [[-3, 2], [7, TAB + 5], [0, 10]]}  # period 3


def _tables(rd, g):
    ang = torch.arange(TAB, dtype=F32)[:, None] * (100.0 ** (-torch.arange(rd // 2, dtype=F32) / (rd // 2)))[None]
    ang = torch.cat([ang, ang], -1)
    return torch.cos(ang).contiguous(), torch.sin(ang).contiguous()


def _hn_host(x, D, nh, hsplit, w0, b0, w1, b1, mode, cos, sin, dt_calc, period=3):
    """x [M, nh * D] -> normalised + rotated [M, nh, D] in `dt_calc` arithmetic (fp32: the model,
    restating hn_affine / hn_rotate without the fused multiply-adds; fp64: the reference)."""
    M = x.shape[0]
    v = x.to(dt_calc).reshape(M, nh, D)
    if w0 is not None:
        inv = torch.tensor(1.0 / D, dtype=F32).to(dt_calc) if dt_calc == F32 else 1.0 / D
        mean = v.sum(-1, keepdim=True) * inv
        d = v - mean
        q = (d * d).sum(-1, keepdim=True) * inv + EPS
        rstd = torch.rsqrt(q) if dt_calc == F32 else 1.0 / torch.sqrt(q)
        W = torch.stack([w0 if h < hsplit else w1 for h in range(nh)]).to(dt_calc)
        z = torch.zeros(D)
        Bv = torch.stack([(b0 if b0 is not None else z) if h < hsplit else (b1 if b1 is not None else z)
                          for h in range(nh)]).to(dt_calc)
        v = d * rstd * W + Bv
    if mode:
        rd = D // 2 if mode == 1 else D
        pos = torch.tensor(POS[1 if mode == 2 else 2]).clamp(0, TAB - 1)
        out = torch.empty_like(v)
        for m in range(M):
            pr = m % period
            for blk in range(D // rd):
                p = int(pos[pr][blk]) if mode == 1 else int(pos[pr])
                c, s = cos[p].to(dt_calc), sin[p].to(dt_calc)
                xb = v[m, :, blk * rd:(blk + 1) * rd]
                rot = torch.cat([-xb[:, rd // 2:], xb[:, :rd // 2]], -1)
                out[m, :, blk * rd:(blk + 1) * rd] = xb * c + rot * s
        v = out
    return v


HN_CFG = [("wb", 0), ("wb", 1), ("wb", 2), ("w", 1), ("w", 2), ("none", 1), ("none", 2)]


def _hn_args(mode, D, g):
    if not mode:
        return (0, None, 1, None, None), None, None
    rd = D // 2 if mode == 1 else D
    cos, sin = _tables(rd, g)
    pos = torch.tensor(POS[1 if mode == 2 else 2], dtype=torch.int32).cuda()
    return (mode, pos, 3, cos.cuda(), sin.cuda()), cos, sin
