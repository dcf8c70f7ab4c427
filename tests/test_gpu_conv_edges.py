"""The DPT convolution family (vggt_conv2d_f32, vggt_conv2d_bf16x3 with the two-deep and the one-deep
gather, vggt_conv2d_bf16x3_pre, vggt_conv2d_upsample_bf16x3) and its element-wise kernels
(vggt_upsample_bilinear_*, vggt_split_act_bf16x2 / vggt_split_bf16x2, vggt_dpt_activate) per element
against fp64 on the host, at the edges of their tiles.

Inputs are drawn on the host from seeded torch.Generators; references are fp64 on the host, computed once
per case and left unchanged.  Every case is small (M <= a few hundred pixels, ci, co <= 160).

Layout of every part 1 / part 2 launch ("poison and sentinels"): x (or x_hi / x_lo) is a column slice of a
wider buffer (ldx = ci + 8 at column 4 for f32, ci + 16 at column 8 for the bf16 halves) whose other
columns hold NaN, with three whole NaN rows before the first and after the last pixel; y, y_hi / y_lo,
res1 and res2 are column slices with pairwise different leading dimensions (co + 3, co + 5, co + 1,
co + 7) of buffers whose gaps and guard rows hold a sentinel that must be unchanged afterwards; weight
rows beyond co' are zero up to a multiple of 128.  Out-of-image taps and rows past M must read zeros
(the pre form's LDS-DMA and the two-deep gather's buffer loads rely on an out-of-range offset for
that): a NaN that leaks in shows in the output.

Which kernel a case reaches: conv2d_f32 -> conv_f32_kernel (128 x 64 tiles); conv2d_bf16x3 ->
conv_bf16x3_kernel<BNX, PF2> and conv2d_bf16x3_pre -> conv_pre_kernel<BNX> with BNX = 128 for
ncols >= 128, 64 for 32 < ncols < 128, 32 for ncols <= 32; PF2 = VGGT_TUNE_CONV_PF2 (two-deep gather with
its 1 / 2 / 3-step tail: nk = kh*kw*ci/32 odd and >= 3 takes the 3-step one).  `_reach` asks the library
(vggt_conv_form) and adds the tail.

Tolerances (none is a measured constant, except dpt_activate's device function error, see `ulp`):
  exact     part 1 / part 3 inputs: x = s (m + q 2^-10), s = +-1, m in {1, 2}, q in {0..3}, ~10 % zeros,
            so hi = bf16(x) = s m and lo = bf16(x - hi) = s q 2^-10 reproduce x; weights alike; bias, pos,
            res1, res2 multiples of 2^-10 in [-2, 2].  Every term of hi.hi + hi.lo + lo.hi and every
            epilogue operand is a multiple of 2^-10 and the sum of their magnitudes stays below 2^14, so
            every partial sum in any order is exact in fp32 and the documented three-term result is
            unique: outputs are compared bit for bit with the fp64 three-term sum (the dropped lo.lo
            term, ~1e-4, and any missing tap or half would show).  conv2d_f32 gets the low part at 2^-4
            (products multiples of 2^-8, the reference the full product).  Both preconditions (the split
            reproduces x and w; sum |terms| * 2^10 < 2^24) are asserted on the host per case.  Split
            outputs: y_hi = bf16(v), y_lo = bf16(v - y_hi) of the reference v (max(v, 0) with split_relu).
  interval  part 2: with s the fp64 three-term sum of the split operands the kernel sees plus the
            epilogue operands, any fp32 evaluation order stays within
              (3K + 2 + e) 2^-24 (sum (|xh| + |xl|)(|wh| + |wl|) + |bias| + |pos| + |res1| + |res2|)
            (e epilogue additions; products of bf16 values are exact in fp32); for conv2d_f32
            (K + 2 + e) 2^-24 (sum |x||w| + ...) against the full fp64 product.
  bitwise   pre == bf16x3 (PF2 = 1) == bf16x3 (PF2 = 0) on every part 1 and part 2 case; fused resize +
            conv == upsample_bilinear_split_sep followed by conv2d_bf16x3_pre on every part 3 shape (both
            kernels take the resize arithmetic from common.h bl_*); split halves == split of the y the
            same launch wrote; identity resize == input; the separable table form == the full table form.
  resize    part 4, against the fp64 bilinear interpolation at the exact rational source coordinates
            (oy (hi-1)/(ho-1), ox (wi-1)/(wo-1)).  The kernel's scale is one fp32 rounding of the quotient
            and its fraction one fused rounding of scale * o - floor, so its coordinate is within
            2^-24 (hi-1) + 2^-25 of the exact one; the interpolant is continuous and piecewise linear with
            slope at most Ly = max |x[r+1] - x[r]| (per image and channel; Lx alike), and a coordinate
            that lands in the neighbouring cell adds the same again, so the coordinate error moves the
            result by at most T = dy Ly + dx Lx with dy = (2 (hi-1) + 1) 2^-24 (0 for hi = 1), dx alike.
            The lerp itself is 1 - l (one rounding), two products and three fused multiply-adds
            on values bounded by V = max |x| (per image and channel), the table add one more rounding:
              |got - ref| <= T + 7 2^-24 (V + |pos|).
  fused     part 3 on the shapes that are not exact: u = the fp64 resize at the kernel's fp32 coordinates
            (restated on the host: correctly rounded division, product, fused fraction) + table, so only
            the lerp roundings remain, E = 7 2^-24 (V + |pos|); the kernel's split (uh', ul') of its
            u' = u + d, |d| <= E, has |uh' + ul' - u| <= E + 2^-17 (|u| + E) and |uh' - u| <= E +
            2^-9 (|u| + E), so against s = sum u (wh + wl) + bias (fp64)
              |got - s| <= sum [(E + 2^-17 (|u| + E)) |wh| + (E + 2^-9 (|u| + E)) |wl|]
                           + (3K + 3) 2^-24 (sum (1 + 2^-8)(|u| + E)(|wh| + |wl|) + |bias|).
  ulp       dpt_activate: the ROCm install carries no HIP math accuracy table, so the device expf /
            expm1f errors were measured once through the kernel (scale = NULL) on the grid below against
            fp64, in ulps of the fp32 value of the fp64 result: expf 0.413, expm1f 0.692.  TOL_FN is
            2 x measured: 0.83 (act 0 and the confidence's exp) and 1.39 (act 1).  With a scale the
            function's TOL_FN ulp(a) |scale| is carried through the multiply and the multiply's own rounding
            (half an ulp of the product) added; conf = 1 + exp(c) likewise with the add's rounding.  An
            exp(x) - 1 implementation misses the bar at |x| <= 1e-4 by more than 100 x (checked on the
            host with the fp32 restatement).
DESIGN.md (DPT convolution edge tests) tabulates what was measured."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
SENT = -1.5e30  # sentinel of every element a launch must not write (compared as bits)
U24 = 2.0 ** -24
TOL_FN = {0: 0.83, 1: 1.39}  # act -> ulps: 2 x the measured device expf / expm1f error (docstring)
VGGT_ERR_SHAPE, VGGT_ERR_ALIGN, VGGT_ERR_UNSUPPORTED = -1, -2, -4
FORMS = ["f32", "pf2", "pf1", "pre"]


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------ cases: nimg, hi, wi, ci, co, kh, kw, stride, pad[, shuffle]
GEOM = {
    "g1_m1": (1, 1, 1, 32, 1, 1, 1, 1, 0),
    "g2_centre_tap": (2, 1, 1, 32, 5, 3, 3, 1, 1),
    "g3_nk9": (2, 5, 7, 32, 33, 3, 3, 1, 1),
    "g4_m132_nk27": (1, 11, 12, 96, 64, 3, 3, 1, 1),
    "g5_three_images": (3, 5, 10, 64, 40, 3, 3, 1, 1),
    "g6_s2_even": (2, 8, 10, 64, 40, 3, 3, 2, 1),
    "g6_s2_odd": (2, 9, 7, 64, 40, 3, 3, 2, 1),
    "g7_ci64": (1, 3, 43, 64, 130, 1, 1, 1, 0),
    "g7_ci96": (1, 3, 43, 96, 130, 1, 1, 1, 0),
    "g7_ci128": (1, 3, 43, 128, 130, 1, 1, 1, 0),
    "g7_ci160": (1, 3, 43, 160, 130, 1, 1, 1, 0),
    "g8_1x3": (1, 4, 6, 32, 16, 1, 3, 1, 1),
    "g8_3x1": (1, 6, 4, 32, 16, 3, 1, 1, 1),
    "g9_valid": (2, 5, 7, 32, 33, 3, 3, 1, 0),
    "g9_pad2": (2, 5, 7, 32, 33, 3, 3, 1, 2),
    "g10_stride3": (2, 5, 7, 32, 33, 1, 1, 3, 0),
    **{f"g11_co{co}": (1, 3, 5, 32, co, 1, 1, 1, 0) for co in (31, 32, 33, 64, 65, 127, 128, 129)},
    "g12_s2_co24": (2, 3, 5, 32, 24, 1, 1, 1, 0, 2),
    "g12_s4_co8": (2, 3, 5, 32, 8, 1, 1, 1, 0, 4),
    "g12_s2_co40": (2, 3, 5, 32, 40, 1, 1, 1, 0, 2),
    "g12_s3_co16": (2, 3, 5, 32, 16, 1, 1, 1, 0, 3),
    "g13_nk2_co16": (1, 4, 6, 64, 16, 1, 1, 1, 0),  # the 2-step tail on the 32-wide N tile
}
EPI_GEOMS = ["g3_nk9", "g4_m132_nk27", "g5_three_images"]
# epilogue combinations: (bias, relu_in, relu_out, pos, res1, res1_relu, res2)
EPI = {
    "bias": (1, 0, 0, 0, 0, 0, 0),
    "nobias": (0, 0, 0, 0, 0, 0, 0),
    "relu_in": (1, 1, 0, 0, 0, 0, 0),
    "relu_out_pos_res1relu_res2": (1, 0, 1, 1, 1, 1, 1),
    "relu_out_pos_res1": (1, 0, 1, 1, 1, 0, 0),
    "rcu": (1, 1, 1, 0, 1, 0, 0),
}
RANDOM_GEOMS = ["g3_nk9", "g4_m132_nk27", "g5_three_images", "g7_ci64", "g7_ci96", "g7_ci128", "g7_ci160",
                "g12_s2_co40"]


def _geom(name):
    g = GEOM[name]
    nimg, hi, wi, ci, co, kh, kw, stride, pad = g[:9]
    sh = g[9] if len(g) > 9 else 0
    ho, wo = (hi + 2 * pad - kh) // stride + 1, (wi + 2 * pad - kw) // stride + 1
    return dict(nimg=nimg, hi=hi, wi=wi, ci=ci, co=co, kh=kh, kw=kw, stride=stride, pad=pad, shuffle=sh, ho=ho, wo=wo,
                M=nimg * ho * wo, K=kh * kw * ci, ncols=sh * sh * co if sh else co,
                orows=nimg * ho * wo * (sh * sh if sh else 1))


def _reach(g, form):
    """The kernel a form launches for a geometry: the library's own answer (vggt_conv_form, host arithmetic,
    which tests/test_conv_form.py pins to the dispatch rules), plus the tail of the two-deep gather's K loop,
    which is this test's knowledge of nk."""
    from aligned_vggt import _native as Nat
    entry = {"f32": Nat.CONV_ENTRY_F32, "pre": Nat.CONV_ENTRY_PRE}.get(form, Nat.CONV_ENTRY_BF16X3)
    prev = Nat.tune(Nat.TUNE_CONV_PF2, 0 if form == "pf1" else 1)
    try:
        f = Nat.conv_form(entry, g["nimg"], g["hi"], g["wi"], g["ci"], g["co"], g["kh"], g["kw"], g["stride"], g["pad"],
                          g["shuffle"])
    finally:
        Nat.tune(Nat.TUNE_CONV_PF2, prev)
    assert f["rc"] == 0, (g, form, f)
    nk = g["K"] // 32
    tail = "" if form != "pf2" else f", {3 if nk % 2 and nk >= 3 else 2 if nk % 2 == 0 else 1}-step tail"
    return f["name"] + tail


def test_cases_reach_every_path():
    """The geometries reach every N tile width, the 1-, 2- and 3-step tails of the two-deep gather, a
    second M tile, and fragments that straddle a pixel-shuffle tap."""
    gs = {k: _geom(k) for k in GEOM}
    seen = {_reach(g, f) for g in gs.values() for f in FORMS}
    for bnx in (32, 64, 128):
        assert f"conv_pre_kernel<{bnx}>" in seen and f"conv_bf16x3_kernel<{bnx}, false>" in seen
        for t in (1, 2, 3):
            assert f"conv_bf16x3_kernel<{bnx}, true>, {t}-step tail" in seen, (bnx, t)
    assert any(g["M"] > 128 for g in gs.values()) and any(g["M"] == 1 for g in gs.values())
    assert any(g["shuffle"] and any((16 * f) // g["co"] != (16 * f + 15) // g["co"] for f in range(g["ncols"] // 16))
               for g in gs.values())


# ------------------------------------------------------------------ bits
def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _split(x):
    """The documented split of an fp32 tensor: hi = bf16(x), lo = bf16(x - hi) (RNE, fp32 subtraction)."""
    x = x.float()
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


def _first_bad(bad):
    return f"{int(bad.sum())} of {bad.numel()} elements, first at {tuple(bad.nonzero()[0].tolist())}"


# ------------------------------------------------------------------ host side: inputs and fp64 references
_HOST = {}


def _draw_exact(g, shape, low):
    """s (m + q low), s = +-1, m in {1, 2}, q in {0..3}, ~10 % exact zeros."""
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    m = torch.randint(1, 3, shape, generator=g).double()
    q = torch.randint(0, 4, shape, generator=g).double()
    keep = (torch.rand(shape, generator=g) >= 0.1).double()
    return (s * (m + q * low) * keep).float()


def _draw_grid(g, shape):
    """Multiples of 2^-10 in [-2, 2] (epilogue operands)."""
    return (torch.randint(-2048, 2049, shape, generator=g).double() / 1024).float()


def _im2col(x, g):
    """[nimg*hi*wi, ci] -> [M, kh*kw*ci] in the (ky, kx, ci) K order, zeros outside the image."""
    x4 = x.reshape(g["nimg"], g["hi"], g["wi"], g["ci"])
    p, s = g["pad"], g["stride"]
    xp = F.pad(x4, (0, 0, p, p, p, p))
    cols = [xp[:, ky:ky + (g["ho"] - 1) * s + 1:s, kx:kx + (g["wo"] - 1) * s + 1:s, :]
            for ky in range(g["kh"]) for kx in range(g["kw"])]
    return torch.cat(cols, -1).reshape(g["M"], g["K"])


def _epilogue(g, acc, cs, ep):
    """fp64 epilogue of the GEMM result acc [M, ncols] -> output rows [orows, co]; also sum |operands|."""
    bias, _, relu_out, pos, res1, res1_relu, res2 = ep
    co = g["co"]
    mag = torch.zeros_like(acc)
    if g["shuffle"]:
        s = g["shuffle"]
        v = acc.reshape(g["nimg"], g["ho"], g["wo"], s, s, co)
        if bias:
            v = v + cs["bias"].double()
            mag = mag + cs["bias"].double().abs().repeat(s * s)
        if relu_out:
            v = v.clamp_min(0)
        v = v.permute(0, 1, 3, 2, 4, 5).reshape(g["orows"], co)
        mag = mag.reshape(g["nimg"], g["ho"], g["wo"], s, s, co).permute(0, 1, 3, 2, 4, 5).reshape(g["orows"], co)
        return v, mag
    v = acc
    if bias:
        v = v + cs["bias"].double()
        mag = mag + cs["bias"].double().abs()
    if relu_out:
        v = v.clamp_min(0)
    if pos:
        v = v + cs["pos"].double().repeat(g["nimg"], 1)
        mag = mag + cs["pos"].double().abs().repeat(g["nimg"], 1)
    if res1:
        r = cs["res1"].double()
        v = v + (r.clamp_min(0) if res1_relu else r)
        mag = mag + r.abs()
    if res2:
        v = v + cs["res2"].double()
        mag = mag + cs["res2"].double().abs()
    return v, mag


def _conv_case(name, kind):
    """Inputs of one geometry.  kind: "split" (exact, low part 2^-10), "f32" (exact, low part 2^-4), "random"."""
    key = (name, kind)
    if key in _HOST:
        return _HOST[key]
    g = _geom(name)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + {"split": 1, "f32": 2, "random": 3}[kind])
    npix = g["nimg"] * g["hi"] * g["wi"]
    if kind == "random":
        x = torch.randn(npix, g["ci"], generator=gen)
        w = torch.randn(g["ncols"], g["K"], generator=gen) * g["K"] ** -0.5
        bias = torch.randn(g["co"], generator=gen)
        pos, res1, res2 = (torch.randn(r, g["co"], generator=gen) for r in (g["ho"] * g["wo"], g["M"], g["M"]))
    else:
        low = 2.0 ** -10 if kind == "split" else 2.0 ** -4
        x = _draw_exact(gen, (npix, g["ci"]), low)
        w = _draw_exact(gen, (g["ncols"], g["K"]), low)
        bias = _draw_grid(gen, (g["co"],))
        pos, res1, res2 = (_draw_grid(gen, (r, g["co"])) for r in (g["ho"] * g["wo"], g["M"], g["M"]))
    cs = dict(g=g, name=name, kind=kind, x=x, w=w, bias=bias, pos=pos, res1=res1, res2=res2, refs={})
    cs["wh"], cs["wl"] = _split(w)
    if kind == "split":  # precondition: the split reproduces the operands
        assert torch.equal(cs["wh"].double() + cs["wl"].double(), w.double())
        for xx in (x, x.clamp_min(0)):
            xh, xl = _split(xx)
            assert torch.equal(xh.double() + xl.double(), xx.double())
    _HOST[key] = cs
    return cs


def _conv_ref(cs, ep, f32):
    """(v, bound) per output element: the fp64 reference of the documented arithmetic and, for random
    inputs, the derived fp32 interval; for exact inputs the precondition of uniqueness is asserted."""
    key = (ep, f32)
    if key in cs["refs"]:
        return cs["refs"][key]
    g = cs["g"]
    xin = cs["x"].clamp_min(0) if ep[1] else cs["x"]
    if f32:
        a, w = _im2col(xin.double(), g), cs["w"].double()
        acc, mag = a @ w.t(), a.abs() @ w.abs().t()
        nterm = g["K"]
    else:
        xh, xl = _split(xin)
        ah, al = _im2col(xh.double(), g), _im2col(xl.double(), g)
        wh, wl = cs["wh"].double(), cs["wl"].double()
        acc = ah @ wh.t() + ah @ wl.t() + al @ wh.t()
        nterm = 3 * g["K"]
        if cs["kind"] == "random":
            mag = (ah.abs() + al.abs()) @ (wh.abs() + wl.abs()).t()
        else:
            mag = ah.abs() @ wh.abs().t() + ah.abs() @ wl.abs().t() + al.abs() @ wh.abs().t()
    v, emag = _epilogue(g, acc, cs, ep)
    if g["shuffle"]:
        s = g["shuffle"]
        mag = mag.reshape(g["nimg"], g["ho"], g["wo"], s, s, g["co"]).permute(0, 1, 3, 2, 4, 5).reshape(g["orows"], g["co"])
    e = sum(ep[i] for i in (0, 3, 4, 6))
    if cs["kind"] == "random":
        bound = (nterm + 2 + e) * U24 * (mag + emag)
    else:  # precondition: every partial sum is an exact fp32 multiple of 2^-10
        assert float((mag + emag).max()) * 2 ** 10 < 2 ** 24
        assert torch.equal(v.float().double(), v) and torch.equal((v * 1024).round(), v * 1024)
        bound = None
    cs["refs"][key] = (v, bound)
    return v, bound


# ------------------------------------------------------------------ device side: poisoned inputs, sentinel outputs
def _slot(rows, cols, ld, off, dtype, fill, data=None, guard=3):
    """A [rows, cols] column slice at column off of a [guard + rows + guard, ld] buffer filled with `fill`."""
    buf = torch.full((rows + 2 * guard, ld), fill, dtype=dtype, device="cuda")
    view = buf[guard:guard + rows, off:off + cols]
    if data is not None:
        view.copy_(data.to(dtype))
    return buf, view


def _untouched(buf, view, what):
    """Everything of buf outside view still holds the sentinel's bits."""
    guard = (buf.shape[0] - view.shape[0]) // 2
    off = view.storage_offset() % buf.shape[1]
    b = buf.clone()
    b[guard:guard + view.shape[0], off:off + view.shape[1]] = SENT
    bad = _bits(b) != _bits(torch.full_like(b, SENT))
    assert not bool(bad.any()), f"{what}: sentinel overwritten, {_first_bad(bad.cpu())}"


def _padw(w):
    """Weight rows zero-padded to a multiple of 128 (the header's requirement), on the device."""
    return torch.cat([w, w.new_zeros((-w.shape[0]) % 128, w.shape[1])]).contiguous().cuda()


def _run_conv(Nat, cs, ep, form, want_y=True, want_split=False, split_relu=False):
    """One launch in the poisoned layout; returns (y or None, (y_hi, y_lo) or None) on the host."""
    g = cs["g"]
    bias, relu_in, relu_out, pos, res1, res1_relu, res2 = ep
    ci, co = g["ci"], g["co"]
    npix = g["nimg"] * g["hi"] * g["wi"]
    kw = dict(relu_out=bool(relu_out), res1_relu=bool(res1_relu), shuffle=g["shuffle"])
    kw["pos"] = cs["pos"].cuda() if pos else None
    kw["res1"] = _slot(g["M"], co, co + 1, 1, torch.float32, NAN, cs["res1"])[1] if res1 else None
    kw["res2"] = _slot(g["M"], co, co + 7, 5, torch.float32, NAN, cs["res2"])[1] if res2 else None
    b = cs["bias"].cuda() if bias else None
    ybuf = yv = sbufs = svs = None
    if want_y:
        ybuf, yv = _slot(g["orows"], co, co + 3, 2, torch.float32, SENT)
    if want_split:
        sbufs, svs = zip(*(_slot(g["orows"], co, co + 5, 3, BF, SENT) for _ in range(2)))
    geo = (g["nimg"], g["hi"], g["wi"], ci)
    kgeo = (co, g["kh"], g["kw"], g["stride"], g["pad"])
    if form == "f32":
        _, xv = _slot(npix, ci, ci + 8, 4, torch.float32, NAN, cs["x"])
        Nat.conv2d_f32(xv, *geo, _padw(cs["w"]), b, *kgeo, yv, relu_in=bool(relu_in), **kw)
    elif form == "pre":
        xh, xl = _split(cs["x"].clamp_min(0) if relu_in else cs["x"])
        _, xhv = _slot(npix, ci, ci + 16, 8, BF, NAN, xh)
        _, xlv = _slot(npix, ci, ci + 16, 8, BF, NAN, xl)
        Nat.conv2d_bf16x3_pre(xhv, xlv, *geo, _padw(cs["wh"]), _padw(cs["wl"]), b, *kgeo, yv, y_split=svs,
                              split_relu=split_relu, **kw)
    else:
        _, xv = _slot(npix, ci, ci + 8, 4, torch.float32, NAN, cs["x"])
        prev = Nat.tune(Nat.TUNE_CONV_PF2, 1 if form == "pf2" else 0)
        try:
            Nat.conv2d_bf16x3(xv, *geo, _padw(cs["wh"]), _padw(cs["wl"]), b, *kgeo, yv, relu_in=bool(relu_in), **kw)
        finally:
            Nat.tune(Nat.TUNE_CONV_PF2, prev)
    torch.cuda.synchronize()
    what = f"{cs['name']} {form}"
    if want_y:
        _untouched(ybuf, yv, what + " y")
    if want_split:
        for bb, vv in zip(sbufs, svs):
            _untouched(bb, vv, what + " y_split")
    return (yv.cpu() if want_y else None), (tuple(v.cpu() for v in svs) if want_split else None)


def _assert_exact(what, got, v):
    bad = _bits(got) != _bits(v.float())
    assert not bool(bad.any()), f"{what}: differs from the unique result, {_first_bad(bad)}"


def _assert_split(what, halves, v, split_relu):
    sv = (v.clamp_min(0) if split_relu else v).float()
    hi, lo = _split(sv)
    for nm, got, ref in (("y_hi", halves[0], hi), ("y_lo", halves[1], lo)):
        bad = _bits(got) != _bits(ref)
        assert not bool(bad.any()), f"{what} {nm}: differs from the split of the reference, {_first_bad(bad)}"


# ------------------------------------------------------------------ part 1: exact arithmetic
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(GEOM))
def test_conv_exact(N, name, form):
    """Every geometry on every form, bias epilogue, poisoned layout: bit for bit the unique result."""
    cs = _conv_case(name, "f32" if form == "f32" else "split")
    v, _ = _conv_ref(cs, EPI["bias"], form == "f32")
    y, _ = _run_conv(N, cs, EPI["bias"], form)
    print(f"exact {name} [{_reach(cs['g'], form)}] M {cs['g']['M']} K {cs['g']['K']} ncols {cs['g']['ncols']}")
    _assert_exact(f"{name} {form}", y, v)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("epi", [e for e in EPI if e != "bias"])
@pytest.mark.parametrize("name", EPI_GEOMS)
def test_conv_exact_epilogues(N, name, epi, form):
    """No bias; relu_in; relu_out before pos / res1 (ReLU'd and not) / res2, on cases 3 to 5."""
    cs = _conv_case(name, "f32" if form == "f32" else "split")
    v, _ = _conv_ref(cs, EPI[epi], form == "f32")
    y, _ = _run_conv(N, cs, EPI[epi], form)
    _assert_exact(f"{name} {epi} {form}", y, v)


@pytest.mark.parametrize("sel", ["y", "split", "both", "split_relu", "both_relu", "both_relu_out_split_relu"])
@pytest.mark.parametrize("name", EPI_GEOMS + ["g7_ci96", "g12_s2_co24"])
def test_conv_pre_output_selection(N, name, sel):
    """conv2d_bf16x3_pre writing y only, the split halves only (y = NULL, the DPT head's call), or both;
    split_relu on and off (relu_out off), and split_relu together with relu_out."""
    cs = _conv_case(name, "split")
    shuffle = cs["g"]["shuffle"]
    ep = (1, 0, 1, 0 if shuffle else 1, 0 if shuffle else 1, 1, 0) if sel == "both_relu_out_split_relu" \
        else EPI["bias"] if shuffle else (1, 0, 0, 1, 1, 0, 1)
    v, _ = _conv_ref(cs, ep, False)
    srelu = "relu" in sel
    y, halves = _run_conv(N, cs, ep, "pre", want_y=not sel.startswith("split"), want_split=sel != "y", split_relu=srelu)
    if y is not None:
        _assert_exact(f"{name} {sel}", y, v)
    if halves is not None:
        _assert_split(f"{name} {sel}", halves, v, srelu)


# ------------------------------------------------------------------ part 2: random inputs, derived interval
@pytest.mark.parametrize("name", RANDOM_GEOMS)
def test_conv_random_interval(N, name):
    """Gaussian inputs: every element of every form inside the derived fp32 interval around the fp64 sum;
    pre == bf16x3 (PF2 = 1) == bf16x3 (PF2 = 0) bit for bit, y and the split halves."""
    cs = _conv_case(name, "random")
    ep = EPI["bias"] if cs["g"]["shuffle"] else EPI["relu_out_pos_res1relu_res2"]
    outs = {}
    for form in FORMS:
        v, bound = _conv_ref(cs, ep, form == "f32")
        y, halves = _run_conv(N, cs, ep, form, want_split=form == "pre")
        outs[form] = y
        err = (y.double() - v).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"interval {name} [{_reach(cs['g'], form)}]: worst |got - s| / bound {ratio:.4f}")
        bad = ~(err <= bound)
        assert not bool(bad.any()), f"{name} {form}: outside the interval, {_first_bad(bad)}, worst ratio {ratio}"
        if halves is not None:
            hi, lo = _split(y)
            assert _same(halves[0], hi) and _same(halves[1], lo), f"{name}: split halves != split of y"
    assert _same(outs["pre"], outs["pf2"]), f"{name}: pre != bf16x3 (two-deep gather)"
    assert _same(outs["pf2"], outs["pf1"]), f"{name}: two-deep != one-deep gather"


@pytest.mark.parametrize("name", list(GEOM))
def test_conv_forms_bitwise(N, name):
    """Part 1 inputs with the full epilogue: the three split-bf16 forms give the same bits."""
    cs = _conv_case(name, "split")
    ep = EPI["bias"] if cs["g"]["shuffle"] else EPI["relu_out_pos_res1relu_res2"]
    v, _ = _conv_ref(cs, ep, False)
    outs = {f: _run_conv(N, cs, ep, f)[0] for f in ("pre", "pf2", "pf1")}
    assert _same(outs["pre"], outs["pf2"]) and _same(outs["pf2"], outs["pf1"])
    _assert_exact(name, outs["pre"], v)


def test_conv_deterministic(N):
    cs = _conv_case("g4_m132_nk27", "random")
    ep = EPI["relu_out_pos_res1relu_res2"]
    for form in FORMS:
        a = _run_conv(N, cs, ep, form, want_split=form == "pre")
        b = _run_conv(N, cs, ep, form, want_split=form == "pre")
        assert _same(a[0], b[0]), form
        if a[1] is not None:
            assert _same(a[1][0], b[1][0]) and _same(a[1][1], b[1][1])


# ------------------------------------------------------------------ resize references (parts 3 and 4)
def _coords32(n_in, n_out):
    """The kernel's fp32 source coordinates (common.h bl_coord) restated: i0, l, h per output index."""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    o = np.arange(n_out, dtype=np.float32)
    f = (s * o).astype(np.float32)
    i0 = f.astype(np.int64)
    l = (np.float64(s) * o.astype(np.float64) - i0).astype(np.float32)  # one rounding of the exact s * o - i0
    h = (np.float32(1) - l).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(l.astype(np.float64)), torch.from_numpy(h.astype(np.float64))


def _coords_exact(n_in, n_out):
    o = torch.arange(n_out, dtype=torch.float64)
    f = o * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=torch.float64)
    i0 = f.floor().clamp(max=n_in - 1).long()
    l = f - i0
    return i0, l, 1 - l


def _resize_ref(x, n, hi, wi, C, ho, wo, pos, exact_coords):
    """fp64 bilinear resize (align_corners) of x [n*hi*wi, C] + pos [ho*wo, C] (or None), and the bound on
    the kernel's fp32 result against it (docstring: resize with exact coordinates, fused's E otherwise)."""
    x4 = x.double().reshape(n, hi, wi, C)
    cy, cx = (_coords_exact if exact_coords else _coords32)(hi, ho), (_coords_exact if exact_coords else _coords32)(wi, wo)
    y0, ly, hy = cy
    x0, lx, hx = cx
    y1, x1 = (y0 + 1).clamp(max=hi - 1), (x0 + 1).clamp(max=wi - 1)
    r0, r1 = x4[:, y0], x4[:, y1]
    top = hx[None, None, :, None] * r0[:, :, x0] + lx[None, None, :, None] * r0[:, :, x1]
    bot = hx[None, None, :, None] * r1[:, :, x0] + lx[None, None, :, None] * r1[:, :, x1]
    u = hy[None, :, None, None] * top + ly[None, :, None, None] * bot
    V = x4.abs().amax((1, 2))[:, None, None, :]
    bound = 7 * U24 * V.expand(n, ho, wo, C).clone()
    if pos is not None:
        p = pos.double().reshape(1, ho, wo, C)
        u = u + p
        bound = bound + 7 * U24 * p.abs()
    if exact_coords:
        Ly = (x4[:, 1:] - x4[:, :-1]).abs().amax((1, 2)) if hi > 1 else torch.zeros(n, C, dtype=torch.float64)
        Lx = (x4[:, :, 1:] - x4[:, :, :-1]).abs().amax((1, 2)) if wi > 1 else torch.zeros(n, C, dtype=torch.float64)
        dy = (2 * (hi - 1) + 1) * U24 if hi > 1 else 0.0
        dx = (2 * (wi - 1) + 1) * U24 if wi > 1 else 0.0
        bound = bound + (dy * Ly + dx * Lx)[:, None, None, :]
    return u.reshape(n * ho * wo, C), bound.reshape(n * ho * wo, C)


def _sep_to_full(sep, ho, wo, C):
    """[wo + ho, C/2] separable table -> the [ho*wo, C] table with the same floats."""
    u = sep[:wo][None].expand(ho, wo, C // 2)
    v = sep[wo:][:, None].expand(ho, wo, C // 2)
    return torch.cat([u, v], -1).reshape(ho * wo, C).contiguous()


# ------------------------------------------------------------------ part 3: fused resize + conv
FUSED_SHAPES = [(3, 5, 3, 5, 32, 32), (5, 9, 9, 17, 32, 32), (1, 1, 5, 33, 32, 32), (6, 40, 1, 1, 32, 32),
                (7, 9, 4, 32, 32, 32), (7, 9, 5, 33, 32, 32), (9, 13, 22, 37, 96, 17)]
FUSED_EXACT = FUSED_SHAPES[:2]


def _fused_case(shape, exact):
    key = ("fused", shape, exact)
    if key in _HOST:
        return _HOST[key]
    hi, wi, ho, wo, C, co = shape
    n = 2
    gen = torch.Generator().manual_seed(hi * 1000 + wo * 10 + C + exact)
    K = 9 * C
    if exact:
        # positive x = 4 (m + q 2^-10) and an integer table: every resized value (weights 1, 1/2, 1/4) + table is
        # A + B 2^-10 with A an integer in [4, 10] and B <= 12, so hi = A and lo = B 2^-10 exactly
        x = 4 * (torch.randint(1, 3, (n * hi * wi, C), generator=gen).double()
                 + torch.randint(0, 4, (n * hi * wi, C), generator=gen).double() * 2.0 ** -10).float()
        sep = torch.randint(0, 3, (wo + ho, C // 2), generator=gen).float()
        w = _draw_exact(gen, (co, K), 2.0 ** -10)
        bias = _draw_grid(gen, (co,))
    else:
        x = torch.randn(n * hi * wi, C, generator=gen)
        sep = torch.randn(wo + ho, C // 2, generator=gen) * 0.1
        w = torch.randn(co, K, generator=gen) * K ** -0.5
        bias = torch.randn(co, generator=gen)
    wh, wl = _split(w)
    cs = dict(shape=shape, n=n, x=x, sep=sep, w=w, wh=wh, wl=wl, bias=bias, refs={})
    _HOST[key] = cs
    return cs


def _fused_ref(cs, use_pos, use_bias, exact):
    key = (use_pos, use_bias)
    if key in cs["refs"]:
        return cs["refs"][key]
    hi, wi, ho, wo, C, co = cs["shape"]
    n = cs["n"]
    full = _sep_to_full(cs["sep"], ho, wo, C) if use_pos else None
    u, E = _resize_ref(cs["x"], n, hi, wi, C, ho, wo, full, exact_coords=False)
    g = dict(nimg=n, hi=ho, wi=wo, ci=C, pad=1, stride=1, kh=3, kw=3, ho=ho, wo=wo, M=n * ho * wo, K=9 * C)
    wh, wl = cs["wh"].double(), cs["wl"].double()
    b = cs["bias"].double() if use_bias else torch.zeros(co, dtype=torch.float64)
    if exact:
        uh, ul = _split(u)
        # preconditions: the resized map is an fp32 value that splits exactly, and the sums are exact
        assert torch.equal(u.float().double(), u) and torch.equal(uh.double() + ul.double(), u)
        assert torch.equal(wh + wl, cs["w"].double())
        ah, al = _im2col(uh.double(), g), _im2col(ul.double(), g)
        v = ah @ wh.t() + ah @ wl.t() + al @ wh.t() + b
        mag = ah.abs() @ wh.abs().t() + ah.abs() @ wl.abs().t() + al.abs() @ wh.abs().t() + b.abs()
        assert float(mag.max()) * 2 ** 10 < 2 ** 24 and torch.equal((v * 1024).round(), v * 1024)
        bound = None
    else:
        au, aE = _im2col(u, g), _im2col(E, g)
        am = _im2col(u.abs(), g) + aE
        v = au @ (wh + wl).t() + b
        bound = (aE + 2.0 ** -17 * am) @ wh.abs().t() + (aE + 2.0 ** -9 * am) @ wl.abs().t() \
            + (3 * 9 * C + 3) * U24 * ((1 + 2.0 ** -8) * am @ (wh.abs() + wl.abs()).t() + b.abs())
    cs["refs"][key] = (v, bound)
    return v, bound


def _run_fused(Nat, cs, use_pos, use_bias, sel, relu_out=False, split_relu=False):
    hi, wi, ho, wo, C, co = cs["shape"]
    n = cs["n"]
    rows = n * ho * wo
    x, sep = cs["x"].cuda(), (cs["sep"].cuda() if use_pos else None)
    whp, wlp = _padw(cs["wh"]), _padw(cs["wl"])
    b = cs["bias"].cuda() if use_bias else None
    ybuf = yv = sbufs = svs = None
    if sel != "split":
        ybuf, yv = _slot(rows, co, co + 3, 2, torch.float32, SENT)
    if sel != "y":
        sbufs, svs = zip(*(_slot(rows, co, co + 5, 3, BF, SENT) for _ in range(2)))
    Nat.conv2d_upsample_bf16x3(x, n, hi, wi, C, sep, ho, wo, whp, wlp, b, co, yv, relu_out=relu_out, y_split=svs,
                               split_relu=split_relu)
    # the unfused sequence: resize (+ table) + split, then the pre-split conv
    uh = torch.empty(rows, C, device="cuda", dtype=BF)
    ul = torch.empty_like(uh)
    if use_pos:
        Nat.upsample_bilinear_split_sep(x, n, hi, wi, C, None, ho, wo, sep, y_split=(uh, ul))
    else:
        Nat.upsample_bilinear_split(x, n, hi, wi, C, None, ho, wo, None, y_split=(uh, ul))
    y2 = torch.empty(rows, co, device="cuda") if sel != "split" else None
    s2 = tuple(torch.empty(rows, co, device="cuda", dtype=BF) for _ in range(2)) if sel != "y" else None
    Nat.conv2d_bf16x3_pre(uh, ul, n, ho, wo, C, whp, wlp, b, co, 3, 3, 1, 1, y2, relu_out=relu_out, y_split=s2,
                          split_relu=split_relu)
    torch.cuda.synchronize()
    what = f"fused {cs['shape']}"
    if yv is not None:
        _untouched(ybuf, yv, what + " y")
        bad = (_bits(yv) != _bits(y2)).cpu()
        assert not bool(bad.any()), f"{what}: y differs from the unfused sequence, {_first_bad(bad)}"
    if svs is not None:
        for i in range(2):
            _untouched(sbufs[i], svs[i], what + " y_split")
            bad = (_bits(svs[i]) != _bits(s2[i])).cpu()
            assert not bool(bad.any()), f"{what}: split half {i} differs from the unfused sequence, {_first_bad(bad)}"
    return (yv.cpu() if yv is not None else None), (tuple(v.cpu() for v in svs) if svs is not None else None)


@pytest.mark.parametrize("use_pos,use_bias,sel", [(1, 1, "both"), (0, 1, "y"), (1, 0, "split"), (0, 0, "both")])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_resize_conv(N, shape, use_pos, use_bias, sel):
    """vggt_conv2d_upsample_bf16x3 on every shape: bitwise the unfused upsample_bilinear_split[_sep] +
    conv2d_bf16x3_pre, ldy > co and ldys > co with sentinels, and inside the derived interval around fp64."""
    cs = _fused_case(shape, False)
    v, bound = _fused_ref(cs, use_pos, use_bias, False)
    y, halves = _run_fused(N, cs, use_pos, use_bias, sel)
    if y is not None:
        err = (y.double() - v).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"fused {shape} pos {use_pos} bias {use_bias}: worst |got - s| / bound {ratio:.4f}")
        bad = ~(err <= bound)
        assert not bool(bad.any()), f"fused {shape}: outside the interval, {_first_bad(bad)}, worst ratio {ratio}"
        if halves is not None:
            hi_, lo_ = _split(y)
            assert _same(halves[0], hi_) and _same(halves[1], lo_)
    else:  # split only: hi + lo is within the split residue 2^-17 |v| of a value inside the interval
        s = halves[0].double() + halves[1].double()
        assert bool(((s - v).abs() <= bound + 2.0 ** -17 * (v.abs() + bound)).all())


@pytest.mark.parametrize("use_pos,use_bias,sel,relu", [(1, 1, "both", 0), (0, 0, "y", 0), (1, 0, "split", 1),
                                                      (1, 1, "both", 1)])
@pytest.mark.parametrize("shape", FUSED_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_fused_resize_conv_exact(N, shape, use_pos, use_bias, sel, relu):
    """Identity and scale-1/2 resize on inputs whose resized map + table splits exactly: bit for bit the
    fp64 three-term result (relu: relu_out with y, split_relu on the halves)."""
    cs = _fused_case(shape, True)
    v, _ = _fused_ref(cs, use_pos, use_bias, True)
    y, halves = _run_fused(N, cs, use_pos, use_bias, sel, relu_out=bool(relu) and sel != "split",
                           split_relu=bool(relu))
    vr = v.clamp_min(0) if relu and sel != "split" else v
    if y is not None:
        _assert_exact(f"fused exact {shape}", y, vr)
    if halves is not None:
        _assert_split(f"fused exact {shape}", halves, vr, bool(relu))


# ------------------------------------------------------------------ part 4: element-wise kernels
RESIZE_SIZES = {"identity": (5, 7, 5, 7), "hi1": (1, 6, 4, 9), "wi1": (6, 1, 9, 4), "ho1": (6, 5, 1, 8),
                "wo1": (5, 6, 8, 1), "down9to4": (9, 9, 4, 4), "up5to9": (5, 5, 9, 9), "up7to20": (7, 9, 20, 13)}


@pytest.mark.parametrize("C", [4, 8, 32])
@pytest.mark.parametrize("size", list(RESIZE_SIZES))
def test_upsample_edges(N, size, C):
    """upsample_bilinear_f32 / _split / _split_sep against the fp64 interpolation at the exact rational
    coordinates, inside the derived bound; every output selection; halves == split of the y of the launch."""
    hi, wi, ho, wo = RESIZE_SIZES[size]
    n = 2
    gen = torch.Generator().manual_seed(hi * 100 + wo + C)
    x = torch.randn(n * hi * wi, C, generator=gen)
    sep = torch.randn(wo + ho, C // 2, generator=gen) if C % 8 == 0 else None
    full = _sep_to_full(sep, ho, wo, C) if sep is not None else torch.randn(ho * wo, C, generator=gen)
    rows = n * ho * wo
    xd, fd = x.cuda(), full.cuda()

    def out(kind):
        return torch.full((rows, C), SENT, device="cuda", dtype=kind)

    worst = 0.0
    for pos in (None, full):
        ref, bound = _resize_ref(x, n, hi, wi, C, ho, wo, pos, exact_coords=True)
        pd = fd if pos is not None else None
        y = N.upsample_bilinear_f32(xd, n, hi, wi, C, out(torch.float32), ho, wo, pd).cpu()
        err = (y.double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        bad = ~(err <= bound)
        assert not bool(bad.any()), f"{size} C {C}: outside the bound, {_first_bad(bad)}"
        if size == "identity" and pos is None:
            assert _same(y, x)
        # y + split, split only (y = NULL), split with split_relu: halves == split of the y this launch wrote
        for want_y, srelu in ((True, False), (False, False), (True, True), (False, True)):
            y2 = out(torch.float32) if want_y else None
            hs = (out(BF), out(BF))
            N.upsample_bilinear_split(xd, n, hi, wi, C, y2, ho, wo, pd, y_split=hs, split_relu=srelu)
            if want_y:
                assert _same(y2.cpu(), y)
            eh, el = _split(y.clamp_min(0) if srelu else y)
            assert _same(hs[0].cpu(), eh) and _same(hs[1].cpu(), el), (size, C, want_y, srelu)
        if sep is not None and pos is not None:  # the separable table form == the full table form
            y3, hs = out(torch.float32), (out(BF), out(BF))
            N.upsample_bilinear_split_sep(xd, n, hi, wi, C, y3, ho, wo, sep.cuda(), y_split=hs)
            eh, el = _split(y)
            assert _same(y3.cpu(), y) and _same(hs[0].cpu(), eh) and _same(hs[1].cpu(), el)
    print(f"resize {size} C {C}: worst |got - ref| / bound {worst:.4f}")


def _split_values():
    f = torch.tensor
    sub = 2.0 ** -130
    vals = [0.0, -0.0, sub, -sub, 2.0 ** -149, 2.0 ** -126, 1.0, -1.0, 1.5, -0.375, 3.0e38, 257.0, 1 + 2.0 ** -7,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,
            1 + 2.0 ** -8 - 2.0 ** -20, 2 - 2.0 ** -9, 2 - 2.0 ** -10, -(4 - 2.0 ** -9), 255.5, 0.99999994,
            float("inf"), float("-inf"), 1e-3, -2.5e-7, 3.1415927, -2.7182817]
    return f(vals, dtype=torch.float32)


def _split_ref(x, relu):
    v = x.clamp_min(0) if relu else x
    v = torch.where((x == 0) & relu, torch.zeros_like(x), v)  # ReLU of -0: fmaxf(-0, 0) may keep either zero
    return v, _split(v)


@pytest.mark.parametrize("relu", [False, True])
def test_split_act_edges(N, relu):
    """split_act_bf16x2 == (x.to(bf16), (x - hi).to(bf16)) bit for bit on +-0, subnormals, exact bf16 values,
    ties to even in both directions, values that round up to the next binade, +-inf; ReLU on negatives and
    -0; ldx > cols with NaN gaps; cols = 4; rows = 1; rows = 0."""
    sv = _split_values()
    gen = torch.Generator().manual_seed(5)
    for rows, cols in ((1, 4), (1, sv.numel() // 4 * 4), (7, 36), (33, 4)):
        x = torch.randn(rows, cols, generator=gen)
        flat = x.reshape(-1)
        k = min(flat.numel(), sv.numel())
        flat[:k] = sv[:k]
        _, xv = _slot(rows, cols, cols + 8, 4, torch.float32, NAN, x)
        hi = torch.full((rows + 2, cols), SENT, device="cuda", dtype=BF)
        lo = torch.full((rows + 2, cols), SENT, device="cuda", dtype=BF)
        N.split_act_bf16x2(xv, relu, out=(hi[1:rows + 1], lo[1:rows + 1]))
        v, (eh, el) = _split_ref(x, relu)
        gh, gl = hi.cpu(), lo.cpu()
        sent = torch.full((cols,), SENT).to(BF)
        for t in (gh, gl):
            assert _same(t[0], sent) and _same(t[-1], sent)
        zero_in = (x == 0) & relu  # -0 under ReLU: either zero, hi and lo alike
        for got, ref in ((gh[1:-1], eh), (gl[1:-1], el)):
            bad = (_bits(got) != _bits(ref)) & ~(zero_in & (got.float() == 0)) & ~(torch.isnan(ref.float()) & torch.isnan(got.float()))
            assert not bool(bad.any()), f"split_act {rows}x{cols} relu {relu}: {_first_bad(bad)}"
    # rows = 0: VGGT_OK, nothing written
    hi = torch.full((2, 8), SENT, device="cuda", dtype=BF)
    lo = hi.clone()
    xz = torch.zeros(0, 8, device="cuda")
    N.split_act_bf16x2(xz, relu, out=(hi[:0], lo[:0]))
    torch.cuda.synchronize()
    assert _same(hi.cpu(), torch.full((2, 8), SENT).to(BF)) and _same(lo.cpu(), torch.full((2, 8), SENT).to(BF))


def test_split_bf16x2_edges(N):
    sv = _split_values()
    hi, lo = N.split_bf16x2(sv.cuda())
    eh, el = _split(sv)
    nan = torch.isnan(el.float())  # inf - inf
    assert _same(hi.cpu(), eh)
    assert _same(lo.cpu()[~nan], el[~nan]) and bool(torch.isnan(lo.cpu().float()[nan]).all())


def test_split_act_grid_stride(N):
    """Just above 16384 * 256 items (8200 x 2048 / 4): the grid-stride loop's second pass."""
    rows, cols = 8200, 2048
    assert rows * cols // 4 > 16384 * 256
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(rows, cols, device="cuda", generator=gen)
    hi, lo = N.split_act_bf16x2(x, False)
    eh = x.to(BF)
    el = (x - eh.float()).to(BF)
    assert torch.equal(_bits(hi), _bits(eh)) and torch.equal(_bits(lo), _bits(el))


ACT_GRID = [0.0, -0.0, 1e-8, -1e-8, 1e-4, -1e-4, 1.0, -1.0, 20.0, -20.0, 80.0, -80.0]


def _ulp(x):
    """Spacing of fp32 at |x| (x fp64)."""
    a = x.float().abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double()


def _act_ref(z, ncl, act, scale, ppi):
    """fp64 activation a, output a * scale, confidence, and the bound on the points: the function's TOL_FN
    ulps of a carried through the multiply, plus the multiply's own rounding (half an ulp of the product)."""
    zd = z.double()
    v = zd[:, :ncl - 1]
    a = v.exp() if act == 0 else torch.sign(v) * torch.expm1(v.abs())
    if scale is None:
        return a, a, 1 + zd[:, ncl - 1].exp(), TOL_FN[act] * _ulp(a)
    s = scale.double().repeat_interleave(ppi)[:, None]
    fn = TOL_FN[act] * _ulp(a) * s.abs()
    return a, a * s, 1 + zd[:, ncl - 1].exp(), fn + 0.5 * _ulp((a * s).abs() + fn)


@pytest.mark.parametrize("ncl", [2, 4])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("use_scale", [False, True])
def test_dpt_activate_edges(N, ncl, act, use_scale):
    """ncl 2 (depth head) and 4, exp and inv_log, scale given and NULL, ldx > ncl with NaN gaps, 3 images of
    77 pixels; inputs on the grid {+-0, +-1e-8, +-1e-4, +-1, +-20, +-80}; ulp tolerance of the docstring."""
    nimg, ppi = 3, 77
    npix = nimg * ppi
    grid = torch.tensor(ACT_GRID)
    idx = (torch.arange(npix)[:, None] * 5 + torch.arange(ncl)[None] * 7) % len(ACT_GRID)
    z = grid[idx]
    _, zv = _slot(npix, ncl, ncl + 3, 2, torch.float32, NAN, z)
    scale = torch.tensor([2.0, 3.0, 0.7]) if use_scale else None
    pts = torch.full((npix + 2, ncl - 1), SENT, device="cuda")
    conf = torch.full((npix + 2,), SENT, device="cuda")
    N.dpt_activate(zv, npix, ppi, ncl, act, scale.cuda() if use_scale else None, pts[1:-1], conf[1:-1])
    pts, conf = pts.cpu(), conf.cpu()
    assert _same(pts[[0, -1]], torch.full((2, ncl - 1), SENT)) and _same(conf[[0, -1]], torch.full((2,), SENT))
    a, ref, cref, bound = _act_ref(z, ncl, act, scale, ppi)
    assert bool(torch.isfinite(ref.float()).all()) and bool(torch.isfinite(cref.float()).all())
    err = (pts[1:-1].double() - ref).abs()
    cerr = (conf[1:-1].double() - cref).abs()
    cbound = TOL_FN[0] * _ulp(cref - 1) + 0.5 * _ulp(cref + TOL_FN[0] * _ulp(cref - 1))
    print(f"dpt_activate ncl {ncl} act {act} scale {use_scale}: worst |got - ref| / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}, in ulps of the result "
          f"{float((err / _ulp(ref)).max()):.3f}; conf / bound {float((cerr / cbound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    if act == 1:  # sign and exact zero
        v = z[:, :ncl - 1]
        assert bool((pts[1:-1][v == 0] == 0).all())
        assert bool((torch.sign(pts[1:-1]) == torch.sign(v)).all())
    # conf = 1 + exp(c): the function's error and the add's rounding
    assert bool((cerr <= cbound).all())


def test_dpt_activate_bar_rejects_exp_minus_one():
    """The small-|x| grid points fail the bar for an exp(x) - 1 implementation (fp32 restatement, host)."""
    v = torch.tensor([1e-8, -1e-8, 1e-4, -1e-4])
    naive = torch.sign(v) * (torch.exp(v.abs()) - 1)
    ref = torch.sign(v.double()) * torch.expm1(v.double().abs())
    assert bool(((naive.double() - ref).abs() > 100 * TOL_FN[1] * _ulp(ref)).all())


# ------------------------------------------------------------------ part 5: rejections
def _rc_conv(Nat, api, *, ci=32, co=8, kh=1, kw=1, ldx=None, ldy=None, shuffle=0, pos=False, res1=False, y=True,
             split=(True, True), ldys=None, npix_side=3):
    """Raw C call of one conv entry point on sentinel-filled outputs; returns (rc, outputs untouched)."""
    L = Nat.lib()
    import ctypes
    hi = wi = npix_side
    ldx = ci if ldx is None else ldx
    ldy = co if ldy is None else ldy
    ldys = co if ldys is None else ldys
    rows = hi * wi * max(shuffle * shuffle, 1)
    width = max(ldx, ci) + 8
    xf = torch.zeros(hi * wi + 2, width, device="cuda")
    xb = torch.zeros(hi * wi + 2, width, device="cuda", dtype=BF)
    w = torch.zeros(128, kh * kw * max(ci, 32) + 32, device="cuda")
    wb = w.to(BF)
    outs = [torch.full((rows + 2, co + 8), SENT, device="cuda"), torch.full((rows + 2, co + 8), SENT, device="cuda", dtype=BF),
            torch.full((rows + 2, co + 8), SENT, device="cuda", dtype=BF)]
    aux = torch.zeros(rows + 2, co + 8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    Z = ctypes.c_void_p(0)
    st = Nat._stream()
    if api == "f32":
        rc = L.vggt_conv2d_f32(P(xf), ldx, 1, hi, wi, ci, P(w), Z, co, kh, kw, 1, 0, P(outs[0]), ldy, 0, 0,
                               P(aux) if res1 else Z, co, 0, Z, 0, P(aux) if pos else Z, shuffle, st)
    elif api == "bf16x3":
        rc = L.vggt_conv2d_bf16x3(P(xf), ldx, 1, hi, wi, ci, P(wb), P(wb), Z, co, kh, kw, 1, 0, P(outs[0]), ldy, 0, 0,
                                  P(aux) if res1 else Z, co, 0, Z, 0, P(aux) if pos else Z, shuffle, st)
    else:
        rc = L.vggt_conv2d_bf16x3_pre(P(xb), P(xb), ldx, 1, hi, wi, ci, P(wb), P(wb), Z, co, kh, kw, 1, 0,
                                      P(outs[0]) if y else Z, ldy, 0, P(aux) if res1 else Z, co, 0, Z, 0,
                                      P(aux) if pos else Z, shuffle, P(outs[1]) if split[0] else Z,
                                      P(outs[2]) if split[1] else Z, ldys, 0, st)
    torch.cuda.synchronize()
    clean = all(_same(o.cpu(), torch.full(o.shape, SENT).to(o.dtype)) for o in outs)
    # the host-only query with the same integers (these buffers are all 16-byte aligned) answers the same code
    has = (Nat.CONV_HAS_Y if y or api != "pre" else 0) | (Nat.CONV_HAS_RES1 if res1 else 0) | (Nat.CONV_HAS_POS if pos else 0)
    if api == "pre":
        has |= (Nat.CONV_HAS_Y_HI if split[0] else 0) | (Nat.CONV_HAS_Y_LO if split[1] else 0)
    entry = {"f32": Nat.CONV_ENTRY_F32, "bf16x3": Nat.CONV_ENTRY_BF16X3, "pre": Nat.CONV_ENTRY_PRE}[api]
    q = Nat.conv_form(entry, 1, hi, wi, ci, co, kh, kw, 1, 0, shuffle, ldx=ldx, ldy=ldy, ldys=ldys, present=has)
    assert q["rc"] == rc, f"{api}: vggt_conv_form answers {q['rc']}, the entry point {rc}"
    return rc, clean


def test_conv_rejections(N):
    """Every documented rejection returns its code and leaves sentinel-filled outputs untouched, including
    the two checks this test added to the entry points: ldy < co, and ldx < ci on a multi-pixel map."""
    S, A, U = VGGT_ERR_SHAPE, VGGT_ERR_ALIGN, VGGT_ERR_UNSUPPORTED
    for api in ("f32", "bf16x3", "pre"):
        cases = [("ci % 32", dict(ci=48, ldx=48), S), ("shuffle kh != 1", dict(shuffle=2, kh=3, kw=3), U),
                 ("shuffle + res1", dict(shuffle=2, res1=True), U), ("shuffle + pos", dict(shuffle=2, pos=True), U),
                 ("ldy < co", dict(ldy=7), S), ("ldx < ci", dict(ldx=24), S)]
        cases.append(("ldx % 8", dict(ldx=36), A) if api == "pre" else ("ldx % 4", dict(ldx=34), A))
        if api == "pre":
            cases += [("no output", dict(y=False, split=(False, False)), S),
                      ("y_hi without y_lo", dict(split=(True, False)), S),
                      ("y_lo without y_hi", dict(split=(False, True)), S), ("ldys < co", dict(ldys=7), S)]
        for what, kw, code in cases:
            rc, clean = _rc_conv(N, api, **kw)
            assert rc == code, f"{api} {what}: returned {rc}, documented {code}"
            assert clean, f"{api} {what}: wrote to its outputs"
        rc, clean = _rc_conv(N, api)  # the same call without a fault is accepted
        assert rc == 0 and not clean, (api, rc)
        rc, _ = _rc_conv(N, api, ldx=24, npix_side=1, ci=32)  # one pixel: its stride is never used
        assert rc == 0, (api, rc)


def test_fused_and_elementwise_rejections(N):
    import ctypes
    L = N.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    Z = ctypes.c_void_p(0)
    st = N._stream()
    S = VGGT_ERR_SHAPE
    x = torch.zeros(2 * 3 * 64 + 64, device="cuda")
    wb = torch.zeros(128, 9 * 64, device="cuda", dtype=BF)
    y = torch.full((5 * 7 + 2, 48), SENT, device="cuda")
    yh = torch.full((5 * 7 + 2, 48), SENT, device="cuda", dtype=BF)
    yl = yh.clone()

    def fused(C=32, co=32, ldy=32, ldys=32, has_y=True, hi_=True, lo_=True):
        return L.vggt_conv2d_upsample_bf16x3(P(x), 1, 2, 3, C, Z, 5, 7, P(wb), P(wb), Z, co, 0, P(y) if has_y else Z, ldy,
                                             P(yh) if hi_ else Z, P(yl) if lo_ else Z, ldys, 0, st)
    assert fused(co=33, ldy=40, ldys=40) == S and fused(C=48) == S and fused(ldy=31) == S and fused(ldys=31) == S
    assert fused(has_y=False, hi_=False, lo_=False) == S and fused(lo_=False) == S and fused(hi_=False) == S
    h = torch.full((4, 8), SENT, device="cuda", dtype=BF)
    l = h.clone()
    assert L.vggt_split_act_bf16x2(P(x), 8, 4, 6, 0, P(h), P(l), st) == S  # cols % 4
    assert L.vggt_split_act_bf16x2(P(x), 4, 4, 8, 0, P(h), P(l), st) == S  # ldx < cols
    pts = torch.full((16, 3), SENT, device="cuda")
    conf = torch.full((16,), SENT, device="cuda")
    assert L.vggt_dpt_activate(P(x), 4, 16, 8, 1, 0, Z, P(pts), P(conf), st) == S  # ncl < 2
    assert L.vggt_dpt_activate(P(x), 4, 16, 8, 4, 2, Z, P(pts), P(conf), st) == S  # act = 2
    torch.cuda.synchronize()
    for t in (y, yh, yl, h, l, pts, conf):
        assert _same(t.cpu(), torch.full(t.shape, SENT).to(t.dtype))
    assert fused() == 0  # the same call without a fault is accepted
    torch.cuda.synchronize()
