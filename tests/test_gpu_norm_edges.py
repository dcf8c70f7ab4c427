"""csrc/norm.hip, csrc/patch.hip and vggt_cast_f32_bf16 at the edges of their row blocks, head
passes, chunks and grid caps, per element or per row, against fp64 (the style and the rules of
test_gpu_train_edges.py; the shared helpers live in edge_rules.py).

Inputs come from a seeded host generator; references are fp64 from the bf16 / fp32 values actually
passed.  Strided operands sit in `Box`es: inputs NaN around the window, outputs a sentinel that
must be intact bit for bit afterwards.  Dense outputs (im2col, dino_assemble) sit between sentinel
guards.  `_reach_*` restate the host dispatch and are printed with the figures.

Entry point, paths reached, rule:
  vggt_layernorm(_grouped)   NV = C / 256 in {1, 2, 3, 4, 8, 16}; 4 rows (waves) per workgroup:
        M = 1 leaves three waves without a row, M = 5 / 9 give the last workgroup one row; all four
        dtype pairs; (w, b), (w, NULL), (NULL, NULL); strided; in place (y is x) for equal dtypes;
        group maps G = 1, G = M, M % G != 0 with row offsets and group strides > G.
        model rule per row.  Row kinds (row index % 4): random; constant 3 (the sum 3 C and the
        mean are exact, so the result must equal b, or 0 without b); 1000 + k / 4 with integer
        |k| <= 8 (every fp32 partial sum of every order is a multiple of 1/4 below 2^24 / 4, so
        the mean is the same fp32 number in the kernel and in the model and the row tests the
        two-pass variance, not the luck of two summation orders at 1000 u); random with one
        element of 10^4.  Error returns on the host side only.
        The first run of this file measured the fp32-output kernels at 5.1 x the model (C = 4096,
        M = 4, bf16 -> f32, the row around 1000: 3.27e-7 against 6.39e-8 of the row norm), 3.0 x
        (f32 -> f32, C = 4096, M = 9) and 2.0 x on a plain random row (C = 768, M = 1): 4 NV
        serial fp32 additions per lane and rsqrtf, which only a bf16 rounding hides.  fp32
        outputs now take statistics and affine step in fp64 with one rounding per stored value;
        bf16 outputs were at 1.00 x and keep their arithmetic.  The model stays the fp32 one.
  vggt_resid_add_layernorm, _nostore, add2   NV in {1, 2, 4, 8}; x' = x + gamma y by the one-op
        rule, out2 bitwise x', xn by the model rule against the fp64 LayerNorm of the stored x';
        b without w must change nothing (b is ignored when w is NULL); the deferred forms bitwise
        the stored forms, x untouched by _nostore; all five matrices strided.  With gamma = 0 the
        xn is bitwise vggt_layernorm of x (one statistics routine, csrc/norm_row.h).
  error returns   every rule of the residual check and of the head-norm check
        broken once per entry point that has the argument, NULL data pointers included; nothing
        may be written.
  vggt_qknorm_rope(_out), vggt_headnorm_rope(_out)   64 / (D / 8) heads per wave pass: D = 64
        with 10 heads (8 + 2, hsplit 5 inside pass 0) and 18 heads (8 + 8 + 2, hsplit 9 inside
        pass 1), D = 128 with 6 (4 + 2, hsplit 3) and 10 heads (4 + 4 + 2, hsplit 5 inside pass
        1); col_off 8 / 72; lds != ldd; M = 1 / 5 with period 3; modes 0 / 1 / 2; w NULL with
        RoPE, b NULL with w; positions -3 and tab_len + 5 (clamped to the first / last table row:
        the reference uses the clamped row).  model rule per (row, head); every column outside
        the heads bitwise untouched; src of the _out forms untouched.
  vggt_patch_im2col   8-wide chunks across channel boundaries and the zero pad; interval rule on
        (raw - mean) / sd: one subtraction, one division, E = gamma_2 (|raw| + |mean|) / sd, then
        one bf16 rounding; pad columns +0 bit for bit; the count equal to host fp32 is printed.
  vggt_dino_assemble, vggt_special_tokens, vggt_copy_rows_f32, vggt_cast_f32_bf16   bit for bit
        (one IEEE add, a copy, one rounding); the two grid-cap cases (2056 x 4096: 2,105,344 work
        items over 8192 x 256 threads) are the only ones on the second trip of the grid-stride loop.
DESIGN.md (Norm, small and token kernel edge tests) tabulates what was measured."""
import math

import pytest
import torch

from edge_rules import (BF, EPS, ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED, F32, F64, FIG, HN_CFG, NAN, OK, POS, SENT, TAB,
                        Box, _bits, _done, _dtn, _eq_bits, _fig, _figures, _gam, _gen, _guarded, _guards_ok, _hn_args,
                        _hn_host, _interval, _model_rule, _raises, _within)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------ the dispatch, restated
def _reach_rows(M, C):
    wgs = -(-M // 4)
    return {"NV": C // 256, "workgroups": wgs, "rows_in_last": M - 4 * (wgs - 1), "idle_waves": 4 * wgs - M}


def _reach_heads(D, heads, hsplit):
    hpp = 64 // (D // 8)
    passes = [min(hpp, heads - h0) for h0 in range(0, heads, hpp)]
    return {"heads_per_pass": hpp, "passes": passes, "hsplit": hsplit, "hsplit_in_pass": hsplit // hpp,
            "hsplit_inside_a_pass": hsplit % hpp != 0}


def _reach_grid(total):
    g = min(8192, max(1, -(-total // 256)))
    return {"work_items": total, "workgroups": g, "trips": -(-total // (g * 256))}


# ================================================================== 1. layernorm
LN_C = [256, 512, 768, 1024, 2048, 4096]
LN_M = [1, 4, 5, 9]


def _ln_rows(M, C, dt, g):
    x = torch.randn(M, C, generator=g)
    for r in range(M if M > 1 else 0):
        kind = r % 4
        if kind == 1:
            x[r] = 3.0
        elif kind == 2:
            x[r] = 1000.0 + torch.randint(-8, 9, (C,), generator=g).float() / 4
            if dt == BF:  # bf16 keeps multiples of 4 at 1000
                x[r] = 1000.0 + 4.0 * torch.randint(-8, 9, (C,), generator=g).float()
        elif kind == 3:
            x[r, int(torch.randint(0, C, (1,), generator=g))] = 1e4
    return x.to(dt)


def _ln_model(x, w, b, odt):
    """layernorm_kernel in plain fp32: two-pass statistics, sums times fl(1 / C), rsqrt, one rounding."""
    C = x.shape[-1]
    x32 = x.float()
    inv = torch.tensor(1.0 / C, dtype=F32)
    mean = x32.sum(-1, keepdim=True) * inv
    d = x32 - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) * inv + torch.tensor(EPS, dtype=F32))
    o = d * rstd
    if w is not None:
        o = o * w
        if b is not None:
            o = o + b
    return o.to(odt)


def _ln_ref(x, w, b):
    x64 = x.double()
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    o = d / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS)
    if w is not None:
        o = o * w.double()
        if b is not None:
            o = o + b.double()
    return o


def _ln_check(errs, tag, x, w, b, got, mtag):
    ref = _ln_ref(x, w, b)
    _model_rule(errs, tag, got, _ln_model(x, w, b, got.dtype), ref, mtag)
    for r in range(1, x.shape[0], 4):  # the constant rows
        want = (b if (w is not None and b is not None) else torch.zeros(x.shape[1])).to(got.dtype)
        if not torch.equal(got[r].float(), want.float()):
            bad = got[r].float() != want.float()
            errs.append(f"{tag}: constant row {r} is not b: {int(bad.sum())} elements, first col "
                        f"{int(bad.nonzero()[0])} got {float(got[r][bad][0])!r} want {float(want[bad][0])!r}")


@pytest.mark.parametrize("C", LN_C)
def test_layernorm(N, C):
    errs = []
    g = _gen(1, C)
    wv, bv = (1 + 0.2 * torch.randn(C, generator=g)), 0.3 * torch.randn(C, generator=g)
    wd, bd = wv.cuda(), bv.cuda()
    for M in LN_M:
        for idt in (F32, BF):
            x = _ln_rows(M, C, idt, g)
            for odt in (F32, BF):
                for aff in ("wb", "w", "none"):
                    w, b = (wv if aff != "none" else None), (bv if aff == "wb" else None)
                    tag = f"layernorm C={C} M={M} {_dtn(idt)}->{_dtn(odt)} {aff}"
                    xb, yb = Box(x, NAN), Box(torch.zeros(M, C, dtype=odt), SENT, cols=(16, 8))
                    N.layernorm(xb.v, wd if w is not None else None, bd if b is not None else None, EPS, yb.v)
                    _ln_check(errs, tag, x, w, b, yb.got(), f"layernorm {_dtn(idt)}->{_dtn(odt)}")
                    if not yb.intact():
                        errs.append(tag + ": y sentinels overwritten")
                    _eq_bits(errs, tag + " x", xb.got(), x)
            # in place: y is x
            xb = Box(x, SENT)
            N.layernorm(xb.v, wd, bd, EPS, xb.v)
            tag = f"layernorm in place C={C} M={M} {_dtn(idt)}"
            _ln_check(errs, tag, x, wv, bv, xb.got(), f"layernorm in place {_dtn(idt)}")
            if not xb.intact():
                errs.append(tag + ": sentinels overwritten")
    # (NULL, b): b is ignored when w is NULL
    x = _ln_rows(5, C, F32, g)
    xb, y0, y1 = Box(x, NAN), Box(torch.zeros(5, C), SENT), Box(torch.zeros(5, C), SENT)
    N.layernorm(xb.v, None, None, EPS, y0.v)
    N.layernorm(xb.v, None, bd, EPS, y1.v)
    _eq_bits(errs, f"layernorm C={C} (NULL, b) vs (NULL, NULL)", y1.got(), y0.got())
    _done(errs, *[("layernorm", C, M, _reach_rows(M, C)) for M in LN_M])


@pytest.mark.parametrize("C", [256, 768])
@pytest.mark.parametrize("M,G", [(9, 1), (5, 5), (7, 3)])
def test_layernorm_grouped(N, C, M, G):
    """Logical row r -> x row (r / G) xgs + xoff + r % G, y row (r / G) ygs + yoff + r % G, with
    xgs = G + 2, ygs = G + 3, xoff = 1, yoff = 2: the skipped x rows are NaN, the skipped y rows
    keep their sentinel.  (7, 3) leaves a last group of one row."""
    errs = []
    g = _gen(2, C, M, G)
    wv, bv = (1 + 0.2 * torch.randn(C, generator=g)), 0.3 * torch.randn(C, generator=g)
    xgs, ygs, xoff, yoff = G + 2, G + 3, 1, 2
    ng = -(-M // G)
    xr = [(r // G) * xgs + xoff + r % G for r in range(M)]
    yr = [(r // G) * ygs + yoff + r % G for r in range(M)]
    for idt, odt in ((F32, BF), (BF, F32), (F32, F32), (BF, BF)):
        x = _ln_rows(M, C, idt, g)
        xf = torch.full((ng * xgs + 2, C), NAN, dtype=idt)
        xf[xr] = x
        xb, yb = Box(xf, NAN), Box(torch.full((ng * ygs + 3, C), SENT, dtype=odt), SENT)
        N.layernorm_grouped(xb.v, wv.cuda(), bv.cuda(), EPS, yb.v, M, C, G, xgs, xoff, ygs, yoff)
        tag = f"layernorm_grouped C={C} M={M} G={G} {_dtn(idt)}->{_dtn(odt)}"
        _ln_check(errs, tag, x, wv, bv, yb.got()[yr], f"layernorm_grouped {_dtn(idt)}->{_dtn(odt)}")
        keep = torch.zeros(yb.host.shape, dtype=torch.bool)
        r0, _, c0, c1 = yb.win
        keep[[r0 + r for r in yr], c0:c1] = True
        if not yb.intact(keep):
            errs.append(tag + ": rows outside the map overwritten")
    _done(errs, ("layernorm_grouped", {"groups": ng, "last_group_rows": M - (ng - 1) * G, "x_rows": xr, "y_rows": yr}))


def test_layernorm_error_returns(N):
    L = N.lib()
    st = N._stream()
    buf = torch.zeros(16, 4400, device="cuda")
    w = torch.zeros(4400 + 4, device="cuda")

    def rc(C=256, idt=0, odt=0, ldx=4400, ldy=4400, xo=0, wo=0, bo=None):
        x = buf.view(-1)[xo:]
        return L.vggt_layernorm(N._p(x), idt, ldx, N._p(w[wo:]), None if bo is None else N._p(w[bo:]), EPS, 4, C,
                                N._p(buf), odt, ldy, st)

    assert rc() == 0
    assert [rc(C=c) for c in (128, 4352, 320)] == [ERR_SHAPE] * 3
    assert rc(idt=7) == ERR_UNSUPPORTED and rc(odt=7) == ERR_UNSUPPORTED
    assert rc(ldx=4401) == ERR_ALIGN and rc(ldy=4402) == ERR_ALIGN
    assert rc(xo=1) == ERR_ALIGN  # x 4 bytes off
    assert rc(wo=1) == ERR_ALIGN and rc(bo=2) == ERR_ALIGN  # w / b feed 16-B loads
    assert L.vggt_layernorm(None, 0, 4400, None, None, EPS, 4, 256, N._p(buf), 0, 4400, st) == ERR_SHAPE
    assert L.vggt_layernorm(N._p(buf), 0, 4400, None, None, EPS, 4, 256, None, 0, 4400, st) == ERR_SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------ error returns of the residual and head-norm forms
# The case tables work on addresses, so that they can be walked without a device as well (every
# rejected call returns before anything is launched).  Each case breaks exactly one rule.  The
# buffers behind the addresses are 16 x 4400 elements (vectors 4404 floats, the tables in their
# middle) and the calls use 4 rows, so that a call whose check was lost stays inside them.
ERR_LD = 4400
RESID_ARGS = {
    "vggt_resid_add_layernorm": "x ldx y ldy gamma out2 ldo2 w b eps M C xn ldn",
    "vggt_resid_add_layernorm_nostore": "x ldx y ldy gamma w b eps M C xn ldn",
    "vggt_resid_add2_layernorm": "x ldx y ldy gamma y2 ldy2 gamma2 out2 ldo2 w b eps M C xn ldn",
}
HN_ARGS = {
    "vggt_headnorm_rope": "buf ld col_off M H D w b eps mode pos period cos sin tab",
    "vggt_qknorm_rope": "buf ld M H D w b kw kb eps mode pos period cos sin tab",
    "vggt_qknorm_rope_out": "src lds dst ldd M H D w b kw kb eps mode pos period cos sin tab",
    "vggt_headnorm_rope_out": "src lds dst ldd M H D w b eps mode pos period cos sin tab",
}


def _off(addr, nbytes):
    return addr + nbytes


def _resid_error_cases(a):
    """(entry point, what is wrong, arguments by name, expected return); `a` maps names to addresses."""
    base = dict(x=a["x"], y=a["y"], gamma=a["gamma"], y2=a["y2"], gamma2=a["gamma2"], out2=a["out2"], w=a["w"],
                b=a["b"], xn=a["xn"], ldx=ERR_LD, ldy=ERR_LD, ldy2=ERR_LD, ldo2=ERR_LD, ldn=ERR_LD, eps=EPS, M=4, C=256)
    changes = [({"C": c}, ERR_SHAPE) for c in (128, 320, 4352)]
    changes += [({"M": -1}, ERR_SHAPE), ({"M": 0}, OK)]
    changes += [({k: None}, ERR_SHAPE) for k in ("x", "y", "gamma")]
    changes += [({k: ERR_LD + 1}, ERR_ALIGN) for k in ("ldx", "ldy", "ldy2", "ldo2", "ldn")]
    changes += [({k: _off(base[k], 4)}, ERR_ALIGN) for k in ("x", "gamma", "gamma2", "out2", "w", "b")]
    changes += [({k: _off(base[k], 2)}, ERR_ALIGN) for k in ("y", "y2", "xn")]
    cases = []
    for entry, names in RESID_ARGS.items():
        names = names.split()
        for ch, want in changes:
            if all(k in names for k in ch):
                cases.append((entry, ch, {**base, **ch}, want))
    two, nostore = "vggt_resid_add2_layernorm", "vggt_resid_add_layernorm_nostore"
    cases.append((two, "add2 without y2", {**base, "y2": None}, ERR_SHAPE))
    cases.append((two, "y2 without gamma2", {**base, "gamma2": None}, ERR_SHAPE))
    cases.append((nostore, "_nostore without xn", {**base, "xn": None}, ERR_SHAPE))
    return cases


def _hn_error_cases(a):
    base = dict(buf=a["y"], src=a["y"], dst=a["xn"], ld=ERR_LD, lds=ERR_LD, ldd=ERR_LD, col_off=8, M=4, H=2, D=64,
                w=a["w"], b=a["b"], kw=a["gamma"], kb=a["gamma2"], eps=EPS, mode=1, pos=a["pos"], period=3,
                cos=a["cos"], sin=a["sin"], tab=TAB)
    changes = [({"D": d}, ERR_SHAPE) for d in (32, 96)]
    changes += [({"H": 0}, ERR_SHAPE), ({"M": -1}, ERR_SHAPE)]
    changes += [({k: ERR_LD - 4}, ERR_ALIGN) for k in ("ld", "lds", "ldd")]  # 4396 = 8 k + 4
    changes += [({"col_off": 4}, ERR_ALIGN)]
    changes += [({k: _off(base[k], 2)}, ERR_ALIGN) for k in ("buf", "src", "dst")]
    changes += [({"w": None}, ERR_SHAPE), ({"kw": None}, ERR_SHAPE)]  # kw without qw, qw without kw
    changes += [({k: None}, ERR_SHAPE) for k in ("pos", "cos", "sin")]
    changes += [({"period": 0}, ERR_SHAPE), ({"tab": 0}, ERR_SHAPE)]
    changes += [({k: _off(base[k], 4)}, ERR_ALIGN) for k in ("cos", "sin")]
    changes += [({"mode": 3}, ERR_UNSUPPORTED)]
    changes += [({k: None}, ERR_SHAPE) for k in ("buf", "src", "dst")]
    cases = []
    for entry, names in HN_ARGS.items():
        names = names.split()
        for ch, want in changes:
            if ("w" in ch or "kw" in ch) and "kw" not in names:
                continue  # one weight set: w NULL only switches the norm off
            if all(k in names for k in ch):
                cases.append((entry, ch, {**base, **ch}, want))
    return cases


def _call(L, names, entry, args, stream):
    return getattr(L, entry)(*[args[k] for k in names[entry].split()], stream)


def _error_buffers():
    g = _gen(13)
    f32 = {k: torch.randn(16, ERR_LD, generator=g).cuda() for k in ("x", "out2")}
    bf = {k: torch.randn(16, ERR_LD, generator=g).to(BF).cuda() for k in ("y", "y2", "xn")}
    vec = {k: torch.randn(ERR_LD + 4, generator=g).cuda() for k in ("gamma", "gamma2", "w", "b", "cos", "sin")}
    bufs = {**f32, **bf, **vec, "pos": torch.tensor(POS[2], dtype=torch.int32).cuda()}
    addr = {k: t.data_ptr() for k, t in bufs.items()}
    addr["cos"] += 4 * 2048  # room on both sides of the tables
    addr["sin"] += 4 * 2048
    return bufs, addr


def _run_error_cases(N, cases, names):
    L, st = N.lib(), N._stream()
    bufs, addr = _error_buffers()
    before = {k: _bits(t.cpu()) for k, t in bufs.items()}
    bad = []
    for entry, what, args, want in cases(addr):
        rc = _call(L, names, entry, args, st)
        if rc != want:
            bad.append(f"{entry} {what}: returned {rc}, want {want}")
    torch.cuda.synchronize()
    for k, t in bufs.items():
        if not torch.equal(_bits(t.cpu()), before[k]):
            bad.append(f"buffer {k} was written by a rejected call")
    assert not bad, "\n".join(bad)
    return L, st, bufs, addr


def test_resid_error_returns(N):
    L, st, bufs, addr = _run_error_cases(N, _resid_error_cases, RESID_ARGS)
    # ldo2 is looked at only with out2: these two calls run (x' = x + gamma y, xn written)
    ok = next(c for c in _resid_error_cases(addr) if c[1] == {"ldo2": ERR_LD + 1})[2]
    for entry in ("vggt_resid_add_layernorm", "vggt_resid_add2_layernorm"):
        assert _call(L, RESID_ARGS, entry, {**ok, "out2": None}, st) == OK
    torch.cuda.synchronize()


def test_headnorm_error_returns(N):
    _run_error_cases(N, _hn_error_cases, HN_ARGS)


@pytest.mark.parametrize("C", [256, 1024, 2048])
def test_resid_xn_is_layernorm_of_x(N, C):
    """One statistics routine, seen from outside: with gamma = 0 (x' = x + 0 y = x bit for bit, y
    finite) the xn of vggt_resid_add_layernorm is bit for bit vggt_layernorm (fp32 -> bf16) of x."""
    errs = []
    g = _gen(14, C)
    wd, bd = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    zero = torch.zeros(C, device="cuda")
    for M in (1, 5):
        x, y, _ = _raln_inputs(M, C, g)
        x[0, :2] = 1.0  # the 0.0 / -0.0 of _raln_inputs: -0 + 0 y would become +0
        for w, b in ((wd, bd), (None, None)):
            tag = f"C={C} M={M} {'wb' if w is not None else 'none'}"
            xb, yb = Box(x, NAN), Box(y, NAN, cols=(16, 8))
            n0 = Box(torch.zeros(M, C, dtype=BF), SENT, cols=(24, 8))
            n1 = Box(torch.zeros(M, C, dtype=BF), SENT, cols=(8, 32))
            N.layernorm(xb.v, w, b, EPS, n0.v)
            N.resid_add_layernorm(xb.v, yb.v, zero, None, w, b, EPS, n1.v)
            _eq_bits(errs, tag + " x after gamma = 0", xb.got(), x)
            _eq_bits(errs, tag + " xn vs layernorm", n1.got(), n0.got())
            if not (n0.intact() and n1.intact() and xb.intact()):
                errs.append(tag + ": padding overwritten")
    _done(errs)


# ================================================================== 2. residual add + layernorm
def _raln_inputs(M, C, g):
    x = torch.randn(M, C, generator=g)
    x[0, :8] = torch.tensor([0.0, -0.0, 1e-30, 1e4, -1e4, 1.0, -1.0, 3.0])
    y = torch.randn(M, C, generator=g).to(BF)
    gam = 0.5 * torch.randn(C, generator=g)
    return x, y, gam


def _raln_check(errs, tag, x, y, gam, got_x, mtag):
    prod = gam.double() * y.double()
    return _within(errs, tag + " x'", got_x, x.double() + prod, 2.0 ** -23 * (x.double().abs() + prod.abs()))


@pytest.mark.parametrize("C", [256, 512, 1024, 2048])
def test_resid_add_layernorm(N, C):
    errs, worst = [], 0.0
    g = _gen(3, C)
    wv, bv = (1 + 0.2 * torch.randn(C, generator=g)), 0.3 * torch.randn(C, generator=g)
    wd, bd = wv.cuda(), bv.cuda()
    for M in (1, 5, 9):
        x, y, gam = _raln_inputs(M, C, g)
        gd = gam.cuda()
        plain = {}
        for has_o2 in (0, 1):
            for has_xn in (0, 1):
                for aff in ("wb", "w", "b", "none"):
                    tag = f"resid_add_layernorm C={C} M={M} out2={has_o2} xn={has_xn} {aff}"
                    xb, yb = Box(x, NAN), Box(y, NAN, cols=(16, 8))
                    o2 = Box(torch.zeros(M, C), SENT, cols=(8, 8)) if has_o2 else None
                    xn = Box(torch.zeros(M, C, dtype=BF), SENT, cols=(24, 8)) if has_xn else None
                    N.resid_add_layernorm(xb.v, yb.v, gd, o2.v if o2 else None, wd if "w" in aff else None,
                                          bd if "b" in aff else None, EPS, xn.v if xn else None)
                    gx = xb.got()
                    worst = max(worst, _raln_check(errs, tag, x, y, gam, gx, None))
                    if not (xb.intact() and yb.intact(torch.zeros(yb.host.shape, dtype=torch.bool))):
                        errs.append(tag + ": x padding or y changed")
                    if o2:
                        _eq_bits(errs, tag + " out2", o2.got(), gx)
                        if not o2.intact():
                            errs.append(tag + ": out2 sentinels overwritten")
                    if xn:
                        w, b = (wv if "w" in aff else None), (bv if aff == "wb" else None)
                        _model_rule(errs, tag + " xn", xn.got(), _ln_model(gx, w, b, BF), _ln_ref(gx, w, b),
                                    "resid_add_layernorm xn")
                        if not xn.intact():
                            errs.append(tag + ": xn sentinels overwritten")
                        if aff in ("b", "none"):
                            plain.setdefault(aff, xn.got())
        if len(plain) == 2:
            _eq_bits(errs, f"C={C} M={M}: xn with (NULL, b) vs (NULL, NULL)", plain["b"], plain["none"])
    _fig(("one-op", "resid_add_layernorm x'"), worst)
    print(f"one-op resid_add_layernorm C={C}: worst error / bound {worst:.3f}")
    _done(errs, *[("resid_add_layernorm", C, M, _reach_rows(M, C)) for M in (1, 5, 9)])


@pytest.mark.parametrize("C", [256, 512, 1024, 2048])
def test_resid_deferred_bitwise_stored(N, C):
    """_nostore + add2 against two stored vggt_resid_add_layernorm passes: x, out2 and both xn
    bitwise; x untouched by _nostore."""
    errs = []
    g = _gen(4, C)
    wd, bd = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    for M in (1, 5, 9):
        x, y, gam = _raln_inputs(M, C, g)
        _, y2, gam2 = _raln_inputs(M, C, g)
        gd, gd2 = gam.cuda(), gam2.cuda()
        for has_o2 in (0, 1):
            for has_xn in (0, 1):
                for aff in ("wb", "none"):
                    w, b = (wd, bd) if aff == "wb" else (None, None)
                    tag = f"deferred C={C} M={M} out2={has_o2} xn={has_xn} {aff}"
                    res = []
                    for deferred in (0, 1):
                        xb, yb, y2b = Box(x, NAN), Box(y, NAN, cols=(16, 8)), Box(y2, NAN, cols=(8, 24))
                        o2 = Box(torch.zeros(M, C), SENT, cols=(8, 8)) if has_o2 else None
                        n1 = Box(torch.zeros(M, C, dtype=BF), SENT, cols=(24, 8))
                        n2 = Box(torch.zeros(M, C, dtype=BF), SENT, cols=(8, 32)) if has_xn else None
                        if deferred:
                            N.resid_add_layernorm_nostore(xb.v, yb.v, gd, w, b, EPS, n1.v)
                            _eq_bits(errs, tag + " x after _nostore", xb.got(), x)
                            N.resid_add2_layernorm(xb.v, yb.v, gd, y2b.v, gd2, o2.v if o2 else None, w, b, EPS,
                                                   n2.v if n2 else None)
                        else:
                            N.resid_add_layernorm(xb.v, yb.v, gd, None, w, b, EPS, n1.v)
                            N.resid_add_layernorm(xb.v, y2b.v, gd2, o2.v if o2 else None, w, b, EPS,
                                                  n2.v if n2 else None)
                        for bx, nm in ((xb, "x"), (o2, "out2"), (n1, "xn1"), (n2, "xn2")):
                            if bx is not None and not bx.intact():
                                errs.append(f"{tag} deferred={deferred}: {nm} padding overwritten")
                        res.append([bx.got() if bx is not None else None for bx in (xb, o2, n1, n2)])
                    for a, d, nm in zip(res[0], res[1], ("x", "out2", "xn1", "xn2")):
                        if a is not None:
                            _eq_bits(errs, f"{tag} {nm} deferred vs stored", d, a)
    _done(errs)


def test_resid_add_layernorm_768_is_shape_error(N):
    x, y = torch.zeros(4, 768, device="cuda"), torch.zeros(4, 768, device="cuda", dtype=BF)
    gam, xn = torch.zeros(768, device="cuda"), torch.zeros(4, 768, device="cuda", dtype=BF)
    _raises(ERR_SHAPE, N.resid_add_layernorm, x, y, gam, None, None, None, EPS, xn)
    _raises(ERR_SHAPE, N.resid_add_layernorm_nostore, x, y, gam, None, None, EPS, xn)
    _raises(ERR_SHAPE, N.resid_add2_layernorm, x, y, gam, y, gam, None, None, None, EPS, xn)
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0


# ================================================================== 3. bf16 head norm + RoPE
@pytest.mark.parametrize("D,H", [(64, 5), (64, 9), (128, 3), (128, 5)])
@pytest.mark.parametrize("out_form", [0, 1])
def test_qknorm_rope(N, D, H, out_form):
    errs = []
    g = _gen(5, D, H, out_form)
    nh, W3 = 2 * H, 3 * H * D
    ws = [1 + 0.2 * torch.randn(D, generator=g) for _ in range(2)]
    bs = [0.3 * torch.randn(D, generator=g) for _ in range(2)]
    for M in (1, 5):
        x = (torch.randn(M, W3, generator=g) * (1 + torch.arange(W3) % 7) * 0.3).to(BF)
        for aff, mode in HN_CFG:
            rope, cos, sin = _hn_args(mode, D, g)
            w0, w1 = (ws if aff != "none" else (None, None))
            b0, b1 = (bs if aff == "wb" else (None, None))
            dv = [None if t is None else t.cuda() for t in (w0, b0, w1, b1)]
            tag = f"qknorm_rope{'_out' if out_form else ''} D={D} H={H} M={M} {aff} mode={mode}"
            if out_form:
                sb, db = Box(x, NAN), Box(torch.zeros(M, nh * D, dtype=BF), SENT, cols=(16, 24))
                N.qknorm_rope_out(sb.v, db.v, H, D, *dv, EPS, *rope)
                _eq_bits(errs, tag + " src", sb.got(), x)
                got = db.got()
                if not db.intact():
                    errs.append(tag + ": dst sentinels overwritten")
                assert sb.dev.stride(0) != db.dev.stride(0)
            else:
                xb = Box(x, SENT)
                N.qknorm_rope(xb.v, H, D, *dv, EPS, *rope)
                got = xb.got()[:, :nh * D]
                _eq_bits(errs, tag + " v columns", xb.got()[:, nh * D:], x[:, nh * D:])
                if not xb.intact():
                    errs.append(tag + ": sentinels overwritten")
            xin = x[:, :nh * D]
            ref = _hn_host(xin, D, nh, H, w0, b0, w1, b1, mode, cos, sin, F64)
            mod = _hn_host(xin, D, nh, H, w0, b0, w1, b1, mode, cos, sin, F32).to(BF)
            _model_rule(errs, tag, got.reshape(M, nh, D), mod, ref, f"qknorm_rope D={D}")
    _done(errs, ("qknorm_rope", D, H, _reach_heads(D, nh, H)))


@pytest.mark.parametrize("D,H", [(64, 3), (128, 5)])
@pytest.mark.parametrize("col_off", [8, 72])
def test_headnorm_rope_col_off(N, D, H, col_off):
    errs = []
    g = _gen(6, D, H, col_off)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    Wd = col_off + H * D + 8
    for M in (1, 5):
        x = torch.randn(M, Wd, generator=g).to(BF)
        for aff, mode in HN_CFG:
            rope, cos, sin = _hn_args(mode, D, g)
            w0, b0 = (w if aff != "none" else None), (b if aff == "wb" else None)
            tag = f"headnorm_rope D={D} H={H} M={M} col_off={col_off} {aff} mode={mode}"
            xb = Box(x, SENT)
            N.headnorm_rope(xb.v, col_off, H, D, None if w0 is None else w0.cuda(), None if b0 is None else b0.cuda(),
                            EPS, *rope)
            got = xb.got()
            _eq_bits(errs, tag + " columns before", got[:, :col_off], x[:, :col_off])
            _eq_bits(errs, tag + " columns after", got[:, col_off + H * D:], x[:, col_off + H * D:])
            if not xb.intact():
                errs.append(tag + ": sentinels overwritten")
            xin = x[:, col_off:col_off + H * D]
            ref = _hn_host(xin, D, H, H, w0, b0, w0, b0, mode, cos, sin, F64)
            mod = _hn_host(xin, D, H, H, w0, b0, w0, b0, mode, cos, sin, F32).to(BF)
            _model_rule(errs, tag, got[:, col_off:col_off + H * D].reshape(M, H, D), mod, ref, f"headnorm_rope D={D}")
            if col_off == 8:  # the out-of-place form, lds != ldd (heads start at column 0)
                sb, db = Box(xin, NAN), Box(torch.zeros(M, H * D, dtype=BF), SENT, cols=(24, 8))
                N.headnorm_rope_out(sb.v, db.v, H, D, None if w0 is None else w0.cuda(),
                                    None if b0 is None else b0.cuda(), EPS, *rope)
                _eq_bits(errs, tag + " _out src", sb.got(), xin)
                _eq_bits(errs, tag + " _out vs in place", db.got(), got[:, col_off:col_off + H * D])
                if not db.intact():
                    errs.append(tag + ": _out dst sentinels overwritten")
    if col_off == 8:  # w NULL: b is ignored
        xb0, xb1 = Box(x, SENT), Box(x, SENT)
        rope, _, _ = _hn_args(1, D, g)
        N.headnorm_rope(xb0.v, col_off, H, D, None, None, EPS, *rope)
        N.headnorm_rope(xb1.v, col_off, H, D, None, b.cuda(), EPS, *rope)
        _eq_bits(errs, f"headnorm_rope D={D} (NULL, b) vs (NULL, NULL)", xb1.got(), xb0.got())
    _done(errs, ("headnorm_rope", D, H, _reach_heads(D, H, H)))


def test_reach_heads():
    assert _reach_heads(64, 10, 5) == {"heads_per_pass": 8, "passes": [8, 2], "hsplit": 5, "hsplit_in_pass": 0,
                                       "hsplit_inside_a_pass": True}
    assert _reach_heads(64, 18, 9)["passes"] == [8, 8, 2] and _reach_heads(64, 18, 9)["hsplit_in_pass"] == 1
    assert _reach_heads(128, 6, 3)["passes"] == [4, 2] and _reach_heads(128, 10, 5)["hsplit_in_pass"] == 1
    assert _reach_grid(2056 * 1024)["trips"] == 2 and _reach_grid(8192 * 256)["trips"] == 1
    assert _reach_rows(5, 768) == {"NV": 3, "workgroups": 2, "rows_in_last": 1, "idle_waves": 3}


# ================================================================== 4. im2col
def _f32(v):
    return float(torch.tensor(v, dtype=F32))


@pytest.mark.parametrize("p,Kp", [(2, 16), (14, 592), (14, 640)])
@pytest.mark.parametrize("Fr", [1, 3])
def test_patch_im2col(N, p, Kp, Fr):
    errs = []
    H, W = 28, 42
    g = _gen(7, p, Kp, Fr)
    img = torch.rand(Fr, 3, H, W, generator=g)
    img[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 0.485, 1e-30])
    mean, sd = [_f32(v) for v in (0.485, 0.456, 0.406)], [_f32(v) for v in (0.229, 0.224, 0.225)]
    h, w = H // p, W // p
    rows, kk = Fr * h * w, 3 * p * p
    buf, out = _guarded((rows, Kp), BF)
    N.patch_im2col(img.cuda(), p, mean, sd, out)
    got = out.cpu()
    # k = c p^2 + ky p + kx of patch (py, px)
    raw = img.view(Fr, 3, h, p, w, p).permute(0, 2, 4, 1, 3, 5).reshape(rows, kk)
    mk = torch.tensor(mean, dtype=F32).repeat_interleave(p * p)[None]
    sk = torch.tensor(sd, dtype=F32).repeat_interleave(p * p)[None]
    s = (raw.double() - mk.double()) / sk.double()
    E = _gam(2) * (raw.double().abs() + mk.double().abs()) / sk.double()
    tag = f"im2col p={p} Kp={Kp} F={Fr}"
    worst = _interval(errs, tag, got[:, :kk], s, E.expand_as(s))
    host = ((raw - mk) / sk).to(BF)
    same = int((_bits(got[:, :kk]) == _bits(host)).sum())
    print(f"interval {tag}: worst ratio {worst:.3f}; {same} of {host.numel()} elements equal host fp32 arithmetic")
    _fig(("interval", "im2col"), worst)
    _fig(("im2col equal host fp32", p, Kp, Fr), f"{same}/{host.numel()}")
    if bool((_bits(got[:, kk:]) != 0).any()):
        bad = _bits(got[:, kk:]) != 0
        errs.append(f"{tag}: pad columns not +0: {int(bad.sum())}, first {bad.nonzero()[0].tolist()}")
    if not _guards_ok(buf, rows * Kp):
        errs.append(tag + ": guards overwritten")
    _done(errs, ("im2col", {"chunks_per_row": Kp // 8, "chunk_with_boundary": kk // 8 if kk % 8 else None,
                            "pad_columns": Kp - kk, **_reach_grid(rows * Kp // 8)}))


def test_patch_im2col_error_returns(N):
    m, s = [0.5] * 3, [0.25] * 3
    out = torch.zeros(4096, dtype=BF, device="cuda")
    _raises(ERR_SHAPE, N.patch_im2col, torch.zeros(1, 3, 29, 42, device="cuda"), 2, m, s, out.view(-1, 16))
    _raises(ERR_SHAPE, N.patch_im2col, torch.zeros(1, 3, 4, 4, device="cuda"), 2, m, s, out[:80].view(4, 20))
    _raises(ERR_SHAPE, N.patch_im2col, torch.zeros(1, 3, 4, 4, device="cuda"), 2, m, s, out[:32].view(4, 8))
    torch.cuda.synchronize()


# ================================================================== 5. dino_assemble
@pytest.mark.parametrize("nreg", [0, 4])
@pytest.mark.parametrize("hw", [1, 6])
@pytest.mark.parametrize("C", [4, 384])
def test_dino_assemble(N, nreg, hw, C):
    errs = []
    for Fr in (1, 3):
        g = _gen(8, nreg, hw, C, Fr)
        patch = torch.randn(Fr * hw, C, generator=g).to(BF)
        cls, pos = torch.randn(C, generator=g), torch.randn(1 + hw, C, generator=g)
        reg = torch.randn(max(nreg, 1), C, generator=g)
        P = 1 + nreg + hw
        buf, x = _guarded((Fr * P, C), F32)
        N.dino_assemble(patch.cuda(), cls.cuda(), reg.cuda() if nreg else None, pos.cuda(), Fr, hw, nreg, C, x)
        got = x.cpu().view(Fr, P, C)
        tag = f"dino_assemble nreg={nreg} hw={hw} C={C} F={Fr}"
        _eq_bits(errs, tag + " cls + pos[0]", got[:, 0], (cls + pos[0]).expand(Fr, C).contiguous())
        if nreg:
            _eq_bits(errs, tag + " registers", got[:, 1:1 + nreg], reg.expand(Fr, nreg, C).contiguous())
        _eq_bits(errs, tag + " patch + pos[t - nreg]", got[:, 1 + nreg:], patch.float().view(Fr, hw, C) + pos[1:])
        if not _guards_ok(buf, Fr * P * C):
            errs.append(tag + ": guards overwritten")
    _done(errs)


# ================================================================== 6. special tokens, row copy
@pytest.mark.parametrize("Fr,S", [(5, 2), (4, 1)])
@pytest.mark.parametrize("n", [1, 5])
def test_special_tokens(N, Fr, S, n):
    errs = []
    P, C = 7, 260
    g = _gen(9, Fr, S, n)
    x0, tok = torch.randn(Fr * P, C, generator=g), torch.randn(2, n, C, generator=g)
    xb = Box(x0, SENT)
    N.special_tokens(xb.v, Fr, S, P, tok.cuda())
    want = x0.clone().view(Fr, P, C)
    for f in range(Fr):
        want[f, :n] = tok[0 if f % S == 0 else 1]
    _eq_bits(errs, f"special_tokens F={Fr} S={S} n={n}", xb.got(), want.view(Fr * P, C))
    if not xb.intact():
        errs.append("columns past C or rows outside overwritten")
    _done(errs, ("special_tokens", {"first_frames": [f for f in range(Fr) if f % S == 0], **_reach_grid(Fr * n * C // 4)}))


def test_copy_rows(N):
    errs = []
    g = _gen(10)
    x = torch.randn(7, 36, generator=g)
    sb, db = Box(x, NAN), Box(torch.zeros(7, 36), SENT, cols=(16, 8))
    N.copy_rows_f32(sb.v, db.v)
    _eq_bits(errs, "copy_rows", db.got(), x)
    if not db.intact():
        errs.append("copy_rows: sentinels overwritten")
    for rs, cs in ((slice(2, 2), slice(8, 44)), (slice(2, 9), slice(8, 8))):  # rows = 0, cols = 0
        db = Box(torch.zeros(7, 36), SENT, cols=(16, 8))
        N.copy_rows_f32(sb.dev[rs, cs], db.dev[rs, slice(16, 16 + cs.stop - cs.start)])
        if not db.intact(torch.zeros(db.host.shape, dtype=torch.bool)):
            errs.append(f"copy_rows with an empty view {rs} {cs} wrote something")
    _done(errs)


# ================================================================== 7. cast
def _cast_specials():
    f = [0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -135, 2.0 ** -126, 1.0 + 2.0 ** -8,
         1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -9, 3.4028234663852886e38,
         -3.4028234663852886e38, 3.3895313892515355e38, 3.39e38, math.inf, -math.inf, 65504.0]
    return torch.tensor(f, dtype=F64).to(F32)


def test_cast_f32_bf16(N):
    errs = []
    g = _gen(11)
    x = torch.randn(5, 24, generator=g)
    sp = _cast_specials()
    x.view(-1)[:sp.numel()] = sp
    xb, yb = Box(x, NAN), Box(torch.zeros(5, 24, dtype=BF), SENT, cols=(16, 8))
    N.cast_f32_bf16(xb.v, yb.v)
    _eq_bits(errs, "cast_f32_bf16", yb.got(), x.to(BF))
    if not yb.intact():
        errs.append("cast: sentinels overwritten")
    _done(errs)


# ================================================================== 8. the grid cap
def test_grid_cap_cast_and_copy(N):
    errs = []
    rows, cols = 2056, 4096
    x = torch.randn(rows, cols, generator=_gen(12))
    xd = x.cuda()
    y = torch.full((rows, cols), SENT, dtype=BF, device="cuda")
    N.cast_f32_bf16(xd, y)
    _eq_bits(errs, "cast 2056 x 4096", y.cpu(), x.to(BF))
    del y
    z = torch.full((rows, cols), SENT, device="cuda")
    N.copy_rows_f32(xd, z)
    _eq_bits(errs, "copy_rows 2056 x 4096", z.cpu(), x)
    _done(errs, ("grid cap", _reach_grid(rows * cols // 4)))


def test_figures_norm():
    """Prints the worst figures gathered by this file (run last; DESIGN.md records them)."""
    _figures("")
    assert all(v[0] <= 2 * v[1] for k, v in FIG.items() if k[0] == "model" and "printed only" not in k[1])
