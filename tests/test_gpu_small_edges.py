"""csrc/small.hip at the edges of its tiles, k ranges, LDS limits and dispatch thresholds, per
element or per row, against fp64: vggt_linear_f32 (three forms, and _grouped),
vggt_attention_small (three kernels), vggt_headnorm_rope_f32 and the GatedUpdate prep / diff /
tail kernels (the cast is in test_gpu_norm_edges.py).  Style, boxes and rules are those of
test_gpu_train_edges.py (helpers in edge_rules.py); the form each case is labelled with is the
library's own answer (vggt_linear_f32_form, vggt_attention_small_form: `_lin_form`, `_attn_form`
below; tests/test_small_form.py pins those answers to the dispatch as it stood), printed with
the figures.

Entry point, paths reached, rule:
  vggt_linear_f32
    in-workgroup split (default, M <= 256): KW = 2 / 4 / 8 waves (K > 64 / K > 128 ...), k ranges
        of kchunk = roundup(ceil(K / KW), 64); K = 129: wave 2 holds one k, wave 3 none; K = 520:
        kchunk 128, wave 4 holds 8 k, waves 5-7 none; K % 4 != 0 (or a row stride or base that
        is not 16-B aligned): scalar loads; MT = 1 (M <= 16) / 4; one to four 64-row slabs.
    cross-workgroup split (TUNE_LINEAR_WK 0): splits doubled while blocks * splits * 2 <= 512
        and K / (2 splits) >= TUNE_LINEAR_SPLIT_K; kchunk = roundup(ceil(K / splits), 16);
        K = 520 at 32: 16 splits of 48, splits 11-15 start past K; N = 17: waves 2 and 3 have
        no column but take part in the last-block protocol; one launch bitwise two launches,
        counters left zero.
    block form without a split: M > 256 (no scratch), or TUNE_LINEAR_WK 0 with K < 2 split_k.
    exact     A integers in [-4, 4], W multiples of 1/8 in [-2, 2], integer bias and residual,
              gamma a power of two: every partial sum is a multiple of 1/16 below 2^24 / 16
              (checked on the host), so every form and every split count must give the same
              bits -- no k dropped or counted twice.  epi F32 and RESID.
    interval  random inputs: E = gamma_(K + 41) sum |terms| (K products of one rounding at
              most, K additions, <= 32 partials, bias; RESID adds its multiply and add: + 2).
    gelu      the bound of test_gpu_train_edges.py on the exact pre-activation, moved through
              |G'| <= 1.13:  |got - G(s)| <= 1.13 E + 2^-22 (|s| + E + |G(s)| + 1.13 E).
    silu      act_in = 1 computes a / (1 + expf(-a)).  expf is within 1 ulp (HIP math API), i.e.
              t = e^-a (1 + d1), |d1| <= 2 u; 1 + t rounds by u (1 + t), so the denominator is off
              by <= 2 u t + u (1 + t) <= 3 u (1 + t) relative; the fp32 division is correctly
              rounded (no fast-math flag; hipcc's default), u more.  (1 + 3 u)(1 + u) - 1 < 4 u
              (1 + 2^-20): |got - silu(a)| <= SILU |silu(a)|, SILU = 2^-22 (1 + 2^-20), for |a| <=
              20 (no overflow of expf).  Checked alone through an identity W (every other product
              is a zero), and inside the interval rule as E = (gamma_(K + 41) + SILU') sum |terms|.
    _grouped  bitwise the per-group vggt_linear_f32 call, group strides larger than the matrices.
  vggt_attention_small   model rule per (row, head), f32 and bf16, strided, batch strides > n.
    MFMA form (bf16, nq, nk <= 16, D % 16 == 0): 4 (batch, head) pairs per workgroup (pairs not a
        multiple of 4); model: fp32 scores, P = bf16(e / l) before P V.
    workgroup form: LDS ((nq + nk)(D + 1) + nk D + nq nk) 4 <= 64 KiB; (38, 38, 128): 64,448 B.
    one-wave form: LDS (2 nk (D + 1) + D) 4 <= 160 KiB; (39, 39, 128) is the first shape past the
        workgroup form (66,300 B there); (2, 79, 256) the largest: 163,448 B; second d0 trip
        for D > 64.  nk = 80 at D = 256 and nk = 129: SHAPE.
    VGGT_ATTN_SMALL_WG / _MFMA are read once per process: two fresh child processes run the
    small list with each set to 0.  Peaked (one dominant key), all-equal keys, scale != D^-1/2.
  vggt_headnorm_rope_f32   one wave per (row, head), scalar loads, any col_off; model rule.  The
        first run of this file measured the kernel at 2.50 x the model (D = 4, H = 1, M = 3,
        col_off 3, norm only: 1.28e-7 against 5.12e-8 of the head norm) and 2.07 x (D = 128, H = 3,
        norm without bias + either RoPE): fp32 sums and rsqrtf.  The kernel now takes the head's
        statistics and affine step in fp64 with one rounding; the model is the plain fp32 one.
  GatedUpdate   prep: update copy bitwise; scale = |u| carries gamma_(D + 8) / 2 + u relative,
        so |u| m within E = gamma_(D + 8) |m| |u| and |u| mean_j m within (gamma_(Nt + 2) +
        gamma_(D + 8)) (sum_j |m_j| / Nt) |u|; zero update: scale 0.  diff: bitwise one
        subtraction.  tail: model rule on well-conditioned rows (the orthogonal part keeps >= 0.1
        of |diff|, asserted on the host; where it cancels fp64 and fp32 both normalise rounding
        noise).  The defined degenerate case deltas == memory gives v = memory exactly and out =
        memory * (1 / max(sqrt(sum memory^2), 1e-12)): sum of squares over ceil(D / 64) serial
        terms, 6 tree levels and the products' roundings (gamma_(ceil(D / 64) + 7), halved by the
        root), the root, the reciprocal and the product (u each):
        |out - normalize(memory)| <= (gamma_(ceil(D / 64) + 7) / 2 + 3 u (1 + 2^-20)) |normalize(memory)|
        per element.  The model rule says nothing there: memory has unit norm, so the plain fp32
        model multiplies by exactly 1 or 1 +- one ulp by the luck of one sum (it measured 3.1e-8
        of the row norm against the kernel's 1.07e-7, 1.8 u, at D = 4) -- the figures are printed.
DESIGN.md (Norm, small and token kernel edge tests) tabulates what was measured."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from edge_rules import (BF, EPS, ERR_SHAPE, F32, F64, FIG, HN_CFG, NAN, SENT, Box, _bits, _done, _dtn, _eq_bits, _fig,
                        _figures, _gam, _gen, _guarded, _guards_ok, _hn_args, _hn_host, _interval, _model_rule,
                        _raises, _within)

pytestmark = pytest.mark.gpu

EPI_GELU, EPI_RESID, EPI_F32 = 1, 2, 3
SILU = 2.0 ** -22 * (1 + 2.0 ** -20)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------ the dispatch, asked
def _lin_form(N, M, Nn, K, **kw):
    """What linear_f32 launches for this shape under the current knobs (the library's answer), with the
    k ranges the form's kchunk gives."""
    f = N.linear_f32_form(M, Nn, K, **kw)
    r = {"form": f["name"], "grid": f["grid"], "threads": f["threads"], "kchunk": f["kchunk"]}
    if f["name"] == "in-workgroup split":
        beg = [min(K, w * f["kchunk"]) for w in range(f["kw"])]
        r.update(KW=f["kw"], MT=f["mt"], slabs=f["grid"][1], k_per_wave=[min(K, b + f["kchunk"]) - b for b in beg])
    elif f["name"] == "cross-workgroup split":
        r.update(splits=f["splits"], one_launch=f["one_launch"],
                 splits_past_K=[z for z in range(f["splits"]) if z * f["kchunk"] > K])
    return r


def _attn_form(N, dt, nq, nk, D, B=1, H=1, **kw):
    """What attention_small launches for this window in this process (the library's answer)."""
    return N.attention_small_form(N.DTYPE_BF16 if dt == BF else N.DTYPE_F32, nq, nk, D, batch=B, heads=H, **kw)


# ================================================================== 9. linear_f32
class _Tune:
    def __init__(self, N, wk=None, split_k=None, one=None):
        self.N, self.set = N, [(N.TUNE_LINEAR_WK, wk), (N.TUNE_LINEAR_SPLIT_K, split_k), (N.TUNE_LINEAR_ONE_LAUNCH, one)]

    def __enter__(self):
        self.prev = [(k, self.N.tune(k, v)) for k, v in self.set if v is not None]

    def __exit__(self, *a):
        for k, v in self.prev:
            self.N.tune(k, v)


_LIN = {}


def _lin_host(M, Nn, K, exact):
    key = (M, Nn, K, exact)
    if key not in _LIN:
        g = _gen(20, M, Nn, K, exact)
        if exact:
            a = torch.randint(-4, 5, (M, K), generator=g).float()
            w = torch.randint(-16, 17, (Nn, K), generator=g).float() / 8
            bias = torch.randint(-4, 5, (Nn,), generator=g).float()
            out0 = torch.randint(-4, 5, (M, Nn), generator=g).float()
            gam = 2.0 ** torch.randint(-1, 2, (Nn,), generator=g).float()
        else:
            a, w = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) / math.sqrt(K)
            bias, out0, gam = torch.randn(Nn, generator=g), torch.randn(M, Nn, generator=g), torch.randn(Nn, generator=g)
        d = {"a": a, "w": w, "bias": bias, "out0": out0, "gam": gam}
        for act in (0, 1):
            a64 = a.double()
            if act:
                a64 = a64 / (1 + torch.exp(-a64))
            s = a64 @ w.double().t() + bias.double()
            ab = a64.abs() @ w.double().abs().t() + bias.double().abs()
            d[act] = (s, ab)
        if exact:  # every partial sum of every order, and the residual step, in 24 bits of 1/16
            assert float((d[0][1] * gam.abs() + out0.abs()).max()) * 16 < 2 ** 24
        _LIN[key] = d
    return _LIN[key]


def _gelu64(s):
    return 0.5 * s * (1 + torch.erf(s / math.sqrt(2.0)))


def _lin_run(N, d, epi, act, a_cols=(8, 16)):
    ab, wb = Box(d["a"], NAN, cols=a_cols), Box(d["w"], NAN, rows=(1, 2))
    ob = Box(d["out0"], SENT, cols=(16, 8))
    bias, gam = d["bias"].cuda(), d["gam"].cuda()
    N.linear_f32(ab.v, wb.v, bias, ob.v, epi, act_in=act, gamma=gam if epi == EPI_RESID else None)
    return ob


def _lin_check(errs, tag, d, epi, act, ob, exact, K):
    got = ob.got()
    if not ob.intact():
        errs.append(tag + ": out sentinels overwritten")
    s, ab = d[act]
    if exact:
        want = s if epi == EPI_F32 else d["out0"].double() + d["gam"].double() * s
        _eq_bits(errs, tag, got, want.float())
        return 0.0
    rel = _gam(K + 41) + (SILU * (1 + 2.0 ** -10) if act else 0.0)
    E = rel * ab
    if epi == EPI_F32:
        r = _interval(errs, tag, got, s, E)
    elif epi == EPI_RESID:
        g64, o64 = d["gam"].double(), d["out0"].double()
        r = _interval(errs, tag, got, o64 + g64 * s, (rel + _gam(2)) * (o64.abs() + g64.abs() * ab))
    else:
        G = _gelu64(s)
        r = _within(errs, tag, got, G, 1.13 * E + 2.0 ** -22 * (s.abs() + E + G.abs() + 1.13 * E))
    _fig(("interval", "linear_f32 " + {EPI_F32: "f32", EPI_RESID: "resid", EPI_GELU: "gelu"}[epi] + (" silu" if act else "")), r)
    return r


LIN_K = [1, 9, 64, 65, 128, 129, 256, 260, 520, 1000]
LIN_M = [1, 15, 16, 17, 63, 64, 65, 256]
LIN_N = [1, 15, 16, 17, 65]


@pytest.mark.parametrize("K", LIN_K)
def test_linear_f32_in_workgroup_split(N, K):
    errs, worst = [], 0.0
    for M in LIN_M:
        for Nn in LIN_N:
            ex, rn = _lin_host(M, Nn, K, True), _lin_host(M, Nn, K, False)
            for epi in (EPI_F32, EPI_RESID):
                tag = f"linear_f32 wk exact M={M} N={Nn} K={K} epi={epi}"
                _lin_check(errs, tag, ex, epi, 0, _lin_run(N, ex, epi, 0), True, K)
            for epi in (EPI_F32, EPI_GELU, EPI_RESID):
                for act in (0, 1):
                    tag = f"linear_f32 wk M={M} N={Nn} K={K} epi={epi} act={act}"
                    worst = max(worst, _lin_check(errs, tag, rn, epi, act, _lin_run(N, rn, epi, act), False, K))
    print(f"interval linear_f32 in-workgroup K={K}: worst ratio {worst:.3f}")
    _done(errs, *[("linear_f32", M, 17, K, _lin_form(N, M, 17, K)) for M in (16, 17, 256)])


XWG = [(M, Nn, K) for K in (64, 65, 129, 520, 1000) for M in (1, 16, 17, 65) for Nn in (1, 17, 65)]


@pytest.mark.parametrize("split_k", [32, 128])
def test_linear_f32_cross_workgroup_split(N, split_k):
    """TUNE_LINEAR_WK 0: the block kernel with its K split over workgroups where the shape allows
    (and unsplit where not): exact inputs bit for bit, one launch bitwise two launches, the tile
    counters zero afterwards."""
    errs, worst, forms = [], 0.0, {}
    for M, Nn, K in XWG:
        with _Tune(N, wk=0, split_k=split_k):
            r = _lin_form(N, M, Nn, K)
        forms[r["form"]] = forms.get(r["form"], 0) + 1
        ex, rn = _lin_host(M, Nn, K, True), _lin_host(M, Nn, K, False)
        for epi in (EPI_F32, EPI_GELU, EPI_RESID):
            for act in (0, 1):
                tag = f"linear_f32 xwg split_k={split_k} M={M} N={Nn} K={K} epi={epi} act={act}"
                outs = []
                for one in (1, 0):
                    with _Tune(N, wk=0, split_k=split_k, one=one):
                        ob = _lin_run(N, rn, epi, act)
                    outs.append(ob.got())
                    worst = max(worst, _lin_check(errs, tag + f" one={one}", rn, epi, act, ob, False, K))
                    if act == 0 and epi != EPI_GELU:
                        with _Tune(N, wk=0, split_k=split_k, one=one):
                            ob = _lin_run(N, ex, epi, 0)
                        _lin_check(errs, tag + f" exact one={one}", ex, epi, 0, ob, True, K)
                _eq_bits(errs, tag + " one launch vs two", outs[0], outs[1])
    cnt = N._split_ws(torch.device("cuda"), 1)[:N.LINEAR_F32_WS_COUNTERS].cpu()
    if bool((_bits(cnt) != 0).any()):
        errs.append("tile counters not left zero")
    print(f"interval linear_f32 cross-workgroup split_k={split_k}: worst ratio {worst:.3f}; forms {forms}")
    with _Tune(N, wk=0, split_k=split_k):
        _done(errs, ("linear_f32", 16, 17, 520, _lin_form(N, 16, 17, 520)))


@pytest.mark.parametrize("M,wk", [(257, None), (300, None), (1, 0), (17, 0), (64, 0), (65, 0)])
def test_linear_f32_block_form_without_split(N, M, wk):
    errs, worst = [], 0.0
    for K in (9, 64, 65, 260) if wk is None else (9, 64, 65):
        for Nn in (1, 17, 65):
            ex, rn = _lin_host(M, Nn, K, True), _lin_host(M, Nn, K, False)
            with _Tune(N, wk=wk):
                r = _lin_form(N, M, Nn, K)
                assert r["form"] == "block, no split", r
                for epi in (EPI_F32, EPI_RESID):
                    _lin_check(errs, f"linear_f32 block exact M={M} N={Nn} K={K} epi={epi}", ex, epi, 0,
                               _lin_run(N, ex, epi, 0), True, K)
                for epi in (EPI_F32, EPI_GELU, EPI_RESID):
                    for act in (0, 1):
                        tag = f"linear_f32 block M={M} N={Nn} K={K} epi={epi} act={act}"
                        worst = max(worst, _lin_check(errs, tag, rn, epi, act, _lin_run(N, rn, epi, act), False, K))
    print(f"interval linear_f32 block M={M}: worst ratio {worst:.3f}")
    with _Tune(N, wk=wk):
        _done(errs, ("linear_f32", M, _lin_form(N, M, 17, 260)))


def test_linear_f32_silu_alone(N):
    """out = silu(a) through an identity W: every other product is a signed zero, so the output
    is the kernel's SiLU itself; |a| <= 20, the zeros, and a grid around the minimum at -1.28."""
    errs = []
    K = 16
    a = torch.cat([torch.linspace(-20, 20, 256 * K - 64), torch.linspace(-1.4, -1.1, 60),
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30])]).view(256, K)
    d = {"a": a, "w": torch.eye(K), "bias": torch.zeros(K), "out0": torch.zeros(256, K), "gam": torch.ones(K)}
    worst = 0.0
    for form, wk in (("in-workgroup", None), ("block", 0)):
        with _Tune(N, wk=wk):
            ob = _lin_run(N, d, EPI_F32, 1)
        a64 = a.double()
        ref = a64 / (1 + torch.exp(-a64))
        worst = max(worst, _within(errs, f"silu {form}", ob.got(), ref, SILU * ref.abs()))
    _fig(("bound", "silu"), worst)
    print(f"bound silu: worst error / bound {worst:.3f}")
    _done(errs)


def test_linear_f32_operands_4_bytes_off(N):
    """A view that starts 4 bytes off a 16-B boundary (a[:, 1:] of an aligned matrix) with K and the
    row strides multiples of 4: wave_linear_f32 requires aligned bases for its 16-B loads, so this
    takes the scalar loads; the sums are those of the aligned run, bit for bit."""
    errs = []
    for M, Nn, K in ((5, 17, 64), (17, 16, 260), (65, 17, 520)):
        for exact in (True, False):
            d = _lin_host(M, Nn, K, exact)
            for wk in (None, 0):
                with _Tune(N, wk=wk):
                    al, off = _lin_run(N, d, EPI_F32, 0), _lin_run(N, d, EPI_F32, 0, a_cols=(9, 15))
                assert Box(d["a"], NAN, cols=(9, 15)).v.data_ptr() % 16 == 4
                tag = f"linear_f32 A 4 bytes off M={M} N={Nn} K={K} wk={wk} exact={exact}"
                _eq_bits(errs, tag + " vs aligned", off.got(), al.got())
                _lin_check(errs, tag, d, EPI_F32, 0, off, exact, K)
    _done(errs)


@pytest.mark.parametrize("G", [1, 3])
def test_linear_f32_grouped(N, G):
    errs = []
    for M, Nn, K in ((5, 17, 129), (17, 65, 260), (64, 16, 64), (256, 1, 9)):
        g = _gen(21, G, M, Nn, K)
        abuf = torch.full((G, M + 3, K + 8), NAN)
        abuf[:, 1:1 + M, 4:4 + K] = torch.randn(G, M, K, generator=g)
        wbuf = torch.full((G, Nn * K + 16), NAN)
        wbuf[:, :Nn * K] = torch.randn(G, Nn * K, generator=g) / math.sqrt(K)
        bbuf = torch.full((G, Nn + 5), NAN)
        bbuf[:, :Nn] = torch.randn(G, Nn, generator=g)
        ad, wd, bd = abuf.cuda(), wbuf.cuda(), bbuf.cuda()
        a, w, b = ad[:, 1:1 + M, 4:4 + K], wd[:, :Nn * K].unflatten(1, (Nn, K)), bd[:, :Nn]
        for epi in (EPI_F32, EPI_GELU):
            og = torch.full((G, M + 2, Nn + 3), SENT, device="cuda")
            o1 = og.clone()
            N.linear_f32_grouped(a, w, b, og[:, 1:1 + M, 2:2 + Nn], epi)
            for i in range(G):
                N.linear_f32(a[i], w[i], b[i], o1[i, 1:1 + M, 2:2 + Nn], epi)
            tag = f"linear_f32_grouped G={G} M={M} N={Nn} K={K} epi={epi}"
            _eq_bits(errs, tag + " vs per-group calls (sentinels included)", og.cpu(), o1.cpu())
            ref = torch.einsum("gmk,gnk->gmn", abuf[:, 1:1 + M, 4:4 + K].double(), wbuf[:, :Nn * K].view(G, Nn, K).double())
            ref = ref + bbuf[:, None, :Nn].double()
            got = og[:, 1:1 + M, 2:2 + Nn].cpu()
            if epi == EPI_F32 and not torch.allclose(got.double(), ref, rtol=0, atol=1e-4):
                errs.append(tag + ": far from fp64")
    _done(errs)


# ================================================================== 10. attention_small
def _attn_inputs(dt, B, H, nq, nk, D, kind, g):
    q, k, v = (torch.randn(B, n, H, D, generator=g) for n in (nq, nk, nk))
    if kind == "peaked":  # one dominant key per (batch, head)
        j = int(torch.randint(0, nk, (1,), generator=g))
        k[:, j] = 3.0 * q[:, 0] / q[:, 0].norm(dim=-1, keepdim=True) * math.sqrt(D)
    elif kind == "equal":
        k[:] = k[:, :1].clone()
    return q.to(dt), k.to(dt), v.to(dt)


def _attn_host(q, k, v, scale, form, calc):
    """[B, n, H, D] -> o [B, nq, H, D] in `calc` arithmetic; fp32 restates the form's documented
    steps (workgroup: P = e (1 / l) then P V; one-wave: (e V)(1 / l); mfma: P rounded to bf16)."""
    qc, kc, vc = (t.to(calc).permute(0, 2, 1, 3) for t in (q, k, v))
    s = (qc @ kc.transpose(-1, -2)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    l = e.sum(-1, keepdim=True)
    if calc == F64:
        o = (e / l) @ vc
    elif form == "mfma":
        o = (e * (1.0 / l)).to(BF).float() @ vc
    elif form == "workgroup":
        o = (e * (1.0 / l)) @ vc
    else:
        o = (e @ vc) * (1.0 / l)
    return o.permute(0, 2, 1, 3)


def _attn_case(N, errs, dt, B, H, nq, nk, D, kind="random", scale=None):
    g = _gen(30, dt == BF, B, H, nq, nk, D, len(kind))
    q, k, v = _attn_inputs(dt, B, H, nq, nk, D, kind, g)
    sc = D ** -0.5 if scale is None else scale
    qbs, kbs, obs = nq + 2, nk + 1, nq + 3

    def rows(t, n, bs, fill):
        full = torch.full((B, bs, H * D), fill, dtype=dt)
        full[:, :n] = t.reshape(B, n, H * D)
        return Box(full.view(B * bs, H * D), fill)

    qb, kb, vb = rows(q, nq, qbs, NAN), rows(k, nk, kbs, NAN), rows(v, nk, kbs, NAN)
    ob = Box(torch.full((B * obs, H * D), SENT, dtype=dt), SENT, cols=(16, 8))
    views = (qb.v, kb.v, vb.v, ob.v)
    align = min(16, *(t.data_ptr() & -t.data_ptr() for t in views))
    form = _attn_form(N, dt, nq, nk, D, B, H, ptr_align=align, **{"ld" + n: t.stride(0) for n, t in zip("qkvo", views)})["name"]
    N.attention_small(qb.v, kb.v, vb.v, ob.v, B, H, nq, nk, D, qbs, kbs, obs, scale=sc)
    full = ob.got().reshape(B, obs, H, D)
    got = full[:, :nq]
    tag = f"attention_small {_dtn(dt)} [{form}] B={B} H={H} ({nq},{nk},{D}) {kind} scale={sc:.4f}"
    if not ob.intact() or bool((full[:, nq:].float() != SENT).any()):
        errs.append(tag + ": rows past nq or sentinels overwritten")
    ref = _attn_host(q, k, v, sc, form, F64)
    mod = _attn_host(q, k, v, sc, form, F32).to(dt)
    _model_rule(errs, tag, got, mod, ref, f"attention_small {_dtn(dt)} {form}")
    return form


MFMA_NQK = [(1, 1), (16, 16), (16, 5), (3, 13)]
SMALL_LIST = [(1, 1, 16), (3, 13, 48), (16, 5, 64), (17, 16, 64), (16, 17, 64), (4, 4, 24), (5, 7, 6), (16, 16, 128),
              (3, 64, 68), (3, 65, 68)]  # the last two: both lanes' keys and a second d0 trip on the one-wave form


@pytest.mark.parametrize("D", [16, 48, 64, 128, 256])
def test_attention_small_mfma(N, D):
    errs = []
    for nq, nk in MFMA_NQK:
        for B, H in ((1, 1), (5, 1), (7, 2)):
            assert _attn_case(N, errs, BF, B, H, nq, nk, D) == "mfma"
    for kind, sc in (("peaked", None), ("equal", None), ("random", 0.3)):
        _attn_case(N, errs, BF, 3, 2, 16, 5, D, kind, sc)
    _done(errs, ("attention_small", {"pairs": [1, 5, 14], "workgroups": [1, 2, 4], "lds_bytes": 4 * 16 * D * 2}))


@pytest.mark.parametrize("dt", [F32, BF], ids=_dtn)
def test_attention_small_workgroup(N, dt):
    errs, forms = [], []
    for nq, nk, D in SMALL_LIST + [(38, 38, 128)]:
        forms.append(((nq, nk, D), _attn_case(N, errs, dt, 2, 3, nq, nk, D), _attn_form(N, dt, nq, nk, D, 2, 3)["lds"]))
    for kind, sc in (("peaked", None), ("equal", None), ("random", 0.3)):
        _attn_case(N, errs, dt, 3, 2, 17, 7, 64, kind, sc)
    assert all(f == ("mfma" if dt == BF and nq <= 16 and nk <= 16 and D % 16 == 0 else "workgroup")
               for (nq, nk, D), f, _ in forms)
    _done(errs, ("attention_small", forms))


@pytest.mark.parametrize("dt", [F32, BF], ids=_dtn)
def test_attention_small_one_wave(N, dt):
    errs, forms = [], []
    for nq, nk, D in [(39, 39, 128), (3, 128, 68), (3, 64, 200), (3, 65, 200), (2, 79, 256)]:
        f = _attn_case(N, errs, dt, 2, 1 if D == 256 else 2, nq, nk, D)
        forms.append(((nq, nk, D), f, _attn_form(N, dt, nq, nk, D)["lds"]))
        assert f == "one-wave"
    for kind, sc in (("peaked", None), ("equal", None), ("random", 0.3)):
        _attn_case(N, errs, dt, 2, 2, 3, 128, 68, kind, sc)
    _done(errs, ("attention_small", forms))


def test_attention_small_shape_errors(N):
    for nq, nk, D in ((2, 80, 256), (1, 129, 16)):
        assert _attn_form(N, F32, nq, nk, D)["rc"] == ERR_SHAPE
        t = torch.zeros(nk + nq, D, device="cuda")
        _raises(ERR_SHAPE, N.attention_small, t, t, t, t, 1, 1, nq, nk, D, nq, nk, nq)
    torch.cuda.synchronize()


def _attn_small_sweep(N):
    """The small list on the forms the two environment switches leave (a child process)."""
    out = {}
    for dt in (F32, BF):
        for nq, nk, D in SMALL_LIST:
            errs = []
            form = _attn_case(N, errs, dt, 2, 3, nq, nk, D)
            out[f"{_dtn(dt)},{nq},{nk},{D}"] = {"form": form, "errs": errs}
    figs = {str(k): v for k, v in FIG.items()}
    return out, figs


_CHILD = """
import json
import torch
from aligned_vggt import _native as N
import test_gpu_small_edges as T
N.lib()
res, figs = T._attn_small_sweep(N)
torch.cuda.synchronize()
print(json.dumps({"cases": res, "figs": figs}))
"""


@pytest.mark.parametrize("var", ["VGGT_ATTN_SMALL_WG", "VGGT_ATTN_SMALL_MFMA"])
def test_attention_small_other_forms_in_a_fresh_process(N, var):
    """Both switches are read once per process: a fresh interpreter with one of them set to 0 runs
    the small list -- without the workgroup form every shape lands on the one-wave kernel (or, bf16
    up to 16 x 16, on the matrix cores); without the matrix-core form bf16 lands on the workgroup
    kernel -- and reports the failures of each case as JSON."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    env[var] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got["cases"]) == 2 * len(SMALL_LIST)
    forms = {k: c["form"] for k, c in got["cases"].items()}
    if var == "VGGT_ATTN_SMALL_WG":
        assert set(forms.values()) == {"one-wave", "mfma"} and forms["f32,3,13,48"] == "one-wave"
    else:
        assert set(forms.values()) == {"workgroup"}
    for k, v in got["figs"].items():
        print("figure (child, %s=0)" % var, k, v)
    print("reach", forms)
    bad = {k: c["errs"] for k, c in got["cases"].items() if c["errs"]}
    assert not bad, json.dumps(bad, indent=1)[:4000]


# ================================================================== 11. headnorm_rope_f32
@pytest.mark.parametrize("D", [4, 60, 64, 68, 128, 1024])
def test_headnorm_rope_f32(N, D):
    errs = []
    for H in (1, 3):
        for col_off in (0, 3):
            g = _gen(40, D, H, col_off)
            w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
            for M in (1, 3):
                x = torch.randn(M, col_off + H * D + 5, generator=g)
                for aff, mode in HN_CFG:
                    rope, cos, sin = _hn_args(mode, D, g)
                    w0, b0 = (w if aff != "none" else None), (b if aff == "wb" else None)
                    tag = f"headnorm_rope_f32 D={D} H={H} M={M} col_off={col_off} {aff} mode={mode}"
                    xb = Box(x, SENT)
                    N.headnorm_rope_any(xb.v, col_off, H, D, None if w0 is None else w0.cuda(),
                                        None if b0 is None else b0.cuda(), EPS, *rope)
                    got = xb.got()
                    _eq_bits(errs, tag + " columns before", got[:, :col_off], x[:, :col_off])
                    _eq_bits(errs, tag + " columns after", got[:, col_off + H * D:], x[:, col_off + H * D:])
                    if not xb.intact():
                        errs.append(tag + ": sentinels overwritten")
                    xin = x[:, col_off:col_off + H * D]
                    ref = _hn_host(xin, D, H, H, w0, b0, w0, b0, mode, cos, sin, F64)
                    mod = _hn_host(xin, D, H, H, w0, b0, w0, b0, mode, cos, sin, F32)
                    _model_rule(errs, tag, got[:, col_off:col_off + H * D].reshape(M, H, D), mod, ref,
                                "headnorm_rope_f32")
            xb0, xb1 = Box(x, SENT), Box(x, SENT)  # w NULL: b is ignored
            rope, _, _ = _hn_args(2, D, g)
            N.headnorm_rope_any(xb0.v, col_off, H, D, None, None, EPS, *rope)
            N.headnorm_rope_any(xb1.v, col_off, H, D, None, b.cuda(), EPS, *rope)
            _eq_bits(errs, f"headnorm_rope_f32 D={D} (NULL, b) vs (NULL, NULL)", xb1.got(), xb0.got())
    _done(errs, ("headnorm_rope_f32", {"D": D, "trips_over_d": -(-D // 64), "lds_bytes": 4 * D}))


def test_headnorm_rope_f32_shape_errors(N):
    for D in (6, 1028):
        buf = torch.zeros(2, 2 * D, device="cuda")
        _raises(ERR_SHAPE, N.headnorm_rope_any, buf, 0, 1, D, None, None, EPS)
    torch.cuda.synchronize()


# ================================================================== 12. GatedUpdate
GU = [(B, Nt, D) for B in (1, 3) for Nt in (1, 5, 8) for D in (4, 96, 260, 1024)]


@pytest.mark.parametrize("zero_update", [0, 1])
def test_gated_update_prep_and_diff(N, zero_update):
    errs, worst = [], 0.0
    for B, Nt, D in GU:
        g = _gen(50, B, Nt, D)
        mem = torch.randn(B, Nt, D, generator=g)
        upd = torch.randn(B, D, generator=g) * (0.0 if zero_update else 1.0)
        if not zero_update and B > 1:
            upd[1] = 0.0  # one batch entry with scale 0 beside live ones
        dl = torch.randn(B, Nt, D, generator=g)
        ibuf, inp = _guarded((B * Nt, 3 * D), F32)
        gbuf, gin = _guarded((B * Nt, 2 * D), F32)
        md = mem.cuda()
        N.gated_update_prep(md, upd.cuda(), inp, gin)
        N.gated_update_diff(md, dl.cuda(), gin)
        gi, gg = inp.cpu().view(B, Nt, 3 * D), gin.cpu().view(B, Nt, 2 * D)
        tag = f"gated_update B={B} Nt={Nt} D={D} zero={zero_update}"
        _eq_bits(errs, tag + " update copy", gi[..., :D], upd[:, None].expand(B, Nt, D).contiguous())
        _eq_bits(errs, tag + " diff", gg[..., :D], dl - mem)
        _eq_bits(errs, tag + " g_in second half vs inp", gg[..., D:], gi[..., D:2 * D])
        sc = upd.double().norm(dim=-1)[:, None, None]
        m64 = mem.double()
        rel = _gam(D + 8)
        worst = max(worst, _interval(errs, tag + " |u| m", gi[..., D:2 * D].contiguous(), m64 * sc, rel * m64.abs() * sc))
        mean = m64.mean(1, keepdim=True).expand(B, Nt, D)
        Em = (_gam(Nt + 2) + rel) * m64.abs().mean(1, keepdim=True).expand(B, Nt, D) * sc
        worst = max(worst, _interval(errs, tag + " |u| mean", gi[..., 2 * D:].contiguous(), mean * sc, Em))
        zero = (upd.abs().sum(-1) == 0)
        if bool(zero.any()) and bool((gi[zero][..., D:] != 0).any()):
            errs.append(tag + ": zero update does not give scale 0")
        if not (_guards_ok(ibuf, inp.numel()) and _guards_ok(gbuf, gin.numel())):
            errs.append(tag + ": guards overwritten")
    _fig(("interval", "gated_update_prep"), worst)
    print(f"interval gated_update_prep: worst ratio {worst:.3f}")
    _done(errs)


def _tail_host(mem, dl, logit, calc):
    """fp64: the reference.  fp32: the kernel's documented steps -- both normalisations multiply by
    a reciprocal 1 / max(sqrt(sum of squares), 1e-12)."""
    m, d, lg = mem.to(calc), dl.to(calc), logit.to(calc)
    diff = d - m
    dot = (diff * m).sum(-1, keepdim=True)
    o = diff - dot * m
    gate = 1.0 / (1.0 + torch.exp(-lg))[..., None]
    if calc == F64:
        o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        v = m + gate * o
        return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    o = o * (1.0 / (o * o).sum(-1, keepdim=True).sqrt().clamp_min(1e-12))
    v = m + gate * o
    return v * (1.0 / (v * v).sum(-1, keepdim=True).sqrt().clamp_min(1e-12))


@pytest.mark.parametrize("degenerate", [0, 1])
def test_gated_update_tail(N, degenerate):
    errs = []
    for B, Nt, D in GU:
        g = _gen(51, B, Nt, D)
        mem = torch.randn(B * Nt, D, generator=g)
        mem = (mem / mem.norm(dim=-1, keepdim=True)).contiguous()
        diff = torch.randn(B * Nt, D, generator=g)
        dl = mem.clone() if degenerate else mem + diff
        logit = torch.randn(B * Nt, generator=g) * 2
        if not degenerate:
            d64 = dl.double() - mem.double()
            o64 = d64 - (d64 * mem.double()).sum(-1, keepdim=True) * mem.double()
            assert bool((o64.norm(dim=-1) >= 0.1 * d64.norm(dim=-1)).all()), (B, Nt, D)
        obuf, out = _guarded((B * Nt, D), F32)
        N.gated_update_tail(mem.cuda(), dl.cuda(), logit.cuda(), out)
        tag = f"gated_update_tail B={B} Nt={Nt} D={D}" + (" deltas == memory" if degenerate else "")
        ref = _tail_host(mem, dl, logit, F64)
        if degenerate:
            assert torch.allclose(ref, mem.double() / mem.double().norm(dim=-1, keepdim=True), rtol=0, atol=1e-15)
        if degenerate:
            rel = _gam(-(-D // 64) + 7) / 2 + 3 * 2.0 ** -24 * (1 + 2.0 ** -20)
            r = _within(errs, tag, out.cpu(), ref, rel * ref.abs())
            _fig(("bound", "gated_update_tail degenerate"), r)
            _model_rule([], tag, out.cpu(), _tail_host(mem, dl, logit, F32), ref, "(printed only) tail degenerate")
        else:
            _model_rule(errs, tag, out.cpu(), _tail_host(mem, dl, logit, F32), ref, "gated_update_tail")
        if not _guards_ok(obuf, out.numel()):
            errs.append(tag + ": guards overwritten")
    _done(errs)


# ================================================================== 13. NULL pointers, first calls from two threads
# Each case sets one required pointer of an otherwise valid call to NULL: VGGT_ERR_SHAPE, and the
# buffers behind every other pointer (guards included) keep their bits -- nothing was launched.
NULL_ARGS = {
    "vggt_linear_f32": "A lda W ldw bias M N K act epi out ldo gamma",
    "vggt_linear_f32_ws": "A lda W ldw bias M N K act epi out ldo gamma ws ws_bytes",
    "vggt_linear_f32_grouped": "A lda a_gs W ldw w_gs bias b_gs M N K groups act epi out ldo o_gs",
    "vggt_attention_small": "q ldq qbs k ldk kbs v ldv o ldo obs dtype batch heads nq nk D scale",
    "vggt_headnorm_rope_f32": "buf ld col_off Mh H Dh w b eps mode pos period cos sin tab",
    "vggt_gated_update_prep": "memory update B Nt Dg inp g_in",
    "vggt_gated_update_diff": "memory deltas rows Dg g_in",
    "vggt_gated_update_tail": "memory deltas logit rows Dg tail_out",
    "vggt_cast_f32_bf16": "x ldx y ldy crows ccols",
}
NULL_RULES = {
    "vggt_linear_f32": ("A", "W", "out", "gamma"),
    "vggt_linear_f32_ws": ("A", "W", "out", "gamma"),
    "vggt_linear_f32_grouped": ("A", "W", "out"),
    "vggt_attention_small": ("q", "k", "v", "o"),
    "vggt_headnorm_rope_f32": ("buf",),
    "vggt_gated_update_prep": ("memory", "update", "inp", "g_in"),
    "vggt_gated_update_diff": ("memory", "deltas", "g_in"),
    "vggt_gated_update_tail": ("memory", "deltas", "logit", "tail_out"),
    "vggt_cast_f32_bf16": ("x", "y"),
}


def test_null_pointers_are_shape_errors(N):
    L, st = N.lib(), N._stream()
    g = _gen(60)
    shapes = {"A": (3, 8), "W": (17, 8), "bias": (1, 17), "out": (3, 24), "gamma": (1, 17), "ws": (1, 4096),
              "q": (2, 16), "k": (2, 16), "v": (2, 16), "o": (2, 16), "buf": (3, 8), "w": (1, 4), "b": (1, 4),
              "memory": (2, 4), "update": (1, 4), "deltas": (2, 4), "logit": (1, 2), "inp": (2, 12), "g_in": (2, 8),
              "tail_out": (2, 4), "x": (3, 8)}
    bufs = {k: Box(torch.randn(*sh, generator=g), SENT) for k, sh in shapes.items()}
    bufs["y"] = Box(torch.randn(3, 8, generator=g).to(BF), SENT)
    addr = {k: b.v.data_ptr() for k, b in bufs.items()}
    ld = {k: b.v.stride(0) for k, b in bufs.items()}
    # M = 3, N = 17, K = 5; nq = nk = 2, D = 16; head norm D = 4, H = 1, M = 3; GatedUpdate rows = 2, D = 4
    base = dict(addr, lda=ld["A"], ldw=ld["W"], ldo=ld["out"], M=3, N=17, K=5, act=0, epi=EPI_RESID, ws_bytes=4096 * 4,
                a_gs=0, w_gs=0, b_gs=0, o_gs=0, groups=1, ldq=ld["q"], ldk=ld["k"], ldv=ld["v"], qbs=2, kbs=2, obs=2,
                dtype=N.DTYPE_F32, batch=1, heads=1, nq=2, nk=2, D=16, scale=0.25, ld=ld["buf"], col_off=0,
                Mh=3, H=1, Dh=4, eps=EPS, mode=0, pos=None, period=1, cos=None, sin=None, tab=0, B=1, Nt=2,
                Dg=4, rows=2, ldx=ld["x"], ldy=ld["y"], crows=3, ccols=8)
    bad = []
    for entry, names in NULL_ARGS.items():
        args = dict(base, epi=EPI_F32) if entry == "vggt_linear_f32_grouped" else dict(base)
        if entry == "vggt_attention_small":
            args["ldo"] = ld["o"]
        for null in NULL_RULES[entry]:
            rc = getattr(L, entry)(*[None if k == null else args[k] for k in names.split()], st)
            if rc != ERR_SHAPE:
                bad.append(f"{entry} with {null} NULL: returned {rc}, want {ERR_SHAPE}")
    torch.cuda.synchronize()
    for k, b in bufs.items():
        if not torch.equal(_bits(b.dev.cpu()), _bits(b.host)):
            bad.append(f"buffer {k} was written by a refused call")
    assert not bad, "\n".join(bad)


_TWO_THREADS = """
import hashlib, json, threading
import torch
from aligned_vggt import _native as N
import edge_rules as R
N.lib()
nq, nk, D = 2, 79, 256
assert N.attention_small_form(N.DTYPE_F32, nq, nk, D)["name"] == "one-wave" and N.attention_small_form(N.DTYPE_F32, nq, nk, D)["lds"] > 65536
g = R._gen(61)
q, k, v = (torch.randn(n, D, generator=g).cuda() for n in (nq, nk, nk))
outs = [torch.full((nq + 2, D), R.SENT, device="cuda") for _ in range(3)]
streams = [torch.cuda.Stream() for _ in range(2)]
torch.cuda.synchronize()
gate, errs = threading.Barrier(2), []
def first_call(i):
    try:
        with torch.cuda.stream(streams[i]):
            gate.wait()
            N.attention_small(q, k, v, outs[i][1:1 + nq], 1, 1, nq, nk, D, nq, nk, nq)
    except Exception as e:
        errs.append(repr(e))
ts = [threading.Thread(target=first_call, args=(i,)) for i in range(2)]
[t.start() for t in ts]
[t.join() for t in ts]
torch.cuda.synchronize()
N.attention_small(q, k, v, outs[2][1:1 + nq], 1, 1, nq, nk, D, nq, nk, nq)
torch.cuda.synchronize()
print(json.dumps({"errs": errs, "sha": [hashlib.sha256(R._bits(o.cpu()).numpy().tobytes()).hexdigest() for o in outs],
                  "finite": bool(torch.isfinite(outs[2]).all()), "guards": bool((outs[2][0] == R.SENT).all() and (outs[2][-1] == R.SENT).all())}))
"""


def test_attention_small_first_calls_from_two_threads(N):
    """The one-wave form at (2, 79, 256) needs 163,448 B of dynamic LDS, which the kernel may only ask for
    once its attribute is set; the entry sets it on its first call.  Two host threads make the first two
    calls of a fresh process at once (on a stream each): both outputs, guard rows included, are the bits of
    a third, single-threaded call."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", _TWO_THREADS], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert not got["errs"], got["errs"]
    assert got["finite"] and got["guards"]
    assert got["sha"][0] == got["sha"][2] == got["sha"][1], got["sha"]


def test_figures_small():
    """Prints the worst figures gathered by this file (run last; DESIGN.md records them)."""
    _figures("")
    assert all(v[0] <= 2 * v[1] for k, v in FIG.items() if k[0] == "model" and "printed only" not in k[1])
