"""Flash-attention forward (vggt_attention_fwd, _fwd_lse, _stamps) and backward
(vggt_attention_bwd) at the edges of their tiles: nq != nk, counts around the
32 / 64 / 128 tile sizes, every batch stride and leading dimension distinct,
non-finite padding and sentinel-filled outputs.

Inputs are unit-variance bf16 values drawn on the host (H = 2 throughout); the
reference is fp64 on the host from those bf16 values: softmax(q k^T D^-1/2) v,
logsumexp * log2(e) and fp64 autograd for dq / dk / dv.

Metric: per (batch, head, row)  ||got_row - ref_row||_2 / sqrt(mean_rows ||ref_row||_2^2);
the worst row is asserted (the denominator is the tensor-wide RMS row norm: a row's
own norm blows up on legitimately tiny gradient rows under a peaked softmax).

Bar: a rounding model, computed here for the same inputs, restates the op in plain
torch with the kernels' documented rounding points and nothing else:
  forward   q * (scale log2 e) rounded to bf16 (prescaling forms only: VAR & 32
            without & 64), fp32 scores, p = exp2(s - m), bf16(p) @ v in fp32, divided
            by the fp32 row sum of the unrounded p -- of the rounded p in the
            exact-score form (96, vggt_attention_fwd_lse) --, rounded to bf16.
            m is the row max for the legacy forms and the row's offset for the
            offset-free ones (VAR & 32): 0 when the max of its first 64 keys lies in
            [-60, 60] log2 units, as it does for every input here (the exact-score
            form always takes that first-tile max).  Offset 0 is a
            rounding point of its own: the largest p is then no power of two, and its
            bf16 rounding (<= 2^-8) does not cancel against the unrounded sum -- with one
            key o = v (1 + eps) (measured: 6e-3 worst row where a max-subtracting model
            has 0);
  backward  P and dS rounded to bf16 before their matrix products,
            delta = sum dO * bf16(O) with the O of the exact-score forward,
            dq / dk / dv rounded to bf16.
The kernel's worst row must be <= FACTOR x the model's worst row.  FACTOR = 2: the
kernels also re-associate fp32 sums per tile and rescale by exp2(m_tile - m) where an
offset moves, both below one bf16 rounding of p.
DESIGN.md (attention edge tests) tabulates model and measured values."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2
FACTOR = 2.0
LOG2E = math.log2(math.e)
SENTINEL = 7.0

RECT = [(1, 129), (129, 1), (33, 64), (64, 33), (65, 128), (128, 65), (130, 200), (257, 63)]
SQUARE = [(n, n) for n in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
SHAPES = RECT + SQUARE
WIDE = (4100, 130)  # the 8-wave form (nq >= 4096)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------ host side: inputs, fp64 reference, rounding model
def _heads(x, B, n, D):
    """[B * n, H * D] -> [B, H, n, D]"""
    return x.view(B, n, H, D).permute(0, 2, 1, 3)


def _rows(x):
    """[B, H, n, D] -> [B * n, H * D]"""
    B, _, n, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * n, H * D)


def _bf(x):
    return x.to(torch.bfloat16)


def _ref64(q, k, v, do, B, nq, nk, D):
    """fp64 o, lse (log2 units, [B * H * nq]) and, with do, autograd dq / dk / dv; all as [B * n, C]."""
    qh = _heads(q.double(), B, nq, D).clone().requires_grad_(do is not None)
    kh = _heads(k.double(), B, nk, D).clone().requires_grad_(do is not None)
    vh = _heads(v.double(), B, nk, D).clone().requires_grad_(do is not None)
    s = (qh @ kh.transpose(-1, -2)) * D ** -0.5
    o = torch.softmax(s, -1) @ vh
    out = {"o": _rows(o.detach()), "lse": (torch.logsumexp(s.detach(), -1) * LOG2E).reshape(-1)}
    if do is not None:
        o.backward(_heads(do.double(), B, nq, D))
        out.update(dq=_rows(qh.grad), dk=_rows(kh.grad), dv=_rows(vh.grad))
    return out


def _model_fwd(q, k, v, B, nq, nk, D, form):
    """The forward's documented rounding points in fp32 torch -> bf16 o [B * nq, C].
    form: "legacy" (row max), "prescale" (offset-free, q prescaled) or "exact" (exact scores,
    the first tile's row max as offset, divided by the sum of the rounded p)."""
    c = torch.tensor(D ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qh, kh, vh = _heads(q.float(), B, nq, D), _heads(k.float(), B, nk, D), _heads(v.float(), B, nk, D)
    if form == "prescale":
        s = _bf(qh * c).float() @ kh.transpose(-1, -2)
    else:
        s = (qh @ kh.transpose(-1, -2)) * c
    if form == "legacy":
        m = s.amax(-1, keepdim=True)
    else:
        m1 = s[..., :64].amax(-1, keepdim=True)  # the row's first tile fixes its offset
        # (later moves of the offset, when a tile's max exceeds it by > 3, are left out)
        m = m1 if form == "exact" else torch.where(m1.abs() <= 60.0, torch.zeros_like(m1), m1)
    p = torch.exp2(s - m)
    pb = _bf(p).float()
    o = (pb @ vh) / (pb if form == "exact" else p).sum(-1, keepdim=True)
    return _rows(_bf(o))


def _model_bwd(q, k, v, do, B, nq, nk, D):
    """The backward's documented rounding points in fp32 torch -> bf16 dq, dk, dv."""
    scale = D ** -0.5
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qh, kh, vh = _heads(q.float(), B, nq, D), _heads(k.float(), B, nk, D), _heads(v.float(), B, nk, D)
    gh = _heads(do.float(), B, nq, D)
    oh = _heads(_model_fwd(q, k, v, B, nq, nk, D, "exact").float(), B, nq, D)
    s = (qh @ kh.transpose(-1, -2)) * c
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))))
    delta = (gh * oh).sum(-1, keepdim=True)
    ds = _bf(p * (gh @ vh.transpose(-1, -2) - delta)).float()
    dq = _bf((ds @ kh) * scale)
    dk = _bf((ds.transpose(-1, -2) @ qh) * scale)
    dv = _bf(_bf(p).float().transpose(-1, -2) @ gh)
    return {"dq": _rows(dq), "dk": _rows(dk), "dv": _rows(dv)}


def _row_err(got, ref, D):
    """(worst row, whole-tensor relative L2) of a [rows, H * D] result against the fp64 reference."""
    g, r = got.double().reshape(-1, D), ref.double().reshape(-1, D)  # one row per (batch, token, head)
    num = (g - r).norm(dim=1)
    den = r.norm(dim=1).pow(2).mean().sqrt()
    return (num.max() / den).item(), ((g - r).norm() / r.norm()).item()


_CASES = {}


def _case(B, nq, nk, D, amp=1.0, grads=True):
    """Inputs, fp64 reference and model results of one shape, computed once and left unchanged."""
    key = (B, nq, nk, D, amp, grads)
    if key not in _CASES:
        C = H * D
        g = torch.Generator().manual_seed(1000 * nq + 10 * nk + D + B)
        q = _bf(torch.randn(B * nq, C, generator=g) * amp)
        k = _bf(torch.randn(B * nk, C, generator=g) * amp)
        v = _bf(torch.randn(B * nk, C, generator=g))
        do = _bf(torch.randn(B * nq, C, generator=g))
        ref = _ref64(q, k, v, do if grads else None, B, nq, nk, D)
        model = {"o_" + f: _model_fwd(q, k, v, B, nq, nk, D, f) for f in ("legacy", "prescale", "exact")}
        if grads:
            model.update(_model_bwd(q, k, v, do, B, nq, nk, D))
        _CASES[key] = {"q": q, "k": k, "v": v, "do": do, "ref": ref, "model": model}
    return _CASES[key]


def _check(what, got, ref, model, D, fails):
    """Print the figures, then record a miss of the model bar in `fails`."""
    e_k, l2_k = _row_err(got, ref, D)
    e_m, l2_m = _row_err(model, ref, D)
    print(f"{what}: worst row kernel {e_k:.3e} model {e_m:.3e} (x{e_k / max(e_m, 1e-30):.2f}); "
          f"rel-L2 kernel {l2_k:.3e} model {l2_m:.3e}")
    if not torch.isfinite(got.float()).all():
        fails.append(f"{what}: non-finite values")
    elif not e_k <= FACTOR * e_m:
        fails.append(f"{what}: worst row {e_k:.3e} > {FACTOR} x model {e_m:.3e}")


# ------------------------------------------------------------------ launches
# form -> (variant, attn16, waves, the model's form)
FORMS = {"default": (33, 0, 4, "prescale"), "mfma16": (161, 0, 4, "prescale"), "exact": (96, 0, 4, "exact"),
         "legacy": (3, 0, 4, "legacy"), "two_wave": (33, 0, 2, "prescale"), "eight_wave": (33, 0, 8, "prescale")}


class _Knobs:
    """The attention knobs of one form, restored on exit."""

    def __init__(self, N, form):
        self.N, self.form = N, form

    def __enter__(self):
        N = self.N
        var, a16, waves, _ = FORMS[self.form]
        self.prev = [(N.TUNE_ATTN_VARIANT, N.tune(N.TUNE_ATTN_VARIANT, var)),
                     (N.TUNE_ATTN16, N.tune(N.TUNE_ATTN16, a16)),
                     (N.TUNE_ATTN_WAVES, N.tune(N.TUNE_ATTN_WAVES, waves)),
                     (N.TUNE_ATTN_TAIL_SPLIT, N.tune(N.TUNE_ATTN_TAIL_SPLIT, -1))]
        return self

    def __exit__(self, *exc):
        for knob, val in reversed(self.prev):
            self.N.tune(knob, val)
        return False


def _fwd(N, form, cs, B, nq, nk, D):
    o = torch.full((B * nq, H * D), SENTINEL, device="cuda", dtype=torch.bfloat16)
    with _Knobs(N, form):
        N.attention(cs["q"].cuda(), cs["k"].cuda(), cs["v"].cuda(), o, B, H, nq, nk, D, nq, nk, nq)
        torch.cuda.synchronize()
    return o.cpu()


def _fwd_lse(N, cs, B, nq, nk, D):
    o = torch.full((B * nq, H * D), SENTINEL, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B * H * nq,), SENTINEL, device="cuda")
    N.attention_fwd_lse(cs["q"].cuda(), cs["k"].cuda(), cs["v"].cuda(), o, lse, B, H, nq, nk, D, nq, nk, nq)
    torch.cuda.synchronize()
    return o, lse


def _bwd(N, cs, o, lse, B, nq, nk, D):
    C = H * D
    dq = torch.full((B * nq, C), SENTINEL, device="cuda", dtype=torch.bfloat16)
    dkv = torch.full((B * nk, 2 * C), SENTINEL, device="cuda", dtype=torch.bfloat16)
    N.attention_bwd(cs["q"].cuda(), cs["k"].cuda(), cs["v"].cuda(), o, cs["do"].cuda(), lse, dq, dkv[:, :C], dkv[:, C:],
                    B, H, nq, nk, D, nq, nk, nq)
    torch.cuda.synchronize()
    return {"dq": dq.cpu(), "dk": dkv[:, :C].cpu(), "dv": dkv[:, C:].cpu()}


def _check_lse(what, lse, ref, fails):
    e = (lse.double().cpu() - ref).abs().max().item()
    print(f"{what}: lse max abs err {e:.3e} (log2 units)")
    if not e <= 2e-3:
        fails.append(f"{what}: lse error {e:.3e} > 2e-3")


def _check_grads(what, got, cs, nk, D, fails):
    """dq / dk / dv against fp64 autograd under the model bar; with one key dq and dk are exactly 0."""
    for nm in ("dq", "dk", "dv"):
        if nk == 1 and nm != "dv":
            # dS = P (dP - delta) with P = 1 and delta = dO . O = dO . v = dP (the training forward
            # gives O = v bit for bit): the only residue is the fp32 re-association between the
            # MFMA's dO . v and sum dO * O, ~2^-24 sqrt(D) ~ 1e-6, times scale |k| ~ 0.1
            a = got[nm].float().abs().max().item()
            print(f"{what} {nm}: max abs {a:.3e} (reference exactly 0)")
            if not a <= 1e-5:
                fails.append(f"{what} {nm}: max abs {a:.3e} > 1e-5 with one key")
        else:
            _check(f"{what} {nm}", got[nm], cs["ref"][nm], cs["model"][nm], D, fails)


# ------------------------------------------------------------------ 1. forward, rectangular and edge counts
@pytest.mark.parametrize("form,D", [("default", 64), ("default", 128), ("mfma16", 64), ("exact", 64), ("exact", 128),
                                    ("legacy", 64), ("legacy", 128), ("two_wave", 64), ("two_wave", 128),
                                    ("eight_wave", 64), ("eight_wave", 128)])
def test_forward_rectangular(N, form, D):
    """Every rectangular and edge shape through one 4-wave or 2-wave forward form; the 8-wave
    form (nq >= 4096; D = 64 is the default path, variant 2081, D = 128 variant 33) at its one shape."""
    fails = []
    for nq, nk in ([WIDE] if form == "eight_wave" else SHAPES):
        cs = _case(1, nq, nk, D, grads=form != "eight_wave")
        o = _fwd(N, form, cs, 1, nq, nk, D)
        _check(f"fwd {form} D={D} ({nq},{nk})", o, cs["ref"]["o"], cs["model"]["o_" + FORMS[form][3]], D, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 2. / 4. strides and poison
def _padded(x, B, n, bstride, ld, fill):
    """[B * n, C] -> a [B * bstride, ld] buffer holding batch b's rows at b * bstride, `fill` elsewhere."""
    C = x.shape[1]
    buf = torch.full((B * bstride, ld), fill, dtype=x.dtype)
    for b in range(B):
        buf[b * bstride:b * bstride + n, :C] = x[b * n:(b + 1) * n]
    return buf


def _valid(buf, B, n, bstride, C):
    """The valid rows of a padded buffer as [B * n, C], and a mask of the valid elements."""
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    for b in range(B):
        mask[b * bstride:b * bstride + n, :C] = True
    return torch.cat([buf[b * bstride:b * bstride + n, :C] for b in range(B)]), mask


def _sentinel_intact(buf, mask):
    return bool((buf[~mask].view(torch.int16) == torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)).all())


@pytest.mark.parametrize("nq,nk", [(130, 200), (33, 64)])
@pytest.mark.parametrize("form,D", [("default", 64), ("default", 128), ("mfma16", 64), ("two_wave", 64),
                                    ("two_wave", 128), ("lse", 64), ("lse", 128)])
def test_forward_strides_and_poison(N, form, D, nq, nk):
    """q, k, v, o as four tensors with four leading dimensions and four batch strides; NaN
    everywhere outside the valid region of the inputs, a sentinel in o."""
    B, C = 3, H * D
    cs = _case(B, nq, nk, D)
    qbs, kbs, vbs, obs = nq + 5, nk + 3, nk + 7, nq + 2

    def run(fill):
        q = _padded(cs["q"], B, nq, qbs, C + 8, fill).cuda()
        k = _padded(cs["k"], B, nk, kbs, C + 16, fill).cuda()
        v = _padded(cs["v"], B, nk, vbs, C + 24, fill).cuda()
        o = torch.full((B * obs, C + 32), SENTINEL, device="cuda", dtype=torch.bfloat16)
        lse = None
        if form == "lse":
            lse = torch.full((B * H * nq + 64,), SENTINEL, device="cuda")
            N.attention_fwd_lse(q[:, :C], k[:, :C], v[:, :C], o[:, :C], lse, B, H, nq, nk, D, qbs, kbs, obs, v_bstride=vbs)
        else:
            with _Knobs(N, form):
                N.attention(q[:, :C], k[:, :C], v[:, :C], o[:, :C], B, H, nq, nk, D, qbs, kbs, obs, v_bstride=vbs)
        torch.cuda.synchronize()
        return o.cpu(), None if lse is None else lse.cpu()

    o_nan, lse_nan = run(float("nan"))
    o_zero, lse_zero = run(0.0)
    got, mask = _valid(o_nan, B, nq, obs, C)
    got_zero, _ = _valid(o_zero, B, nq, obs, C)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.view(torch.int16), got_zero.view(torch.int16))
    assert _sentinel_intact(o_nan, mask)
    fails = []
    mform = "exact" if form == "lse" else FORMS[form][3]
    _check(f"fwd strided {form} D={D} ({nq},{nk})", got, cs["ref"]["o"], cs["model"]["o_" + mform], D, fails)
    if form == "lse":
        # compact [batch * H * nq]: nothing past it is written
        assert torch.equal(lse_nan, lse_zero)
        assert (lse_nan[B * H * nq:] == SENTINEL).all()
        _check_lse(f"fwd strided lse D={D} ({nq},{nk})", lse_nan[:B * H * nq], cs["ref"]["lse"], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nq,nk", [(130, 200), (33, 64)])
@pytest.mark.parametrize("D", [64, 128])
def test_backward_strides_and_poison(N, D, nq, nk):
    """The layout of the forward test on q, k, v, o, dO (o and dO share one leading dimension
    and batch stride, v takes k's batch stride: the backward ABI has one of each); dq at q's
    batch stride, dk / dv at k's, dq and dk / dv with different leading dimensions."""
    B, C = 3, H * D
    cs = _case(B, nq, nk, D)
    qbs, kbs, obs = nq + 5, nk + 3, nq + 2

    def run(fill):
        q = _padded(cs["q"], B, nq, qbs, C + 8, fill).cuda()
        k = _padded(cs["k"], B, nk, kbs, C + 16, fill).cuda()
        v = _padded(cs["v"], B, nk, kbs, C + 24, fill).cuda()
        do = _padded(cs["do"], B, nq, obs, C + 32, fill).cuda()
        o = torch.full((B * obs, C + 32), fill, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B * H * nq, device="cuda")
        N.attention_fwd_lse(q[:, :C], k[:, :C], v[:, :C], o[:, :C], lse, B, H, nq, nk, D, qbs, kbs, obs)
        dq = torch.full((B * qbs, C + 40), SENTINEL, device="cuda", dtype=torch.bfloat16)
        dk = torch.full((B * kbs, C + 48), SENTINEL, device="cuda", dtype=torch.bfloat16)
        dv = torch.full((B * kbs, C + 48), SENTINEL, device="cuda", dtype=torch.bfloat16)
        N.attention_bwd(q[:, :C], k[:, :C], v[:, :C], o[:, :C], do[:, :C], lse, dq[:, :C], dk[:, :C], dv[:, :C],
                        B, H, nq, nk, D, qbs, kbs, obs)
        torch.cuda.synchronize()
        return {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}

    g_nan, g_zero = run(float("nan")), run(0.0)
    fails = []
    for nm, n, bs in (("dq", nq, qbs), ("dk", nk, kbs), ("dv", nk, kbs)):
        got, mask = _valid(g_nan[nm], B, n, bs, C)
        got_zero, _ = _valid(g_zero[nm], B, n, bs, C)
        assert torch.isfinite(got.float()).all(), nm
        assert torch.equal(got.view(torch.int16), got_zero.view(torch.int16)), nm
        assert _sentinel_intact(g_nan[nm], mask), nm
        _check(f"bwd strided D={D} ({nq},{nk}) {nm}", got, cs["ref"][nm], cs["model"][nm], D, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. backward, rectangular and edge counts
@pytest.mark.parametrize("nq,nk", SHAPES)
@pytest.mark.parametrize("D,B", [(64, 1), (64, 2), (128, 1), (128, 2)])
def test_backward_rectangular(N, D, B, nq, nk):
    """fwd_lse then bwd: o, lse, dq, dk, dv.  With one key dq = dk = 0 up to 1e-5: before the
    training forward normalised o by the rounded row sum, (129,1) read max |dq| 1.7e-2 .. 2.9e-2
    and max |dk| 4.2e-2 .. 5.9e-2 here (o = v bf16(p) / p, so delta = dO . o did not cancel dP)."""
    cs = _case(B, nq, nk, D)
    o, lse = _fwd_lse(N, cs, B, nq, nk, D)
    got = _bwd(N, cs, o, lse, B, nq, nk, D)
    what = f"D={D} B={B} ({nq},{nk})"
    fails = []
    _check(f"fwd_lse {what} o", o.cpu(), cs["ref"]["o"], cs["model"]["o_exact"], D, fails)
    _check_lse(f"fwd_lse {what}", lse, cs["ref"]["lse"], fails)
    _check_grads(f"bwd {what}", got, cs, nk, D, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 5. determinism
def test_backward_deterministic(N):
    """Two launches, no atomics: the same call twice gives the same bits."""
    B, nq, nk, D = 2, 257, 300, 128
    cs = _case(B, nq, nk, D)
    o, lse = _fwd_lse(N, cs, B, nq, nk, D)
    a = _bwd(N, cs, o, lse, B, nq, nk, D)
    b = _bwd(N, cs, o, lse, B, nq, nk, D)
    for nm in ("dq", "dk", "dv"):
        assert torch.equal(a[nm].view(torch.int16), b[nm].view(torch.int16)), nm


# ------------------------------------------------------------------ 6. peaked softmax
@pytest.mark.parametrize("D", [64, 128])
def test_backward_peaked_softmax(N, D):
    """q and k at amplitude 2: rows are near one-hot, so dP - delta cancels."""
    B, nq, nk = 1, 130, 200
    cs = _case(B, nq, nk, D, amp=2.0)
    o, lse = _fwd_lse(N, cs, B, nq, nk, D)
    got = _bwd(N, cs, o, lse, B, nq, nk, D)
    fails = []
    _check(f"peaked D={D} o", o.cpu(), cs["ref"]["o"], cs["model"]["o_exact"], D, fails)
    _check_lse(f"peaked D={D}", lse, cs["ref"]["lse"], fails)
    _check_grads(f"peaked D={D}", got, cs, nk, D, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 7. the stamped diagnostic kernel
@pytest.mark.parametrize("nq,nk", [(700, 700), (4100, 200)])
def test_stamps_output_bitwise(N, nq, nk):
    """vggt_attention_stamps computes the plain default forward's o bit for bit (key-split tail
    off: the stamped kernel never splits) and fills one stamp row per launched wave."""
    D, C = 64, H * 64
    cs = _case(1, nq, nk, D, grads=False)
    q, k, v = cs["q"].cuda(), cs["k"].cuda(), cs["v"].cuda()
    o = torch.full((nq, C), SENTINEL, device="cuda", dtype=torch.bfloat16)
    o_st = torch.full((nq, C), SENTINEL, device="cuda", dtype=torch.bfloat16)
    with _Knobs(N, "eight_wave"):
        N.attention(q, k, v, o, 1, H, nq, nk, D, nq, nk, nq)
        st = N.attention_stamps(q, k, v, o_st, 1, H, nq, nk, nq, nk, nq)
        torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), o_st.view(torch.int16))
    # sized for the larger of the 4-wave (128-row) and 8-wave (256-row) grids
    assert tuple(st.shape) == (max(-(-nq // 128) * 4, -(-nq // 256) * 8) * H, 8)
    nw = 8 if nq >= 4096 else 4
    launched = -(-nq // (32 * nw)) * nw * H
    st = st.cpu()
    assert (st[:launched] != 0).any(dim=1).all()  # every launched wave left its stamps
    assert (st[launched:] == 0).all()
