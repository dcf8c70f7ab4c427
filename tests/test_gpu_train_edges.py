"""The backward (training) kernels of csrc/train.hip at the edges of their tiles, chunks and
dispatch thresholds, per element or per row, against fp64: vggt_wgrad_bf16 (both forms),
vggt_wgrad_f32 / vggt_wgrad_bias_f32, vggt_colsum, vggt_layerscale_bwd, vggt_gelu_fwd / _bwd,
vggt_resid_scale_add(_from), vggt_layernorm_bwd, vggt_headnorm_rope_bwd, vggt_attention_small_bwd,
vggt_transpose_b16 and vggt_batch_dot_f32.

Inputs are drawn on the host from a seeded torch.Generator; references are fp64 on the host from
the bf16 / fp32 inputs actually passed.  Every strided case puts its operands inside larger
buffers (`Box`): inputs NaN-filled around the valid window (rows before and after, columns on both
sides), outputs sentinel-filled; outputs must be finite and the sentinels outside the documented
output window intact bit for bit.  Failures are reported with their first indices and values.

Which path a case reaches (`_reach_*` below restate the host dispatch of train.hip and are printed
with the figures):

  wgrad_bf16      LDS-DMA form unless VGGT_WGRAD_DMA=0 (read once per process: a child process
                  runs the exact-input list with it) or mchunk * max(ldy, ldx) * 2 >= 2^31 (row
                  stride 2^25 elements: the dispatcher's own fallback) -> register-staged form.
                  splits = min(16, ceil(M / 256), ceil(1024 / tiles)); mchunk = splits' share of
                  M rounded up to 32; nz = ceil(M / mchunk) launched (M = 4097 at 128 x 128: 16
                  requested, mchunk 288, 15 launched).  M < 32 stages whole zero tiles.
  colred family   nc = min(1024, ceil(M / 16)) chunks of rpc = ceil(M / nc) rows (M = 16400: 1024
                  chunks of 17 rows, the last 59 empty); finalize adds chunks c = s, s + 16, ...
                  in 16 slices (M = 241 / 257 / 273: 16 / 17 / 18 chunks); column blocks of 1024
                  (N = 1028 / 2052: a second / third block with one live thread).
  layernorm_bwd   NV = C / 256 in {1, 2, 4}; nblk = min(2048, ceil(M / 16)) blocks of
                  ceil(M / nblk) rows, 4 waves a block (M < 4: waves without a row; M = 32784:
                  2048 blocks of 17 rows, the last 119 empty).
  headnorm_rope   64 / (D / 8) heads per wave pass (8 at D = 64, 4 at D = 128); ragged last pass
                  for H % that != 0.
  attention_small 16-B staging when D % 8 == 0 and every operand row start is 16-B aligned, else
                  element by element; LDS (2 nq (D+1) + 2 nk (D+1) + 2 nq nk) 4 <= 64 KiB.
  batch_dot       min(256, ceil(n / 65536)) chunks.

Tolerances (none is a measured constant; u = 2^-24, gamma_n = n u / (1 - n u)):
  exact     inputs whose every fp32 partial sum is exact in any order (dY integers in [-4, 4], X
            multiples of 1/8 in [-2, 2]; +-1 / 0 for the long dots), checked on the host (the sum
            of the absolute terms, which bounds every partial sum of every order, fits in 24 bits
            of the terms' unit), so the result is unique and compared bit for bit: both bf16
            wgrad forms (after the documented bf16 rounding, accumulate 0 and 1), wgrad_f32,
            wgrad_bias_f32, colsum, dgamma / dbias / db, batch_dot, transpose_b16.
  one-op    dbranch = odtype(gamma * dout) is one fp32 multiply and one rounding: bit for bit
            against the same operation in host fp32.  out = x + gamma * branch is one multiply
            and one add, or one fma: each rounds by at most u relative, so
            |got - ref| <= 2^-23 (|x| + |gamma b|) (the `resid` bound of the GEMM edge tests).
  interval  any fp32 summation order of n terms with c further additions (chunk partials, the 16
            finalize slices, the final +=, the rounding of a product that is not exact) stays
            within E = gamma_(n + c) sum |terms| of the fp64 sum s; rounding is monotone, so
            odtype(s - E) <= got <= odtype(s + E).  dbias / db1 of layerscale_bwd / gelu_bwd are
            compared with the fp64 column sum of the stored (rounded) output, as the contract says.
  gelu      y = 0.5 x (1 + erf(x / sqrt 2)).  Assumed (the ROCm documentation is not on the build
            host; these are the figures of the HIP math API reference): erff within 4 ulp, i.e.
            4 u absolute since |erf| <= 1; the hardware exp2 behind __expf within 1 ulp.
            t = fl(x / sqrt 2) is off by <= 2 u |t| (constant and product), which moves erf by
            <= 2 u |t| erf'(t) <= 2 u * 0.484 (max of t (2 / sqrt pi) exp(-t^2) at t = 1 / sqrt 2);
            1 + erf rounds by <= u (1 + erf) <= 2 u.  So A = |err(1 + erf)| <= (4 + 0.97 + 2) u <
            7 u, absolute -- the form cancels in the negative tail, so no relative bound exists --
            and |err y| <= 0.5 |x| A + u |G(x)| (0.5 x exact, one product rounding)
            <= 3.5 u |x| + u |G| <= 2^-22 (|x| + |G(x)|).
            G'(x) = Phi(x) + x phi(x): Phi = 0.5 (1 + erf) is off by <= 3.5 u; the argument
            a = fl(fl(-0.5 x) x) of __expf is off by <= u x^2 / 2, its scaling by log2 e by as much
            again, exp2 and the product with 1 / sqrt(2 pi) by <= 3 u relative, so x phi is off by
            <= |x| phi(x) (x^2 + 3) u <= (0.47 + 0.73) u (maxima of |x|^3 phi at sqrt 3 and of
            |x| phi at 1), the product x * pdf by <= 0.25 u, the sum by u |G'| <= 1.13 u: together
            <= 6.1 u; dh * G' adds one rounding, u |dh G'| <= 1.13 u |dh|.  So
            |err| <= 7.3 u |dh| <= 2^-21 |dh|.  bf16 outputs add half a bf16 ulp of the reference.
            The worst ratio of error to bound is printed and must be below 1.
  model     the row-statistics kernels (layernorm_bwd dx and dw, headnorm_rope_bwd,
            attention_small_bwd): the documented arithmetic restated in plain fp32 torch on the
            host with one rounding to the output dtype; per row (or row and head)
            ||got - ref64||_2 over the RMS row norm of the fp64 reference; the kernel's worst
            value must be <= 2 x the model's on the same inputs (the rule of the attention and
            GEMM edge tests: lane-tree re-association and rsqrtf stay below one output rounding).
            Sums of exact quantities (db = sum dy) use the exact or the interval rule instead.
            With fp32 outputs the bar is a matter of a few fp32 roundings: the first run of this
            file measured vggt_attention_small_bwd at 2.20 x (dk) and 2.09 x (dv) the model at
            D = 6, (5, 60) -- fp32 score sums, the fast exponential and a reciprocal multiply, on a
            row with one dominant key -- and its fp32 path now keeps the softmax stage in fp64
            with one rounding per stored value (worst 1.65 x, at D = 6, (1, 12)).
  poison    as above.
Determinism: each reduction runs twice on the same inputs and the parameter gradients must be
bitwise equal.
Argument checks: `test_train_entry_error_returns` walks every entry's rules (dimensions, leading
dimensions, pointer alignment, dtype codes, required pointers, workspace), one broken rule a call,
against the codes the header documents; `test_dbias_is_colsum_of_the_stored_output` pins the one
chunk plan and finalize behind the three column reductions.  DESIGN.md (Training kernel edge tests) tabulates what was measured."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import vggt_oracle as O  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SENT = 7.0
U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=F32))
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _gam(n):
    return n * U / (1 - n * U)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _dtn(dt):
    return "bf16" if dt == BF else "f32"


# ------------------------------------------------------------------ the dispatch, restated for the printed figures
def _reach_wgrad(M, Nn, K, ldy, ldx, dma_env=True):
    tiles = (Nn // 128) * (K // 128)
    splits = max(1, min(1 if tiles >= 1024 else -(-1024 // tiles), -(-M // 256), 16))
    mchunk = -(-(-(-M // splits)) // 32) * 32
    nz = -(-M // mchunk)
    dma = dma_env and mchunk * max(ldy, ldx) * 2 < 2 ** 31
    return {"form": "lds-dma" if dma else "register", "splits": splits, "mchunk": mchunk, "launched": nz,
            "zero_tiles_staged": M < 32}


def _reach_chunks(M, maxc, rows=16):
    nc = min(maxc, max(1, -(-M // rows)))
    rpc = -(-M // nc)
    return {"chunks": nc, "rows": rpc, "empty": nc - (-(-M // rpc)), "finalize_rounds": -(-nc // 16)}


def _reach_colred(M, Nn):
    d = _reach_chunks(M, 1024)
    d["column_blocks"] = -(-(Nn // 4) // 256)
    return d


def _reach_attn(dt, D, lds, ptrs):
    esz = 2 if dt == BF else 4
    vec = D % 8 == 0 and all(ld % (16 // esz) == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs)
    return "16-B staging" if vec else "scalar staging"


def _attn_lds(nq, nk, D):
    return (2 * nq * (D + 1) + 2 * nk * (D + 1) + 2 * nq * nk) * 4


# ------------------------------------------------------------------ bits, boxes, checks
def _bits(x):
    if x.dtype == torch.int16:
        return x.contiguous()
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


class Box:
    """A host tensor inside a larger buffer filled with `fill`: `rows` extra rows before / after,
    `cols` extra columns left / right (multiples of 8 elements, so the window keeps 16-B alignment)."""

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

    def set(self, x):
        self.v.copy_(x)

    def got(self):
        return self.v.cpu()

    def intact(self, keep=None):
        """Everything outside the window (or outside the boolean mask `keep` of written elements)
        holds its original bits."""
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
    w = ((got.double() - s).abs() / E.clamp_min(1e-300))[E > 0]
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
    """The kernel's worst row must be within 2 x the fp32 model's worst row."""
    if not bool(torch.isfinite(got.float()).all()):
        errs.append(f"{name}: non-finite output")
        return
    eg, em = _row_err(got, ref), _row_err(model, ref)
    wg, wm = float(eg.max()), float(em.max())
    old = FIG.get(("model", tag), (0.0, 0.0, 0.0))
    ratio = wg / wm if wm > 0 else (0.0 if wg == 0 else math.inf)
    if ratio >= old[2]:
        FIG[("model", tag)] = (wg, wm, ratio)
    if wg > 2 * wm:
        i = int(eg.reshape(-1).argmax())
        errs.append(f"{name}: kernel worst row {wg:.3e} > 2 x model {wm:.3e} (row {i} of {tuple(eg.shape)})")


def _done(errs, *reach):
    for r in reach:
        print("reach", r)
    assert not errs, "\n".join(errs)


def _raises(code, fn, *a, **k):
    with pytest.raises(RuntimeError, match=r"\(code %d\)" % code):
        fn(*a, **k)


# ================================================================== 1. wgrad_bf16
WG_NK = [(128, 128), (128, 384), (384, 128), (256, 256)]
WG_M = [1, 31, 32, 33, 64, 65, 255, 256, 257, 513, 4097]
_HOST = {}


def _wgrad_host(M, Nn, K, exact):
    key = ("wg", M, Nn, K, exact)
    if key not in _HOST:
        g = _gen(11, M, Nn, K, exact)
        if exact:
            dy = torch.randint(-4, 5, (M, Nn), generator=g).to(BF)
            x = (torch.randint(-16, 17, (M, K), generator=g).float() / 8).to(BF)
        else:
            dy = torch.randn(M, Nn, generator=g).to(BF)
            x = (torch.randn(M, K, generator=g) + torch.arange(K) * 1e-3).to(BF)
        dw0 = torch.randint(-4, 5, (Nn, K), generator=g).float()
        s = dy.double().t() @ x.double() + 0.0  # (a sum starts from +0: a lone -0 product gives +0)
        a = dy.double().abs().t() @ x.double().abs()
        if exact:  # every partial sum of every order is a multiple of 1/8 below 2^24 / 8
            assert float(a.max()) * 8 < 2 ** 24
            assert torch.equal((dy.float().t() @ x.float()).double(), s)
        _HOST[key] = {"dy": dy, "x": x, "dw0": dw0, "s": s, "abs": a, "ref": s.to(BF).float()}
    return _HOST[key]


def _wgrad_case(N, M, Nn, K, exact, errs, dma_env=True):
    """One (M, N, K): column-slice dY / X views in NaN boxes, a strided dW in a sentinel box,
    accumulate 1 (onto integers) then 0, and again for determinism.  Returns the worst interval ratio."""
    cs = _wgrad_host(M, Nn, K, exact)
    tag = f"wgrad_bf16 M={M} N={Nn} K={K} {'exact' if exact else 'random'}"
    dyb, xb, dwb = Box(cs["dy"], NAN), Box(cs["x"], NAN), Box(cs["dw0"], SENT)
    worst = 0.0
    N.wgrad_bf16(dyb.v, xb.v, dwb.v, True)
    acc = dwb.got()
    N.wgrad_bf16(dyb.v, xb.v, dwb.v, False)
    wr = dwb.got()
    N.wgrad_bf16(dyb.v, xb.v, dwb.v, False)
    _eq_bits(errs, tag + " second run", dwb.got(), wr)
    if not dwb.intact():
        errs.append(tag + ": dW sentinels overwritten")
    if exact:
        _eq_bits(errs, tag + " write", wr, cs["ref"])
        _eq_bits(errs, tag + " accumulate", acc, cs["dw0"] + cs["ref"])
    else:
        r = _reach_wgrad(M, Nn, K, dyb.dev.stride(0), xb.dev.stride(0), dma_env)
        E = _gam(M + r["launched"]) * cs["abs"]
        lo, hi = (cs["s"] - E).to(BF).float(), (cs["s"] + E).to(BF).float()
        for nm, got, off in (("write", wr, 0), ("accumulate", acc, cs["dw0"])):
            bad = ~torch.isfinite(got) | (got < (off + lo)) | (got > (off + hi))  # (the fp32 add is monotone)
            if bool(bad.any()):
                errs.append(f"{tag} {nm} outside its interval: " + _first(bad, got, off + lo, off + hi))
        worst = float(((wr.double() - cs["s"]).abs() / (E + _half_ulp(cs["s"], BF))).max())
    return worst


@pytest.mark.parametrize("Nn,K", WG_NK)
@pytest.mark.parametrize("M", WG_M)
def test_wgrad_bf16(N, M, Nn, K):
    errs = []
    _wgrad_case(N, M, Nn, K, True, errs)
    w = _wgrad_case(N, M, Nn, K, False, errs)
    print(f"wgrad_bf16 random M={M} N={Nn} K={K}: worst |got - s| / (E + half bf16 ulp) = {w:.3f}")
    _fig(("interval", "wgrad_bf16"), w)
    _done(errs, ("wgrad_bf16", M, Nn, K, _reach_wgrad(M, Nn, K, Nn + 24, K + 24)))


def _wgrad_exact_sweep(N):
    """The exact-input list of test_wgrad_bf16 in one go (the child process of the register form)."""
    out = {}
    for Nn, K in WG_NK:
        for M in WG_M:
            errs = []
            _wgrad_case(N, M, Nn, K, True, errs)
            out[f"{M},{Nn},{K}"] = errs
    return out


_CHILD = """
import json, sys
import torch
from aligned_vggt import _native as N
import test_gpu_train_edges as T
N.lib()
res = T._wgrad_exact_sweep(N)
torch.cuda.synchronize()
print(json.dumps({"dma": __import__("os").environ.get("VGGT_WGRAD_DMA"), "cases": res}))
"""


def test_wgrad_bf16_register_form_in_a_fresh_process(N):
    """VGGT_WGRAD_DMA is read once per process: a fresh interpreter with VGGT_WGRAD_DMA=0 runs every
    exact-input case on the register-staged kernel and reports the failures of each as JSON."""
    env = dict(os.environ, VGGT_WGRAD_DMA="0", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["dma"] == "0" and len(got["cases"]) == len(WG_NK) * len(WG_M)
    bad = {k: v for k, v in got["cases"].items() if v}
    print("reach", ("wgrad_bf16 child", _reach_wgrad(4097, 128, 128, 152, 152, dma_env=False)), len(got["cases"]),
          "cases")
    assert not bad, json.dumps(bad, indent=1)[:4000]


def test_wgrad_bf16_dispatcher_fallback(N):
    """Row stride 2^25 elements: mchunk (32) * ld * 2 = 2^31, so the dispatcher itself takes the
    register-staged kernel.  M = 3 rows in ~134 MB buffers, NaN just before and past each window."""
    ld, M = 2 ** 25, 3
    cs = _wgrad_host(M, 128, 128, True)
    r = _reach_wgrad(M, 128, 128, ld, ld)
    assert r["form"] == "register" and _reach_wgrad(M, 128, 128, ld // 2, ld // 2)["form"] == "lds-dma"
    views = []
    for t in (cs["dy"], cs["x"]):
        buf = torch.empty((M - 1) * ld + 64 + 128 + 64, dtype=BF, device="cuda")
        v = buf.as_strided((M, 128), (ld, 1), 64)
        for m in range(M):
            buf[m * ld:m * ld + 64] = NAN
            buf[m * ld + 192:m * ld + 256] = NAN
        v.copy_(t)
        views.append(v)
    dwb = Box(cs["dw0"], SENT)
    errs = []
    N.wgrad_bf16(views[0], views[1], dwb.v, True)
    _eq_bits(errs, "fallback accumulate", dwb.got(), cs["dw0"] + cs["ref"])
    N.wgrad_bf16(views[0], views[1], dwb.v, False)
    _eq_bits(errs, "fallback write", dwb.got(), cs["ref"])
    if not dwb.intact():
        errs.append("fallback: dW sentinels overwritten")
    _done(errs, ("wgrad_bf16 fallback", r))


def test_wgrad_bf16_error_returns(N):
    import ctypes
    dy = torch.zeros(40, 256 + 8, dtype=BF, device="cuda")
    x = torch.zeros(40, 128 + 8, dtype=BF, device="cuda")
    dw = torch.full((256, 128), SENT, device="cuda")
    _raises(ERR_SHAPE, N.wgrad_bf16, dy[:, :192], x[:, :128], dw[:192])         # N % 128 != 0
    _raises(ERR_SHAPE, N.wgrad_bf16, dy[:, :256], x[:, :64], dw[:, :64])         # K % 128 != 0
    _raises(ERR_ALIGN, N.wgrad_bf16, dy[:, 4:260], x[:, :128], dw)               # base 8 B off a 16-B boundary
    _raises(ERR_ALIGN, N.wgrad_bf16, dy[:, :256], x[:, 4:132], dw)
    L = N.lib()
    need = int(L.vggt_wgrad_bf16_workspace_bytes(40, 256, 128))
    assert need == 256 * 128 * 4
    ws = torch.empty(need // 4, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for ptr, nbytes in ((p(ws), need - 4), (None, need)):
        rc = L.vggt_wgrad_bf16(p(dy), dy.stride(0), p(x), x.stride(0), 40, 256, 128, p(dw), 128, 0, ptr, nbytes, None)
        assert rc == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((dw == SENT).all())


# ================================================================== 2. wgrad_f32 / wgrad_bias_f32
@pytest.mark.parametrize("K", [1, 255, 256, 257, 511])
def test_wgrad_f32(N, K):
    errs, worst = [], 0.0
    for M in (1, 9):
        for Nn in (1, 300):
            for exact in (True, False):
                g = _gen(2, M, Nn, K, exact)
                if exact:
                    dy = torch.randint(-4, 5, (M, Nn), generator=g).float()
                    x = torch.randint(-16, 17, (M, K), generator=g).float() / 8
                    dw0, db0 = (torch.randint(-4, 5, s, generator=g).float() for s in ((Nn, K), (Nn,)))
                else:
                    dy, x = torch.randn(M, Nn, generator=g), torch.randn(M, K, generator=g)
                    dw0, db0 = torch.randn(Nn, K, generator=g), torch.randn(Nn, generator=g)
                s, sb = dy.double().t() @ x.double() + 0.0, dy.double().sum(0) + 0.0
                a, ab = dy.double().abs().t() @ x.double().abs(), dy.double().abs().sum(0)
                if exact:
                    assert (float(a.max()) + 4) * 8 < 2 ** 24
                tag = f"wgrad_f32 M={M} N={Nn} K={K} {'exact' if exact else 'random'}"
                # cols (8, 16) shifts the windows; Nn = 1 / K = 1 make 4-byte-aligned views, which fp32 allows
                dyb, xb = Box(dy, NAN), Box(x, NAN)
                for bias in (False, True):
                    for accum in (False, True):
                        dwb = Box(dw0, SENT)
                        db = db0.cuda()
                        if bias:
                            N.wgrad_bias_f32(dyb.v, xb.v, dwb.v, db, accum)
                        else:
                            N.wgrad_f32(dyb.v, xb.v, dwb.v, accum)
                        got, gb = dwb.got(), db.cpu()
                        nm = f"{tag} bias={bias} acc={accum}"
                        if not dwb.intact():
                            errs.append(nm + ": dW sentinels overwritten")
                        base, bb = (dw0.double(), db0.double()) if accum else (0.0, 0.0)
                        if exact:
                            _eq_bits(errs, nm + " dw", got, (s + base).float())
                            _eq_bits(errs, nm + " db", gb, (sb + bb).float() if bias else db0)
                        else:  # M products (each rounded, or fused), M - 1 additions, the +=
                            E = _gam(M + 2) * (a + (dw0.double().abs() if accum else 0))
                            worst = max(worst, _interval(errs, nm + " dw", got, s + base, E))
                            if bias:
                                Eb = _gam(M + 1) * (ab + (db0.double().abs() if accum else 0))
                                worst = max(worst, _interval(errs, nm + " db", gb, sb + bb, Eb))
                            else:
                                _eq_bits(errs, nm + " db untouched", gb, db0)
    print(f"wgrad_f32 K={K}: worst |got - s| / E = {worst:.3f}")
    _fig(("interval", "wgrad_f32"), worst)
    _done(errs)


# ================================================================== 3. column reductions and elementwise
CR_N = [4, 1020, 1024, 1028, 2052]
CR_M = [1, 15, 16, 17, 33, 241, 257, 273]
CR_CASES = [(M, Nn) for Nn in CR_N for M in CR_M] + [(16400, 4)]


def _colred_extra(M):
    """Additions beyond the M terms: one per chunk partial, the 16 slice sums, the final +=."""
    return _reach_chunks(M, 1024)["chunks"] + 17


@pytest.mark.parametrize("M,Nn", CR_CASES)
def test_colsum(N, M, Nn):
    errs, worst = [], 0.0
    for dt in (BF, F32):
        for exact in (True, False):
            g = _gen(3, M, Nn, dt == BF, exact)
            x = (torch.randint(-4, 5, (M, Nn), generator=g).float() if exact else
                 torch.randn(M, Nn, generator=g) + 0.25).to(dt)
            o0 = torch.randint(-4, 5, (Nn,), generator=g).float()
            s, a = x.double().sum(0) + 0.0, x.double().abs().sum(0)
            if exact:
                assert float(a.max()) + 4 < 2 ** 24
            xb = Box(x, NAN)
            for accum in (False, True):
                ob = Box(o0[None], SENT, rows=(1, 1), cols=(4, 4))
                nm = f"colsum M={M} N={Nn} {_dtn(dt)} {'exact' if exact else 'random'} acc={accum}"
                N.colsum(xb.v, ob.v[0], accum)
                got = ob.got()[0]
                N.colsum(xb.v, ob.v[0], False)
                N.colsum(xb.v, ob.v[0], False)
                if accum is False:
                    _eq_bits(errs, nm + " second run", ob.got()[0], got)
                if not ob.intact():
                    errs.append(nm + ": sentinels overwritten")
                ref = s + (o0.double() if accum else 0)
                if exact:
                    _eq_bits(errs, nm, got, ref.float())
                else:
                    E = _gam(M + _colred_extra(M)) * (a + (o0.double().abs() if accum else 0))
                    worst = max(worst, _interval(errs, nm, got, ref, E))
    print(f"colsum M={M} N={Nn}: worst |got - s| / E = {worst:.4f}")
    _fig(("interval", "colsum"), worst)
    _done(errs, ("colsum", M, Nn, _reach_colred(M, Nn)))


@pytest.mark.parametrize("M,Nn", CR_CASES)
def test_layerscale_bwd(N, M, Nn):
    """dbranch = odtype(gamma * dout) one-op; dgamma += sum dout * branch; dbias += sum dbranch."""
    i = CR_CASES.index((M, Nn))
    errs, worst = [], 0.0
    for j, exact in enumerate((True, False)):
        bdt, odt = (BF, F32)[(i + j) % 2], (BF, F32)[((i + j) // 2) % 2]
        want = ((True, True), (True, False), (False, True), (False, False))[(i + j) % 4 if exact else 0]
        g = _gen(4, M, Nn, exact)
        if exact:  # integers x multiples of 1/8; gamma powers of two
            dout = torch.randint(-4, 5, (M, Nn), generator=g).float()
            br = (torch.randint(-16, 17, (M, Nn), generator=g).float() / 8).to(bdt)
            gamma = torch.pow(2.0, torch.randint(-3, 2, (Nn,), generator=g).float())
        else:
            dout, br = torch.randn(M, Nn, generator=g), torch.randn(M, Nn, generator=g).to(bdt)
            gamma = 0.01 * torch.randn(Nn, generator=g)
        dg0, dbi0 = (torch.randint(-4, 5, (Nn,), generator=g).float() for _ in range(2))
        nm = f"layerscale_bwd M={M} N={Nn} branch {_dtn(bdt)} out {_dtn(odt)} {'exact' if exact else 'random'} want={want}"
        db_, bb, ob = Box(dout, NAN), Box(br, NAN), Box(torch.full((M, Nn), SENT).to(odt), SENT)
        runs = []
        for _ in range(2):
            dg, dbi = dg0.cuda(), dbi0.cuda()
            N.layerscale_bwd(db_.v, bb.v, gamma.cuda(), ob.v, dg if want[0] else None, dbi if want[1] else None)
            runs.append((ob.got(), dg.cpu(), dbi.cpu()))
        got, gg, gb = runs[0]
        for k, part in enumerate(("dbranch", "dgamma", "dbias")):
            _eq_bits(errs, nm + f" {part} second run", runs[1][k], runs[0][k])
        if not ob.intact():
            errs.append(nm + ": dbranch sentinels overwritten")
        _eq_bits(errs, nm + " dbranch", got, (gamma * dout).to(odt))
        sg = (dout.double() * br.double()).sum(0) + dg0.double()
        sb = got.double().sum(0) + dbi0.double()  # of the stored, rounded dbranch
        ag = (dout.double() * br.double()).abs().sum(0) + dg0.abs().double()
        ab = got.double().abs().sum(0) + dbi0.abs().double()
        if not want[0]:
            _eq_bits(errs, nm + " dgamma untouched", gg, dg0)
        elif exact:
            assert float(ag.max()) * 8 < 2 ** 24
            _eq_bits(errs, nm + " dgamma", gg, sg.float())
        else:
            worst = max(worst, _interval(errs, nm + " dgamma", gg, sg, _gam(M + 1 + _colred_extra(M)) * ag))
        if not want[1]:
            _eq_bits(errs, nm + " dbias untouched", gb, dbi0)
        elif exact:
            assert float(ab.max()) * 64 < 2 ** 24
            _eq_bits(errs, nm + " dbias", gb, sb.float())
        else:
            worst = max(worst, _interval(errs, nm + " dbias", gb, sb, _gam(M + _colred_extra(M)) * ab))
    print(f"layerscale_bwd M={M} N={Nn}: worst |got - s| / E = {worst:.4f}")
    _fig(("interval", "layerscale_bwd"), worst)
    _done(errs, ("layerscale_bwd", M, Nn, _reach_colred(M, Nn)))


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def _gelu_d64(x):
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _gelu_fwd_bound(x64, ref, odt):
    return 2.0 ** -22 * (x64.abs() + ref.abs()) + _half_ulp(ref, odt) + 2.0 ** -149


def _gelu_bwd_bound(dh64, ref, odt):
    return 2.0 ** -21 * dh64.abs() + _half_ulp(ref, odt) + 2.0 ** -149


@pytest.mark.parametrize("M,Nn", CR_CASES)
def test_gelu_and_resid(N, M, Nn):
    """gelu_fwd, gelu_bwd (out of place, and in place where dh and dpre share a dtype),
    resid_scale_add and resid_scale_add_from (out == x and out != x), dtype combinations cycling."""
    i = CR_CASES.index((M, Nn))
    errs = []
    g = _gen(5, M, Nn)
    # ---- gelu_fwd
    xdt, ydt = (BF, F32)[i % 2], (BF, F32)[(i // 2) % 2]
    x = (torch.randn(M, Nn, generator=g) * 3).to(xdt)
    xb, yb = Box(x, NAN), Box(torch.full((M, Nn), SENT).to(ydt), SENT)
    N.gelu_fwd(xb.v, yb.v)
    ref = _gelu64(x.double())
    w = _within(errs, f"gelu_fwd M={M} N={Nn} {_dtn(xdt)}->{_dtn(ydt)}", yb.got(), ref, _gelu_fwd_bound(x.double(), ref, ydt))
    _fig(("gelu_fwd", "random"), w)
    if not yb.intact():
        errs.append("gelu_fwd: sentinels overwritten")
    # ---- gelu_bwd
    hdt, pdt, odt = (BF, F32)[i % 2], (BF, F32)[(i // 2) % 2], (BF, F32)[(i // 4) % 2 if i % 3 else i % 2]
    dh = torch.randn(M, Nn, generator=g).to(hdt)
    pre = (torch.randn(M, Nn, generator=g) * 2).to(pdt)
    db0 = torch.randint(-4, 5, (Nn,), generator=g).float()
    nm = f"gelu_bwd M={M} N={Nn} dh {_dtn(hdt)} pre {_dtn(pdt)} out {_dtn(odt)}"
    hb, pb = Box(dh, NAN), Box(pre, NAN)
    runs = []
    for want in (True, True, False):
        ob = Box(torch.full((M, Nn), SENT).to(odt), SENT)
        db = db0.cuda()
        N.gelu_bwd(hb.v, pb.v, ob.v, db if want else None)
        runs.append((ob.got(), db.cpu()))
        if not ob.intact():
            errs.append(nm + ": sentinels overwritten")
    got, gb = runs[0]
    _eq_bits(errs, nm + " dpre second run", runs[1][0], got)
    _eq_bits(errs, nm + " dbias second run", runs[1][1], gb)
    _eq_bits(errs, nm + " dpre without dbias", runs[2][0], got)
    _eq_bits(errs, nm + " NULL dbias untouched", runs[2][1], db0)
    ref = dh.double() * _gelu_d64(pre.double())
    w = _within(errs, nm + " dpre", got, ref, _gelu_bwd_bound(dh.double(), ref, odt))
    _fig(("gelu_bwd", "random"), w)
    sb, ab = got.double().sum(0) + db0.double(), got.double().abs().sum(0) + db0.abs().double()
    wi = _interval(errs, nm + " dbias", gb, sb, _gam(M + _colred_extra(M)) * ab)
    _fig(("interval", "gelu_bwd dbias"), wi)
    if hdt == odt:  # in place, as the MLP backward calls it: dpre is dh
        hb2 = Box(dh, NAN)
        db = db0.cuda()
        N.gelu_bwd(hb2.v, pb.v, hb2.v, db)
        _eq_bits(errs, nm + " in place dpre", hb2.got(), got)
        _eq_bits(errs, nm + " in place dbias", db.cpu(), gb)
        if not hb2.intact():
            errs.append(nm + " in place: poison around dh changed")
    # ---- resid_scale_add / _from
    bdt = (BF, F32)[i % 2]
    x0 = torch.randn(M, Nn, generator=g)
    br = torch.randn(M, Nn, generator=g).to(bdt)
    gamma = torch.rand(Nn, generator=g) - 0.5
    ref = x0.double() + gamma.double() * br.double()
    bound = 2.0 ** -23 * (x0.double().abs() + (gamma.double() * br.double()).abs())
    bb, gd = Box(br, NAN), gamma.cuda()
    nm = f"resid_scale_add M={M} N={Nn} branch {_dtn(bdt)}"
    xa = Box(x0, SENT)
    N.resid_scale_add(xa.v, bb.v, gd)
    wr = _within(errs, nm, xa.got(), ref, bound)
    xf = Box(x0, SENT)
    N.resid_scale_add_from(xf.v, xf.v, bb.v, gd)
    _eq_bits(errs, nm + " _from out == x", xf.got(), xa.got())
    xs, of = Box(x0, NAN), Box(torch.full((M, Nn), SENT), SENT, cols=(16, 8))
    N.resid_scale_add_from(of.v, xs.v, bb.v, gd)
    _eq_bits(errs, nm + " _from out != x", of.got(), xa.got())
    _eq_bits(errs, nm + " _from leaves x", xs.got(), x0)
    if not (xa.intact() and xf.intact() and of.intact() and xs.intact()):
        errs.append(nm + ": sentinels overwritten")
    _fig(("one-op", "resid_scale_add"), wr)
    print(f"gelu / resid M={M} N={Nn}: gelu_fwd err/bound {FIG[('gelu_fwd', 'random')]:.3f} (worst so far), "
          f"gelu_bwd {w:.3f}, dbias interval {wi:.4f}, resid {wr:.3f}")
    _done(errs, ("gelu_bwd", M, Nn, _reach_colred(M, Nn)))


def test_gelu_fwd_every_bf16_pattern(N):
    """bf16 -> bf16 over all 65536 bit patterns in one 64 x 1024 launch; the finite ones are checked."""
    allb = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).view(64, 1024)
    y = torch.empty(64, 1024, dtype=BF, device="cuda")
    N.gelu_fwd(allb.cuda(), y)
    got = y.cpu()
    fin = torch.isfinite(allb.float())
    x64 = torch.where(fin, allb.double(), torch.zeros((), dtype=F64))
    ref = _gelu64(x64)
    errs = []
    w = _within(errs, "gelu_fwd all bf16", torch.where(fin, got, torch.zeros((), dtype=BF)), ref,
                _gelu_fwd_bound(x64, ref, BF))
    # the fp32 value before the rounding, through an fp32 output of the same launch shape
    yf = torch.empty(64, 1024, device="cuda")
    N.gelu_fwd(allb.cuda(), yf)
    wf = _within(errs, "gelu_fwd all bf16 -> f32", torch.where(fin, yf.cpu(), torch.zeros(())), ref,
                 _gelu_fwd_bound(x64, ref, F32))
    print(f"gelu_fwd over every finite bf16: worst err / bound {w:.3f} (bf16 out), {wf:.3f} (fp32 out)")
    _fig(("gelu_fwd", "all bf16 -> bf16"), w)
    _fig(("gelu_fwd", "all bf16 -> f32"), wf)
    # and the derivative over the same grid, dh = 1 and a random bf16 dh
    g = _gen(55)
    for nm, dh in (("dh = 1", torch.ones(64, 1024).to(BF)), ("random dh", torch.randn(64, 1024, generator=g).to(BF))):
        o = torch.empty(64, 1024, device="cuda")
        pre = torch.where(fin, allb, torch.zeros((), dtype=BF))
        N.gelu_bwd(dh.cuda(), pre.cuda(), o, None)
        refd = dh.double() * _gelu_d64(pre.double())
        wd = _within(errs, "gelu_bwd all bf16 " + nm, o.cpu(), refd, _gelu_bwd_bound(dh.double(), refd, F32))
        print(f"gelu_bwd over every finite bf16 pre, {nm}: worst err / bound {wd:.3f}")
        _fig(("gelu_bwd", "all bf16 pre, " + nm), wd)
    _done(errs)


# ================================================================== 4. layernorm_bwd
LN_CASES = [(C, M) for C in (256, 512, 1024) for M in (1, 2, 3, 4, 5, 16, 17, 65)] + [(256, 32784)]


def _ln_rows(M, C, dt, g):
    """Gaussian rows, plus (from the second row on) one constant row and one row of 100 + small.
    The two special rows hold values whose fp32 sums are exact in any order (1.5; 100 + k / 64), so
    a kernel that subtracts the mean keeps them exact and one that forms E[x^2] - mean^2 does not."""
    x = torch.randn(M, C, generator=g) * 3 + 1
    if M >= 2:
        x[1] = 1.5
    if M >= 3:
        x[2] = 100 + torch.randint(-32, 33, (C,), generator=g).float() / 64
    return x.to(dt)


def _ln_ref64(x, w, dy):
    xr = x.double().requires_grad_(True)
    C = x.shape[-1]
    wr = (torch.ones(C, dtype=F64) if w is None else w.double()).requires_grad_(True)
    br = torch.zeros(C, dtype=F64, requires_grad=True)
    F.layer_norm(xr, (C,), wr, br, EPS).backward(dy.double())
    return xr.grad, wr.grad, br.grad


def _ln_model(x, w, dy):
    """The kernel's documented arithmetic in plain fp32."""
    x, dy = x.float(), dy.float()
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) * (1.0 / C)
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) * (1.0 / C) + EPS)
    xh = d * rstd
    gd = dy if w is None else dy * w
    m1, m2 = gd.sum(-1, keepdim=True) * (1.0 / C), (gd * xh).sum(-1, keepdim=True) * (1.0 / C)
    return rstd * (gd - m1 - xh * m2), (dy * xh).sum(0)


@pytest.mark.parametrize("C,M", LN_CASES)
def test_layernorm_bwd(N, C, M):
    i = LN_CASES.index((C, M))
    errs = []
    for j in range(2):
        k = 2 * i + j
        xdt, ydt, ddt = (F32, BF)[k % 2], (F32, BF)[(k // 2) % 2], (F32, BF)[(k // 4) % 2]
        acc = ddt == F32 and k % 3 != 1
        has_w = k % 5 != 4
        want = ((True, True), (True, False), (False, True), (False, False))[(k // 3) % 4]
        pwrite = (k // 2) % 3 == 1
        g = _gen(6, C, M, j)
        x = _ln_rows(M, C, xdt, g)
        dy = (torch.randint(-32, 33, (M, C), generator=g).float() / 8).to(ydt)  # db = sum dy is exact
        w = 1 + 0.1 * torch.randn(C, generator=g) if has_w else None
        prev = torch.randn(M, C, generator=g)
        dw0, db0 = (torch.randint(-4, 5, (C,), generator=g).float() for _ in range(2))
        nm = (f"layernorm_bwd C={C} M={M} x {_dtn(xdt)} dy {_dtn(ydt)} dx {_dtn(ddt)} acc={acc} w={has_w} "
              f"dw/db={want} write={pwrite}")
        xb, yb = Box(x, NAN), Box(dy, NAN, cols=(16, 8))
        runs = []
        for _ in range(2):
            dxb = Box(prev if acc else torch.full((M, C), SENT).to(ddt), SENT, cols=(8, 8))
            dw, db = dw0.cuda(), db0.cuda()
            N.layernorm_bwd(xb.v, None if w is None else w.cuda(), EPS, yb.v, dxb.v, acc, dw if want[0] else None,
                            db if want[1] else None, params_write=pwrite)
            runs.append((dxb.got(), dw.cpu(), db.cpu()))
            if not dxb.intact():
                errs.append(nm + ": dx sentinels overwritten")
        got, gw, gb = runs[0]
        for t, part in enumerate(("dx", "dw", "db")):
            _eq_bits(errs, nm + f" {part} second run", runs[1][t], runs[0][t])
        dx64, dw64, db64 = _ln_ref64(x, w, dy)
        mdx, mdw = _ln_model(x, w, dy)
        if acc:
            dx64, mdx = dx64 + prev.double(), mdx + prev
        _model_rule(errs, nm + " dx", got, mdx.to(ddt), dx64, "layernorm_bwd dx")
        base = 0.0 if pwrite else dw0
        if want[0]:
            _model_rule(errs, nm + " dw", gw[None], (mdw + base)[None], (dw64 + base)[None], "layernorm_bwd dw")
        else:
            _eq_bits(errs, nm + " NULL dw untouched", gw, dw0)
        if want[1]:
            assert float(dy.double().abs().sum(0).max() + 4) * 8 < 2 ** 24
            _eq_bits(errs, nm + " db", gb, (db64 + (0.0 if pwrite else db0.double())).float())
        else:
            _eq_bits(errs, nm + " NULL db untouched", gb, db0)
    print(f"layernorm_bwd C={C} M={M}: kernel / model worst row so far (worst, model, ratio): dx "
          f"{FIG.get(('model', 'layernorm_bwd dx'))}, dw {FIG.get(('model', 'layernorm_bwd dw'))}")
    _done(errs, ("layernorm_bwd", {"NV": C // 256}, M, _reach_chunks(M, 2048)))


def test_layernorm_bwd_group_map(N):
    """Logical row r -> group r / 3: x / dx rows g * 5 + 1 + i (x_off != 0, stride > group), dy rows
    g * 4 + i; 7 rows (a ragged last group).  Skipped x / dy rows hold NaN, skipped dx rows sentinels."""
    C, M, G, xgs, xoff, ygs, yoff = 512, 7, 3, 5, 1, 4, 0
    g = _gen(61)
    errs = []
    xl = _ln_rows(M, C, BF, g)
    dyl = torch.randint(-32, 33, (M, C), generator=g).float() / 8
    w = 1 + 0.1 * torch.randn(C, generator=g)
    r = torch.arange(M)
    xrow, yrow = (r // G) * xgs + xoff + r % G, (r // G) * ygs + yoff + r % G
    xfull, yfull = torch.full((14, C), NAN).to(BF), torch.full((12, C), NAN)
    xfull[xrow], yfull[yrow] = xl, dyl
    xb, yb, dxb = Box(xfull, NAN), Box(yfull, NAN), Box(torch.full((14, C), SENT), SENT)
    dw, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    N.layernorm_bwd(xb.v, w.cuda(), EPS, yb.v, dxb.v, False, dw, db, M=M, group=G, x_gstride=xgs, x_off=xoff,
                    y_gstride=ygs, y_off=yoff)
    dx64, dw64, db64 = _ln_ref64(xl, w, dyl)
    mdx, mdw = _ln_model(xl, w, dyl)
    _model_rule(errs, "group map dx", dxb.got()[xrow], mdx, dx64, "layernorm_bwd dx")
    _model_rule(errs, "group map dw", dw.cpu()[None], mdw[None], dw64[None], "layernorm_bwd dw")
    _eq_bits(errs, "group map db", db.cpu(), db64.float())
    keep = torch.zeros(dxb.host.shape, dtype=torch.bool)
    keep[2 + xrow, 8:8 + C] = True
    if not dxb.intact(keep):
        errs.append("group map: skipped dx rows or the padding were written")
    _done(errs)


def test_layernorm_bwd_error_returns(N):
    outs = []

    def call(C, ddt=F32, acc=False, ld_extra=0, flags_write=False):
        x = torch.zeros(4, C + ld_extra, device="cuda")[:, :C]
        dy = torch.zeros(4, C, device="cuda")
        dx = torch.full((4, C), SENT, device="cuda").to(ddt)
        dw, db = torch.full((C,), SENT, device="cuda"), torch.full((C,), SENT, device="cuda")
        outs.extend((dx, dw, db))
        return lambda: N.layernorm_bwd(x, None, EPS, dy, dx, acc, dw, db, params_write=flags_write)

    _raises(ERR_SHAPE, call(768))
    _raises(ERR_SHAPE, call(2048))
    _raises(ERR_UNSUPPORTED, call(512, ddt=BF, acc=True))
    _raises(ERR_ALIGN, call(512, ld_extra=1))
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.float() == SENT).all())


# ================================================================== 5. headnorm_rope_bwd
ROPE_NONE, ROPE_2D, ROPE_1D = 0, 1, 2
HN_M = [1, 3, 4, 5, 17, 40]


def _hn_tables(D, mode, tab_len):
    rd = D // 2 if mode == ROPE_2D else D
    return O.rope_cos_sin(rd, tab_len, 100.0)


def _hn_positions(M, mode, period, tab_len, pos):
    """Per-row clamped table rows, as the forward kernel clamps: (M,) or (M, 2)."""
    rows = torch.arange(M) % period
    return pos.long()[rows].clamp(0, tab_len - 1)


def _rope_T(dz, p, cos, sin):
    """Transpose of y -> y cos + rotate_half(y) sin over the last dim (tables are cat(angles, angles))."""
    c, s = cos.to(dz.dtype)[p][:, None, :], sin.to(dz.dtype)[p][:, None, :]
    h = dz.shape[-1] // 2
    return dz * c + torch.cat((dz[..., h:], -dz[..., :h]), -1) * s, (dz * c).abs() + (dz * s).abs().roll(h, -1)


def _hn_model(pre, grad, H, hsplit, D, w0, w1, mode, p, cos, sin, dt):
    """du, the four parameter sums and sum |terms| of the db sums, in dtype dt (fp32: the model)."""
    M = pre.shape[0]
    u, dz = pre.to(dt).view(M, H, D), grad.to(dt).view(M, H, D)
    if mode == ROPE_1D:
        dy, ady = _rope_T(dz, p, cos, sin)
    elif mode == ROPE_2D:
        a, aa = _rope_T(dz[..., :D // 2], p[:, 0], cos, sin)
        b, ab = _rope_T(dz[..., D // 2:], p[:, 1], cos, sin)
        dy, ady = torch.cat((a, b), -1), torch.cat((aa, ab), -1)
    else:
        dy, ady = dz, dz.abs()
    du = dy.clone()
    sums = []
    for lo, hi, w in ((0, hsplit, w0), (hsplit, H, w1)):
        if w is None or hi == lo:
            sums.append((torch.zeros(D, dtype=dt), torch.zeros(D, dtype=dt), torch.zeros(D, dtype=dt)))
            continue
        uu, dd = u[:, lo:hi], dy[:, lo:hi]
        mean = uu.sum(-1, keepdim=True) * (1.0 / D)
        d = uu - mean
        rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) * (1.0 / D) + EPS)
        xh = d * rstd
        gd = dd * w.to(dt)
        m1, m2 = gd.sum(-1, keepdim=True) * (1.0 / D), (gd * xh).sum(-1, keepdim=True) * (1.0 / D)
        du[:, lo:hi] = rstd * (gd - m1 - xh * m2)
        sums.append(((dd * xh).sum((0, 1)), dd.sum((0, 1)), ady[:, lo:hi].sum((0, 1))))
    return du.reshape(M, H * D), sums


def _hn_ref64(pre, grad, H, hsplit, D, w0, w1, mode, p, cos, sin):
    """fp64 autograd of LayerNorm in doubles followed by the oracle's rope in doubles."""
    M = pre.shape[0]
    u = pre.double().view(M, H, D).requires_grad_(True)
    ws = [None if w is None else w.double().requires_grad_(True) for w in (w0, w1)]
    bs = [None if w is None else torch.zeros(D, dtype=F64, requires_grad=True) for w in (w0, w1)]
    parts = []
    for lo, hi, w, b in ((0, hsplit, ws[0], bs[0]), (hsplit, H, ws[1], bs[1])):
        if hi > lo:
            parts.append(u[:, lo:hi] if w is None else F.layer_norm(u[:, lo:hi], (D,), w, b, EPS))
    y = torch.cat(parts, 1).transpose(0, 1)[None]  # (1, H, M, D)
    c64, s64 = (None, None) if mode == ROPE_NONE else (cos.double(), sin.double())
    if mode == ROPE_1D:
        y = O._rope_apply(y, p[None], c64, s64)
    elif mode == ROPE_2D:
        y = torch.cat((O._rope_apply(y[..., :D // 2], p[None, :, 0], c64, s64),
                       O._rope_apply(y[..., D // 2:], p[None, :, 1], c64, s64)), -1)
    y.backward(grad.double().view(M, H, D).transpose(0, 1)[None])
    zero = torch.zeros(D, dtype=F64)
    pg = [(zero, zero) if w is None or w.grad is None else (w.grad, b.grad) for w, b in zip(ws, bs)]
    return u.grad.reshape(M, H * D), pg


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mode", [ROPE_NONE, ROPE_2D, ROPE_1D], ids=["none", "2d", "1d"])
@pytest.mark.parametrize("D", [64, 128])
def test_headnorm_rope_bwd(N, D, mode, dt):
    hpp = 64 // (D // 8)
    errs, reach, worst = [], [], 0.0
    tab_len = 9

    def period_of(M):  # a period that does not divide M
        p = (2 * M) // 3 if M > 2 else M + 1
        return p + 1 if M % p == 0 else p

    cfg = 0
    for H in (1, hpp - 1, hpp, hpp + 1, 2 * hpp + 1):
        for wset in ("both", "w0 only", "none"):
            splits = (0, H // 2, H) if wset == "both" else (H,) if wset == "w0 only" else (H // 2,)
            for hsplit in splits:
                cfg += 1
                M = HN_M[cfg % len(HN_M)]
                period = period_of(M)
                g = _gen(7, D, mode, dt == BF, H, cfg)
                C = H * D
                pre = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dt)
                grad = torch.randn(M, C, generator=g).to(dt)
                w0 = 1 + 0.1 * torch.randn(D, generator=g) if wset != "none" else None
                w1 = 1 + 0.1 * torch.randn(D, generator=g) if wset == "both" else None
                pos = cos = sin = p = None
                if mode != ROPE_NONE:
                    pos = torch.randint(-2, tab_len + 3, (period, 2) if mode == ROPE_2D else (period,), generator=g,
                                        dtype=torch.int32)
                    cos, sin = _hn_tables(D, mode, tab_len)
                    p = _hn_positions(M, mode, period, tab_len, pos)
                p0 = [torch.randint(-4, 5, (D,), generator=g).float() for _ in range(4)]
                ask = [(cfg >> b) & 1 == 0 or cfg % 5 == 0 for b in range(4)]  # a partial set of dw0 db0 dw1 db1
                nm = (f"headnorm_rope_bwd D={D} mode={mode} {_dtn(dt)} H={H} hsplit={hsplit} M={M} weights={wset} "
                      f"period={period} ask={ask}")
                pb = Box(pre, NAN, cols=(8, 16))
                runs = []
                for _ in range(2):
                    gb = Box(grad, SENT, rows=(1, 2), cols=(16, 24))
                    outs = [t.cuda() for t in p0]
                    N.headnorm_rope_bwd(pb.v, gb.v, H, hsplit, D, None if w0 is None else w0.cuda(),
                                        None if w1 is None else w1.cuda(), EPS, mode,
                                        None if pos is None else pos.cuda(), period,
                                        None if cos is None else cos.cuda().contiguous(),
                                        None if sin is None else sin.cuda().contiguous(),
                                        *[o if a else None for o, a in zip(outs, ask)])
                    runs.append([gb.got()] + [o.cpu() for o in outs])
                    if not gb.intact():
                        errs.append(nm + ": sentinels around grad overwritten")
                for t in range(5):
                    _eq_bits(errs, nm + f" output {t} second run", runs[1][t], runs[0][t])
                du64, pg64 = _hn_ref64(pre, grad, H, hsplit, D, w0, w1, mode, p, cos, sin)
                mdu, msum = _hn_model(pre, grad, H, hsplit, D, w0, w1, mode, p, cos, sin, F32)
                _, sum64 = _hn_model(pre, grad, H, hsplit, D, w0, w1, mode, p, cos, sin, F64)
                view = lambda t: t.reshape(M, H, D)  # noqa: E731
                _model_rule(errs, nm + " du", view(runs[0][0]), view(mdu.to(dt)), view(du64),
                            f"headnorm_rope_bwd du {_dtn(dt)}")
                nblk = _reach_chunks(M, 2048)["chunks"]
                for s, (lo, hi, w) in enumerate(((0, hsplit, w0), (hsplit, H, w1))):
                    gw, gbias = runs[0][1 + 2 * s], runs[0][2 + 2 * s]
                    live = w is not None and hi > lo and any(ask)
                    if live and ask[2 * s]:
                        _model_rule(errs, nm + f" dw{s}", gw[None], (msum[s][0] + p0[2 * s])[None],
                                    (pg64[s][0] + p0[2 * s])[None], "headnorm_rope_bwd dw")
                    elif not (w is not None and any(ask) and ask[2 * s]):
                        _eq_bits(errs, nm + f" dw{s} untouched", gw, p0[2 * s])
                    else:  # asked for, no head in the set: += 0
                        _eq_bits(errs, nm + f" dw{s} empty set", gw, p0[2 * s])
                    if live and ask[2 * s + 1]:
                        n = M * (hi - lo)
                        E = _gam(n + nblk + 16 + 4) * (sum64[s][2] + p0[2 * s + 1].abs().double())
                        worst = max(worst, _interval(errs, nm + f" db{s}", gbias, pg64[s][1] + p0[2 * s + 1].double(), E))
                    else:
                        _eq_bits(errs, nm + f" db{s} untouched or empty", gbias, p0[2 * s + 1])
                reach.append((H, hsplit, M, wset, "passes", -(-H // hpp), "ragged" if H % hpp else "full"))
    print(f"headnorm_rope_bwd D={D} mode={mode} {_dtn(dt)}: {cfg} configurations, db worst |got - s| / E = {worst:.4f}; "
          f"du (worst, model, ratio) {FIG.get(('model', 'headnorm_rope_bwd du ' + _dtn(dt)))}, "
          f"dw {FIG.get(('model', 'headnorm_rope_bwd dw'))}")
    _fig(("interval", "headnorm_rope_bwd db"), worst)
    _done(errs, ("headnorm_rope_bwd heads per pass", hpp, reach))


# ================================================================== 6. attention_small_bwd
def _attn_ref(q, k, v, do, scale, dt):
    """(B, H, n, D) operands in dtype dt: the documented arithmetic (fp32: the model; fp64: the reference)."""
    q, k, v, do = (t.to(dt) for t in (q, k, v, do))
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, -1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return (ds @ k) * scale, (ds.transpose(-1, -2) @ q) * scale, p.transpose(-1, -2) @ do


def _attn_case(N, dt, D, nq, nk, errs, layout="dense", gain=1.0, scale=None, B=2, H=3, seed=0):
    """One launch with batch strides nq + 2 / nk + 3 (NaN rows between the batches) and the layout:
    dense (16-B rows), 'stride' (row stride not a multiple of 16 B), 'base' (base pointer two
    elements in), 'odd' (heads * D plus an odd pad on the inputs)."""
    g = _gen(8, dt == BF, D, nq, nk, seed)
    C = H * D
    qbs, kbs = nq + 2, nk + 3
    mk = lambda n: (torch.randn(B, n, H, D, generator=g) * gain).to(dt)  # noqa: E731
    q, do, k, v = mk(nq), mk(nq) / gain, mk(nk), mk(nk) / gain
    sc = D ** -0.5 if scale is None else scale
    ipad = {"dense": (8, 16), "stride": (8, 12 if dt == BF else 6), "base": (2, 22), "odd": (8, 17)}[layout]
    opad = {"dense": (8, 16), "stride": (8, 12 if dt == BF else 6), "base": (2, 22), "odd": (8, 18)}[layout]

    def rows(t, bs, fill):  # (B, n, H, D) -> (B * bs, C) with `fill` rows after each batch
        out = torch.full((B, bs, C), fill, dtype=dt)
        out[:, :t.shape[1]] = t.reshape(B, t.shape[1], C)
        return out.reshape(B * bs, C)

    qb, dob = Box(rows(q, qbs, NAN), NAN, cols=ipad), Box(rows(do, qbs, NAN), NAN, cols=ipad)
    kb, vb = Box(rows(k, kbs, NAN), NAN, cols=ipad), Box(rows(v, kbs, NAN), NAN, cols=ipad)
    dqb = Box(torch.full((B * qbs, C), SENT, dtype=dt), SENT, cols=opad)
    dkb, dvb = (Box(torch.full((B * kbs, C), SENT, dtype=dt), SENT, cols=opad) for _ in range(2))
    N.attention_small_bwd(qb.v, kb.v, vb.v, dob.v, dqb.v, dkb.v, dvb.v, B, H, nq, nk, D, qbs, kbs, qbs, qbs, kbs,
                          scale=scale)
    reach = _reach_attn(dt, D, [b.dev.stride(0) for b in (qb, kb, vb, dob)], [b.v.data_ptr() for b in (qb, kb, vb, dob)])
    nm = f"attention_small_bwd {_dtn(dt)} D={D} nq={nq} nk={nk} {layout} gain={gain} scale={sc:.4f}"
    tr = lambda t: t.transpose(1, 2)  # noqa: E731  (B, n, H, D) -> (B, H, n, D)
    ref = _attn_ref(tr(q), tr(k), tr(v), tr(do), sc, F64)
    mod = _attn_ref(tr(q), tr(k), tr(v), tr(do), sc, F32)
    for box, bs, n, r64, m32, part in ((dqb, qbs, nq, ref[0], mod[0], "dq"), (dkb, kbs, nk, ref[1], mod[1], "dk"),
                                       (dvb, kbs, nk, ref[2], mod[2], "dv")):
        full = box.got().view(B, bs, H, D)
        got = tr(full[:, :n])
        _model_rule(errs, f"{nm} {part}", got, m32.to(dt), r64, f"attention_small_bwd {_dtn(dt)}")
        keep = torch.zeros(box.host.shape, dtype=torch.bool)
        r0, _, c0, _ = box.win
        for b in range(B):
            keep[r0 + b * bs:r0 + b * bs + n, c0:c0 + C] = True
        if not box.intact(keep):
            errs.append(f"{nm} {part}: rows between the batches or the padding were written")
    return nm, reach


AT_CASES = [(2, 1, 1), (2, 17, 17), (6, 1, 12), (6, 5, 60), (8, 15, 1), (8, 257, 1), (8, 17, 17),
            (64, 1, 1), (64, 1, 12), (64, 15, 1), (64, 17, 17), (64, 5, 60),
            (128, 1, 12), (128, 15, 1), (128, 17, 17), (128, 29, 28)]


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D,nq,nk", AT_CASES)
def test_attention_small_bwd(N, dt, D, nq, nk):
    errs = []
    assert _attn_lds(nq, nk, D) <= 64 * 1024
    nm, reach = _attn_case(N, dt, D, nq, nk, errs)
    assert reach == ("16-B staging" if D % 8 == 0 else "scalar staging")
    print(nm, "->", reach, "LDS", _attn_lds(nq, nk, D), FIG.get(("model", "attention_small_bwd " + _dtn(dt))))
    _done(errs, (nm, reach))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("layout", ["stride", "base", "odd"])
def test_attention_small_bwd_scalar_staging_at_64(N, dt, layout):
    errs = []
    nm, reach = _attn_case(N, dt, 64, 17, 17, errs, layout=layout, seed=1)
    assert reach == "scalar staging"
    nm2, reach2 = _attn_case(N, dt, 64, 5, 60, errs, layout=layout, scale=0.2, seed=2)
    assert reach2 == "scalar staging"
    print(nm, "->", reach, FIG.get(("model", "attention_small_bwd " + _dtn(dt))))
    _done(errs, (nm, reach), (nm2, reach2))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_attention_small_bwd_scale_and_peaked(N, dt):
    errs = []
    r = [_attn_case(N, dt, 64, 17, 17, errs, scale=0.31, seed=3), _attn_case(N, dt, 64, 17, 17, errs, gain=8.0, seed=4),
         _attn_case(N, dt, 8, 257, 1, errs, gain=8.0, seed=5), _attn_case(N, dt, 128, 15, 1, errs, scale=1.0, seed=6)]
    print(FIG.get(("model", "attention_small_bwd " + _dtn(dt))))
    _done(errs, *r)


def test_attention_small_bwd_lds_limit(N):
    """(29, 28) at D = 128 is the largest admitted shape (run in test_attention_small_bwd); (29, 29) at
    D = 128 and (1, 125) at D = 64 exceed (2 nq (D+1) + 2 nk (D+1) + 2 nq nk) 4 <= 64 KiB: VGGT_ERR_SHAPE,
    outputs untouched."""
    assert _attn_lds(29, 28, 128) <= 65536 < _attn_lds(29, 29, 128) and _attn_lds(1, 125, 64) > 65536
    assert (2 * 1 * 64 + 2 * 125 * 64 + 2 * 125) * 4 <= 65536  # the formula without the pad column would admit it
    for D, nq, nk in ((128, 29, 29), (64, 1, 125)):
        for dt in (BF, F32):
            q, do = (torch.zeros(nq, D, dtype=dt, device="cuda") for _ in range(2))
            k, v = (torch.zeros(nk, D, dtype=dt, device="cuda") for _ in range(2))
            dq = torch.full((nq, D), SENT, dtype=dt, device="cuda")
            dk, dv = (torch.full((nk, D), SENT, dtype=dt, device="cuda") for _ in range(2))
            _raises(ERR_SHAPE, N.attention_small_bwd, q, k, v, do, dq, dk, dv, 1, 1, nq, nk, D, nq, nk, nq, nq, nk)
            torch.cuda.synchronize()
            assert all(bool((t.float() == SENT).all()) for t in (dq, dk, dv))
    print("reach", ("attention_small_bwd LDS", {"29x28 D128": _attn_lds(29, 28, 128), "29x29 D128": _attn_lds(29, 29, 128),
                                                "1x125 D64": _attn_lds(1, 125, 64)}))


# ================================================================== 7. transpose_b16
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 70])
def test_transpose_b16(N, rows):
    errs = []
    for cols in (1, 63, 64, 65, 200):
        for rows_pad in (rows, rows + 1, (rows // 64 + 1) * 64, rows + 130):
            g = _gen(9, rows, cols, rows_pad)
            src = torch.randint(-32768, 32768, (rows, cols), generator=g).to(torch.int16)
            sb = Box(src, 0x7fc0, rows=(1, 2), cols=(3, 5))  # (the bf16 NaN pattern)
            dbx = Box(torch.full((cols + 2, rows_pad + 3), 0x4242, dtype=torch.int16), 0x4242, rows=(1, 1), cols=(1, 2))
            r0, _, c0, _ = dbx.win
            dst = dbx.dev[r0:r0 + cols, c0:c0 + rows_pad] if rows_pad else dbx.dev[r0:r0 + cols, c0:c0 + 1]
            N.transpose_b16(sb.v, dst, rows_pad)
            got = dbx.dev.cpu()[r0:r0 + cols, c0:c0 + rows_pad]
            ref = torch.zeros(cols, rows_pad, dtype=torch.int16)
            ref[:, :rows] = src.t()
            nm = f"transpose_b16 rows={rows} cols={cols} rows_pad={rows_pad}"
            if not torch.equal(got, ref):
                errs.append(f"{nm}: " + _first(got != ref, got, ref))
            keep = torch.zeros(dbx.host.shape, dtype=torch.bool)
            keep[r0:r0 + cols, c0:c0 + rows_pad] = True
            if not dbx.intact(keep):
                errs.append(f"{nm}: destination columns >= rows_pad or rows >= cols were written")
    _done(errs)


# ================================================================== 8. batch_dot_f32
def _bd_reach(n):
    nc = min(256, -(-n // 65536))
    return {"chunks": nc, "per_chunk": -(-n // nc)}


def _batch_dot_case(N, B, n, errs, bs=None):
    worst = 0.0
    bs = n + 24 if bs is None else bs
    for exact in (True, False):
        g = _gen(10, B, n, exact)
        if exact:
            a, c = (torch.randint(-1, 2, (B, n), generator=g).float() for _ in range(2))
        else:
            a, c = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g) + 0.5
        ab_, cb = (torch.full((B, bs), NAN) for _ in range(2))
        ab_[:, :n], cb[:, :n] = a, c
        ad, cd = ab_.cuda(), cb.cuda()
        out = torch.full((B + 2,), SENT, device="cuda")
        N.batch_dot_f32(ad[:, :n], cd[:, :n], out[1:1 + B])
        first = out.cpu()
        N.batch_dot_f32(ad[:, :n], cd[:, :n], out[1:1 + B])
        got = out.cpu()
        nm = f"batch_dot_f32 B={B} n={n} bs={bs} {'exact' if exact else 'random'}"
        _eq_bits(errs, nm + " second run", got, first)
        if not (got[0] == SENT and got[-1] == SENT):
            errs.append(nm + ": sentinels overwritten")
        s = (a.double() * c.double()).sum(1) + 0.0
        t = (a.double() * c.double()).abs().sum(1)
        if exact:
            assert float(t.max()) < 2 ** 24
            _eq_bits(errs, nm, got[1:-1], s.float())
        else:  # n rounded (or fused) products, the wave / block tree, the chunk partials and 16 slices
            E = _gam(n + 1 + _bd_reach(n)["chunks"] + 16) * t
            worst = max(worst, _interval(errs, nm, got[1:-1], s, E))
    return worst


@pytest.mark.parametrize("n", [1, 255, 257, 65536, 65537, 200000])
def test_batch_dot_f32(N, n):
    errs, worst = [], 0.0
    for B in (1, 3, 17):
        worst = max(worst, _batch_dot_case(N, B, n, errs))
    print(f"batch_dot_f32 n={n}: worst |got - s| / E = {worst:.5f}")
    _fig(("interval", "batch_dot_f32"), worst)
    _done(errs, ("batch_dot_f32", n, _bd_reach(n)))


def test_batch_dot_f32_chunk_cap(N):
    """n = 256 * 65536 + 1: 257 chunks asked, 256 launched, 65537 elements each (+-1 / 0 inputs: exact)."""
    n = 256 * 65536 + 1
    g = _gen(101)
    a, c = (torch.randint(-1, 2, (1, n), generator=g).float() for _ in range(2))
    s = (a.double() * c.double()).sum(1)
    assert float((a.double() * c.double()).abs().sum()) < 2 ** 24
    out = torch.full((3,), SENT, device="cuda")
    N.batch_dot_f32(a.cuda(), c.cuda(), out[1:2])
    got = out.cpu()
    errs = []
    _eq_bits(errs, "batch_dot_f32 chunk cap", got[1:2], s.float())
    assert got[0] == SENT and got[2] == SENT
    assert _bd_reach(n) == {"chunks": 256, "per_chunk": 65537}
    _done(errs, ("batch_dot_f32", n, _bd_reach(n)))


# ================================================================== 9. the argument checks, rule by rule
def _buf(rows, cols, dt=F32):
    return torch.full((rows, cols), SENT, dtype=dt, device="cuda")


def _rule_walk(L, entry, args, outs, rules):
    """One valid call of the raw ctypes entry (VGGT_OK), then one call per rule with exactly that
    argument changed; every call must return the documented code, and after a synchronise every
    buffer of `outs` (refilled after the valid call) holds its sentinel bit for bit.  Returns the
    number of calls."""
    fn, base = getattr(L, entry), dict(args)
    assert len(base) == len(args) == len(fn.argtypes), entry
    rc = fn(*base.values())
    assert rc == OK, f"{entry}: the valid call returned {rc}"
    torch.cuda.synchronize()
    for t in outs:
        t.fill_(SENT)
    calls = 1
    for change, code in rules:
        assert set(change) <= set(base), (entry, change)
        rc = fn(*{**base, **change}.values())
        assert rc == code, f"{entry} with {change}: returned {rc}, documented {code}"
        calls += 1
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        assert bool((_bits(t.cpu()) == _bits(torch.full_like(t, SENT).cpu())).all()), f"{entry}: buffer {i} was written"
    return calls


def _rules(shape=(), align=(), dtype=(), null=(), ok=()):
    """(argument, broken value) pairs per documented code; `null` names required pointers."""
    return ([({k: v}, ERR_SHAPE) for k, v in shape] + [({k: v}, ERR_ALIGN) for k, v in align] +
            [({k: 7}, ERR_UNSUPPORTED) for k in dtype] + [({k: None}, ERR_SHAPE) for k in null] +
            [({k: v}, OK) for k, v in ok])


def test_train_entry_error_returns(N):
    """Every entry point of train.hip at M = 4, N = 8 (or its smallest legal shape), through the raw
    ctypes entries (`_native._dt` would refuse a bad dtype first): each dimension rule, each leading
    dimension and pointer alignment rule, each dtype argument set to 7, each required pointer NULL, a
    short and a NULL workspace -- and M == 0, which is VGGT_OK with nothing launched on the elementwise
    and the row-backward entries and VGGT_ERR_SHAPE on the column reductions and the weight gradients.
    Buffers are larger than any broken call could reach (a 16-column pitch, spare rows)."""
    L = N.lib()
    M, Nn, LD = 4, 8, 16
    total = {}
    ws = torch.empty(1 << 16, device="cuda")
    wsr = [("ws", ws.data_ptr()), ("ws_bytes", ws.numel() * 4), ("stream", None)]
    dims = [("M", 0), ("M", -1), ("N", 0), ("N", 6)]
    ew_dims = [("M", -1), ("N", 0), ("N", 6)]

    def short(nbytes):  # one float less than the entry needs; no workspace at all
        return [("ws_bytes", nbytes - 4), ("ws", None)]

    # ---- column reductions (one chunk at M = 4: a partial vector is N floats)
    x, o = _buf(M + 2, LD), _buf(1, LD)
    total["vggt_colsum"] = _rule_walk(
        L, "vggt_colsum", [("x", x.data_ptr()), ("dtype", 0), ("ldx", LD), ("M", M), ("N", Nn), ("out", o.data_ptr()),
                           ("accumulate", 0)] + wsr, [x, o],
        _rules(shape=dims + short(Nn * 4), align=[("ldx", LD + 1), ("x", x.data_ptr() + 4)], dtype=["dtype"],
               null=["x", "out"]))
    assert int(L.vggt_colred_workspace_bytes(M, Nn)) == 2 * Nn * 4
    d, b, g, ob, dg, db = _buf(M + 2, LD), _buf(M + 2, LD, BF), _buf(1, LD), _buf(M + 2, LD, BF), _buf(1, LD), _buf(1, LD)
    total["vggt_layerscale_bwd"] = _rule_walk(
        L, "vggt_layerscale_bwd",
        [("dout", d.data_ptr()), ("ldd", LD), ("branch", b.data_ptr()), ("bdtype", 1), ("ldb", LD), ("gamma", g.data_ptr()),
         ("dbranch", ob.data_ptr()), ("odtype", 1), ("ldo", LD), ("M", M), ("N", Nn), ("dgamma", dg.data_ptr()),
         ("dbias", db.data_ptr())] + wsr, [ob, dg, db],
        _rules(shape=dims + short(2 * Nn * 4),
               align=[("ldd", LD + 1), ("ldb", LD + 1), ("ldo", LD + 1), ("dout", d.data_ptr() + 8),
                      ("gamma", g.data_ptr() + 8), ("branch", b.data_ptr() + 4), ("dbranch", ob.data_ptr() + 4)],
               dtype=["bdtype", "odtype"], null=["dout", "branch", "gamma", "dbranch"]))
    h, p = _buf(M + 2, LD, BF), _buf(M + 2, LD)
    total["vggt_gelu_bwd"] = _rule_walk(
        L, "vggt_gelu_bwd",
        [("dh", h.data_ptr()), ("dhdtype", 1), ("lddh", LD), ("pre", p.data_ptr()), ("predtype", 0), ("ldp", LD),
         ("dpre", ob.data_ptr()), ("odtype", 1), ("ldo", LD), ("M", M), ("N", Nn), ("dbias", db.data_ptr())] + wsr,
        [ob, db],
        _rules(shape=dims + short(Nn * 4),
               align=[("lddh", LD + 1), ("ldp", LD + 1), ("ldo", LD + 1), ("dh", h.data_ptr() + 4),
                      ("pre", p.data_ptr() + 4), ("dpre", ob.data_ptr() + 4)],
               dtype=["dhdtype", "predtype", "odtype"], null=["dh", "pre", "dpre"]))
    # ---- elementwise
    total["vggt_gelu_fwd"] = _rule_walk(
        L, "vggt_gelu_fwd", [("x", p.data_ptr()), ("xdtype", 0), ("ldx", LD), ("y", ob.data_ptr()), ("ydtype", 1),
                             ("ldy", LD), ("M", M), ("N", Nn), ("stream", None)], [ob],
        _rules(shape=ew_dims, align=[("ldx", LD + 1), ("ldy", LD + 1), ("x", p.data_ptr() + 4), ("y", ob.data_ptr() + 4)],
               dtype=["xdtype", "ydtype"], null=["x", "y"], ok=[("M", 0)]))
    xo = _buf(M + 2, LD)
    total["vggt_resid_scale_add_from"] = _rule_walk(
        L, "vggt_resid_scale_add_from",
        [("out", xo.data_ptr()), ("ldo", LD), ("x", x.data_ptr()), ("ldx", LD), ("branch", b.data_ptr()), ("bdtype", 1),
         ("ldb", LD), ("gamma", g.data_ptr()), ("M", M), ("N", Nn), ("stream", None)], [xo],
        _rules(shape=ew_dims,
               align=[("ldo", LD + 1), ("ldx", LD + 1), ("ldb", LD + 1), ("out", xo.data_ptr() + 8),
                      ("x", x.data_ptr() + 8), ("gamma", g.data_ptr() + 8), ("branch", b.data_ptr() + 4)],
               dtype=["bdtype"], null=["out", "x", "branch", "gamma"], ok=[("M", 0)]))
    total["vggt_resid_scale_add"] = _rule_walk(
        L, "vggt_resid_scale_add",
        [("x", xo.data_ptr()), ("ldx", LD), ("branch", b.data_ptr()), ("bdtype", 1), ("ldb", LD), ("gamma", g.data_ptr()),
         ("M", M), ("N", Nn), ("stream", None)], [xo],
        _rules(shape=ew_dims,
               align=[("ldx", LD + 1), ("ldb", LD + 1), ("x", xo.data_ptr() + 8), ("gamma", g.data_ptr() + 8),
                      ("branch", b.data_ptr() + 4)],
               dtype=["bdtype"], null=["x", "branch", "gamma"], ok=[("M", 0)]))
    # ---- transpose (no alignment or dtype rule: 2-byte elements one by one)
    ts, td = _buf(M + 2, LD, BF), _buf(LD, LD, BF)
    total["vggt_transpose_b16"] = _rule_walk(
        L, "vggt_transpose_b16", [("src", ts.data_ptr()), ("lds", LD), ("rows", M), ("cols", Nn), ("dst", td.data_ptr()),
                                  ("ldd", LD), ("rows_pad", M + 2), ("stream", None)], [td],
        _rules(shape=[("rows", -1), ("cols", 0), ("rows_pad", M - 1)], null=["src", "dst"]))
    # ---- LayerNorm backward (smallest C = 256; one block: a partial vector is C floats)
    C = 256
    lx, ly, ldx_, lw, lb = _buf(M + 2, C + 8), _buf(M + 2, C + 8, BF), _buf(M + 2, C + 8), _buf(1, C), _buf(1, C)
    assert int(L.vggt_layernorm_bwd_workspace_bytes(M, C)) == 2 * C * 4
    total["vggt_layernorm_bwd"] = _rule_walk(
        L, "vggt_layernorm_bwd",
        [("x", lx.data_ptr()), ("xdtype", 0), ("ldx", C + 8), ("w", None), ("eps", EPS), ("dy", ly.data_ptr()),
         ("dydtype", 1), ("ldy", C + 8), ("dx", ldx_.data_ptr()), ("dxdtype", 0), ("lddx", C + 8), ("accumulate", 0),
         ("M", M), ("C", C), ("group", M), ("xgs", 0), ("xoff", 0), ("ygs", 0), ("yoff", 0), ("dw", lw.data_ptr()),
         ("db", lb.data_ptr())] + wsr, [ldx_, lw, lb],
        _rules(shape=[("M", -1), ("C", 0), ("C", 768), ("C", 2048), ("group", 0)] + short(2 * C * 4),
               align=[("ldx", C + 9), ("ldy", C + 9), ("lddx", C + 9), ("x", lx.data_ptr() + 4), ("dy", ly.data_ptr() + 4),
                      ("dx", ldx_.data_ptr() + 4)],
               dtype=["xdtype", "dydtype", "dxdtype"], null=["x", "dy", "dx"], ok=[("M", 0)]) +
        [({"accumulate": 4}, ERR_UNSUPPORTED), ({"accumulate": 1, "dxdtype": 1}, ERR_UNSUPPORTED)])
    # ---- per-head norm + RoPE backward (one head of 64, 2-D RoPE: every table is required)
    D, tab = 64, 9
    hp, hg = _buf(M + 2, D + 8, BF), _buf(M + 2, D + 8, BF)
    hw = torch.ones(D, device="cuda")
    pos = torch.zeros(M, 2, dtype=torch.int32, device="cuda")
    cs, sn = (torch.zeros(tab, D // 2, device="cuda") for _ in range(2))
    hd = [_buf(1, D) for _ in range(4)]
    assert int(L.vggt_headnorm_rope_bwd_workspace_bytes(M, D)) == 4 * D * 4
    total["vggt_headnorm_rope_bwd"] = _rule_walk(
        L, "vggt_headnorm_rope_bwd",
        [("pre", hp.data_ptr()), ("ldp", D + 8), ("grad", hg.data_ptr()), ("ldg", D + 8), ("dtype", 1), ("M", M), ("H", 1),
         ("hsplit", 1), ("D", D), ("w0", hw.data_ptr()), ("w1", None), ("eps", EPS), ("rope_mode", ROPE_2D),
         ("pos", pos.data_ptr()), ("period", M), ("cos", cs.data_ptr()), ("sin", sn.data_ptr()), ("tab_len", tab),
         ("dw0", hd[0].data_ptr()), ("db0", hd[1].data_ptr()), ("dw1", hd[2].data_ptr()), ("db1", hd[3].data_ptr())] + wsr,
        [hg] + hd,
        _rules(shape=[("M", -1), ("H", 0), ("D", 32), ("hsplit", -1), ("hsplit", 2), ("period", 0), ("tab_len", 0)] +
               short(4 * D * 4),
               align=[("ldp", D + 4), ("ldg", D + 4), ("pre", hp.data_ptr() + 8), ("grad", hg.data_ptr() + 8)],
               dtype=["dtype", "rope_mode"], null=["pre", "grad", "pos", "cos", "sin"], ok=[("M", 0)]))
    # ---- small attention backward (bf16 pairs: 4-B output alignment, even output pitch)
    Da = 8
    aq, ak, av, ao = (_buf(M + 2, LD, BF) for _ in range(4))
    gq, gk, gv = (_buf(M + 2, LD, BF) for _ in range(3))
    total["vggt_attention_small_bwd"] = _rule_walk(
        L, "vggt_attention_small_bwd",
        [("q", aq.data_ptr()), ("ldq", LD), ("qbs", M), ("k", ak.data_ptr()), ("ldk", LD), ("kbs", M), ("v", av.data_ptr()),
         ("ldv", LD), ("dout", ao.data_ptr()), ("ldo", LD), ("obs", M), ("dq", gq.data_ptr()), ("lddq", LD), ("dqbs", M),
         ("dk", gk.data_ptr()), ("dv", gv.data_ptr()), ("lddkv", LD), ("dkvbs", M), ("dtype", 1), ("batch", 1),
         ("heads", 1), ("nq", M), ("nk", M), ("D", Da), ("scale", 0.5), ("stream", None)], [gq, gk, gv],
        _rules(shape=[("batch", 0), ("heads", 0), ("nq", 0), ("nk", 0), ("D", 0), ("D", 3)],
               align=[("lddq", LD + 1), ("lddkv", LD + 1), ("dq", gq.data_ptr() + 2), ("dk", gk.data_ptr() + 2),
                      ("dv", gv.data_ptr() + 2)],
               dtype=["dtype"], null=["q", "k", "v", "dout", "dq", "dk", "dv"]))
    # ---- weight gradients
    wy, wx, ww, wb = _buf(M + 2, LD), _buf(M + 2, LD), _buf(Nn + 2, LD), _buf(1, LD)
    wargs = [("dy", wy.data_ptr()), ("ldy", LD), ("x", wx.data_ptr()), ("ldx", LD), ("M", M), ("N", Nn), ("K", Nn),
             ("dw", ww.data_ptr()), ("ldw", LD)]
    wshape = [("M", 0), ("M", -1), ("N", 0), ("K", 0), ("N", 65536)]
    total["vggt_wgrad_f32"] = _rule_walk(L, "vggt_wgrad_f32", wargs + [("accumulate", 0), ("stream", None)], [ww],
                                         _rules(shape=wshape, null=["dy", "x", "dw"]))
    total["vggt_wgrad_bias_f32"] = _rule_walk(
        L, "vggt_wgrad_bias_f32", wargs + [("db", wb.data_ptr()), ("accumulate", 0), ("stream", None)], [ww, wb],
        _rules(shape=wshape, null=["dy", "x", "dw", "db"]))
    by, bx, bw = _buf(M + 2, 128 + 8, BF), _buf(M + 2, 128 + 8, BF), _buf(128, 128)
    need = int(L.vggt_wgrad_bf16_workspace_bytes(M, 128, 128))
    assert need == 128 * 128 * 4
    total["vggt_wgrad_bf16"] = _rule_walk(
        L, "vggt_wgrad_bf16", [("dy", by.data_ptr()), ("ldy", 136), ("x", bx.data_ptr()), ("ldx", 136), ("M", M),
                               ("N", 128), ("K", 128), ("dw", bw.data_ptr()), ("ldw", 128), ("accumulate", 0)] + wsr, [bw],
        _rules(shape=[("M", 0), ("M", -1), ("N", 0), ("K", 0), ("N", 192), ("K", 64)] + short(need),
               align=[("ldy", 140), ("ldx", 140), ("dy", by.data_ptr() + 8), ("x", bx.data_ptr() + 8)],
               null=["dy", "x", "dw"]))
    # ---- batch dot
    ba, bc, bo = _buf(2, 64), _buf(2, 64), _buf(1, 4)
    need = int(L.vggt_batch_dot_workspace_bytes(2, 40))
    total["vggt_batch_dot_f32"] = _rule_walk(
        L, "vggt_batch_dot_f32", [("a", ba.data_ptr()), ("c", bc.data_ptr()), ("bs", 64), ("B", 2), ("n", 40),
                                  ("out", bo.data_ptr())] + wsr, [bo],
        _rules(shape=[("B", 0), ("n", 0)] + short(need), null=["a", "c", "out"]))
    print("rule walk:", sum(total.values()), "calls;", total)


# ================================================================== 10. one reducer behind every column sum
@pytest.mark.parametrize("Nn", [4, 1028])
@pytest.mark.parametrize("M", [1, 17, 273])
def test_dbias_is_colsum_of_the_stored_output(N, M, Nn):
    """dbias of vggt_gelu_bwd / vggt_layerscale_bwd into a zeroed buffer is, bit for bit, vggt_colsum of
    the stored bf16 dpre / dbranch into a zeroed buffer: both add the same rounded values in the same
    chunk and slice order (one chunk, a ragged second chunk, the 18-chunk finalize; N = 1028: a second
    column block with one live thread).  The same with an fp32 output, where the stored value is the
    unrounded product: the compiler would be free to contract it into the sum, and does not (the
    property held on the library before the three entries shared their launcher, in both forms)."""
    g = _gen(12, M, Nn)
    errs = []
    dh, pre = torch.randn(M, Nn, generator=g).to(BF).cuda(), (torch.randn(M, Nn, generator=g) * 2).to(BF).cuda()
    dout, br = torch.randn(M, Nn, generator=g).cuda(), torch.randn(M, Nn, generator=g).to(BF).cuda()
    gamma = (0.5 + torch.rand(Nn, generator=g)).cuda()
    for nm, run in (("gelu_bwd", lambda o, s: N.gelu_bwd(dh, pre, o, s)),
                    ("layerscale_bwd", lambda o, s: N.layerscale_bwd(dout, br, gamma, o, None, s))):
        for odt in (BF, F32):
            stored = torch.empty(M, Nn, dtype=odt, device="cuda")
            dbias, cs = torch.zeros(Nn, device="cuda"), torch.zeros(Nn, device="cuda")
            run(stored, dbias)
            N.colsum(stored, cs, True)
            _eq_bits(errs, f"{nm} M={M} N={Nn} out {_dtn(odt)}: dbias vs colsum of the stored output", dbias.cpu(),
                     cs.cpu())
    _done(errs, ("shared reducer", M, Nn, _reach_colred(M, Nn)))


def test_zz_figures():
    """Prints what the tests above measured (Training kernel edge tests)."""
    for k in sorted(FIG, key=str):
        print("figure", k, FIG[k])
