"""Which kernel the skinny fp32 linears and small-window attention launch, or the error they return
(vggt_linear_f32_form, vggt_attention_small_form): host arithmetic only, so it runs without a device.
`_reach_linear` and `_reach_attn` below restate the dispatch as it stood before small.hip had one
resolver per family -- vggt_linear_f32_ws's and vggt_linear_f32_grouped's argument checks,
linear_wk_dispatch / launch_linear_wk, the split-K arithmetic of vggt_linear_f32_ws, and the three
`if`s of vggt_attention_small -- read off that code rule by rule, not off the resolver (they lived in
test_gpu_small_edges.py, which now asks the library instead).  The library's answer (family, KW, MT,
splits, kchunk, one launch or two, grid, threads, dynamic LDS bytes, or the error code) must equal the
restatement's on both sides of every threshold, under every value of the three linear knobs, with no
scratch, a full scratch and one too small for the full split, for every (act_in, epi) and group count
the entries accept or refuse, and for attention on every shape the edge tests name, both dtypes, the
EXACT bit, and leading dimensions and pointers off the matrix-core form's alignment.  The two
environment switches are read when the library loads: a child interpreter per switch answers with it
at 0."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest

OK, S, U = 0, -1, -4
EPI_GELU, EPI_RESID, EPI_F32 = 1, 2, 3
F32, BF, EXACT = 0, 1, 0x100
TUNE_ONE_LAUNCH, TUNE_SPLIT_K, TUNE_WK = 6, 7, 8
WS_COUNTERS, MAX_SPLITS = 1024, 32
WK, BLOCK, SPLIT = "in-workgroup split", "block, no split", "cross-workgroup split"
FAMILY = (WK, BLOCK, SPLIT)
ATTN_FAMILY = ("mfma", "workgroup", "one-wave")


# ------------------------------------------------------------------ the dispatch, restated
def _cdiv(a, b):
    return -(-a // b)


def _reach_linear(M, Nn, K, wk=64, split_k=128, ws=True, one=1, act=0, epi=EPI_F32, groups=0, has_gamma=True):
    """vggt_linear_f32_ws (groups == 0) and vggt_linear_f32_grouped as they stood.  ws: True the scratch
    aligned_vggt._native.linear_f32 passes (the full split for M <= 256, none above), False none, an int
    that many bytes."""
    if groups:  # vggt_linear_f32_grouped: its own checks, then always the in-workgroup form
        if M <= 0 or M > 256 or Nn <= 0 or K <= 0 or groups <= 0 or groups > 65535:
            return {"rc": S}
        if act not in (0, 1) or epi not in (EPI_F32, EPI_GELU):
            return {"rc": U}
    else:
        if M <= 0 or Nn <= 0 or K <= 0:
            return {"rc": S}
        if epi == EPI_RESID and not has_gamma:
            return {"rc": S}
        if act not in (0, 1) or epi not in (EPI_F32, EPI_GELU, EPI_RESID):
            return {"rc": U}
    gy = _cdiv(M, 64)
    if groups or (M <= 256 and wk > 0):
        per_wave = wk if wk > 0 else 64
        kw = 2
        while kw < 8 and K > kw * per_wave:
            kw *= 2
        kchunk = -(-(-(-K // kw)) // 64) * 64
        ranges = [(min(K, w * kchunk), min(K, min(K, w * kchunk) + kchunk)) for w in range(kw)]
        return {"rc": OK, "form": WK, "KW": kw, "MT": 1 if M <= 16 else 4, "slabs": gy,
                "kchunk": kchunk, "k_per_wave": [b - a for a, b in ranges], "splits": 1, "one_launch": 1,
                "grid": (_cdiv(Nn, 16), gy, groups or 1), "threads": 64 * kw}
    blocks = _cdiv(Nn, 64) * gy
    splits = 1
    while splits < MAX_SPLITS and blocks * splits * 2 <= 512 and K // (splits * 2) >= split_k:
        splits *= 2
    if ws is True:
        ws = 4 * (WS_COUNTERS + MAX_SPLITS * gy * 64 * Nn) if M <= 256 else 0
    while splits > 1 and int(ws) < 4 * WS_COUNTERS + splits * gy * 64 * Nn * 4:
        splits //= 2
    if splits == 1:
        return {"rc": OK, "form": BLOCK, "blocks": blocks, "KW": 0, "MT": 4, "splits": 1, "kchunk": K, "one_launch": 1,
                "grid": (_cdiv(Nn, 64), gy, 1), "threads": 256}
    kchunk = -(-(-(-K // splits)) // 16) * 16
    return {"rc": OK, "form": SPLIT, "splits": splits, "kchunk": kchunk, "KW": 0, "MT": 4,
            "one_launch": int(blocks <= WS_COUNTERS and bool(one)),
            "splits_past_K": [z for z in range(splits) if z * kchunk > K],
            "waves_without_a_column": max(0, 4 - -(-(Nn - (-(-Nn // 64) - 1) * 64) // 16)),
            "grid": (_cdiv(Nn, 64), gy, splits), "threads": 256}


def _attn_lds_wg(nq, nk, D):
    return ((nq + nk) * (D + 1) + nk * D + nq * nk) * 4


def _attn_lds_wave(nk, D):
    return (2 * nk * (D + 1) + D) * 4


def _reach_attn(dt, nq, nk, D, use_mfma=True, use_wg=True, exact=False, lds=(0, 0, 0, 0), ptr_align=16, batch=1,
                heads=1):
    """vggt_attention_small as it stood: the form's name, or "SHAPE" / "UNSUPPORTED".  The matrix-core form
    reads 8 bytes at a time: it asked for (ldq | ldk | ldv | ldo) % 4 == 0 and the four pointers 8-byte
    aligned.  lds: the four leading dimensions (0: dense, heads * D)."""
    if batch <= 0 or heads <= 0 or nq <= 0 or nk <= 0 or nk > 128 or D <= 0 or D > 256:
        return "SHAPE"
    if _attn_lds_wave(nk, D) > 160 * 1024:
        return "SHAPE"
    ldq, ldk, ldv, ldo = (ld or heads * D for ld in lds)
    if use_mfma and not exact and dt == BF and nq <= 16 and nk <= 16 and D % 16 == 0 and D <= 256 and \
            (ldq | ldk | ldv | ldo) % 4 == 0 and ptr_align % 8 == 0:
        return "mfma"
    if dt not in (F32, BF):
        return "UNSUPPORTED"
    if use_wg and _attn_lds_wg(nq, nk, D) <= 64 * 1024:
        return "workgroup"
    return "one-wave"


def _attn_launch(form, nq, nk, D, batch, heads):
    """(dt, grid, threads, dynamic LDS bytes) of a form's launch line as it stood."""
    pairs = batch * heads
    if form == "mfma":
        return (D if D in (64, 128) else 0, _cdiv(pairs, 4), 256, 4 * 16 * D * 2)
    if form == "workgroup":
        return (0, pairs, 256, _attn_lds_wg(nq, nk, D))
    return (0, pairs, 64, _attn_lds_wave(nk, D))


def test_reach_restated():
    r = _reach_linear(16, 17, 129)
    assert r["KW"] == 4 and r["k_per_wave"] == [64, 64, 1, 0] and r["MT"] == 1
    r = _reach_linear(256, 16, 520)
    assert r["KW"] == 8 and r["kchunk"] == 128 and r["k_per_wave"] == [128] * 4 + [8, 0, 0, 0] and r["slabs"] == 4
    assert [_reach_linear(1, 1, k)["KW"] for k in (1, 64, 65, 128, 129, 256, 260, 1000)] == [2, 2, 2, 2, 4, 4, 8, 8]
    r = _reach_linear(16, 17, 520, wk=0, split_k=32)
    assert r["splits"] == 16 and r["kchunk"] == 48 and r["splits_past_K"] == [11, 12, 13, 14, 15]
    assert r["waves_without_a_column"] == 2
    assert _reach_linear(257, 17, 260)["form"] == "block, no split" == _reach_linear(300, 65, 64, ws=False)["form"]
    assert _reach_linear(17, 17, 65, wk=0)["form"] == "block, no split"
    assert _attn_lds_wg(38, 38, 128) == 64448 and _attn_lds_wg(39, 39, 128) == 66300
    assert _reach_attn(F32, 38, 38, 128) == "workgroup" and _reach_attn(F32, 39, 39, 128) == "one-wave"
    assert _attn_lds_wave(79, 256) == 163448 and _reach_attn(F32, 2, 79, 256) == "one-wave"
    assert _reach_attn(F32, 2, 80, 256) == "SHAPE" == _reach_attn(BF, 1, 129, 16)
    assert _reach_attn(BF, 16, 16, 64) == "mfma" and _reach_attn(BF, 17, 16, 64) == "workgroup"
    assert _reach_attn(BF, 16, 17, 64) == "workgroup" == _reach_attn(BF, 4, 4, 24)
    assert [_reach_attn(F32, 3, nk, D) for nk, D in ((128, 68), (64, 200), (65, 200))] == ["one-wave"] * 3
    # the alignment rule of the matrix-core form
    assert _reach_attn(BF, 16, 16, 64, lds=(66, 0, 0, 0)) == "workgroup" == _reach_attn(BF, 16, 16, 64, ptr_align=4)
    assert _reach_attn(BF, 16, 16, 64, lds=(68, 72, 76, 80), ptr_align=8) == "mfma"


# ------------------------------------------------------------------ the library's answers
class LinForm(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("family", "kw", "mt", "splits", "kchunk", "one_launch", "gx", "gy", "gz",
                                            "threads", "rc")]


class AttnForm(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("family", "dt", "grid", "threads", "lds", "rc")]


def bind_linear(lib):
    fn = lib.vggt_linear_f32_form
    fn.argtypes = [ctypes.c_int] * 7 + [ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    form = LinForm()
    ref = ctypes.addressof(form)

    def ask(M, Nn, K, act, epi, groups, has_gamma, ws_bytes):
        rc = fn(M, Nn, K, act, epi, groups, has_gamma, ws_bytes, ref)
        assert rc == form.rc
        if rc != OK:
            return (rc,)
        return (rc, FAMILY[form.family], form.kw, form.mt, form.splits, form.kchunk, form.one_launch,
                (form.gx, form.gy, form.gz), form.threads)
    return ask


def _want_linear(r):
    if r["rc"] != OK:
        return (r["rc"],)
    return (OK, r["form"], r["KW"], r["MT"], r["splits"], r["kchunk"], r["one_launch"], r["grid"], r["threads"])


def bind_attn(lib):
    fn = lib.vggt_attention_small_form
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_int64] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    form = AttnForm()
    ref = ctypes.addressof(form)

    def ask(dtype, nq, nk, D, lds, ptr_align, batch, heads):
        ld = [x or heads * D for x in lds]
        rc = fn(dtype, nq, nk, D, *ld, ptr_align, batch, heads, ref)
        assert rc == form.rc
        if rc != OK:
            return {S: "SHAPE", U: "UNSUPPORTED"}[rc]
        return (ATTN_FAMILY[form.family], form.dt, form.grid, form.threads, form.lds)
    return ask


def _want_attn(dtype, nq, nk, D, lds, ptr_align, batch, heads, use_mfma, use_wg):
    form = _reach_attn(dtype & ~EXACT, nq, nk, D, use_mfma, use_wg, bool(dtype & EXACT), lds, ptr_align, batch, heads)
    if form in ("SHAPE", "UNSUPPORTED"):
        return form
    return (form,) + _attn_launch(form, nq, nk, D, batch, heads)


@pytest.fixture(scope="module")
def native():
    from aligned_vggt import _native
    _native.lib()
    return _native


class _Knobs:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.prev = [(k, self.lib.vggt_tune(k, v)) for k, v in ((TUNE_WK, 64), (TUNE_SPLIT_K, 128), (TUNE_ONE_LAUNCH, 1))]
        return self

    def set(self, wk, split_k, one):
        for k, v in ((TUNE_WK, wk), (TUNE_SPLIT_K, split_k), (TUNE_ONE_LAUNCH, one)):
            assert self.lib.vggt_tune(k, v) >= 0

    def __exit__(self, *a):
        for k, v in self.prev:
            self.lib.vggt_tune(k, v)


LIN_M = (1, 16, 17, 64, 65, 256, 257, 300)
LIN_K = (1, 64, 65, 128, 129, 256, 260, 520, 1000)
LIN_N = (1, 16, 17, 64, 65)
GROUPS = (0, 1, 3, 65535, 65536)


def _scratches(M, Nn):
    """None, the full split's, and one that holds the counters and two slabs (the split is halved down to it)."""
    slab = _cdiv(M, 64) * 64 * Nn * 4
    return (0, 4 * WS_COUNTERS + MAX_SPLITS * slab, 4 * WS_COUNTERS + 2 * slab, 4 * WS_COUNTERS + 2 * slab - 4)


def test_linear_resolver_matches_the_entry_points_as_they_stood(native):
    lib = native.lib()
    ask = bind_linear(lib)
    n, seen, wrong = 0, set(), []
    with _Knobs(lib) as knobs:
        for wk, split_k, one in itertools.product((0, 64, 128), (32, 128), (1, 0)):
            knobs.set(wk, split_k, one)
            for M, K, Nn in itertools.product(LIN_M, LIN_K, LIN_N):
                for groups in (0, 1, 3):
                    for ws in _scratches(M, Nn) if groups == 0 else (0,):
                        want = _want_linear(_reach_linear(M, Nn, K, wk, split_k, ws, one, groups=groups))
                        got = ask(M, Nn, K, 0, EPI_F32, groups, 1, ws)
                        if want != got:
                            wrong.append((wk, split_k, one, M, Nn, K, groups, ws, got, want))
                        seen.add(got[:4] + got[6:7])
                        n += 1
            # every (act_in, epi), with and without gamma, every group count: accepted or refused as before
            for (M, Nn, K), act, epi, gam, groups in itertools.product(((16, 17, 129), (257, 17, 260), (0, 17, 129)), (0, 1, 2, -1),
                                                                       (EPI_GELU, EPI_RESID, EPI_F32, 0, 4), (0, 1), GROUPS):
                want = _want_linear(_reach_linear(M, Nn, K, wk, split_k, True, one, act, epi, groups, bool(gam)))
                got = ask(M, Nn, K, act, epi, groups, gam, 4 * (WS_COUNTERS + MAX_SPLITS * _cdiv(max(M, 1), 64) * 64 * Nn) if M <= 256 else 0)
                if want != got:
                    wrong.append((wk, split_k, one, M, Nn, K, act, epi, gam, groups, got, want))
                seen.add(got[:1] if len(got) == 1 else got[:4] + got[6:7])
                n += 1
    assert not wrong, wrong[:5]
    assert n > 30000
    # every instantiation's (KW, MT), the block form, the split with one launch and with two, every error code
    forms = {s for s in seen if len(s) > 1}
    assert forms == {(OK, WK, kw, mt, 1) for kw in (2, 4, 8) for mt in (1, 4)} | {(OK, BLOCK, 0, 4, 1)} \
        | {(OK, SPLIT, 0, 4, o) for o in (0, 1)}
    assert {s[0] for s in seen if len(s) == 1} == {S, U}


def test_linear_spot_values(native):
    """Spot values of the sweep, so that a restatement and a resolver that were wrong together would still show."""
    lib = native.lib()
    ask = bind_linear(lib)
    full = lambda M, Nn: 4 * (WS_COUNTERS + MAX_SPLITS * _cdiv(M, 64) * 64 * Nn)
    with _Knobs(lib) as knobs:
        assert ask(16, 17, 129, 0, EPI_F32, 0, 1, 0) == (OK, WK, 4, 1, 1, 64, 1, (2, 1, 1), 256)
        assert ask(256, 16, 520, 1, EPI_RESID, 0, 1, 0) == (OK, WK, 8, 4, 1, 128, 1, (1, 4, 1), 512)
        assert ask(257, 17, 260, 0, EPI_F32, 0, 1, 0) == (OK, BLOCK, 0, 4, 1, 260, 1, (1, 5, 1), 256)
        assert ask(257, 17, 260, 0, EPI_F32, 0, 1, full(257, 17)) == (OK, SPLIT, 0, 4, 2, 144, 1, (1, 5, 2), 256)
        assert ask(17, 65, 1000, 0, EPI_GELU, 3, 0, 0) == (OK, WK, 8, 4, 1, 128, 1, (5, 1, 3), 512)
        knobs.set(0, 32, 1)
        assert ask(16, 17, 520, 0, EPI_F32, 0, 1, full(16, 17)) == (OK, SPLIT, 0, 4, 16, 48, 1, (1, 1, 16), 256)
        # a scratch of the counters and two slabs of 64 x 17 floats: two splits; four bytes less: none
        two = 4 * WS_COUNTERS + 2 * 64 * 17 * 4
        assert ask(16, 17, 520, 0, EPI_F32, 0, 1, two) == (OK, SPLIT, 0, 4, 2, 272, 1, (1, 1, 2), 256)
        assert ask(16, 17, 520, 0, EPI_F32, 0, 1, two - 4) == (OK, BLOCK, 0, 4, 1, 520, 1, (1, 1, 1), 256)
        assert ask(16, 17, 520, 0, EPI_F32, 3, 1, 0)[1:4] == (WK, 8, 1)  # the grouped entry ignores the knob at 0
        knobs.set(0, 32, 0)
        assert ask(16, 17, 520, 0, EPI_F32, 0, 1, full(16, 17))[6] == 0
        knobs.set(64, 128, 1)
        # the rules, SHAPE before UNSUPPORTED
        assert ask(16, 17, 129, 0, EPI_RESID, 0, 0, 0) == (S,) and ask(16, 17, 129, 2, EPI_RESID, 0, 0, 0) == (S,)
        assert ask(16, 17, 129, 2, EPI_F32, 0, 1, 0) == (U,) and ask(16, 17, 129, 0, 0, 0, 1, 0) == (U,)
        assert ask(16, 17, 129, 0, EPI_RESID, 1, 1, 0) == (U,) and ask(257, 17, 129, 0, EPI_RESID, 1, 1, 0) == (S,)
        assert ask(16, 17, 129, 0, EPI_F32, 65535, 0, 0)[7] == (2, 1, 65535) and ask(16, 17, 129, 0, EPI_F32, 65536, 0, 0) == (S,)
        assert ask(16, 17, 129, 0, EPI_F32, -1, 0, 0) == (S,)
    assert lib.vggt_linear_f32_form(16, 17, 129, 0, EPI_F32, 0, 1, 0, None) == OK


# every shape test_reach_restated and the edge tests' lists name, and the neighbours of each limit
ATTN_SHAPES = [(38, 38, 128), (39, 39, 128), (2, 79, 256), (2, 80, 256), (1, 129, 16), (16, 16, 64), (17, 16, 64),
               (16, 17, 64), (4, 4, 24), (3, 128, 68), (3, 64, 200), (3, 65, 200), (1, 1, 16), (3, 13, 48), (16, 5, 64),
               (5, 7, 6), (16, 16, 128), (3, 64, 68), (3, 65, 68), (16, 16, 256), (16, 16, 272), (1, 128, 256), (16, 5, 16),
               (0, 4, 16), (4, 0, 16), (4, 4, 0), (17, 7, 64)]
ATTN_LDS = [(0, 0, 0, 0), (66, 0, 0, 0), (0, 0, 0, 1030), (520, 528, 536, 544), (0, 514, 0, 0), (0, 0, 258, 0)]


def _attn_cases():
    for (nq, nk, D), dt, ex, lds, al, (batch, heads) in itertools.product(ATTN_SHAPES, (F32, BF), (0, EXACT), ATTN_LDS, (16, 8, 4, 2),
                                                                         ((1, 1), (2, 3), (5, 1), (7, 2))):
        yield (dt | ex, nq, nk, D, lds, al, batch, heads)
    for dtype in (2, 7, 2 | EXACT, 0x200, -1):  # an unknown dtype: after the shape rules
        for nq, nk, D in ((16, 16, 64), (2, 80, 256), (39, 39, 128)):
            yield (dtype, nq, nk, D, (0, 0, 0, 0), 16, 2, 3)
    for batch, heads in ((0, 1), (1, 0), (-1, 2)):
        yield (BF, 16, 16, 64, (0, 0, 0, 0), 16, batch, heads)


def _attn_sweep(ask, use_mfma, use_wg):
    n, seen, wrong = 0, set(), []
    for c in _attn_cases():
        want, got = _want_attn(*c, use_mfma, use_wg), ask(*c)
        if want != got:
            wrong.append((c, got, want))
        seen.add(got if isinstance(got, str) else got[:2])
        n += 1
    return n, sorted(seen, key=str), wrong


def _switches():
    return os.environ.get("VGGT_ATTN_SMALL_MFMA", "1") != "0", os.environ.get("VGGT_ATTN_SMALL_WG", "1") != "0"


def test_attention_resolver_matches_the_entry_point_as_it_stood(native):
    use_mfma, use_wg = _switches()
    n, seen, wrong = _attn_sweep(bind_attn(native.lib()), use_mfma, use_wg)
    assert not wrong, wrong[:5]
    assert n > 10000
    if use_mfma and use_wg:
        assert set(seen) == {"SHAPE", "UNSUPPORTED", ("mfma", 0), ("mfma", 64), ("mfma", 128), ("workgroup", 0), ("one-wave", 0)}


def test_attention_spot_values(native):
    ask = bind_attn(native.lib())
    use_mfma, use_wg = _switches()
    if use_mfma:
        assert ask(BF, 16, 16, 64, (0, 0, 0, 0), 16, 2, 3) == ("mfma", 64, 2, 256, 8192)
        assert ask(BF, 16, 5, 128, (0, 0, 0, 0), 8, 7, 2) == ("mfma", 128, 4, 256, 16384)
        assert ask(BF, 3, 13, 48, (0, 0, 0, 0), 256, 1, 1) == ("mfma", 0, 1, 256, 6144)
    if use_wg:
        assert ask(BF | EXACT, 16, 16, 64, (0, 0, 0, 0), 16, 2, 3) == ("workgroup", 0, 6, 256, (32 * 65 + 16 * 64 + 256) * 4)
        assert ask(BF, 16, 16, 64, (0, 0, 0, 0), 4, 2, 3)[0] == "workgroup" == ask(BF, 16, 16, 64, (0, 194, 0, 0), 16, 2, 3)[0]
        assert ask(F32, 38, 38, 128, (0, 0, 0, 0), 16, 2, 3) == ("workgroup", 0, 6, 256, 64448)
    assert ask(F32, 39, 39, 128, (0, 0, 0, 0), 16, 2, 3) == ("one-wave", 0, 6, 64, (2 * 39 * 129 + 128) * 4)
    assert ask(F32, 2, 79, 256, (0, 0, 0, 0), 16, 2, 1) == ("one-wave", 0, 2, 64, 163448)
    assert ask(F32, 2, 80, 256, (0, 0, 0, 0), 16, 2, 1) == "SHAPE" == ask(BF, 1, 129, 16, (0, 0, 0, 0), 16, 1, 1)
    assert ask(5, 2, 80, 256, (0, 0, 0, 0), 16, 2, 1) == "SHAPE" and ask(5, 2, 79, 256, (0, 0, 0, 0), 16, 2, 1) == "UNSUPPORTED"
    assert native.lib().vggt_attention_small_form(BF, 16, 16, 64, 64, 64, 64, 64, 16, 1, 1, None) == OK


_CHILD = """
import json
from aligned_vggt import _native
import test_small_form as T
n, seen, wrong = T._attn_sweep(T.bind_attn(_native.lib()), *T._switches())
print(json.dumps({"n": n, "seen": [s if isinstance(s, str) else s[0] for s in seen], "wrong": wrong[:5]}))
"""


@pytest.mark.parametrize("var", ["VGGT_ATTN_SMALL_WG", "VGGT_ATTN_SMALL_MFMA"])
def test_attention_switches_are_read_when_the_library_loads(native, var):
    """A fresh interpreter with one switch at 0: without the workgroup form nothing lands on it, without the
    matrix-core form nothing lands there; setting the variable in this process afterwards changes nothing."""
    ask = bind_attn(native.lib())
    before = ask(BF, 16, 16, 64, (0, 0, 0, 0), 16, 2, 3), ask(F32, 4, 4, 24, (0, 0, 0, 0), 16, 2, 3)
    saved = os.environ.get(var)
    os.environ[var] = "0" if saved != "0" else "1"
    try:
        assert before == (ask(BF, 16, 16, 64, (0, 0, 0, 0), 16, 2, 3), ask(F32, 4, 4, 24, (0, 0, 0, 0), 16, 2, 3))
    finally:
        if saved is None:
            del os.environ[var]
        else:
            os.environ[var] = saved
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    env.update({"VGGT_ATTN_SMALL_WG": "1", "VGGT_ATTN_SMALL_MFMA": "1", var: "0"})
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert not got["wrong"], got["wrong"]
    assert got["n"] > 10000
    gone = "workgroup" if var == "VGGT_ATTN_SMALL_WG" else "mfma"
    assert set(got["seen"]) == {"SHAPE", "UNSUPPORTED", "mfma", "workgroup", "one-wave"} - {gone}


def test_wrapper_names(native):
    f = native.linear_f32_form(16, 17, 129)
    assert f["rc"] == 0 and f["name"] == WK and (f["kw"], f["mt"], f["kchunk"], f["grid"], f["threads"]) == (4, 1, 64, (2, 1, 1), 256)
    assert native.linear_f32_form(300, 65, 64)["name"] == BLOCK
    assert native.linear_f32_form(17, 65, 260, groups=3)["grid"] == (5, 1, 3)
    assert native.linear_f32_form(17, 65, 260, epi=EPI_RESID, has_gamma=False) == dict(
        native.linear_f32_form(0, 1, 1), name=None)
    prev = native.tune(native.TUNE_LINEAR_WK, 0), native.tune(native.TUNE_LINEAR_SPLIT_K, 32)
    try:
        f = native.linear_f32_form(16, 17, 520)  # the scratch linear_f32 itself passes
        assert f["name"] == SPLIT and (f["splits"], f["kchunk"], f["one_launch"]) == (16, 48, 1)
        assert native.linear_f32_form(16, 17, 520, ws_bytes=0)["name"] == BLOCK
    finally:
        native.tune(native.TUNE_LINEAR_WK, prev[0])
        native.tune(native.TUNE_LINEAR_SPLIT_K, prev[1])
    if _switches() == (True, True):
        f = native.attention_small_form(native.DTYPE_BF16, 16, 16, 64, batch=2, heads=3)
        assert f["name"] == "mfma" and (f["dt"], f["grid"], f["threads"], f["lds"]) == (64, 2, 256, 8192)
        assert native.attention_small_form(native.DTYPE_BF16, 16, 16, 64, exact=True)["name"] == "workgroup"
        assert native.attention_small_form(native.DTYPE_BF16, 16, 16, 64, ptr_align=4)["name"] == "workgroup"
    f = native.attention_small_form(native.DTYPE_F32, 2, 79, 256)
    assert f["name"] == "one-wave" and f["lds"] == 163448
    f = native.attention_small_form(native.DTYPE_F32, 2, 80, 256)
    assert f["rc"] == S and f["name"] is None
