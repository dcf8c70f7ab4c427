"""Which kernel the four DPT convolution entry points launch, or the error they return
(vggt_conv_form): host arithmetic only, so it runs without a device.  `ladder_f32`, `ladder_split`,
`ladder_pre` and `ladder_fused` below restate the dispatch as it stood before the library had one
resolver -- vggt_conv2d_f32's own argument check, conv_args with the two `if` ladders of
vggt_conv2d_bf16x3 and vggt_conv2d_bf16x3_pre, and vggt_conv2d_upsample_bf16x3's checks -- read off
that code rule by rule, not off the resolver.  The library's answer (family, tile width, gather depth,
grid, LDS bytes, descriptor bytes, weight rows, or the error code) must equal the ladder's for every
entry, GEMM widths on either side of every tile threshold (with pixel shuffles on top), M on either
side of one and two 128-row tiles, kernel / stride / padding combinations, both values of
VGGT_TUNE_CONV_PF2, maps on either side of the two byte limits and of the 2^31 - 1 grid guard, every
rejection of tests/test_gpu_conv_edges.py::test_conv_rejections, and pairs of simultaneous faults.

The LDS figures are restated from the kernels' tile arithmetic (and are the code objects' values):
conv_f32_kernel 2 x (128 + 64) rows x 32 floats = 49152; the split forms 2 stages x 2 halves x
(128 + bn) rows x 64 B = 40960 / 49152 / 65536 for bn = 32 / 64 / 128; conv_up_kernel 2 patch halves of
6 x 34 pixels x 64 B + 2 x 9 weight tiles of 32 rows x 64 B = 62976."""
import ctypes
import itertools

import pytest

OK, S, A, U = 0, -1, -2, -4
E_F32, E_SPLIT, E_PRE, E_UP = range(4)
F_F32, F_SPLIT, F_PRE, F_UP = range(4)
Y, YH, YL, R1, R2, POS = 1, 2, 4, 8, 16, 32
TUNE_CONV_PF2 = 4
LDS_F32, LDS_SPLIT, LDS_UP = 49152, {32: 40960, 64: 49152, 128: 65536}, 62976
IMAX = 0x7fffffff


def _cdiv(a, b):
    """C integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _case(**kw):
    c = dict(nimg=1, hi=3, wi=3, ci=32, co=8, kh=1, kw=1, stride=1, pad=0, shuffle=0, ho=0, wo=0, ldx=None, ldy=None,
             ldys=None, has=Y)
    c.update(kw)
    for k, d in (("ldx", c["ci"]), ("ldy", c["co"]), ("ldys", c["co"])):
        if c[k] is None:
            c[k] = d
    return c


# ------------------------------------------------------------------ the entry points, restated
def _conv_args(c, ldx_mod=4):
    """The head the three implicit-GEMM entries shared (vggt_conv2d_f32 carried its own copy): the
    error code, or (ho, wo, ncols, nwg) with nwg counted on 64-wide tiles."""
    if min(c["nimg"], c["hi"], c["wi"], c["ci"], c["co"], c["kh"], c["kw"], c["stride"]) <= 0 or c["pad"] < 0:
        return S
    if c["ci"] % 32:
        return S
    if (c["ldx"] < c["ci"] and c["nimg"] * c["hi"] * c["wi"] > 1) or (c["has"] & Y and c["ldy"] < c["co"]):
        return S
    if c["shuffle"] and (c["kh"] != 1 or c["kw"] != 1 or c["stride"] != 1 or c["pad"] != 0 or c["has"] & (R1 | R2 | POS)):
        return U
    if c["ldx"] % ldx_mod:
        return A
    ho = _cdiv(c["hi"] + 2 * c["pad"] - c["kh"], c["stride"]) + 1
    wo = _cdiv(c["wi"] + 2 * c["pad"] - c["kw"], c["stride"]) + 1
    ncols = c["shuffle"] * c["shuffle"] * c["co"] if c["shuffle"] else c["co"]
    nwg = _cdiv(c["nimg"] * ho * wo + 127, 128) * _cdiv(ncols + 63, 64)
    if nwg > IMAX:
        return S
    return ho, wo, ncols, nwg


def _width(ncols, nwg):
    """The `if` ladder both split entries carried: (tile width, grid); the 128-wide grid derived from the 64-wide one."""
    if ncols >= 128:
        return 128, _cdiv(nwg, _cdiv(ncols + 63, 64)) * _cdiv(ncols + 127, 128)
    if ncols > 32:
        return 64, nwg
    return 32, nwg


def ladder_f32(c, pf2):
    r = _conv_args(c)
    if isinstance(r, int):
        return (r,)
    ho, wo, ncols, nwg = r
    return (OK, F_F32, 64, 0, nwg, LDS_F32, 0, _cdiv(ncols + 63, 64) * 64)


def ladder_split(c, pf2):
    r = _conv_args(c)
    if isinstance(r, int):
        return (r,)
    ho, wo, ncols, nwg = r
    xb = (c["nimg"] * c["hi"] * c["wi"] - 1) * c["ldx"] * 4 + c["ci"] * 4
    two = xb < 0xffffff00 and bool(pf2)
    bn, grid = _width(ncols, nwg)
    return (OK, F_SPLIT, bn, int(two), grid, LDS_SPLIT[bn], xb if two else 0, _cdiv(ncols + bn - 1, bn) * bn)


def ladder_pre(c, pf2):
    r = _conv_args(c)
    if isinstance(r, int):
        return (r,)
    ho, wo, ncols, nwg = r
    if not c["has"] & Y and not c["has"] & YH:
        return (S,)
    if bool(c["has"] & YH) != bool(c["has"] & YL) or (c["has"] & YH and c["ldys"] < c["co"]):
        return (S,)
    if c["ldx"] % 8:
        return (A,)
    xb = (c["nimg"] * c["hi"] * c["wi"] - 1) * c["ldx"] * 2 + c["ci"] * 2
    if xb >= 0x7fffff00:
        return (S,)
    bn, grid = _width(ncols, nwg)
    return (OK, F_PRE, bn, 0, grid, LDS_SPLIT[bn], xb, _cdiv(ncols + bn - 1, bn) * bn)


def ladder_fused(c, pf2):
    C = c["ci"]
    if min(c["nimg"], c["hi"], c["wi"], c["ho"], c["wo"], C, c["co"]) <= 0 or C % 32 or c["co"] > 32:
        return (S,)
    if not c["has"] & Y and not c["has"] & YH:
        return (S,)
    if bool(c["has"] & YH) != bool(c["has"] & YL) or (c["has"] & Y and c["ldy"] < c["co"]) or \
            (c["has"] & YH and c["ldys"] < c["co"]):
        return (S,)
    if 31 * 9 * C + 9 * C > 0x3fffffff:
        return (S,)
    nwg = c["nimg"] * _cdiv(c["ho"] + 3, 4) * _cdiv(c["wo"] + 31, 32)
    if nwg > IMAX:
        return (S,)
    return (OK, F_UP, 32, 0, nwg, LDS_UP, 0, 32)


LADDER = {E_F32: ladder_f32, E_SPLIT: ladder_split, E_PRE: ladder_pre, E_UP: ladder_fused}


# ------------------------------------------------------------------ the cases
NCOLS = (1, 31, 32, 33, 64, 65, 127, 128, 129)
# (nimg, hi, wi): M on either side of one and two 128-row tiles for a 1x1 stride-1 kernel, and maps a 3x3 kernel fits
MAPS = ((1, 1, 1), (1, 1, 127), (1, 8, 16), (1, 3, 43), (1, 1, 255), (2, 8, 16), (1, 1, 257), (2, 5, 7), (3, 11, 12))
KERNELS = ((1, 1), (3, 3), (1, 3))
# 2^37 pixels exactly (2^30 row tiles) and 128 x (2^30 - 1) pixels (2^30 - 1 = 3^2 7 11 31 151 331)
BIG_ABOVE, BIG_BELOW = (1 << 19, 512, 512), (128 * 331, 9 * 7 * 11 * 31, 151)


def geometry_cases():
    for (nimg, hi, wi), co, (kh, kw), stride, pad in itertools.product(MAPS, NCOLS, KERNELS, (1, 2, 3), (0, 1, 2)):
        yield _case(nimg=nimg, hi=hi, wi=wi, co=co, kh=kh, kw=kw, stride=stride, pad=pad)
    for (nimg, hi, wi), co, s in itertools.product(MAPS, NCOLS, (2, 3, 4)):  # shuffles on top: ncols = s s co
        yield _case(nimg=nimg, hi=hi, wi=wi, co=co, shuffle=s)
    for ci in (64, 96):
        for co in NCOLS:
            yield _case(nimg=2, hi=5, wi=7, ci=ci, co=co, kh=3, kw=3, pad=1, ldx=ci + 8, ldy=co + 3, ldys=co + 5,
                        has=Y | YH | YL | R1 | POS)


def limit_cases():
    # the f32 map's last byte on either side of 0xffffff00 (split), the bf16 map's of 0x7fffff00 (pre): by ldx, by image count
    for ldx in (1073741720, 1073741724, 1073741728, 1073741732, 1073741656, 1073741664, 536870816, 536870824, 536870832):
        yield _case(nimg=1, hi=1, wi=2, ldx=ldx)
    for nimg in (16383, 16384, 32767, 32768, 65535, 65536):
        yield _case(nimg=nimg, hi=32, wi=32, co=40)
    # the 2^31 - 1 grid guard, judged on 64-wide tiles: co = 64 (one tile column), 128 and 129 (where the 128-wide count is half)
    for co in (64, 65, 128, 129, 256):
        for nimg, hi, wi in (BIG_ABOVE, BIG_BELOW, (1 << 20, 512, 512), (1 << 18, 512, 512)):
            yield _case(nimg=nimg, hi=hi, wi=wi, co=co)


# a fault each, keyed by the check it trips; FAULTS[name] = (entries it applies to, overrides)
FAULTS = {
    "dims": ((E_F32, E_SPLIT, E_PRE), dict(stride=0)),
    "pad": ((E_F32, E_SPLIT, E_PRE), dict(pad=-1)),
    "ci % 32": ((E_F32, E_SPLIT, E_PRE), dict(ci=48, ldx=48)),
    "ldx < ci": ((E_F32, E_SPLIT, E_PRE), dict(ldx=24)),
    "ldy < co": ((E_F32, E_SPLIT, E_PRE), dict(ldy=7)),
    "shuffle kh != 1": ((E_F32, E_SPLIT, E_PRE), dict(shuffle=2, kh=3, kw=3)),
    "shuffle + res1": ((E_F32, E_SPLIT, E_PRE), dict(shuffle=2, has_or=R1)),
    "shuffle + pos": ((E_F32, E_SPLIT, E_PRE), dict(shuffle=2, has_or=POS)),
    "ldx % 4": ((E_F32, E_SPLIT, E_PRE), dict(ldx=34)),
    "ldx % 8": ((E_PRE,), dict(ldx=36)),
    "grid": ((E_F32, E_SPLIT, E_PRE), dict(nimg=1 << 20, hi=512, wi=512)),
    "no output": ((E_PRE,), dict(has_clear=Y | YH | YL)),
    "y_hi without y_lo": ((E_PRE,), dict(has_clear=YL)),
    "y_lo without y_hi": ((E_PRE,), dict(has_clear=YH)),
    "ldys < co": ((E_PRE,), dict(ldys=7)),
    "pre map": ((E_PRE,), dict(nimg=32768, hi=32, wi=32)),
}
# what two faults at once return, where the order of the checks decides it
PRECEDENCE = [("dims", "shuffle kh != 1", S), ("ci % 32", "shuffle + res1", S), ("ldx < ci", "shuffle + pos", S),
              ("ldy < co", "shuffle + res1", S), ("shuffle kh != 1", "ldx % 4", U), ("shuffle + pos", "grid", U),
              ("ldx % 4", "grid", A), ("ldx % 4", "no output", A), ("no output", "ldx % 8", S), ("ldys < co", "ldx % 8", S),
              ("ldx % 8", "pre map", A), ("grid", "ldx % 8", S), ("y_hi without y_lo", "pre map", S)]


def _with_faults(entry, names):
    c = _case(has=Y | YH | YL if entry == E_PRE else Y)
    for n in names:
        for k, v in FAULTS[n][1].items():
            if k == "has_or":
                c["has"] |= v
            elif k == "has_clear":
                c["has"] &= ~v
            else:
                c[k] = v
    return c


def fault_cases():
    """(entry, case) for every single fault and every pair of faults an entry knows."""
    for entry in (E_F32, E_SPLIT, E_PRE):
        mine = [n for n, (es, _) in FAULTS.items() if entry in es]
        yield entry, _with_faults(entry, ())
        for n in mine:
            yield entry, _with_faults(entry, (n,))
        for a, b in itertools.permutations(mine, 2):
            yield entry, _with_faults(entry, (a, b))


def fused_cases():
    for C, co, (ho, wo), nimg in itertools.product((32, 64, 96, 48, 0), (1, 31, 32, 33, 0), ((5, 7), (4, 32), (5, 33), (1, 1), (0, 3)),
                                                   (1, 2, 0)):
        for has, ldy, ldys in ((Y, co, co), (Y | YH | YL, co + 3, co + 5), (YH | YL, 0, co), (0, co, co), (Y | YH, co, co),
                               (Y | YL, co, co), (Y, co - 1, co), (YH | YL, co, co - 1)):
            yield _case(nimg=nimg, hi=2, wi=3, ci=C, co=co, ho=ho, wo=wo, ldy=ldy, ldys=ldys, has=has)
    for C in (3728256, 3728288):  # 32-bit weight DMA offsets: 288 C on either side of 2^30
        yield _case(ci=C, co=32, ho=5, wo=7)
    for nimg in (2047, 2048):  # the grid guard: nimg x 2^10 x 2^10 tiles
        yield _case(nimg=nimg, ci=32, co=32, ho=1 << 12, wo=1 << 15)


class Form(ctypes.Structure):
    _fields_ = [("family", ctypes.c_int), ("bn", ctypes.c_int), ("pf2", ctypes.c_int), ("grid", ctypes.c_int),
                ("lds", ctypes.c_int), ("xbytes", ctypes.c_uint), ("w_rows", ctypes.c_int), ("rc", ctypes.c_int)]


def bind(lib):
    fn = lib.vggt_conv_form
    fn.argtypes = [ctypes.c_int] * 13 + [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    form = Form()
    ref = ctypes.addressof(form)

    def ask(entry, c):
        rc = fn(entry, c["nimg"], c["hi"], c["wi"], c["ci"], c["co"], c["kh"], c["kw"], c["stride"], c["pad"], c["shuffle"],
                c["ho"], c["wo"], c["ldx"], c["ldy"], c["ldys"], c["has"], ref)
        assert rc == form.rc
        if rc != OK:
            return (rc,)
        return (rc, form.family, form.bn, form.pf2, form.grid, form.lds, form.xbytes, form.w_rows)
    return ask


@pytest.fixture(scope="module")
def native():
    from aligned_vggt import _native
    _native.lib()
    return _native


def test_resolver_matches_the_entry_points_as_they_stood(native):
    lib = native.lib()
    ask = bind(lib)
    before = lib.vggt_tune(TUNE_CONV_PF2, 1)
    n, seen, wrong = 0, set(), []
    try:
        for pf2 in (1, 0):
            lib.vggt_tune(TUNE_CONV_PF2, pf2)
            cases = [(e, c) for c in itertools.chain(geometry_cases(), limit_cases()) for e in (E_F32, E_SPLIT, E_PRE)]
            cases += list(fault_cases()) + [(E_UP, c) for c in fused_cases()]
            for entry, c in cases:
                want, got = LADDER[entry](c, pf2), ask(entry, c)
                if want != got:
                    wrong.append((pf2, entry, c, got, want))
                seen.add(got[:4])
                n += 1
    finally:
        lib.vggt_tune(TUNE_CONV_PF2, before)
    assert not wrong, wrong[:5]
    assert n > 20000
    # every kernel of the list, every error code
    assert {s for s in seen if len(s) > 1} == {(OK, F_F32, 64, 0), (OK, F_UP, 32, 0)} | {(OK, F_PRE, bn, 0) for bn in (32, 64, 128)} \
        | {(OK, F_SPLIT, bn, p) for bn in (32, 64, 128) for p in (0, 1)}
    assert {s[0] for s in seen if len(s) == 1} == {S, A, U}


def test_limits_and_guards_land_where_the_header_says(native):
    """Spot values of the cases above, so that a ladder and a resolver that were wrong together would still show."""
    ask = bind(native.lib())
    prev = native.tune(native.TUNE_CONV_PF2, 1)
    try:
        # two pixels of 32 channels: the f32 map ends at 4 ldx + 128 bytes, the bf16 one at 2 ldx + 64
        below, at = _case(nimg=1, hi=1, wi=2, ldx=1073741724), _case(nimg=1, hi=1, wi=2, ldx=1073741728)
        assert ask(E_SPLIT, below)[3] == 1 and ask(E_SPLIT, below)[6] == 0xffffff00 - 16
        assert ask(E_SPLIT, at)[3] == 0 and ask(E_SPLIT, at)[6] == 0        # 0xffffff00: one-deep
        native.tune(native.TUNE_CONV_PF2, 0)
        assert ask(E_SPLIT, below)[3] == 0 and ask(E_SPLIT, below)[6] == 0  # the knob off: one-deep
        assert ask(E_PRE, _case(nimg=1, hi=1, wi=2, ldx=1073741656))[6] == 0x7fffff00 - 16
        assert ask(E_PRE, _case(nimg=1, hi=1, wi=2, ldx=1073741664)) == (S,)
        # 2^30 row tiles x 2 tile columns of 64 is over the guard although 128-wide tiles would fit
        assert ask(E_SPLIT, _case(nimg=1 << 19, hi=512, wi=512, co=128)) == (S,)
        assert ask(E_SPLIT, _case(nimg=128 * 331, hi=9 * 7 * 11 * 31, wi=151, co=128))[2:5] == (128, 0, (1 << 30) - 1)
        assert ask(E_F32, _case(nimg=128 * 331, hi=9 * 7 * 11 * 31, wi=151, co=128))[4] == (1 << 31) - 2
        # weight rows: the N tile's multiple, not 64's
        assert [ask(E_PRE, _case(co=co))[7] for co in (8, 32, 33, 127, 128, 129)] == [32, 32, 64, 128, 128, 256]
        assert [ask(E_F32, _case(co=co))[7] for co in (8, 64, 65, 129)] == [64, 64, 128, 192]
    finally:
        native.tune(native.TUNE_CONV_PF2, prev)


def test_rejections_and_precedence(native):
    """Every rejection of test_gpu_conv_edges.py::test_conv_rejections with the same integers, and what pairs
    of simultaneous faults return."""
    ask = bind(native.lib())
    for entry, api in ((E_F32, "f32"), (E_SPLIT, "bf16x3"), (E_PRE, "pre")):
        full = Y | YH | YL if entry == E_PRE else Y
        cases = [(dict(ci=48, ldx=48), S), (dict(shuffle=2, kh=3, kw=3), U), (dict(shuffle=2, has=full | R1), U),
                 (dict(shuffle=2, has=full | POS), U), (dict(ldy=7), S), (dict(ldx=24), S),
                 (dict(ldx=36), A) if entry == E_PRE else (dict(ldx=34), A)]
        if entry == E_PRE:
            cases += [(dict(has=0), S), (dict(has=Y | YH), S), (dict(has=Y | YL), S), (dict(ldys=7), S)]
        for kw, code in cases:
            assert ask(entry, _case(**dict(dict(has=full), **kw))) == (code,), (api, kw)
        assert ask(entry, _case(has=full))[0] == OK
        assert ask(entry, _case(hi=1, wi=1, ldx=24, has=full))[0] == OK  # one pixel: its stride is never used
        for a, b, code in PRECEDENCE:
            if entry in FAULTS[a][0] and entry in FAULTS[b][0]:
                for pair in ((a, b), (b, a)):
                    assert ask(entry, _with_faults(entry, pair)) == (code,), (api, pair)


def test_wrapper_names(native):
    f = native.conv_form(native.CONV_ENTRY_PRE, 2, 5, 7, 32, 40, 3, 3, 1, 1)
    assert f["rc"] == 0 and f["name"] == "conv_pre_kernel<64>" and f["w_rows"] == 64 and f["lds"] == LDS_SPLIT[64]
    assert native.conv_form(native.CONV_ENTRY_F32, 2, 5, 7, 32, 40)["name"] == "conv_f32_kernel"
    prev = native.tune(native.TUNE_CONV_PF2, 1)
    try:
        assert native.conv_form(native.CONV_ENTRY_BF16X3, 2, 5, 7, 32, 130)["name"] == "conv_bf16x3_kernel<128, true>"
        native.tune(native.TUNE_CONV_PF2, 0)
        assert native.conv_form(native.CONV_ENTRY_BF16X3, 2, 5, 7, 32, 8, shuffle=2)["name"] == "conv_bf16x3_kernel<32, false>"
    finally:
        native.tune(native.TUNE_CONV_PF2, prev)
    f = native.conv_form(native.CONV_ENTRY_UPSAMPLE, 2, 3, 5, 32, 17, ho=5, wo=33)
    assert f["name"] == "conv_up_kernel<32>" and f["grid"] == 2 * 2 * 2 and f["lds"] == LDS_UP and f["w_rows"] == 32
    assert native.conv_form(native.CONV_ENTRY_PRE, 2, 5, 7, 48, 40)["rc"] == S
    assert native.conv_form(native.CONV_ENTRY_PRE, 2, 5, 7, 48, 40)["name"] is None
    assert native.lib().vggt_conv_form(7, 1, 1, 1, 32, 8, 1, 1, 1, 0, 0, 0, 0, 32, 8, 8, 1, None) == U
