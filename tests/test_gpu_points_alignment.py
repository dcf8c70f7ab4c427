"""vggt_gt_points_align (csrc/gt_points.hip): GT alignment sim3_from_points on the device.

Threshold and selection are exact: the state record's thr must have the bits of np.percentile on the
same float32 confidences, and n must be numpy's selection count.  The solve accumulates in fp64 and
rounds once, so it is held to the model rule of edge_rules: the kernel's worst row is at most 2 x that of
the fp32 host function (the reference's numpy code), both against the fp64 restatement in
points_alignment_rules.  Seeds are chosen from the host alone so that the host function's own error is
at least 3 fp32 roundings where 40 seeds hold one (_inexact_host): a model that happens to be exact
would decide the rule.

Sizes come from the header: one workgroup takes G = VGGT_GT_POINTS_GROUP pixels and there is no grid
cap, so no workgroup makes a second trip; G - 1, G, G + 1 and 70,003 (18 workgroups, a partial last one)
are the sizes at which the code can go wrong."""
import math

import numpy as np
import pytest
import torch

from edge_rules import ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED, F32, F64, U, _done, _eq_bits, _model_rule, _row_err
from points_alignment_rules import CASES, GOLDEN, load_case, percentile32, select, solve_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLS = {"reference": 0, "points": 1}


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _bits32(v):
    return int(np.float32(v).view(np.uint32))


def _cloud(shape, seed, mirror=False):
    """pred, gt (shape + (3,)) fp32: gt = 1.4 R0 (M) pred + t0 + noise."""
    g = np.random.default_rng(seed)
    pred = (g.standard_normal(shape + (3,)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)
    c, s = math.cos(0.7), math.sin(0.7)
    R0 = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    x = pred.astype(np.float64) * (np.array([1.0, 1.0, -1.0]) if mirror else 1.0)
    gt = (1.4 * x @ R0.T + np.array([0.5, -1.0, 2.0]) + 0.05 * g.standard_normal(shape + (3,))).astype(np.float32)
    return pred, gt


def _conf(shape, seed):
    g = np.random.default_rng(seed)
    return np.exp2(g.uniform(-6, 4, shape)).astype(np.float32)


def _run(N, pred, conf, gt, mask, q, columns="reference"):
    """Host arrays (B, P...) -> (T, scale) on the host and the decoded state."""
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pred, conf, gt, mask)]
    T, sc, st = N.gt_points_align(*t, q, COLS[columns])
    return T.cpu(), sc.cpu(), N.gt_points_state(st)


def _check_state(errs, tag, st, conf, mask, q):
    for b, s in enumerate(st):
        keep, thr = select(conf[b], mask[b], q)
        _, a, c = percentile32(conf[b], q)
        print(f"{tag} b={b}: thr {s['thr']!r} numpy {float(thr)!r} n {s['n']} numpy {int(keep.sum())}")
        if np.isnan(thr):
            if not (math.isnan(s["thr"]) and s["n"] == 0):
                errs.append(f"{tag} b={b}: NaN threshold expected, got thr {s['thr']} n {s['n']}")
            continue
        if _bits32(s["thr"]) != _bits32(thr):
            errs.append(f"{tag} b={b}: thr {s['thr']!r} != numpy {float(thr)!r}")
        if (_bits32(s["a"]), _bits32(s["c"])) != (_bits32(a), _bits32(c)):
            errs.append(f"{tag} b={b}: order statistics ({s['a']!r}, {s['c']!r}) != ({float(a)!r}, {float(c)!r})")
        if s["n"] != int(keep.sum()) or s["nan"] != 0:
            errs.append(f"{tag} b={b}: n {s['n']} nan {s['nan']} != {int(keep.sum())}, 0")


# --------------------------------------------------------------------------------- threshold and selection
def _sizes(N):
    G = N.GT_POINTS_GROUP
    return [1, 2, 3, 70, G - 1, G, G + 1, 70003]


@pytest.mark.parametrize("k", range(8))
def test_threshold_and_count_are_numpys(N, k):
    P = _sizes(N)[k]
    g = np.random.default_rng(100 + k)
    conf = _conf((1, P), 200 + k)
    mask = g.random((1, P)) < 0.7
    pred, gt = _cloud((1, P), 300 + k)
    errs = []
    for q in (0.0, 37.5, 50.0, 90.0, 100.0):
        _, _, st = _run(N, pred, conf, gt, mask, q)
        _check_state(errs, f"P={P} q={q}", st, conf, mask, q)
    _done(errs)


def _strided(full_shape, width, inner, dtype, fill):
    """A (B, S, H, W[, 3]) device tensor that starts one element after a 16-byte boundary, and its
    [:, :width] view: batch stride above the block."""
    n = int(np.prod(full_shape))
    buf = torch.zeros(n + 1 + 16, dtype=dtype, device=DEV)
    off = 1
    while (buf.data_ptr() + off * buf.element_size()) % 16 != buf.element_size() % 16:
        off += 1
    full = buf[off:off + n].view(full_shape)
    full.copy_(fill)
    assert (full.data_ptr() - buf.element_size()) % 16 == 0
    return full[:, :width]


def test_batch_strides_and_misaligned_bases(N):
    """B = 3 of [:, :seq_width] views with seq_width < S, every base one element off a 16-byte boundary
    (the scalar loads): the state is numpy's, and every element has the bits of the same element run
    alone from aligned contiguous copies (the 128-bit loads)."""
    B, S, H, W, wd = 3, 5, 37, 41, 3
    P = wd * H * W
    conf = _conf((B, S, H, W), 1)
    mask = np.random.default_rng(2).random((B, S, H, W)) < 0.6
    pred, gt = _cloud((B, S, H, W), 3)
    views = [_strided((B, S, H, W, 3), wd, 3 * P, torch.float32, torch.from_numpy(pred)),
             _strided((B, S, H, W), wd, P, torch.float32, torch.from_numpy(conf)),
             _strided((B, S, H, W, 3), wd, 3 * P, torch.float32, torch.from_numpy(gt)),
             _strided((B, S, H, W), wd, P, torch.bool, torch.from_numpy(mask))]
    errs = []
    for q in (50.0, 37.5):
        T, sc, st = N.gt_points_align(*views, q)
        state = N.gt_points_state(st)
        _check_state(errs, f"strided q={q}", state, conf[:, :wd].reshape(B, P), mask[:, :wd].reshape(B, P), q)
        for b in range(B):
            Tb, scb, stb = _run(N, pred[b:b + 1, :wd], conf[b:b + 1, :wd], gt[b:b + 1, :wd], mask[b:b + 1, :wd], q)
            _eq_bits(errs, f"q={q} T[{b}] alone", T[b:b + 1].cpu(), Tb)
            _eq_bits(errs, f"q={q} scale[{b}] alone", sc[b:b + 1].cpu(), scb)
            assert stb[0] == state[b]
        T2, sc2, _ = N.gt_points_align(*views, q)
        _eq_bits(errs, "T again", T2.cpu(), T.cpu())
        _eq_bits(errs, "scale again", sc2.cpu(), sc.cpu())
    _done(errs)


def test_thousands_of_confidences_equal_the_threshold(N):
    P = 70003
    g = np.random.default_rng(5)
    conf = (1.0 + np.floor(g.random((1, P)) * 5.0)).astype(np.float32)
    mask = g.random((1, P)) < 0.8
    pred, gt = _cloud((1, P), 6)
    errs = []
    for q in (50.0, 37.5, 90.0):
        thr = np.percentile(conf[0], q)
        assert int((conf[0] == thr).sum()) > 5000
        _, _, st = _run(N, pred, conf, gt, mask, q)
        _check_state(errs, f"ties q={q}", st, conf, mask, q)
    _done(errs)


def test_adjacent_floats_straddle_the_threshold(N):
    """a = 1.5 and c = the next float with g = 0.375: d g is under half an ulp and the lerp rounds down
    to a, so every pixel is kept; with g >= 0.5 numpy's second form is taken."""
    G = N.GT_POINTS_GROUP
    P = G + 10
    nxt = np.nextafter(np.float32(1.5), np.float32(2.0))
    errs = []
    for q in (37.5, 50.0, 90.0):
        h = np.float32(P - 1) * (np.float32(q) / np.float32(100.0))
        lo = int(np.floor(h))
        conf = np.full((1, P), nxt, np.float32)
        conf[0, :lo + 1] = 1.5
        conf = conf[:, np.random.default_rng(7).permutation(P)]
        thr, a, c = percentile32(conf[0], q)
        assert (a, c) == (np.float32(1.5), nxt)
        if q == 37.5:
            assert thr == a
        mask = np.ones((1, P), bool)
        pred, gt = _cloud((1, P), 8)
        _, _, st = _run(N, pred, conf, gt, mask, q)
        _check_state(errs, f"adjacent q={q}", st, conf, mask, q)
    _done(errs)


def test_confidences_at_and_just_above_the_floor(N):
    e = np.float32(1e-5)
    levels = np.array([e, np.nextafter(e, np.float32(1.0)), np.float32(0.5) * e, np.float32(2.0) * e], np.float32)
    P = 1000
    conf = levels[np.random.default_rng(9).integers(0, 4, (1, P))]
    mask = np.ones((1, P), bool)
    pred, gt = _cloud((1, P), 10)
    errs = []
    for q in (0.0, 25.0):
        _, _, st = _run(N, pred, conf, gt, mask, q)
        _check_state(errs, f"floor q={q}", st, conf, mask, q)
        if q == 0.0:  # thr = e / 2: the floor alone decides, and e itself is not above it
            assert st[0]["n"] == int((conf[0] > e).sum()) == int((conf[0] >= levels[1]).sum())
    _done(errs)


def test_a_nan_confidence_gives_nan(N):
    P = N.GT_POINTS_GROUP + 5
    conf = _conf((2, P), 11)
    conf[1, P - 2] = np.nan
    mask = np.ones((2, P), bool)
    pred, gt = _cloud((2, P), 12)
    T, sc, st = _run(N, pred, conf, gt, mask, 50.0)
    assert math.isnan(st[1]["thr"]) and st[1]["n"] == 0 and st[1]["nan"] == 1
    assert bool(torch.isnan(T[1, :3]).all()) and math.isnan(float(sc[1]))
    assert T[1, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    errs = []
    _check_state(errs, "nan", st[:1], conf[:1], mask[:1], 50.0)  # the other element is untouched by it
    assert bool(torch.isfinite(T[0]).all()) and math.isfinite(float(sc[0]))
    _done(errs)


# ------------------------------------------------------------------------------------------------ the solve
def _host(pred, conf, gt, mask, q, columns):
    from aligned_vggt.utils.alignment import umeyama_alignment_from_points
    T, sc = umeyama_alignment_from_points(pred, conf, gt, mask, q, columns=columns)
    return torch.from_numpy(np.asarray(T, dtype=np.float64)), torch.from_numpy(np.asarray(sc, dtype=np.float64))


def _exact_n(n, seed, mirror=False):
    """One element with exactly n kept pixels: q = 0 keeps every masked pixel."""
    P = n + n // 3 + 7
    g = np.random.default_rng(seed)
    mask = np.zeros((1, P), bool)
    mask[0, g.permutation(P)[:n]] = True
    pred, gt = _cloud((1, P), seed + 1, mirror)
    return pred, _conf((1, P), seed + 2), gt, mask


def _inexact_host(make, columns, q=0.0, parts=("T", "c"), tries=40):
    """The first of `tries` seeds at which the fp32 host function is off by at least 3 roundings on `parts`
    (host alone; the kernel is not run).  Where none reaches that, the seed at which the host's smaller
    error is largest: in the reference layout from n = 4099 up, the host's transform is within 0.5 to 1.3
    roundings at every seed tried (numpy sums pairwise), so 3 cannot be had there."""
    best = None
    for seed in range(0, 10 * tries, 10):
        pred, conf, gt, mask = make(seed)
        T64, c64, n, _ = solve_batch(pred, conf, gt, mask, q, columns, F64)
        Th, ch = _host(pred, conf, gt, mask, q, columns)
        B = len(n)
        e = [float(_row_err(Th[:, :3], T64[:, :3]).max()) if "T" in parts else math.inf,
             float(_row_err(ch.reshape(B, 1), c64.reshape(B, 1)).max()) if "c" in parts else math.inf]
        if best is None or min(e) > best[0]:
            best = (min(e), seed, (pred, conf, gt, mask), (T64, c64, n), (Th, ch))
        if min(e) >= 3 * U:
            break
    print(f"host model: seed {best[1]}, smaller error {best[0] / U:.2f} roundings")
    assert best[0] > 0
    return best[2:]


def _solve_rule(errs, tag, T, sc, ref, host):
    T64, c64, n = ref
    B = len(n)
    _eq_bits(errs, f"{tag} last row", T[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4).contiguous())
    _model_rule(errs, f"{tag} T", T[:, :3], host[0][:, :3], T64[:, :3], "gt_points")
    _model_rule(errs, f"{tag} scale", sc.reshape(B, 1), host[1].reshape(B, 1), c64.reshape(B, 1), "gt_points")


@pytest.mark.parametrize("columns", ["reference", "points"])
@pytest.mark.parametrize("n", [3, 4, 5, 4099, 50001])
def test_solve_against_fp64(N, n, columns):
    """n mod 3 = 0, 1, 2, 1, 0; one workgroup, two, and thirteen with a partial last one."""
    args, ref, host = _inexact_host(lambda seed: _exact_n(n, 1000 * n + seed), columns, tries=40 if n < 10000 else 8)
    T, sc, st = _run(N, *args, 0.0, columns)
    assert st[0]["n"] == n == ref[2][0]
    errs = []
    _solve_rule(errs, f"n={n} {columns}", T, sc, ref, host)
    _done(errs)


@pytest.mark.parametrize("columns", ["reference", "points"])
def test_kernel_reproduces_the_fixture(N, columns):
    """The six cases of points_alignment.npz: thr, the order statistics and n bit for bit, and the model
    rule over the fixture as a whole: the kernel's worst row of any case is at most 2 x the fp32 model's
    worst row of any case (each case's rows over that case's RMS row norm), for the transform rows and
    for the scale.  The model is the reference's own output in its layout and the fp32 host function in
    the per-point layout.  The rule is not applied case by case: the fixture is fixed, and on single
    cases the reference's fp32 scale happens to be nearly exact (`mid`: 8.0e-9, 0.13 roundings), where a
    correctly rounded kernel result (4.8e-8, under one rounding) is six times further off."""
    z = np.load(GOLDEN)
    errs, worst = [], {"kernel T": 0.0, "model T": 0.0, "kernel scale": 0.0, "model scale": 0.0}
    for name in CASES:
        c = load_case(z, name)
        q = float(c["q"])
        T, sc, st = _run(N, c["pred"], c["conf"], c["gt"], c["mask"], q, columns)
        B = T.shape[0]
        flat = lambda a: a.reshape(B, -1)  # noqa: E731
        _check_state(errs, name, st, flat(c["conf"]), flat(c["mask"]), q)
        assert [s["n"] for s in st] == c["n"].tolist()
        assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(sc).all())
        _eq_bits(errs, f"{name} last row", T[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4).contiguous())
        T64, c64, n, _ = solve_batch(c["pred"], c["conf"], c["gt"], c["mask"], q, columns, F64)
        if columns == "reference":  # the reference's own output is the fp32 model
            model = (torch.from_numpy(c["T"]).double(), torch.from_numpy(c["scale"]).double())
        else:
            model = _host(c["pred"], c["conf"], c["gt"], c["mask"], q, columns)
        fig = {"kernel T": _row_err(T[:, :3], T64[:, :3]), "model T": _row_err(model[0][:, :3], T64[:, :3]),
               "kernel scale": _row_err(sc.reshape(B, 1), c64.reshape(B, 1)),
               "model scale": _row_err(model[1].reshape(B, 1), c64.reshape(B, 1))}
        print(f"fixture {name} {columns}: " + ", ".join(f"{k} {float(v.max()):.3e}" for k, v in fig.items()))
        for k, v in fig.items():
            worst[k] = max(worst[k], float(v.max()))
    print(f"fixture {columns} worst: {worst}")
    for part in ("T", "scale"):
        if not worst[f"kernel {part}"] <= 2 * worst[f"model {part}"]:
            errs.append(f"{columns} {part}: kernel worst row {worst['kernel ' + part]:.3e} > 2 x model "
                        f"{worst['model ' + part]:.3e}")
    _done(errs)


def _proper(errs, tag, R):
    Rd = R.double()
    det, rtr = abs(float(torch.det(Rd)) - 1.0), float((Rd.T @ Rd - torch.eye(3, dtype=F64)).abs().max())
    print(f"{tag}: |det - 1| {det:.3e} |RtR - I| {rtr:.3e}")
    if not (det <= 1e-6 and rtr <= 1e-6):
        errs.append(f"{tag}: not a proper rotation (|det - 1| {det:.3e}, |RtR - I| {rtr:.3e})")


def test_one_sample_is_non_finite(N):
    for columns in COLS:
        pred, conf, gt, mask = _exact_n(1, 21)
        T, sc, st = _run(N, pred, conf, gt, mask, 0.0, columns)
        assert st[0]["n"] == 1
        assert not math.isfinite(float(sc[0])) and not bool(torch.isfinite(T[0, :3, 3]).any())
        assert T[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


def _line(n, seed):
    """n collinear points in general direction, kept by q = 0 with a full mask; gt a similarity of them."""
    g = np.random.default_rng(seed)
    d = g.standard_normal(3)
    s = g.standard_normal((n, 1)) * 2.0
    pred = (np.array([0.3, -0.7, 1.1]) + s * d).astype(np.float32)[None]
    c, sn = math.cos(0.7), math.sin(0.7)
    R0 = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
    gt = (1.4 * pred.astype(np.float64) @ R0.T + np.array([0.5, -1.0, 2.0])).astype(np.float32)
    return pred, _conf((1, n), seed + 1), gt, np.ones((1, n), bool)


@pytest.mark.parametrize("kind", ["two reference", "two points", "line points"])
def test_rank_one_clouds_give_a_proper_rotation(N, kind):
    """Two samples, and collinear samples: the rotation about the line is free, so R is held to be a
    proper rotation (det = 1 and R^T R = I within 1e-6, as _svd_pair_check holds the line case) and the
    scale to the model rule."""
    columns = kind.split()[1]
    make = (lambda seed: _line(5, 500 + seed)) if kind.startswith("line") else (lambda seed: _exact_n(2, 600 + seed))
    args, ref, host = _inexact_host(make, columns, parts=("c",))
    T, sc, st = _run(N, *args, 0.0, columns)
    assert st[0]["n"] == (5 if kind.startswith("line") else 2)
    errs = []
    _proper(errs, kind, T[0, :3, :3])
    _model_rule(errs, f"{kind} scale", sc.reshape(1, 1), host[1].reshape(1, 1), ref[1].reshape(1, 1), "gt_points")
    _done(errs)


def test_mirrored_points_take_the_reflection_branch(N):
    args, ref, host = _inexact_host(lambda seed: _exact_n(200, 700 + seed, mirror=True), "points")
    X = args[0].reshape(-1, 3)[args[3].reshape(-1)].astype(np.float64)
    Y = args[2].reshape(-1, 3)[args[3].reshape(-1)].astype(np.float64)
    Uu, _, Vh = np.linalg.svd((Y - Y.mean(0)).T @ (X - X.mean(0)))
    assert np.linalg.det(Uu) * np.linalg.det(Vh) < 0  # d = -1
    T, sc, _ = _run(N, *args, 0.0, "points")
    errs = []
    _proper(errs, "mirrored", T[0, :3, :3])
    _solve_rule(errs, "mirrored", T, sc, ref, host)
    _done(errs)


def test_unselected_pixels_may_hold_anything(N):
    G = N.GT_POINTS_GROUP
    B, P = 2, G + 70
    conf = _conf((B, P), 31)
    mask = np.random.default_rng(32).random((B, P)) < 0.6
    pred, gt = _cloud((B, P), 33)
    errs = []
    for columns in COLS:
        T, sc, st = _run(N, pred, conf, gt, mask, 50.0, columns)
        p2, g2 = pred.copy(), gt.copy()
        for b in range(B):
            keep, _ = select(conf[b], mask[b], 50.0)
            out = np.flatnonzero(~keep)
            assert 0 < st[b]["n"] == int(keep.sum()) < P
            p2[b, out[0::3]], p2[b, out[1::3]], p2[b, out[2::3]] = np.nan, np.inf, -np.inf
            g2[b, out[0::2]], g2[b, out[1::2]] = np.inf, np.nan
        T2, sc2, st2 = _run(N, p2, conf, g2, mask, 50.0, columns)
        assert st2 == st
        _eq_bits(errs, f"{columns} T", T2, T)
        _eq_bits(errs, f"{columns} scale", sc2, sc)
        assert bool(torch.isfinite(T).all())
    _done(errs)


def test_repeatable_and_independent_of_the_batch(N):
    G = N.GT_POINTS_GROUP
    B, P = 3, 2 * G + 5
    conf = _conf((B, P), 41)
    mask = np.random.default_rng(42).random((B, P)) < 0.7
    pred, gt = _cloud((B, P), 43)
    errs = []
    for columns in COLS:
        T, sc, st = _run(N, pred, conf, gt, mask, 50.0, columns)
        T2, sc2, st2 = _run(N, pred, conf, gt, mask, 50.0, columns)
        _eq_bits(errs, "T again", T2, T)
        _eq_bits(errs, "scale again", sc2, sc)
        assert st2 == st
        for b in range(B):
            Tb, scb, stb = _run(N, pred[b:b + 1], conf[b:b + 1], gt[b:b + 1], mask[b:b + 1], 50.0, columns)
            _eq_bits(errs, f"{columns} T[{b}] alone", Tb, T[b:b + 1])
            _eq_bits(errs, f"{columns} scale[{b}] alone", scb, sc[b:b + 1])
            assert stb[0] == st[b]
    _done(errs)


# --------------------------------------------------------------------------------------------------- errors
def test_every_refusal_of_the_entry_point(N):
    L = N.lib()
    B, P = 2, 8
    t = {"pred": torch.zeros(B, P, 3, device=DEV), "conf": torch.ones(B, P, device=DEV),
         "gt": torch.zeros(B, P, 3, device=DEV), "mask": torch.ones(B, P, dtype=torch.uint8, device=DEV),
         "T": torch.zeros(B, 16, device=DEV), "scale": torch.zeros(B, device=DEV),
         "state": torch.zeros(B, N.GT_POINTS_STATE_WORDS, dtype=torch.int64, device=DEV)}
    need = N.gt_points_align_ws_bytes(B, P)
    assert need > 0 and need % 16 == 0
    ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device=DEV)
    assert ws.data_ptr() % 16 == 0
    base = dict(pred=t["pred"].data_ptr(), pred_bs=3 * P, conf=t["conf"].data_ptr(), conf_bs=P,
                gt=t["gt"].data_ptr(), gt_bs=3 * P, mask=t["mask"].data_ptr(), mask_bs=P, B=B, P=P, q=50.0,
                columns=0, T=t["T"].data_ptr(), scale=t["scale"].data_ptr(), state=t["state"].data_ptr(),
                ws=ws.data_ptr(), ws_bytes=need)

    def call(**over):
        a = dict(base, **over)
        return L.vggt_gt_points_align(a["pred"], a["pred_bs"], a["conf"], a["conf_bs"], a["gt"], a["gt_bs"], a["mask"],
                                      a["mask_bs"], a["B"], a["P"], a["q"], a["columns"], a["T"], a["scale"],
                                      a["state"], a["ws"], a["ws_bytes"], None)
    assert call() == 0
    torch.cuda.synchronize()
    shape = [dict(B=0), dict(B=65536), dict(P=0), dict(P=2 ** 31 - 256), dict(pred_bs=3 * P - 1), dict(gt_bs=3 * P - 1),
             dict(conf_bs=P - 1), dict(mask_bs=P - 1), dict(q=-0.5), dict(q=100.5), dict(q=float("nan")),
             dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 8)]
    shape += [{k: None} for k in ("pred", "conf", "gt", "mask", "T", "scale", "state")]
    for over in shape:
        assert call(**over) == ERR_SHAPE, over
    for k in ("pred", "conf", "gt", "T", "scale"):
        assert call(**{k: base[k] + 2}) == ERR_ALIGN, k
    assert call(state=base["state"] + 4) == ERR_ALIGN
    assert call(columns=2) == ERR_UNSUPPORTED and call(columns=-1) == ERR_UNSUPPORTED
    assert call(B=1, pred_bs=0, conf_bs=0, gt_bs=0, mask_bs=0) == 0  # strides are ignored without a batch
    assert N.gt_points_align_ws_bytes(0, P) == 0 and N.gt_points_align_ws_bytes(B, 2 ** 31 - 256) == 0
    assert N.gt_points_align_ws_bytes(1, 2 ** 31 - 257) > 24 * (2 ** 31 - 257)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="fp32"):
        N.gt_points_align(t["pred"].double(), t["conf"], t["gt"], t["mask"], 50.0)
    with pytest.raises(RuntimeError, match="per-batch"):
        N.gt_points_align(t["pred"], t["conf"].t().contiguous().t(), t["gt"], t["mask"], 50.0)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        N.gt_points_align(t["pred"].cpu(), t["conf"], t["gt"], t["mask"], 50.0)


# ----------------------------------------------------------------------------------------------- end to end
def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _rot64(q):
    from aligned_vggt.utils.rotation import quat_to_mat
    return quat_to_mat(q.double())


def _poses(B, S, g):
    """(pose_enc (B, S, 9), gt_extr (B, S, 3, 4)) fp32 (test_gpu_training_metrics._poses)."""
    x = torch.randn(B, S, 3, generator=g, dtype=F64) * torch.tensor([3.0, 2.0, 1.0], dtype=F64)
    q = torch.randn(B, S, 4, generator=g, dtype=F64)
    q = (q / q.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(B, S, 1, generator=g, dtype=F64))).float()
    R = _rot64(q)
    t = -(R @ x[..., None])[..., 0]
    enc = torch.cat([t.float(), q, 0.8 + 0.5 * torch.rand(B, S, 2, generator=g)], -1).contiguous()
    y = 1.7 * x @ _rot64(torch.tensor([0.3, -0.2, 0.5, 0.8])).T + torch.tensor([0.4, -1.0, 2.0], dtype=F64)
    Rg = _rot64(torch.randn(B, S, 4, generator=g))
    tg = -(Rg @ y[..., None])[..., 0]
    return enc, torch.cat([Rg, tg[..., None]], -1).float().contiguous()


def _step(B=2, S=7, H=6, W=9, seed=0):
    g = _gen(9, seed)
    enc, extr = _poses(B, S, g)
    wp = torch.randn(B, S, H, W, 3, generator=g) * torch.tensor([3.0, 2.0, 1.0])
    gt = 1.4 * wp @ _rot64(torch.tensor([0.3, -0.2, 0.5, 0.8])).float().T + torch.tensor([0.4, -1.0, 2.0]) \
        + 0.05 * torch.randn(B, S, H, W, 3, generator=g)
    pred = {"pose_enc": enc, "depth": 0.5 + torch.rand(B, S, H, W, 1, generator=g), "world_points": wp,
            "world_points_conf": 1.0 + 4.0 * torch.rand(B, S, H, W, generator=g)}
    batch = {"extrinsics": extr, "images": torch.zeros(B, S, 3, H, W), "world_points": gt,
             "point_masks": torch.rand(B, S, H, W, generator=g) < 0.8}
    return pred, batch


def _chunked(pred, batch, cuts):
    return ({k: [v[:, a:b].clone() for a, b in cuts] for k, v in pred.items()},
            {k: [v[:, a:b].clone() for a, b in cuts] for k, v in batch.items()})


class _no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        self.before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.before)


CUTS = ((0, 4), (2, 6), (4, 7))  # chunk 4, overlap 2


def _e2e(dev, guard=False, seed=0):
    from aligned_vggt.utils.data import alignAndConvertOutputs
    pred, batch = _step(seed=seed)
    p, cb = _chunked(pred, batch, CUTS)
    p = {k: [t.to(dev) for t in v] for k, v in p.items()}
    cb = {k: [t.to(dev) for t in v] for k, v in cb.items()}
    merged = {}
    if guard:
        with _no_sync():
            alignAndConvertOutputs(p, merged, cb, "sim3_from_points", 4, 2)
    else:
        alignAndConvertOutputs(p, merged, cb, "sim3_from_points", 4, 2)
    return p, merged


def _e2e_fp64(seed=0):
    """The same steps in fp64 from the fp32 inputs: the restatement's transform and scale, then
    apply_sim3_alignment's chain (w2c -> c2w, translation x scale, T ., -> w2c, the FoV round trip)."""
    from aligned_vggt.utils.rotation import mat_to_quat
    pred, batch = _step(seed=seed)
    w = 4
    T, c, _, _ = solve_batch(pred["world_points"][:, :w].numpy(), pred["world_points_conf"][:, :w].numpy(),
                             batch["world_points"][:, :w].numpy(), batch["point_masks"][:, :w].numpy(), 50.0,
                             "reference", F64)
    enc = pred["pose_enc"]
    R, t = _rot64(enc[..., 3:7]), enc[..., :3].double()
    Rp = R.transpose(-1, -2)
    tp = -(Rp @ t[..., None])[..., 0] * c[:, None, None]
    Rt, tt = T[:, None, :3, :3], T[:, None, :3, 3]
    Ra, ta = Rt @ Rp, (Rt @ tp[..., None])[..., 0] + tt
    Rw = Ra.transpose(-1, -2)
    tw = -(Rw @ ta[..., None])[..., 0]
    H, Wd = batch["images"].shape[-2:]
    size = torch.tensor([H / 2.0, Wd / 2.0], dtype=F64)
    fov = 2 * torch.atan(size / (size / torch.tan(enc[..., 7:9].double() / 2)))
    pts = (c.view(-1, 1, 1, 1, 1) * pred["world_points"].double()) @ T[:, None, None, :3, :3].transpose(-1, -2) \
        + T[:, None, None, None, :3, 3]
    return {"pose_enc": torch.cat([tw, mat_to_quat(Rw), fov], -1), "world_points": pts,
            "depth": pred["depth"].double() * c.view(-1, 1, 1, 1, 1)}


def _same_hemisphere(enc, ref):
    """q and -q are one rotation: give enc's quaternion the sign of ref's."""
    enc = enc.clone()
    sign = torch.where((enc[..., 3:7].double() * ref[..., 3:7]).sum(-1, keepdim=True) < 0, -1.0, 1.0)
    enc[..., 3:7] = (enc[..., 3:7].double() * sign).to(enc.dtype)
    return enc


def test_align_and_convert_outputs_on_the_device(N, monkeypatch):
    """sim3_from_points on three device chunks: no synchronisation (the parent's host route calls
    .cpu() here), the values against the fp64 composition with the CPU run as the fp32 model, and
    under VGGT_GT_ALIGN=torch the numpy route's transform and scale bit for bit.  (The dense outputs of
    that route go through torch on the device, which is not bitwise torch on the host: they are held to
    2^-14 of the largest magnitude, as test_gpu_training_metrics holds sim3_from_poses.)"""
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    _e2e(DEV)  # the library is loaded, the allocator is warm
    got, merged = _e2e(DEV, guard=True)
    cpu, _ = _e2e("cpu")
    ref = _e2e_fp64()
    assert got["pose_enc"].shape == (2, 7, 9) and merged["world_points"].shape == (2, 7, 6, 9, 3)
    errs = []
    for k in ("pose_enc", "world_points", "depth"):
        assert got[k].is_cuda and got[k].dtype == F32 and not got[k].requires_grad
        g, m = got[k].cpu(), cpu[k]
        if k == "pose_enc":
            g, m = _same_hemisphere(g, ref[k]), _same_hemisphere(m, ref[k])
        last = ref[k].shape[-1]
        _model_rule(errs, k, g.reshape(-1, last), m.reshape(-1, last), ref[k].reshape(-1, last), "gt_points_e2e")
    # the knob: the numpy route on device tensors, never the kernel; its transform and scale have the bits
    # of the CPU run's, and the torch chain that applies them agrees with the CPU's as the pose types' does
    from aligned_vggt.utils.alignment import umeyama_alignment_from_points
    pred, batch = _step()
    args = (pred["world_points"][:, :4], pred["world_points_conf"][:, :4], batch["world_points"][:, :4],
            batch["point_masks"][:, :4])
    want = umeyama_alignment_from_points(*args, 50.0)
    monkeypatch.setenv("VGGT_GT_ALIGN", "torch")

    def refuse(*a, **k):
        raise AssertionError("vggt_gt_points_align launched under VGGT_GT_ALIGN=torch")
    monkeypatch.setattr(N, "gt_points_align", refuse)
    have = umeyama_alignment_from_points(*(t.to(DEV) for t in args), 50.0)
    for a, b in zip(have, want):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    knob, _ = _e2e(DEV)
    for k in ("pose_enc", "world_points", "depth"):
        torch.testing.assert_close(knob[k].cpu(), cpu[k], rtol=0, atol=2.0 ** -14 * float(cpu[k].abs().max()))
    _done(errs)
