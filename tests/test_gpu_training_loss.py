"""The training objective on the GPU (csrc/loss.hip, aligned_vggt/training/loss.py).

Values stage: `val` of vggt_depth_loss_values against an fp64 evaluation of the formula, element by element, within
c u (|log p| + |log g'| + 1) conf_n, u = 2^-24.  c is not fixed in advance: it is 4 x the error, in those units, of
the CPU torch fp32 evaluation of the same formula on the same inputs (two independent logf implementations each
stand a few ulp from the truth), and never below 4.  Everything after the values stage is exact in its decisions: n,
k, thr', m and the case the device reports equal what torch takes on the CPU from the device's own `val`; the loss is
the fp64 mean of the chosen terms to n u relative (an fp64 sum rounded to fp32); two runs are bitwise equal.  The
backward is non-zero on exactly the set that decision predicts and matches the fp64 autograd of the restatement
(test_training_loss.py) there to the values-stage bound over p denom."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_training_loss as R
from edge_rules import _guarded, _guards_ok

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------- inputs
def _random_inputs(shape, seed, mask_p=0.85):
    g = torch.Generator().manual_seed(seed)
    pred = 0.5 + 4.0 * torch.rand(shape, generator=g)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    gt = pred * torch.exp(sign * (0.02 + 0.8 * torch.rand(shape, generator=g)))  # |log p - log g| >= 0.02: no sign ties
    conf = 1.0 + torch.exp(torch.randn(shape, generator=g))
    mask = torch.rand(shape, generator=g) < mask_p
    return pred, conf, gt, mask


@functools.lru_cache(maxsize=None)
def _edge_inputs():
    """2 x 3 x 14 x 37 (H W = 518: no multiple of 4 or 64) with every special input of the values stage."""
    shape = (2, 3, 14, 37)
    pred, conf, gt, mask = _random_inputs(shape, 7)
    g = torch.Generator().manual_seed(8)
    pick = lambda p: torch.rand(shape, generator=g) < p  # noqa: E731
    conf[0, 1] = 0.0                      # a frame whose confidences are all 0: clamp_min(1e-8) of the amax
    conf[1, 0] = -0.0                     # all -0: torch.amax gives -0 (the amax key keeps the zeros apart)
    assert bool(mask[1, 0].any())
    pred[pick(0.02)] = 1e-9               # below the clamp
    pred[pick(0.01)] = 0.0
    pred[pick(0.01)] = -1.5
    gt[pick(0.02)] = NAN                  # scrubbed to 0, then clamped to 1e-8
    gt[pick(0.02)] = INF
    gt[pick(0.01)] = -INF
    pred[pick(0.03)] = NAN                # a NaN value
    conf[1, 2, 3, 5] = NAN                # a NaN amax: the whole frame
    eq = pick(0.02)
    gt[eq] = pred[eq]                     # exact ties: sign 0
    return pred, conf, gt, mask


@functools.lru_cache(maxsize=None)
def _reference(key):
    """fp64 val, conf_n, logs and the measured c of the inputs named by `key`, computed once."""
    pred, conf, gt, mask = _inputs(key)
    val64, cn, lp, lg = R.depth_values64(pred, conf, gt, mask)
    unit = U * (lp.abs() + lg.abs() + 1) * cn.abs()
    g32 = R.fix(gt, None)
    eps = torch.tensor(1e-8, dtype=torch.float32)
    cn32 = conf / conf.amax(dim=(2, 3), keepdim=True).clamp_min(eps)
    val32 = (torch.log(pred.clamp_min(eps)) - torch.log(g32.clamp_min(eps))).abs() * cn32
    ok = mask & torch.isfinite(val64) & (unit > 0)
    measured = float(((val32.double() - val64).abs()[ok] / unit[ok]).max()) if ok.any() else 0.0
    return {"val": val64, "cn": cn, "lp": lp, "lg": lg, "unit": unit, "measured": measured, "c": max(4.0, 4 * measured)}


def _inputs(key):
    if key == "edge":
        return _edge_inputs()
    if key == "big":
        return _random_inputs((1, 2, 154, 518), 31, 0.9)
    if key == "nan_thr":  # more than 2 % of the set pixels have a NaN prediction: the 0.98 quantile is NaN
        pred, conf, gt, mask = _random_inputs((2, 3, 14, 37), 41, 0.9)
        pred = pred.clone()
        pred[torch.rand(pred.shape, generator=torch.Generator().manual_seed(42)) < 0.04] = NAN
        return pred, conf, gt, mask
    z, cases = R.golden()
    tag, _, n = key.partition("@")  # a fixture case, optionally with the mask cut down to n set pixels
    t = lambda k: torch.from_numpy(z[f"{tag}.in.{k}"])  # noqa: E731
    mask = t("point_masks").clone()
    if n:
        flat = mask.view(-1)
        on = flat.nonzero()[:, 0]
        flat[on[torch.randperm(on.numel(), generator=torch.Generator().manual_seed(5))[int(n):]]] = False
        assert int(mask.sum()) == int(n)
    return t("depth")[..., 0].contiguous(), t("depth_conf"), t("depths"), mask


def _check_values(key, got, amax, n):
    """`got` (host fp32) against the fp64 formula; returns the worst error in units of the bound."""
    pred, conf, gt, mask = _inputs(key)
    ref = _reference(key)
    assert int(n) == int(mask.sum())
    assert torch.equal(_bits(amax), _bits(conf.amax(dim=(2, 3))))  # a maximum: exact, NaN propagated
    assert bool((_bits(got)[~mask] == 0x7fc00000).all())
    want = ref["val"]
    nan = torch.isnan(want) & mask
    assert torch.equal(torch.isnan(got) & mask, nan)
    inf = torch.isinf(want) & mask
    assert torch.equal(got[inf].double(), want[inf])
    fin = mask & torch.isfinite(want)
    err, bound = (got.double() - want).abs()[fin], ref["c"] * ref["unit"][fin]
    print(f"values[{key}]: CPU fp32 vs fp64 {ref['measured']:.3f}, c = {ref['c']:.3f}, "
          f"worst GPU error / (u (|log p| + |log g'| + 1) conf_n) = "
          f"{float((err / ref['unit'][fin].clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def _values_raw(N, pred, conf, gt, mask):
    """vggt_depth_loss_values through the C ABI into guarded outputs."""
    B, S, H, W = mask.shape
    vbuf, val = _guarded((B, S, H, W), torch.float32)
    abuf, amax = _guarded((B, S), torch.float32)
    nbuf, n = _guarded((2,), torch.int64, fill=7)
    ws = torch.empty(N.depth_loss_ws_bytes(B, S, H, W) // 8 + 1, dtype=torch.int64, device="cuda")
    rc = N.lib().vggt_depth_loss_values(N._p(pred), N._p(conf), N._p(gt), N._p(mask), B, S, H, W, N._p(val),
                                        N._p(amax), N._p(n), N._p(ws), ws.numel() * 8, N._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _guards_ok(vbuf, val.numel()) and _guards_ok(abuf, amax.numel())
    nh = nbuf.cpu()
    assert nh[:64].eq(7).all() and nh[66:].eq(7).all() and int(nh[65]) == 7
    return val, amax, n[0]


# ------------------------------------------------------------------------------------------- values stage
def test_values_stage_against_fp64(N):
    for key in ("edge", "big", "filtered_b2"):
        pred, conf, gt, mask = (t.cuda() for t in _inputs(key))
        val, amax, n = _values_raw(N, pred, conf, gt, mask)
        _check_values(key, val.cpu(), amax.cpu(), int(n))
        if key == "edge":  # the all -0 frame: torch.amax's -0 (checked here on the CPU), bit for bit
            assert int(_bits(torch.full((518,), -0.0).amax())) == -0x80000000
            assert int(_bits(amax)[1, 0]) == -0x80000000 and int(_bits(amax)[0, 1]) == 0
        if key == "big":
            continue
        # the element-by-element path (pointers 4 bytes off a 16-byte boundary): the same bits
        off = [torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape).copy_(t) for t in (pred, conf, gt)]
        assert all(t.data_ptr() % 16 == 4 for t in off)
        val2, amax2, n2, _ = N.depth_loss_values(*off, mask)
        assert torch.equal(_bits(val2), _bits(val)) and torch.equal(_bits(amax2), _bits(amax)) and int(n2) == int(n)


def test_values_rejects_bad_arguments(N):
    B, S, H, W = 1, 2, 14, 37
    x = torch.ones(B, S, H, W, device="cuda")
    m = torch.ones(B, S, H, W, dtype=torch.bool, device="cuda")
    n = torch.zeros((), dtype=torch.int64, device="cuda")
    amax = torch.zeros(B, S, device="cuda")
    ws = torch.zeros(N.depth_loss_ws_bytes(B, S, H, W) // 8 + 1, dtype=torch.int64, device="cuda")
    L, p, st = N.lib(), N._p, N._stream()
    call = lambda pred, b, w, wsb: L.vggt_depth_loss_values(pred, p(x), p(x), p(m), b, S, H, w, p(x), p(amax), p(n),  # noqa: E731
                                                             p(ws), wsb, st)
    assert call(p(x), B, W, ws.numel() * 8) == 0
    assert call(None, B, W, ws.numel() * 8) == N.VGGT_ERR_SHAPE
    assert call(p(x), 0, W, ws.numel() * 8) == N.VGGT_ERR_SHAPE
    assert call(p(x), B, -W, ws.numel() * 8) == N.VGGT_ERR_SHAPE
    assert call(p(x), B, W, 4) == N.VGGT_ERR_SHAPE
    assert call(ctypes.c_void_p(x.data_ptr() + 2), B, W, ws.numel() * 8) == N.VGGT_ERR_ALIGN
    assert call(p(x), 200000, W, ws.numel() * 8) == N.VGGT_ERR_UNSUPPORTED  # past 10^8 elements; nothing is read
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        N.depth_loss_values(x.cpu(), x.cpu(), x.cpu(), m.cpu())


# ----------------------------------------------------------------------------------------- after the values
def _check_reduce(N, val, mask, valid_range, expect_kind=None, expect_m=None):
    """Reduce `val` (device; NaN at unset pixels) twice; the device's state and loss against torch on the CPU."""
    n = mask.sum().cuda()
    runs = [N.depth_loss_reduce(val, n, valid_range) for _ in range(2)]
    torch.cuda.synchronize()
    (loss, state), (loss2, state2) = runs
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(state.cpu(), state2.cpu())
    v = val.cpu()[mask.cpu()]
    d = R.decide(v, valid_range)
    st = N.depth_loss_state(state)
    assert (st["n"], st["k"], st["m"], st["kind"]) == (d["n"], d["k"], d["m"], d["kind"]), (st, d)
    assert st["denom"] == d["denom"]
    want_thr = torch.tensor(d["thr"], dtype=torch.float32)
    got_thr = torch.tensor(st["thr"], dtype=torch.float32)
    assert torch.equal(_bits(got_thr), _bits(want_thr)) or (torch.isnan(got_thr) and torch.isnan(want_thr)), (st, d)
    if expect_kind is not None:
        assert d["kind"] == expect_kind, d
    if expect_m is not None:
        assert d["m"] == expect_m, d
    terms = R.chosen_terms(v.double(), d, keep=R.chosen_mask(v, d))
    if terms is None:
        assert float(loss) == 0.0
    else:
        mean = float(terms.sum() / d["denom"])
        assert abs(float(loss) - mean) <= d["n"] * U * float(terms.abs().sum() / d["denom"]), (float(loss), mean)
    return d, state


REDUCE_CASES = [  # inputs, valid_range, the case, m
    ("skipped", 0.98, R.SKIPPED, 0), ("unfiltered", 0.98, R.CLAMPED, 985), ("filtered", 0.98, R.FILTERED, 1014),
    ("filtered_b2", 0.98, R.FILTERED, None), ("no_range", -1, R.UNCLAMPED, 0),
    ("filtered@99", 0.98, R.SKIPPED, 0), ("filtered@100", 0.98, R.UNCLAMPED, 0),
    ("filtered@1000", 0.98, R.UNCLAMPED, 0), ("filtered@1001", 0.98, R.CLAMPED, 980),
    ("nan_thr", 0.98, R.CLAMPED, 0), ("edge", 0.5, R.FILTERED, None), ("big", 0.98, R.FILTERED, None),
]


@pytest.mark.parametrize("key,valid_range,kind,m", REDUCE_CASES)
def test_decisions_loss_and_backward(N, key, valid_range, kind, m):
    pred, conf, gt, mask = _inputs(key)
    dev = [t.cuda() for t in (pred, conf, gt, mask)]
    val, amax, n, ws = N.depth_loss_values(*dev)
    d, state = _check_reduce(N, val, dev[3], valid_range, kind, m)
    if key == "nan_thr":
        assert np.isnan(d["thr"]) and d["k"] > 0

    # backward: twice (bitwise equal), against the fp64 autograd of the restatement under the device's decision
    up = torch.tensor(0.75, device="cuda")
    dbuf, dpred = _guarded(mask.shape, torch.float32)
    N.depth_loss_bwd(*dev, amax, state, up, dpred=dpred)
    again = N.depth_loss_bwd(*dev, amax, state, up)
    torch.cuda.synchronize()
    assert _guards_ok(dbuf, dpred.numel()) and torch.equal(_bits(dpred), _bits(again))
    got = dpred.cpu()
    ref = _reference(key)
    v32 = val.cpu()
    p64 = pred.double().requires_grad_(True)
    val64 = R.depth_values64(p64, conf, gt, mask)[0]
    keep = torch.zeros_like(mask)
    keep[mask] = R.chosen_mask(v32[mask], d)
    terms = R.chosen_terms(val64[mask], d, keep=keep[mask])
    if terms is not None:
        (0.75 * terms.sum() / d["denom"]).backward()
    want = p64.grad if p64.grad is not None else torch.zeros_like(p64)
    # the contributing set, from the device's own values: kept, finite, within +-100, prediction not clamped
    on = keep & torch.isfinite(v32) & (v32.abs() <= 100) & (pred >= torch.tensor(1e-8, dtype=torch.float32))
    gap = (ref["lp"] - ref["lg"]).abs()
    assert not bool(((gap > 0) & (gap < 1e-5) & on).any())  # precondition: no sign decided by rounding
    # autograd leaves 0 x NaN = NaN at scrubbed pixels (a NaN prediction or confidence); the kernel's rule is 0
    assert not bool((torch.isnan(want) & on).any())
    want = torch.where(torch.isnan(want), torch.zeros_like(want), want)
    nonzero = on & (gap > 0) & (ref["cn"] != 0)
    assert torch.equal(got != 0, nonzero), (int((got != 0).sum()), int(nonzero.sum()))
    assert torch.equal(want != 0, nonzero)
    if nonzero.any():
        p = pred.double().clamp_min(R.EPS32)
        bound = 0.75 * ref["c"] * ref["unit"] / (p * d["denom"])
        err = (got.double() - want).abs()
        assert bool((err[nonzero] <= bound[nonzero]).all()), float((err[nonzero] / bound[nonzero]).max())


def _planted(n_small, n_at, total, thr, extra=(), top=None):
    """A (1, 1, 1, total) value buffer: n_small distinct values in [0.1, 0.9) top (top = thr unless given), n_at
    equal to thr, `extra` others, the rest unset; in a seeded order."""
    small = (top or thr) * (0.1 + 0.8 * torch.arange(n_small, dtype=torch.float32) / max(n_small, 1))
    v = torch.cat([small, torch.full((n_at,), thr), torch.tensor(list(extra), dtype=torch.float32)])
    n = v.numel()
    assert n <= total
    out = torch.full((total,), NAN)
    at = torch.randperm(total, generator=torch.Generator().manual_seed(total + n))[:n]
    out[at] = v
    mask = torch.zeros(total, dtype=torch.bool)
    mask[at] = True
    return out.view(1, 1, 1, total), mask.view(1, 1, 1, total)


def test_decisions_on_planted_values(N):
    # n = 1030: k = round(0.98 * 1029) + 1 = 1009 falls among the values equal to thr, so m is the count below it
    for m, kind in ((1000, R.CLAMPED), (1001, R.FILTERED)):
        val, mask = _planted(m, 1030 - m, 1500, 0.5)
        d, _ = _check_reduce(N, val.cuda(), mask.cuda(), 0.98, kind, m)
        assert d["k"] == 1009 and d["thr"] == 0.5
    # a threshold above 100 (k = 2548 of 2600 lands on 150): thr' = 100, and min(val, 100) < 100 keeps the 1100
    # below 90 with -inf and -250
    val, mask = _planted(1100, 1495, 4099, 150.0, extra=(INF, -INF, 250.0, -250.0, NAN), top=90.0)
    d, _ = _check_reduce(N, val.cuda(), mask.cuda(), 0.98, R.FILTERED, 1102)
    assert d["thr"] == 100.0
    # the same values with no quantile: +inf counts as 0 here and as 100 under the clamp
    _check_reduce(N, val.cuda(), mask.cuda(), -1, R.UNCLAMPED, 0)
    val, mask = _planted(900, 300, 4099, 150.0, extra=(INF, -INF, 250.0, -250.0, NAN), top=90.0)
    _check_reduce(N, val.cuda(), mask.cuda(), 0.98, R.CLAMPED, 902)


# ---------------------------------------------------------------------------------------- device-rank select
def test_kth_value_devrank_matches_the_host_rank_entry(N):
    import test_gpu_point_preparation as P
    g = torch.Generator().manual_seed(9)
    for n in (1, 257, 4099):
        x = torch.randn(n, generator=g)
        if n > 1:
            x[torch.rand(n, generator=g) < 0.1] = NAN
            x[::7] = x[3]
        xg = x.cuda()
        for k in P._ranks(n):
            want = N.kth_value(xg, k)
            got = N.kth_value_devrank(xg, torch.tensor(k, device="cuda"))
            assert torch.equal(_bits(got), _bits(want)), (n, k)
        for k in (0, n + 1, -3):
            assert int(_bits(N.kth_value_devrank(xg, torch.tensor(k, device="cuda")))) == 0x7fc00000, (n, k)


# ----------------------------------------------------------------------------------------------- end to end
def _depth_tolerances(case):
    """(loss tolerance, per-element gradient tolerance) of the depth term of a fixture case, from the values-stage
    bound: the mean of the bounds over the n set pixels scaled to the denominator, and bound / (p denom)."""
    key = case["tag"]
    pred, conf, gt, mask = _inputs(key)
    ref = _reference(key)
    v = ref["val"][mask]
    d = R.decide(v, case["valid_range"])
    if d["kind"] == R.SKIPPED:
        return 0.0, torch.zeros_like(ref["unit"])
    bound = ref["c"] * ref["unit"]
    return float(bound[mask].sum() / d["denom"]), bound / (pred.double().clamp_min(R.EPS32) * d["denom"])


@pytest.mark.parametrize("ci", range(5))
def test_multitask_loss_against_the_reference_fixture(N, ci):
    """Every key and every gradient of the fixture (the reference's own loss.py in fp64).  The torch-composed terms:
    1e-5 relative (fp32 against fp64, values of order 1; gradients relative to the largest entry of their tensor);
    the depth term: the values-stage bounds."""
    z, cases = R.golden()
    c = cases[ci]
    pred, batch = R.golden_case(c, device="cuda", dtype=torch.float32)
    loss, weights = R.golden_weights(c)
    torch.manual_seed(int(z["seed"]))
    out = loss(pred, batch, int(z["current_step"]))
    out["objective"].backward()
    torch.cuda.synchronize()
    ref = {k: float(z[f"{c['tag']}.loss.{k}"]) for k in out}
    dtol, dgrad_tol = _depth_tolerances(c)
    for k, v in out.items():
        tol = 1e-5 * abs(ref[k])
        if k == "loss_depth":
            tol = dtol + U * abs(ref[k])
        elif k == "objective":
            tol += weights["depth"] * dtol
        assert abs(float(v.detach()) - ref[k]) <= tol, (k, float(v.detach()), ref[k], tol)
    for k in R.GRAD_KEYS:
        want = torch.from_numpy(z[f"{c['tag']}.grad.{k}"])
        got = pred[k].grad.cpu().double() if pred[k].grad is not None else torch.zeros_like(want)
        if k == "depth":
            tol = weights["depth"] * dgrad_tol[..., None] + U * want.abs()
            assert torch.equal(got != 0, want != 0)
        else:
            tol = 1e-5 * want.abs().max()
        assert bool(((got - want).abs() <= tol).all()), (k, float((got - want).abs().max()))


def test_depth_loss_under_a_captured_graph(N):
    """No host synchronisation: forward and backward capture into one HIP graph and replay with new inputs."""
    from aligned_vggt.runtime import GraphedStep
    from aligned_vggt.training.loss import compute_depth_loss
    first, second = _inputs("filtered_b2"), _inputs("nan_thr")
    pred, conf, gt, mask = (t.cuda().clone() for t in first)
    pred = pred[..., None].requires_grad_(True)

    def step():
        pred.grad = None
        loss = compute_depth_loss({"depth": pred, "depth_conf": conf}, {"depths": gt, "point_masks": mask},
                                  valid_range=0.98)["loss_depth"]
        loss.backward()
        return loss.detach(), pred.grad

    graphed = GraphedStep(step, warmup=1)
    graphed()
    with torch.no_grad():
        for dst, src in zip((pred, conf, gt, mask), second):
            dst.copy_(src.view(dst.shape))
    loss, grad = graphed()
    torch.cuda.synchronize()
    loss, grad = loss.clone(), grad.clone()
    eager_loss, eager_grad = step()
    assert torch.equal(_bits(loss), _bits(eager_loss)) and torch.equal(_bits(grad), _bits(eager_grad))
    assert float(loss) > 0 and bool((grad != 0).any())


# -------------------------------------------------------------------------------------- through the model
def test_objective_through_the_model(N):
    """A train-mode toy-size FeatureAlignedVGGT chunk (as test_gpu_train.test_feature_aligned_training_step, whose
    set-up is inline there and cannot be imported):
    objective.backward() reaches the alignment head's parameters and nothing else, and with the depth term alone
    d chunk_scale = sum(d depth * depth_raw), the product ScaleFn's backward forms."""
    from aligned_vggt.models.featureAligned_vggt import FeatureAlignedVGGT
    from aligned_vggt.training.loss import MultitaskLoss
    from aligned_vggt.utils.synthetic import condition_pose_outputs_, synthetic_images, synthetic_init_
    # The model is built on the device and only the heads take the seeded host-side initialisation; the frozen
    # aggregator's matrices are drawn on the device (N(0, 0.02), as synthetic_init_ draws them): its output only has
    # to be finite here, and drawing a billion parameters on the host would be most of the test's time.
    with torch.device("cuda"):
        m = FeatureAlignedVGGT(enable_point=False, enable_track=False, num_memory_tokens=8)
    for part in (m.alignment_head, m.depth_head, m.camera_head):
        synthetic_init_(part, seed=11)
    with torch.no_grad():
        for p in m.aggregator.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.02)
    condition_pose_outputs_(m)
    m = m.cuda().train()
    m.alignment_head.drop_prob_nonoverlap = 0.0
    for name, p in m.named_parameters():
        p.requires_grad_(name.startswith("alignment_head."))
    S, H, W = 3, 42, 56
    imgs = synthetic_images(1, S, H, W, seed=5).cuda()
    enc = m.encode_chunk(imgs)
    depth_raw = enc["depth"].detach().clone()
    pred = m.align_chunk(enc, 1, None)
    depth, chunk = pred["depth"][0], pred["chunk_sim3_alignment_enc"]
    depth.retain_grad()
    chunk.retain_grad()
    g = torch.Generator().manual_seed(3)
    gt = (depth.detach()[..., 0].cpu() * torch.exp(0.3 * torch.randn(1, S, H, W, generator=g))).cuda()
    batch = {"depths": gt, "point_masks": (torch.rand(1, S, H, W, generator=g) < 0.8).cuda()}
    loss = MultitaskLoss(depth={"weight": 1.0, "valid_range": 0.98})
    loss.setupScheduling(10)
    out = loss({"depth": depth, "depth_conf": pred["depth_conf"][0]}, batch, 0)
    assert set(out) == {"loss_depth", "objective"} and float(out["loss_depth"].detach()) > 0
    assert bool(torch.isfinite(depth).all())
    out["objective"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert all(gr is None for n, gr in grads.items() if not n.startswith("alignment_head."))
    reached = [n for n, gr in grads.items() if gr is not None and bool((gr != 0).any())]
    assert reached and all(torch.isfinite(grads[n]).all() for n in reached)
    terms = depth.grad.double().cpu().reshape(1, -1) * depth_raw.double().cpu().reshape(1, -1)
    want, scale = terms.sum(-1), terms.abs().sum(-1)
    got = chunk.grad[..., 7].reshape(1).double().cpu()
    assert bool((got != 0).all())
    assert bool(((got - want).abs() <= terms.shape[1] * U * scale).all()), (got, want)  # an fp32 sum of n products
