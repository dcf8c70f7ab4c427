"""GT depth-scale alignment on the GPU (csrc/gt_align.hip, aligned_vggt/utils/alignment.py).

The kernel is held to the numpy oracle of test_gt_depth_scale.py in two stages.  Stage 1: the state's mean is within
1 fp32 ulp of the fsum mean (the kernel's fp64 sum of n terms is within n 2^-53 relative of the exact sum, then one
rounding to fp32).  Stage 2: with the state's own mean fed to the oracle, the scale, e, sum q, the selected key and
both cumulative sums are bitwise equal: everything after the mean is integer arithmetic on per-pixel fp32 values that
have one correctly rounded answer each."""
import copy
import functools

import numpy as np
import pytest
import torch

import test_gt_depth_scale as R

pytestmark = pytest.mark.gpu

F = np.float32
NAN, INF = float("nan"), float("inf")
SLICE = 256 * 16  # the pixels of one workgroup before the grid grows (GA_THREADS * GA_PER_THREAD)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------------------------------------- helpers
def _wide_inputs(B, n, seed, mask_p=0.7):
    """Ratios over many binades and both signs: all four radix digits vary.  (B, n) torch CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    y = 0.5 + 79.5 * torch.rand(B, n, generator=g)
    x = y * torch.exp(2.0 * torch.randn(B, n, generator=g))
    x = torch.where(torch.rand(B, n, generator=g) < 0.05, -x, x)
    conf = 1.0 + torch.exp(torch.randn(B, n, generator=g))
    mask = torch.rand(B, n, generator=g) < mask_p
    return x, conf, y, mask


def _offset_copy(t, dev):
    """A contiguous device copy whose first element sits one element past an allocation's start."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) == t.element_size()
    return v


def _run(N, x, conf, y, m, offset=False):
    dev = torch.device("cuda:0")
    put = (lambda t: _offset_copy(t, dev)) if offset else (lambda t: t.to(dev).contiguous())
    scales, state = N.depth_scale_l1(put(x), put(conf), put(y), put(m))
    assert scales.shape == (x.shape[0],) and scales.dtype == torch.float32 and scales.is_cuda
    return scales.cpu().numpy(), N.depth_scale_state(state)


def _check_against_oracle(N, x, conf, y, m, offset=False):
    """Both stages for every batch element; returns (scales, states, oracles)."""
    scales, states = _run(N, x, conf, y, m, offset)
    oracles = []
    for b in range(x.shape[0]):
        xb, cb, yb, mb = (t[b].numpy() for t in (x, conf, y, m))
        st = states[b]
        ref_mean = R.fsum_mean(yb, mb)
        print(f"b={b} n={xb.size} mean {st['mean']!r} fsum {float(ref_mean)!r} scale {scales[b]!r} e {st['e']} "
              f"total {st['total']}")
        assert abs(float(F(st["mean"])) - float(ref_mean)) <= float(np.spacing(np.abs(ref_mean))), (st, ref_mean)
        o = R.oracle(xb, cb, yb, mb, mean=F(st["mean"]))
        got = (R.bits(scales[b]), st["e"], st["total"], st["key"], st["below"], st["through"], st["cnt"],
               R.bits(st["wmax"]))
        want = (R.bits(o["scale"]), o["e"], o["total"], o["key"], o["below"], o["through"], o["cnt"], R.bits(o["wmax"]))
        assert got == want, (b, got, want)
        oracles.append(o)
    return scales, states, oracles


# ------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("B,n", [(1, 1), (1, 70), (1, SLICE - 1), (1, SLICE), (1, SLICE + 1), (1, 70003), (3, 4099),
                                 (3, 4100)],
                         ids=["n1", "n70", "slice-1", "slice", "slice+1", "n70k", "b3", "b3-wide"])
def test_kernel_matches_oracle(N, B, n):
    """b3: n % 4 != 0, the later elements start off a 16-byte boundary and the call reads element by element;
    b3-wide: n % 4 == 0, 128-bit loads at a non-zero element offset."""
    x, conf, y, m = _wide_inputs(B, n, seed=n)
    if B == 3:
        g = torch.Generator().manual_seed(9)
        m = torch.stack([torch.rand(n, generator=g) < p for p in (0.9, 0.5, 0.1)])  # a different mask each
    if n == 1:
        m[:] = True
    _, _, oracles = _check_against_oracle(N, x, conf, y, m)
    if n == 70003:  # all four digits of the key vary over the pixels that carry weight
        k = oracles[0]["keys"][oracles[0]["q"] > 0]
        assert all(len(np.unique((k >> s) & 0xff)) > 1 for s in (24, 16, 8, 0))


@pytest.mark.parametrize("B,n", [(1, 70), (2, 4099)], ids=["n70", "b2"])
def test_offset_pointers_take_the_scalar_path(N, B, n):
    x, conf, y, m = _wide_inputs(B, n, seed=77 + n)
    s_off, st_off, _ = _check_against_oracle(N, x, conf, y, m, offset=True)
    s, st = _run(N, x, conf, y, m)
    assert s.tobytes() == s_off.tobytes() and st == st_off  # the lane-to-pixel map does not depend on alignment


# ------------------------------------------------------------------------------------------------- decisions
def _realistic(n, seed):
    d, c, g, m = R.seeded_inputs((1, n), seed)
    return d, c, g, m


def test_every_ratio_equal(N):
    n = 333
    _, conf, _, m = _realistic(n, 1)
    x, y = torch.full((1, n), 2.0), torch.full((1, n), 3.0)
    scales, states, _ = _check_against_oracle(N, x, conf, y, m)
    assert scales[0] == F(1.5) and states[0]["below"] == 0 and states[0]["through"] == states[0]["total"] > 0


def test_mask_all_false_selects_the_smallest_ratio(N):
    n = 301
    x, conf, y, m = _realistic(n, 2)
    m[:] = False
    scales, states, o = _check_against_oracle(N, x, conf, y, m)
    assert states[0]["total"] == 0 and states[0]["cnt"] == 0 and states[0]["mean"] == 0.0
    assert scales[0] == F((y / x).min().item())
    x[0, 17] = -x[0, 17]  # the smallest ratio is now negative: it comes back negated
    scales, states, o = _check_against_oracle(N, x, conf, y, m)
    assert o[0]["r"] < 0 and scales[0] == -o[0]["r"] and scales[0] == F(-(y / x).min().item())


def test_negative_and_zero_predictions(N):
    n = 1001
    x, conf, y, m = _realistic(n, 3)
    x[0, ::3] *= -1.0
    x[0, 5::7] = 0.0
    x[0, 6::49] = -0.0
    _check_against_oracle(N, x, conf, y, m)
    m[:] = True
    x[:] = -x.abs().clamp_min(0.5)  # every prediction negative: every ratio negative, the scale positive
    scales, _, o = _check_against_oracle(N, x, conf, y, m)
    assert o[0]["r"] < 0 and scales[0] > 0


def test_gt_below_min_depth(N):
    n = 1001
    x, conf, y, m = _realistic(n, 4)
    y[0, ::4] = 0.01      # far below 0.1 * mean: the weight's denominator is min_depth
    y[0, 1::16] = 1e-9    # below 1e-6 too
    y[0, 2::16] = 0.0
    _, states, o = _check_against_oracle(N, x, conf, y, m)
    assert 0.1 * states[0]["mean"] > 0.5


def test_boundary_takes_the_left_ratio(N):
    one = torch.ones(1, 2)
    scales, states, _ = _check_against_oracle(N, one, torch.tensor([[1.0, 2.0]]), torch.tensor([[1.0, 2.0]]),
                                              torch.ones(1, 2, dtype=torch.bool))
    assert scales[0] == F(1.0) and states[0]["e"] == 36 and states[0]["total"] == 2 ** 37
    assert states[0]["below"] == 0 and states[0]["through"] == 2 ** 36


def test_one_dominant_weight(N):
    n = 777
    x, conf, y, m = _realistic(n, 5)
    m[0, 400] = True
    conf[0, 400] = 1e6
    scales, _, o = _check_against_oracle(N, x, conf, y, m)
    assert scales[0] == o[0]["ratios"][400]


def test_non_finite_weights_count_as_zero(N):
    n = 1500
    x, conf, y, m = _realistic(n, 6)
    m[0, 100] = m[0, 200] = True
    x0, c0 = x.clone(), conf.clone()
    c0[0, 100] = 0.0       # the same mean, wmax and total, with the two pixels' weight 0 by their confidence
    c0[0, 200] = 0.0
    conf[0, 100] = NAN
    x[0, 200] = INF
    scales, states, o = _check_against_oracle(N, x, conf, y, m)
    assert np.isnan(o[0]["w_eff"][100]) and np.isinf(o[0]["w_eff"][200]) and o[0]["q"][100] == o[0]["q"][200] == 0
    s0, st0, _ = _check_against_oracle(N, x0, c0, y, m)
    assert s0.tobytes() == scales.tobytes() and st0 == states


def test_weights_spanning_more_than_2_36(N):
    n = 2000
    x, conf, y, m = _realistic(n, 7)
    conf[0, ::2] *= 1e-13
    _, states, o = _check_against_oracle(N, x, conf, y, m)
    small = (o[0]["w_eff"] > 0) & (o[0]["q"] == 0)
    assert small.sum() > 100 and float(o[0]["w_eff"].max()) / float(o[0]["w_eff"][small].max()) > 2.0 ** 36


# ------------------------------------------------------------------------------------------------- independence
def test_batch_elements_are_independent_and_runs_repeat(N):
    B, n = 3, 9001
    x, conf, y, m = _wide_inputs(B, n, seed=11)
    s, st = _run(N, x, conf, y, m)
    s2, st2 = _run(N, x, conf, y, m)
    assert s.tobytes() == s2.tobytes() and st == st2
    for b in range(B):
        sb, stb = _run(N, x[b:b + 1], conf[b:b + 1], y[b:b + 1], m[b:b + 1])
        assert sb.tobytes() == s[b:b + 1].tobytes() and stb[0] == st[b]


# ------------------------------------------------------------------------------------------------- real weights
def test_distance_from_the_real_weight_median(N):
    """q_i = w_i 2^e + eps_i with |eps_i| <= 1/2.  The select gives 2 Q_<=(r*) >= Q and 2 Q_<(r*) < Q.  With
    Q_<= = 2^e W_<= + E1 and Q = 2^e 2T + E2, |E1|, |E2| <= N / 2:  W_<= >= T + (E2 / 2 - E1) 2^-e >= T - (3/4) N 2^-e,
    and likewise W_< < T + (3/4) N 2^-e.  ldexp(wmax, e) > 2^35 gives 2^-e < wmax 2^-35, so the distance is below
    delta = 1.5 N wmax 2^-36: half a unit per weight on the cumulative sum plus half of that on the total."""
    n = 2 * 37 * 53 * 9
    x, conf, y, m = _realistic(n, 12)
    scales, states, o = _check_against_oracle(N, x, conf, y, m)
    o = o[0]
    w = R.valid_weights(o["w_eff"]).astype(np.float64)
    r = o["ratios"]
    T = 0.5 * w.sum()
    delta = 1.5 * n * float(o["wmax"]) * 2.0 ** -36
    w_lt, w_le = w[r < o["r"]].sum(), w[r <= o["r"]].sum()
    print("T", T, "delta", delta, "W_<", w_lt, "W_<=", w_le)
    assert w_lt < T + delta and w_le >= T - delta


# ------------------------------------------------------------------------------------------------- python path
def _to_dev(d):
    return {k: (v.to("cuda:0") if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _step(seed=0):
    depth, conf, gt, mask = R.seeded_inputs(R.SHAPE, seed)
    pred = R.predictions_of(depth, conf, seed)
    return pred, {"depths": gt, "point_masks": mask}


def _cpu_result(seed=0):
    from aligned_vggt.utils import alignment as A
    pred, batch = _step(seed)
    pred = copy.deepcopy(pred)
    A.scale_align_from_depths(pred, batch)
    return pred


def test_python_device_path_matches_cpu(N):
    from aligned_vggt.utils import alignment as A
    pred, batch = _step()
    ref = _cpu_result()
    p = _to_dev(copy.deepcopy(pred))
    A.scale_align_from_depths(p, _to_dev(batch))
    sc = p["alignment_scales"]
    assert isinstance(sc, list) and len(sc) == R.SHAPE[0]
    assert all(isinstance(s, torch.Tensor) and s.is_cuda and s.dim() == 0 and s.dtype == torch.float32 for s in sc)
    assert [R.bits(s.item()) for s in sc] == [R.bits(s) for s in ref["alignment_scales"]]
    assert torch.tensor(sc).mean().item() == pytest.approx(float(np.mean(ref["alignment_scales"])), rel=1e-6)
    for k in ("depth", "world_points", "pose_enc"):
        torch.testing.assert_close(p[k].cpu(), ref[k], rtol=1e-6, atol=0)
    assert torch.equal(p["depth_conf"].cpu(), pred["depth_conf"])


def test_python_device_path_non_contiguous_inputs(N):
    from aligned_vggt.utils import alignment as A
    pred, batch = _step()
    ref = _cpu_result()
    p, b = _to_dev(copy.deepcopy(pred)), _to_dev(batch)
    p["depth_conf"] = p["depth_conf"].transpose(2, 3).contiguous().transpose(2, 3)
    b["depths"] = b["depths"].transpose(2, 3).contiguous().transpose(2, 3)
    assert not p["depth_conf"].is_contiguous()
    A.scale_align_from_depths(p, b)
    assert [R.bits(s.item()) for s in p["alignment_scales"]] == [R.bits(s) for s in ref["alignment_scales"]]


def test_python_device_path_keeps_the_graph(N):
    from aligned_vggt.utils import alignment as A
    pred, batch = _step()
    p = _to_dev(copy.deepcopy(pred))
    leaf = p["depth"].clone().requires_grad_(True)
    p["depth"] = leaf * 1.0
    A.scale_align_from_depths(p, _to_dev(batch))
    scale = torch.stack(p["alignment_scales"])
    assert not scale.requires_grad and p["depth"].requires_grad
    g = torch.randn(p["depth"].shape, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    (p["depth"] * g).sum().backward()
    assert torch.equal(leaf.grad, g * scale.view(-1, 1, 1, 1, 1))
    torch.testing.assert_close(p["depth"].detach(), leaf.detach() * scale.view(-1, 1, 1, 1, 1), rtol=1e-6, atol=0)


def _parent_chain(predictions, batch):
    """The torch chain as it stood before the kernel path, op for op."""
    with torch.no_grad():
        d_pred, conf, d_gt, mask = predictions["depth"], predictions["depth_conf"], batch["depths"], batch["point_masks"]
        B, S, H, W, _ = d_pred.shape
        n = S * H * W
        x = d_pred.reshape(B, n).float()
        y = d_gt.reshape(B, n).float()
        m = mask.reshape(B, n).float()
        w_conf = conf.reshape(B, n).float()
        sum_valid = m.sum(dim=-1, keepdim=True).clamp_min(1.0)
        mean_depth = (y * m).sum(dim=-1, keepdim=True) / sum_valid
        y_clamped = torch.max(y, 0.1 * mean_depth)
        w = m * w_conf * (1.0 / y_clamped.clamp_min(1e-6))
        sign = torch.sign(x)
        sign = torch.where(sign == 0, torch.ones_like(sign), sign)
        x_pos, y_pos = x * sign, y * sign
        r = y_pos / x_pos.clamp_min(1e-6)
        w_eff = w * x_pos
        r_sorted, idx = torch.sort(r, dim=-1)
        cumsum = torch.gather(w_eff, -1, idx).cumsum(-1)
        idx_med = torch.searchsorted(cumsum, 0.5 * cumsum[:, -1:], side="left").clamp(max=n - 1)
        scales = torch.gather(r_sorted, -1, idx_med).squeeze(-1)
        scales[scales <= 0] *= -1
        predictions["depth"] *= scales[:, None, None, None, None]
        predictions["world_points"] *= scales[:, None, None, None, None]
        predictions["pose_enc"][..., :3] *= scales[:, None, None]
        predictions["alignment_scales"] = [scales[b].item() for b in range(B)]


def test_knob_runs_the_parent_chain_bitwise(N, monkeypatch):
    from aligned_vggt.utils import alignment as A
    pred, batch = _step()
    want = _to_dev(copy.deepcopy(pred))
    _parent_chain(want, _to_dev(batch))
    monkeypatch.setenv("VGGT_GT_ALIGN", "torch")
    got = _to_dev(copy.deepcopy(pred))
    A.scale_align_from_depths(got, _to_dev(batch))
    assert got["alignment_scales"] == want["alignment_scales"] and isinstance(got["alignment_scales"][0], float)
    for k in ("depth", "world_points", "pose_enc"):
        assert torch.equal(got[k], want[k])


def test_kernel_path_does_not_synchronise(N, monkeypatch):
    from aligned_vggt.utils import alignment as A
    monkeypatch.delenv("VGGT_GT_ALIGN", raising=False)
    pred, batch = _step()
    b = _to_dev(batch)
    A.scale_align_from_depths(_to_dev(copy.deepcopy(pred)), b)  # the library is loaded, the allocator is warm
    p = _to_dev(copy.deepcopy(pred))
    p["depth_conf"] = p["depth_conf"].transpose(2, 3).contiguous().transpose(2, 3)  # made contiguous inside
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        A.scale_align_from_depths(p, b)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert [R.bits(s.item()) for s in p["alignment_scales"]] == [R.bits(s) for s in _cpu_result()["alignment_scales"]]


# ------------------------------------------------------------------------------------------------- merged chunks
def test_align_and_convert_outputs_on_device_chunks(N):
    from aligned_vggt.utils.data import alignAndConvertOutputs
    overlap = 1
    chunks = []
    for seed in (20, 21):
        depth, conf, gt, mask = R.seeded_inputs((2, 3, 21, 29), seed)
        p = R.predictions_of(depth, conf, seed)
        chunks.append((p, gt, mask))

    def run(dev):
        preds = {k: [c[0][k].clone().to(dev) for c in chunks] for k in ("depth", "depth_conf", "world_points", "pose_enc")}
        chunked = {"depths": [c[1].clone().to(dev) for c in chunks], "point_masks": [c[2].clone().to(dev) for c in chunks]}
        batch = {}
        alignAndConvertOutputs(preds, batch, chunked, "scale_from_depths", 3, overlap)
        return preds, batch

    ref, ref_batch = run("cpu")
    got, got_batch = run("cuda:0")
    assert got["depth"].shape == (2, 5, 21, 29, 1) and got["depth"].is_cuda
    assert torch.equal(got_batch["depths"].cpu(), ref_batch["depths"])
    assert [R.bits(s.item()) for s in got["alignment_scales"]] == [R.bits(s) for s in ref["alignment_scales"]]
    for k in ("depth", "world_points", "pose_enc"):
        torch.testing.assert_close(got[k].cpu(), ref[k], rtol=1e-6, atol=0)
