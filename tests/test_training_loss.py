"""aligned_vggt.training.loss without a device: the warm-up schedule, the argument rules, and an fp64 torch
restatement of all five terms (`restated_losses`) that reproduces tests/golden/multitask_loss.npz -- the reference's
own training/loss.py run in fp64 (tests/golden/gen_loss.py) -- in values and gradients.  The GPU tests
(test_gpu_training_loss.py) lean on this restatement and on `decide` / `chosen_terms`, the depth term's branch taken
with torch on a vector of values."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from aligned_vggt.utils.pose_enc import pose_encoding_to_extri_intri
from aligned_vggt.utils.rotation import mat_to_quat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multitask_loss.npz")
F64 = torch.float64
EPS32 = float(np.float32(1e-8))  # clamp_min(1e-8) on an fp32 tensor clamps at the fp32 value
SKIPPED, FILTERED, CLAMPED, UNCLAMPED = 0, 1, 2, 3
GRAD_KEYS = ("depth", "pose_enc", "frame_se3_alignment_enc", "chunk_sim3_alignment_enc")


# ---------------------------------------------------------------------------------------- the restatement
def fix(t, hard_max=100):
    t = torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    return t if hard_max is None else t.clamp(min=-hard_max, max=hard_max)


def depth_values64(pred, conf, gt, mask):
    """val over (B, S, H, W) in fp64 (NaN at unset pixels), the normalised confidence and the two logs."""
    pred, conf, gt = pred.to(F64), conf.to(F64), gt.to(F64)
    g = fix(gt, None)
    cn = conf / conf.amax(dim=(2, 3), keepdim=True).clamp_min(EPS32)
    lp, lg = torch.log(pred.clamp_min(EPS32)), torch.log(g.clamp_min(EPS32))
    val = (lp - lg).abs() * cn
    return torch.where(mask, val, torch.full_like(val, float("nan"))), cn, lp, lg


def quantile_rank(n, q):
    return round(q * (n - 1)) + 1


def decide(v, valid_range):
    """The reference's branches (compute_depth_loss, filter_by_quantile) on the 1-D tensor `v` of the set pixels'
    values: n, the rank k (0: no quantile), thr' (NaN then), m and the case."""
    n = v.numel()
    d = {"n": n, "k": 0, "m": 0, "thr": float("nan"), "kind": UNCLAMPED}
    if n < 100:
        d["kind"] = SKIPPED
    elif valid_range > 0 and n > 1000:
        c = v.detach().clamp(max=100)
        d["k"] = quantile_rank(n, float(valid_range))
        thr = torch.kthvalue(c, d["k"]).values
        d["thr_t"] = thr = torch.full_like(thr, 100.0) if 100 < thr else thr  # min(thr, 100); a NaN stays
        d["thr"] = float(thr)
        d["m"] = int((c < thr).sum())
        d["kind"] = FILTERED if d["m"] > 1000 else CLAMPED
    d["denom"] = {SKIPPED: 0, FILTERED: d["m"]}.get(d["kind"], n)
    return d


def chosen_mask(v, d):
    """Which entries of `v` enter the mean."""
    if d["kind"] == SKIPPED:
        return torch.zeros_like(v, dtype=torch.bool)
    if d["kind"] == FILTERED:
        return v.detach().clamp(max=100) < d["thr_t"]
    return torch.ones_like(v, dtype=torch.bool)


def chosen_terms(v, d, keep=None):
    """The terms whose mean is the loss (differentiable in `v`); None when skipped.  `keep`: the entries that
    enter, decided elsewhere (on the fp32 values, when `v` is their fp64 evaluation)."""
    if d["kind"] == SKIPPED:
        return None
    c = v if d["kind"] == UNCLAMPED else v.clamp(max=100)
    return fix(c[chosen_mask(v, d) if keep is None else keep])


def depth_loss64(pred, conf, gt, mask, valid_range):
    val = depth_values64(pred, conf, gt, mask)[0]
    v = val[mask]
    terms = chosen_terms(v, decide(v, valid_range))
    return (0.0 * pred).mean() if terms is None else terms.mean()


def _relative_poses64(extr, offset=1):
    B, S = extr.shape[:2]
    w2c = torch.eye(4, dtype=F64).repeat(B, S, 1, 1)
    w2c[:, :, :3, :4] = extr
    return (w2c[:, offset:] @ torch.inverse(w2c)[:, :-offset])[:, :, :3, :4]


def _unit(q):
    return q / q.norm(dim=-1, keepdim=True).clamp(min=1e-8)


def restated_losses(pred, batch, cfg, weights, large_offset):
    """The five terms and the objective in fp64, l1 form; `weights[name]` is the warm-up weight of config `name`."""
    out = {}
    enc = pred["frame_se3_alignment_enc"].reshape(-1, 7)
    out["loss_per_frame_reg"] = fix(enc[:, :3].norm(dim=-1, keepdim=True)).clamp(max=100).mean() + \
        fix((1 - _unit(enc[:, 3:7])[:, -1] ** 2).abs()).mean()
    enc = pred["chunk_sim3_alignment_enc"]
    out["loss_per_chunk_reg"] = fix(enc[..., :3].norm(dim=-1, keepdim=True)).clamp(max=100).mean() + \
        fix((1 - _unit(enc[..., 3:7])[..., -1] ** 2).abs()).mean() + fix(torch.log(enc[..., 7].clamp_min(1e-6)) ** 2).mean()
    mask = batch["point_masks"]
    out["loss_depth"] = depth_loss64(pred["depth"][..., 0], pred["depth_conf"], batch["depths"], mask,
                                     cfg["depth"]["valid_range"])
    ok = bool(((mask[:, 0].sum(dim=[-1, -2]) > 100).sum() != 0))
    pe, extr, intr = pred["pose_enc"], batch["extrinsics"], batch["intrinsics"]
    zero = (pe * 0).mean()
    H, W = mask.shape[-2:]
    gt_enc = torch.cat([extr[..., :3, 3], mat_to_quat(extr[..., :3, :3]), 2 * torch.atan((H / 2) / intr[..., 1:2, 1]),
                        2 * torch.atan((W / 2) / intr[..., 0:1, 0])], -1)
    out["loss_T"] = fix((pe[..., :3] - gt_enc[..., :3]).abs()).clamp(max=100).mean() if ok else zero
    out["loss_R"] = fix((pe[..., 3:7] - gt_enc[..., 3:7]).abs()).mean() if ok else zero
    out["loss_camera"] = out["loss_T"] + out["loss_R"]
    if ok:
        pextr = pose_encoding_to_extri_intri(pe, build_intrinsics=False)[0]
        g = torch.cat((_relative_poses64(extr), _relative_poses64(extr, large_offset)), 1)
        p = torch.cat((_relative_poses64(pextr), _relative_poses64(pextr, large_offset)), 1)
        out["loss_T_rel"] = fix((p[..., :3, 3] - g[..., :3, 3]).abs()).clamp(max=100).mean()
        out["loss_R_rel"] = fix((mat_to_quat(p[..., :3, :3]) - mat_to_quat(g[..., :3, :3])).abs()).mean()
        c = cfg["cameraPoseRel"]
        out["loss_camera_rel"] = c["weight_trans"] * out["loss_T_rel"] + c["weight_rot"] * out["loss_R_rel"]
    else:
        out["loss_T_rel"] = out["loss_R_rel"] = out["loss_camera_rel"] = zero
    out["objective"] = 0
    for key, name in (("loss_per_frame_reg", "perFrameReg"), ("loss_per_chunk_reg", "perChunkReg"),
                      ("loss_depth", "depth"), ("loss_camera", "cameraPose"), ("loss_camera_rel", "cameraPoseRel")):
        out["objective"] = out["objective"] + out[key] * weights[name]
    return out


# ------------------------------------------------------------------------------------------------ fixture
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))


def golden_case(case, device="cpu", dtype=F64):
    """(predictions with requires_grad, batch) of one fixture case."""
    z, _ = golden()
    t = lambda k: torch.from_numpy(z[f"{case['tag']}.in.{k}"])  # noqa: E731
    f = lambda k: t(k).to(device=device, dtype=dtype)  # noqa: E731
    pred = {k: f(k).requires_grad_(k in GRAD_KEYS) for k in GRAD_KEYS + ("depth_conf",)}
    B, S, H, W = case["shape"]
    batch = {"depths": f("depths"), "point_masks": t("point_masks").to(device), "extrinsics": f("extrinsics"),
             "intrinsics": f("intrinsics"), "images": torch.zeros(B, S, 3, H, W, device=device)}
    return pred, batch


def golden_weights(case):
    from aligned_vggt.training.loss import MultitaskLoss
    z, _ = golden()
    loss = MultitaskLoss(**case["config"])
    loss.setupScheduling(int(z["total_steps"]))
    return loss, {k: loss.compute_warmup_weight(v, int(z["current_step"])) for k, v in case["config"].items()}


def test_fixture_covers_the_depth_branches():
    z, cases = golden()
    kinds = {}
    for c in cases:
        pred, batch = golden_case(c)
        v = depth_values64(pred["depth"][..., 0].detach(), pred["depth_conf"], batch["depths"], batch["point_masks"])[0]
        d = decide(v[batch["point_masks"]], c["valid_range"])
        assert d["n"] == c["n"]
        kinds[c["tag"]] = (d["kind"], d["m"])
    assert kinds == {"skipped": (SKIPPED, 0), "unfiltered": (CLAMPED, 985), "filtered": (FILTERED, 1014),
                     "filtered_b2": (FILTERED, kinds["filtered_b2"][1]), "no_range": (UNCLAMPED, 0)}
    assert kinds["filtered_b2"][1] > 1000


@pytest.mark.parametrize("ci", range(5))
def test_restatement_reproduces_the_reference(ci):
    z, cases = golden()
    c = cases[ci]
    pred, batch = golden_case(c)
    _, weights = golden_weights(c)
    out = restated_losses(pred, batch, c["config"], weights, int(z[f"{c['tag']}.large_offset"]))
    out["objective"].backward()
    for k, v in out.items():
        ref = float(z[f"{c['tag']}.loss.{k}"])
        assert abs(float(v.detach()) - ref) <= 1e-12 * max(1.0, abs(ref)), (k, float(v.detach()), ref)
    for k in GRAD_KEYS:
        ref = torch.from_numpy(z[f"{c['tag']}.grad.{k}"])
        got = pred[k].grad if pred[k].grad is not None else torch.zeros_like(ref)
        assert torch.allclose(got, ref, rtol=1e-10, atol=1e-13), (k, (got - ref).abs().max().item())


# ------------------------------------------------------------------------------------------------ warm-up
def _loss(**kw):
    from aligned_vggt.training.loss import MultitaskLoss
    m = MultitaskLoss(**kw)
    m.setupScheduling(200)
    return m


def test_warmup_weights_linear_and_exp():
    cfg = {"weight": 2.0, "warmup_percent": 0.25, "warmup_start_percent": 0.1, "warmup_start_weight": 0.5}
    lin = _loss()
    lcfg = dict(cfg, warmup_type="linear")
    exp = _loss(weight_warmup_exp=3.0)
    # start step 20, 50 warm-up steps
    assert lin.compute_warmup_weight(lcfg, 19) == 0.0 and exp.compute_warmup_weight(cfg, 0) == 0.0  # before the start
    assert lin.compute_warmup_weight(lcfg, 71) == 2.0 and exp.compute_warmup_weight(cfg, 199) == 2.0  # after it
    for step in (20, 33, 45, 70):
        f = min(1.0, (step - 20) / 50)
        assert lin.compute_warmup_weight(lcfg, step) == 0.5 + 1.5 * f
        assert exp.compute_warmup_weight(cfg, step) == 0.5 + 1.5 * f ** 3.0  # "exp" is the default type
    assert lin.compute_warmup_weight({"weight": 0.7}, 0) == 0.7  # no warmup_percent
    assert lin.compute_warmup_weight({"weight": 0.7, "warmup_type": "linear", "warmup_start_percent": 0.5}, 3) == 0.7
    assert lin.compute_warmup_weight({"weight": 3.0, "warmup_percent": 0.5, "warmup_type": "linear"}, 25) == 0.75
    with pytest.raises(ValueError, match="weight_warmup_exp"):
        lin.compute_warmup_weight(cfg, 30)
    with pytest.raises(ValueError, match="warmup type"):
        lin.compute_warmup_weight(dict(cfg, warmup_type="cosine"), 30)


def test_check_and_fix_inf_nan():
    from aligned_vggt.training.loss import check_and_fix_inf_nan
    x = torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), 250.0, -250.0], requires_grad=True)
    y = check_and_fix_inf_nan(x, "x")
    assert y.tolist() == [1.0, 0.0, 0.0, 0.0, 100.0, -100.0]
    y.sum().backward()
    assert x.grad.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert check_and_fix_inf_nan(x.detach(), hard_max=None).tolist() == [1.0, 0.0, 0.0, 0.0, 250.0, -250.0]
    assert check_and_fix_inf_nan(0.0) == 0.0


def test_depth_loss_argument_rules():
    from aligned_vggt.training.loss import compute_depth_loss
    shape = (1, 2, 4, 5)
    pred = {"depth": torch.ones(*shape, 1), "depth_conf": torch.ones(shape)}
    batch = {"depths": torch.ones(shape), "point_masks": torch.ones(shape, dtype=torch.bool)}
    with pytest.raises(RuntimeError, match="HIP devices only"):
        compute_depth_loss(pred, batch, valid_range=0.98)
    pred["depth_conf"].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="depth_conf"):
        compute_depth_loss(pred, batch)


def test_entries_in_header_library_and_bindings():
    from aligned_vggt import _native as N
    names = {"vggt_depth_loss_values", "vggt_depth_loss_reduce", "vggt_depth_loss_bwd", "vggt_kth_value_f32_devrank"}
    header = open(N.HEADER_PATH).read()
    assert "Training losses" in header
    assert names <= set(N._SIGS) and "vggt_depth_loss_ws_bytes" in N._WS_FNS
    assert all(n + "(" in header for n in names | {"vggt_depth_loss_ws_bytes"})
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built")
    N.lib()  # binds every name, so all are exported
    assert N.depth_loss_ws_bytes(0, 1, 1, 1) == 0
    assert N.depth_loss_ws_bytes(1, 1, 10001, 10000) == 0  # past 10^8 elements: unsupported
    small, big = N.depth_loss_ws_bytes(1, 2, 14, 37), N.depth_loss_ws_bytes(1, 16, 518, 518)
    assert 0 < small <= big < 1 << 20 and small % 8 == 0
    assert big - small == 48  # only the per-frame keys grow (16-byte granules)
