"""CPU checks of the metrics module (aligned_vggt/training/training_metrics.py) and what it
calls: ScaleConsistency, the metrics' plot(), log_additional_data and the GT normalisation
against tests/golden/ref_metrics.npz, produced by the reference's own bodies
(tests/golden/gen_metrics.py); the hydra-free construction, the sequence gathering and the
files plot() writes without a fixture.

The fixture values are fp32 results of the same torch operations in the same order; the
tolerances (rtol 1e-6 for sums of a few dozen terms, 2e-5 for the RPE chain of three 4x4
inverses, as test_eval_alignment.py) leave room for another box's summation order only."""
import os

import numpy as np
import pytest
import torch

from aligned_vggt.eval import AbsoluteTrajectoryError, RelativePoseError, ScaleConsistency
from aligned_vggt.training import training_metrics as TM
from aligned_vggt.utils.data import check_valid_tensor, normalize_camera_extrinsics_and_points_batch


def _traj(g, i):
    return torch.from_numpy(g[f"traj{i}.pred"]), torch.from_numpy(g[f"traj{i}.gt"])


def test_scale_consistency_matches_reference(golden):
    g = golden("ref_metrics")
    m = ScaleConsistency()
    assert m.compute() == {"scale_var": 0.0}
    for i in range(3):
        pred, gt = _traj(g, i)
        m.update(pred, gt)
        d, path = m.plot(pred, gt, title=f"traj {i}")
        assert list(d) == ["scale_var"] and isinstance(d["scale_var"], torch.Tensor) and d["scale_var"].dim() == 0
        assert path == "Nonetraj_scale_cons.png"  # the reference formats its missing outpath the same way
        np.testing.assert_allclose(d["scale_var"].numpy(), g[f"traj{i}.scale_plot.scale_var"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m.var_sum.numpy(), g["scale.var_sum"], rtol=1e-6)
    assert int(m.count) == int(g["scale.count"]) == 3
    out = m.compute()
    assert list(out) == ["scale_var"]
    np.testing.assert_allclose(out["scale_var"].numpy(), g["scale.compute.scale_var"], rtol=1e-6)
    m.reset()
    assert float(m.var_sum) == 0.0 and int(m.count) == 0
    m.sync()  # no process group: a no-op


def test_ate_rpe_plot_dicts_match_reference(golden):
    g = golden("ref_metrics")
    for i in range(3):
        pred, gt = _traj(g, i)
        d, path = AbsoluteTrajectoryError().plot(pred, gt)
        assert list(d) == ["ate_rmse"] and isinstance(d["ate_rmse"], float) and path.endswith("traj_ate.png")
        np.testing.assert_allclose(d["ate_rmse"], g[f"traj{i}.ate_plot.ate_rmse"], rtol=1e-6)
        for delta in (1, 3):
            d, path = RelativePoseError(delta=delta).plot(pred, gt, title="t")
            assert list(d) == ["rpe_trans_rmse", "rpe_rot_rmse"] and path.endswith("traj_rpe.png")
            for k in d:
                np.testing.assert_allclose(d[k], g[f"traj{i}.rpe_plot{delta}.{k}"], rtol=2e-5, atol=1e-6)
    pred, gt = _traj(g, 2)
    d, _ = RelativePoseError(delta=5).plot(pred, gt)  # N <= delta: compute()'s empty-state values
    assert d == {"rpe_trans_rmse": 0.0, "rpe_rot_rmse": 0.0}


def test_log_additional_data_matches_reference(golden):
    g = golden("ref_metrics")
    pred = {"alignment_scales_per_chunk": [torch.from_numpy(a) for a in g["log.in.alignment_scales_per_chunk"]],
            "alignment_scales": [float(v) for v in g["log.in.alignment_scales"]],
            "frame_se3_alignment_enc": torch.from_numpy(g["log.in.frame_se3_alignment_enc"]),
            "chunk_sim3_alignment_enc": torch.from_numpy(g["log.in.chunk_sim3_alignment_enc"]),
            "memory_tokens": [torch.from_numpy(a) for a in g["log.in.memory_tokens"]]}
    out = {}
    TM.log_additional_data(pred, out)
    want = {k[len("log.out."):]: float(g[k]) for k in g if k.startswith("log.out.")}
    assert len(want) == 9 and list(out) == list(want)  # every key the reference writes, in its order
    for k, v in want.items():
        assert isinstance(out[k], float)
        np.testing.assert_allclose(out[k], v, rtol=1e-6, atol=1e-8, err_msg=k)
    assert "memory_tokens" not in pred
    # the kernel route's scales are tensors: same mean
    out2 = {}
    TM.log_additional_data({"alignment_scales": [torch.tensor(v) for v in g["log.in.alignment_scales"]]}, out2)
    np.testing.assert_allclose(out2["avg_alignment_scale"], want["avg_alignment_scale"], rtol=1e-6)
    out3 = {}
    TM.log_additional_data({"chunk_sim3_alignment_enc": pred["chunk_sim3_alignment_enc"][..., :7]}, out3)
    assert "avg_per_chunk_scale" not in out3 and len(out3) == 2


@pytest.mark.parametrize("scale_by_points", [False, True])
def test_normalize_extrinsics_and_points_matches_reference(golden, scale_by_points):
    g = golden("ref_metrics")
    x = {k[len("norm.in."):]: torch.from_numpy(g[k]) for k in g if k.startswith("norm.in.")}
    before = {k: v.clone() for k, v in x.items()}
    got = normalize_camera_extrinsics_and_points_batch(**x, scale_by_points=scale_by_points)
    for name, t in zip(("extrinsics", "cam_points", "world_points", "depths"), got):
        want = g[f"norm.out{int(scale_by_points)}.{name}"]
        assert tuple(t.shape) == want.shape and t.dtype == torch.float32
        np.testing.assert_allclose(t.numpy(), want, rtol=1e-6, atol=1e-6, err_msg=name)
    assert got[0].shape[-2:] == (3, 4)
    for k in x:
        assert torch.equal(x[k], before[k]), k  # inputs untouched
    # the first camera becomes the identity
    np.testing.assert_allclose(got[0][:, 0, :, :3].numpy(), np.broadcast_to(np.eye(3), (2, 3, 3)), atol=1e-6)


def test_check_valid_tensor_warns(caplog):
    with caplog.at_level("WARNING"):
        check_valid_tensor(torch.ones(3), "fine")
        check_valid_tensor(None, "absent")
    assert not caplog.records
    with caplog.at_level("WARNING"):
        check_valid_tensor(torch.tensor([1.0, float("inf")]), "depths")
    assert "depths" in caplog.text


def _metrics(**kw):
    args = dict(mode="test", overlap=[2], chunk_width=[4], gt_alignment_type="scale_from_poses",
                full_seq_sample_mode="chunk_overlap")
    args.update(kw)
    return TM.Metrics(**args)


def test_metrics_builds_from_target_mappings_without_hydra():
    ready = AbsoluteTrajectoryError(detailed=True)
    m = _metrics(trajectory_metrics=[{"_target_": "eval.trajectory_metrics.AbsoluteTrajectoryError"},
                                     {"_target_": "eval.trajectory_metrics.RelativePoseError", "delta": 3},
                                     {"_target_": "aligned_vggt.eval.trajectory_metrics.ScaleConsistency"}, ready],
                 reconstruction_metrics=[{"_target_": "eval.reconstruction_metrics.ChamferDistanceMetrics",
                                          "norm": 1, "rmse": False}],
                 some_future_keyword=1)
    assert isinstance(m, torch.nn.Module)
    assert [type(x).__name__ for x in m.trajectory_metrics] == ["AbsoluteTrajectoryError", "RelativePoseError",
                                                                "ScaleConsistency", "AbsoluteTrajectoryError"]
    assert m.trajectory_metrics[1].delta == 3 and m.trajectory_metrics[3] is ready
    assert type(m.trajectory_metrics[0]).__module__ == "aligned_vggt.eval.trajectory_metrics"
    c = m.reconstruction_metrics[0]
    assert type(c).__name__ == "ChamferDistanceMetrics" and c.norm == 1 and c.rmse is False
    assert m.sequence_outputs == "device" and m.num_overlap == [2] and m.log_dir is None
    assert _metrics(sequence_outputs="host").sequence_outputs == "host"
    assert _metrics().trajectory_metrics == [] and _metrics().reconstruction_metrics == []
    other = _metrics(trajectory_metrics=[{"_target_": "collections.OrderedDict", "a": 1}])
    assert other.trajectory_metrics[0] == {"a": 1}  # any other dotted path is imported as given
    with pytest.raises(NotImplementedError, match="viser"):
        _metrics(visualize=True)
    with pytest.raises(ValueError):
        _metrics(sequence_outputs="disk")


class _ToyDataset:
    """What gather_sequences / get_sequence_data read of a dataset."""

    def __init__(self, lengths, H=4, W=6, seed=0):
        self.seq_frame_num = list(lengths)
        self.sequence_list_len = len(lengths)
        self.H, self.W, self.seed = H, W, seed
        self.calls = []

    def get_seq_name(self, i):
        return f"seq{i}"

    def get_data(self, seq_index, img_per_seq, seq_name, ids):
        self.calls.append((seq_index, img_per_seq, seq_name, list(ids)))
        r = np.random.RandomState(self.seed + seq_index)
        n, H, W = len(ids), self.H, self.W
        extr = []
        for k in range(n):
            a = 0.3 + 0.1 * k
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            extr.append(np.concatenate([R, r.randn(3, 1)], 1))
        return {"images": [r.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)],
                "depths": [r.rand(H, W) + 1.0 for _ in range(n)], "extrinsics": extr,
                "intrinsics": [np.array([[5.0, 0, W / 2], [0, 5.0, H / 2], [0, 0, 1]]) for _ in range(n)],
                "cam_points": [r.randn(H, W, 3) for _ in range(n)], "world_points": [r.randn(H, W, 3) for _ in range(n)],
                "point_masks": [r.rand(H, W) < 0.8 for _ in range(n)], "ids": np.asarray(ids)}


def test_gather_sequences_and_get_sequence_data():
    a, b = _ToyDataset([3, 5]), _ToyDataset([4], seed=9)
    seqs = TM.gather_sequences([a, b], use_random_sequences=False)
    assert [(s[0], s[1], s[2], s[3]) for s in seqs] == [(a, 0, "seq0", 3), (a, 1, "seq1", 5), (b, 0, "seq0", 4)]
    np.random.seed(5)
    one = TM.gather_sequences([a, b], use_random_sequences=True)
    np.random.seed(5)
    ds = [a, b][np.random.randint(0, 2)]
    j = np.random.randint(0, ds.sequence_list_len)
    assert len(one) == 1 and one[0] == (ds, j, f"seq{j}", ds.seq_frame_num[j])

    d = TM.get_sequence_data(*seqs[1])
    assert a.calls[-1] == (1, -1, None, [0, 1, 2, 3, 4])
    assert d["dataset_name"] == "_ToyDataset" and d["seq_name"] == "seq1"
    shapes = {k: tuple(v.shape) for k, v in d.items() if isinstance(v, torch.Tensor)}
    assert shapes == {"ids": (1, 5), "images": (1, 5, 3, 4, 6), "depths": (1, 5, 4, 6), "extrinsics": (1, 5, 3, 4),
                      "intrinsics": (1, 5, 3, 3), "cam_points": (1, 5, 4, 6, 3), "world_points": (1, 5, 4, 6, 3),
                      "point_masks": (1, 5, 4, 6)}
    assert d["images"].dtype == torch.float32 and 0.0 <= float(d["images"].min()) and float(d["images"].max()) <= 1.0
    assert d["point_masks"].dtype == torch.bool and all(not v.is_cuda for v in d.values() if isinstance(v, torch.Tensor))
    raw = _ToyDataset([3, 5]).get_data(1, -1, None, np.arange(5))
    np.testing.assert_allclose(d["images"][0, 2].permute(1, 2, 0).numpy() * 255, raw["images"][2], atol=1e-4)
    # first-camera frame: extrinsics[0] is the identity, world points follow, depths are not rescaled
    np.testing.assert_allclose(d["extrinsics"][0, 0].numpy(), np.eye(4)[:3], atol=1e-6)
    e0 = raw["extrinsics"][0]
    want = raw["world_points"][3] @ e0[:, :3].T + e0[:, 3]
    np.testing.assert_allclose(d["world_points"][0, 3].numpy(), want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(d["depths"][0].numpy(), np.stack(raw["depths"]), rtol=1e-6)


def test_apply_sequence_to_model_offload_flag_on_host_tensors():
    """The module's driver: the default is dist.pipeline's, offload=False runs the same chunks through
    the same calls (on host tensors the offload copies nothing, so all three results are equal)."""
    from aligned_vggt.dist import pipeline
    from toy_model import ToyAlignModel
    g = torch.Generator().manual_seed(3)
    images = torch.rand(2, 7, 3, 4, 6, generator=g)
    extr = torch.randn(2, 7, 3, 4, generator=g)

    def run(fn, **kw):
        batch = {"images": images.clone(), "extrinsics": extr.clone()}
        return fn(batch, ToyAlignModel(), [4], [2], "chunk_overlap", "scale_from_poses", **kw), batch
    (want, wb), (default, db), (kept, kb) = run(pipeline.apply_sequence_to_model), run(TM.apply_sequence_to_model), \
        run(TM.apply_sequence_to_model, offload=False)
    assert want["pose_enc"].shape == (2, 7, 9) and want["depth"].shape == (2, 7, 4, 6, 1)
    for got, gb in ((default, db), (kept, kb)):
        assert set(got) == set(want)
        for k in ("pose_enc", "depth", "depth_conf", "chunk_sim3_alignment_enc", "frame_se3_alignment_enc"):
            assert torch.equal(got[k], want[k]), k
        assert [float(a) for a in got["alignment_scales"]] == [float(a) for a in want["alignment_scales"]]
        assert torch.equal(gb["extrinsics"], wb["extrinsics"])


def test_chunk_outputs_stay_in_place_switches_the_host_copies_off():
    """A meta tensor cannot be copied to the host, so it shows on the CPU whether a copy was tried."""
    from aligned_vggt.utils.data import chunk_outputs_stay_in_place, moveDictListItemToCPU
    d = {"depth": [torch.empty(2, 3, device="meta")], "pose_enc_list": [[torch.empty(1, device="meta")]]}
    with chunk_outputs_stay_in_place():
        moveDictListItemToCPU(d, -1)
        moveDictListItemToCPU(d, -1, [])
    assert d["depth"][0].device.type == "meta" and d["pose_enc_list"][0][0].device.type == "meta"
    with pytest.raises(NotImplementedError):  # outside the context the copy is made
        moveDictListItemToCPU(d, -1)
    with pytest.raises(KeyError):
        with chunk_outputs_stay_in_place():
            raise KeyError("left early")
    with pytest.raises(NotImplementedError):  # and an exception inside does not leave the switch on
        moveDictListItemToCPU(d, -1)


def test_plot_writes_its_two_files(tmp_path, golden):
    g = golden("ref_metrics")
    pred, gt = _traj(g, 2)
    prefix = str(tmp_path / "seq_")
    cases = ((AbsoluteTrajectoryError(), "traj_ate", {"pred_xyz", "gt_xyz", "rmse", "rmse_per_dim"}),
             (RelativePoseError(delta=1), "traj_rpe", {"steps", "trans_error", "rot_error", "trans_rmse", "rot_rmse"}),
             (ScaleConsistency(), "traj_scale_cons", {"steps", "scale_factors", "scale_var"}))
    for metric, stem, keys in cases:
        d, path = metric.plot(pred, gt, "title", prefix)
        assert path == f"{prefix}{stem}.png" and os.path.getsize(path) > 0
        data = np.load(f"{prefix}{stem}.npy", allow_pickle=True).item()
        assert set(data) == keys
    assert sorted(os.listdir(tmp_path)) == sorted(f"seq_{s}.{e}" for _, s, _ in cases for e in ("npy", "png"))
    data = np.load(f"{prefix}traj_ate.npy", allow_pickle=True).item()
    np.testing.assert_array_equal(data["pred_xyz"], pred[:, :3, 3].numpy())
    AbsoluteTrajectoryError().plot(pred, gt)  # no outpath: nothing more is written
    assert len(os.listdir(tmp_path)) == 6


def test_torch_quantile_is_the_kth_value():
    x = torch.randn(3, 101, generator=torch.Generator().manual_seed(1))
    flat = x.reshape(-1).sort().values
    assert TM.torch_quantile(x, 0.25) == flat[round(0.25 * (x.numel() - 1))]
    assert torch.equal(TM.torch_quantile(x, 0.5, dim=1), x.sort(dim=1).values[:, 50])
    assert TM.torch_quantile(x, 0.5, dim=1, keepdim=True).shape == (3, 1)
    with pytest.raises(ValueError):
        TM.torch_quantile(x, 1.5)


def test_metric_state_moves_with_to():
    for m in (AbsoluteTrajectoryError(), RelativePoseError(), ScaleConsistency()):
        assert m.to(torch.zeros(1)) is m and m.to("cpu") is m
        assert all(getattr(m, n).device.type == "cpu" for n in m._state)
    g = torch.Generator().manual_seed(2)
    p, t = torch.eye(4).repeat(2, 6, 1, 1), torch.eye(4).repeat(2, 6, 1, 1)
    p[..., :3, 3], t[..., :3, 3] = torch.randn(2, 6, 3, generator=g), torch.randn(2, 6, 3, generator=g)
    for cls in (AbsoluteTrajectoryError, RelativePoseError, ScaleConsistency):
        a, b = cls(), cls()
        a.update_batch(p, t)  # host state: a loop of update
        for i in range(2):
            b.update(p[i], t[i])
        assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in a._state)
