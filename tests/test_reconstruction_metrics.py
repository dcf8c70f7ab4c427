"""CPU-side checks of the reconstruction metrics: the header's nearest-neighbour
entry points, the host-only split plan (vggt_nn1_plan), ChamferDistanceMetrics'
compute() arithmetic on hand-filled state (the reference's keys, its double
squaring under rmse=True and its length checks, reconstruction_metrics.py:58-84),
and the refusal of CPU tensors.  No GPU call."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024  # reference points per LDS tile of vggt_nn1 (csrc/nn.hip NN_TILE)
QB = 1024  # query points per workgroup (NN_QB)


def test_header_declares_nn_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vggt_mi355x.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(vggt_[a-z0-9_]+)\s*\(", src))
    assert {"vggt_nn1", "vggt_nn1_plan", "vggt_nn1_workspace_bytes", "vggt_nn1_pair_stats"} <= names


@pytest.fixture(scope="module")
def plan():
    from aligned_vggt import _native
    _native.lib()
    return _native.nn1_plan


def test_plan_is_one_when_queries_fill_the_device(plan):
    # 16 rounds of 4 workgroup slots per compute unit from the query blocks alone
    assert plan(1, 256 * 4 * 16 * QB, 500_000, 256) == 1
    assert plan(64, 256 * QB, 500_000, 256) == 1
    assert plan(1, 8 * 4 * 4 * QB, 500_000, 8) == 1


def test_plan_splits_short_query_sets(plan):
    assert plan(1, 256, 500_000, 256) > 1
    assert plan(1, 250_000, 250_000, 256) > 1
    assert plan(1, 500_000, 500_000, 256) > 1


@pytest.mark.parametrize("nr", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE, 3 * TILE + 1, 100 * TILE, 500_000])
@pytest.mark.parametrize("nq", [1, 256, 5000])
def test_plan_never_splits_below_one_tile_per_part(plan, nq, nr):
    s = plan(1, nq, nr, 256)
    assert 1 <= s <= max(1, math.ceil(nr / TILE))


def test_plan_is_monotone_in_nr(plan):
    for nq in (1, 256, 3000, 100_000):
        prev = 0
        for nr in [1, 100, TILE, TILE + 1, 2 * TILE, 5 * TILE + 3, 17 * TILE, 64 * TILE, 250_000, 500_000, 2_000_000,
                   2 ** 31 - 1]:
            s = plan(1, nq, nr, 256)
            assert s >= prev, (nq, nr, s, prev)
            prev = s


def test_plan_degenerate_arguments_do_not_split(plan):
    assert plan(0, 100, 100, 256) == 1
    assert plan(1, 0, 100, 256) == 1
    assert plan(1, 100, 0, 256) == 1
    assert plan(1, 100, 100, 0) == 1


def test_workspace_covers_keys_and_partials():
    from aligned_vggt import _native
    L = _native.lib()
    assert L.vggt_nn1_workspace_bytes(1, 0, 10) == 0
    assert L.vggt_nn1_workspace_bytes(2, 5000, 10) >= 2 * 5000 * 8
    assert L.vggt_nn1_workspace_bytes(3, 1, 10) >= 3 * 17 * 8  # one workgroup's pair_stats partials


def test_status_codes_are_decided_on_the_host():
    """The argument checks of vggt_nn1 come before any device call (null pointers are never touched)."""
    from aligned_vggt import _native as N
    L = N.lib()

    def call(B, nq, nr, norm, split=0):
        return L.vggt_nn1(None, 0, None, None, 0, None, B, nq, nr, norm, None, None, split, None, 0, None)
    assert call(0, 10, 10, 2) == N.VGGT_ERR_SHAPE
    assert call(-3, 10, 10, 2) == N.VGGT_ERR_SHAPE
    assert call(1, 10, 2 ** 31, 2) == N.VGGT_ERR_SHAPE
    assert call(1, 10, 10, 3) == N.VGGT_ERR_UNSUPPORTED
    assert call(1, 10, 10, 0) == N.VGGT_ERR_UNSUPPORTED
    assert call(1, 0, 10, 2) == N.VGGT_OK  # nothing to do
    assert call(1, 0, 10, 1, 5) == N.VGGT_OK


def _filled(norm, rmse, max_dist=None):
    from aligned_vggt.eval import ChamferDistanceMetrics
    m = ChamferDistanceMetrics(norm=norm, max_dist=max_dist, rmse=rmse)
    m.pred_to_gt = torch.tensor([0.5, 2.0, 0.25, 1.0])
    m.gt_to_pred = torch.tensor([4.0, 0.125, 1.5])
    return m


def test_compute_rmse_mode_keys_and_values():
    out = _filled(2, True).compute()
    assert list(out) == ["chamfer_distance_rmse", "accuracy_rmse", "completion_rmse"]
    p = np.array([0.5, 2.0, 0.25, 1.0], np.float32)
    g = np.array([4.0, 0.125, 1.5], np.float32)
    acc = math.sqrt(float((p.astype(np.float64) ** 2).mean()))  # the stored (squared) distances squared again
    comp = math.sqrt(float((g.astype(np.float64) ** 2).mean()))
    assert float(out["accuracy_rmse"]) == pytest.approx(acc, rel=1e-6)
    assert float(out["completion_rmse"]) == pytest.approx(comp, rel=1e-6)
    assert float(out["chamfer_distance_rmse"]) == pytest.approx(0.5 * acc + 0.5 * comp, rel=1e-6)
    assert isinstance(out["accuracy_rmse"], torch.Tensor) and out["accuracy_rmse"].dim() == 0


def test_compute_mean_mode_keys_and_values():
    out = _filled(1, False).compute()
    assert list(out) == ["chamfer_distance", "accuracy", "completion"]
    assert out["accuracy"] == pytest.approx(3.75 / 4, rel=1e-6)
    assert out["completion"] == pytest.approx(5.625 / 3, rel=1e-6)
    assert out["chamfer_distance"] == pytest.approx(0.5 * 3.75 / 4 + 0.5 * 5.625 / 3, rel=1e-6)
    assert isinstance(out["accuracy"], float)


@pytest.mark.parametrize("rmse", [True, False])
def test_compute_on_empty_state_is_zero(rmse):
    from aligned_vggt.eval import ChamferDistanceMetrics
    out = ChamferDistanceMetrics(rmse=rmse).compute()
    assert len(out) == 3 and all(v == 0.0 for v in out.values())


def test_compute_length_checks_follow_the_reference():
    """rmse=True tests pred_to_gt's length for BOTH terms (reconstruction_metrics.py:64-65); rmse=False tests
    each vector's own (:74-75)."""
    from aligned_vggt.eval import ChamferDistanceMetrics
    m = ChamferDistanceMetrics(rmse=True)
    m.gt_to_pred = torch.tensor([3.0])
    assert m.compute() == {"chamfer_distance_rmse": 0.0, "accuracy_rmse": 0.0, "completion_rmse": 0.0}
    m = ChamferDistanceMetrics(rmse=False)
    m.gt_to_pred = torch.tensor([3.0])
    assert m.compute() == {"chamfer_distance": 1.5, "accuracy": 0.0, "completion": 3.0}


def test_reset_clears_state():
    m = _filled(2, True)
    m.reset()
    assert len(m.pred_to_gt) == 0 and len(m.gt_to_pred) == 0
    m.sync()  # no process group: a no-op
    assert len(m.pred_to_gt) == 0


def test_max_dist_clamps(monkeypatch):
    """update() clamps what the search returns at max_dist before it accumulates (the search itself stubbed)."""
    from aligned_vggt.eval import ChamferDistanceMetrics
    from aligned_vggt.eval import reconstruction_metrics as RM
    vals = {4: torch.tensor([0.5, 2.0, 0.25, 9.0]), 3: torch.tensor([4.0, 0.125, 1.5])}
    monkeypatch.setattr(RM, "nearest_neighbors", lambda q, r, norm=2, return_idx=True: (vals[q.shape[0]], None))
    m = ChamferDistanceMetrics(norm=2, max_dist=1.0, rmse=False)
    m.update(torch.zeros(4, 3), torch.zeros(3, 3))
    assert m.pred_to_gt.tolist() == [0.5, 1.0, 0.25, 1.0]
    assert m.gt_to_pred.tolist() == [1.0, 0.125, 1.0]
    p2g, g2p = ChamferDistanceMetrics(norm=2, max_dist=None).distances(torch.zeros(4, 3), torch.zeros(3, 3))
    assert p2g.tolist() == [0.5, 2.0, 0.25, 9.0] and g2p.tolist() == [4.0, 0.125, 1.5]


def test_cpu_tensors_are_refused():
    from aligned_vggt.eval import ChamferDistanceMetrics, iterative_closest_point, nearest_neighbors
    a = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        nearest_neighbors(a, a)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ChamferDistanceMetrics().update(a, a)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        iterative_closest_point([a], [a])


def test_solve_similarity_recovers_a_known_transform():
    """The host half of an ICP iteration: from exact sums of (x, y = s x R + T) the solve returns (R, T, s)."""
    from aligned_vggt.eval.reconstruction_metrics import solve_similarity
    g = np.random.default_rng(3)
    x = g.normal(size=(50, 3)) + np.array([800.0, -650.0, 30.0])
    a = np.deg2rad(20.0)
    R = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    T = np.array([0.3, -2.0, 5.0])
    for s, est in ((1.0, False), (1.7, True)):
        y = s * x @ R + T
        st = np.concatenate([[len(x)], x.sum(0), y.sum(0), (x.T @ y).reshape(-1), [((x - y) ** 2).sum()]])
        Rs, Ts, ss = solve_similarity(torch.from_numpy(st)[None], torch.tensor([(x * x).sum()]), est, False)
        np.testing.assert_allclose(Rs[0].numpy(), R, atol=1e-7)
        np.testing.assert_allclose(Ts[0].numpy(), T, atol=1e-4)
        assert float(ss[0]) == pytest.approx(s, rel=1e-7)
