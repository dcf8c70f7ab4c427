"""CPU checks of the host half of eval/point_preparation.py: the quantile rank,
the subsampling-factor search (against a restatement of the reference loop,
training_metrics.py:281-320, written here) and the workspace-size functions
(host arithmetic, callable without a device)."""
import os
from math import ceil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aligned_vggt.eval import quantile_rank, search_subsample_factor


# ------------------------------------------------------------------ quantile rank
def test_quantile_rank_half_cases_round_to_even():
    assert quantile_rank(3, 0.25) == 1   # round(0.5) = 0
    assert quantile_rank(7, 0.25) == 3   # round(1.5) = 2
    assert quantile_rank(11, 0.25) == 3  # round(2.5) = 2
    assert quantile_rank(5, 0.25) == 2   # round(1.0) = 1


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1000, 40_800_000])
def test_quantile_rank_ends(n):
    assert quantile_rank(n, 0.0) == 1
    assert quantile_rank(n, 1.0) == n
    assert quantile_rank(n, 0) == 1


def test_quantile_rank_lower_higher_and_errors():
    assert quantile_rank(8, 0.25, "lower") == 2   # floor(1.75) + 1
    assert quantile_rank(8, 0.25, "higher") == 3  # ceil(1.75) + 1
    assert quantile_rank(8, 0.25) == 3            # round(1.75) + 1
    for bad in (-0.1, 1.1, "x"):
        with pytest.raises(ValueError):
            quantile_rank(8, bad)
    with pytest.raises(ValueError):
        quantile_rank(8, 0.5, "linear")
    with pytest.raises(ValueError):
        quantile_rank(0, 0.5)


def test_quantile_rank_matches_kthvalue_protocol():
    """The rank is what torch_quantile hands to torch.kthvalue."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1001, generator=g)
    for q in (0.0, 0.25, 0.5, 0.9, 1.0):
        k = quantile_rank(x.numel(), q)
        assert torch.kthvalue(x, k).values == x.sort().values[k - 1]


# ------------------------------------------------------------------ factor search
def _reference_loop(interp_count, valid_points_gt, max_points_icp, H, W):
    """training_metrics.py:281-320 restated, the count of a factor left to ``interp_count``."""
    assert max_points_icp and valid_points_gt > max_points_icp
    subsample_factor = ceil(np.sqrt(valid_points_gt / max_points_icp))
    last_subsample_factor = 0
    while valid_points_gt > max_points_icp:
        if last_subsample_factor > 0:
            last_subsample_factor = subsample_factor
            subsample_factor = subsample_factor * 2
        else:
            last_subsample_factor = subsample_factor
        if subsample_factor > max(H, W):
            break
        valid_points_gt = interp_count(subsample_factor)
    if last_subsample_factor != subsample_factor:
        while last_subsample_factor + 1 < subsample_factor:
            mid = (last_subsample_factor + subsample_factor) // 2
            v = interp_count(mid)
            if v <= max_points_icp:
                subsample_factor, valid_points_gt = mid, v
            else:
                last_subsample_factor = mid
    return subsample_factor, valid_points_gt


def _reference_search(mask, max_points_icp):
    """The reference loop on a mask: (factor, valid points, factors whose count was taken)."""
    H, W = mask.shape[-2:]
    visited = []
    f, v = _reference_loop(_count_fn(mask, visited), mask.sum().item(), max_points_icp, H, W)
    return f, v, visited


def _bernoulli(shape, p, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < p


def _lattice(shape, period, offset, extra, seed):
    """Valid pixels on a lattice that a subsample by ``period`` hits (odd factors sample pixel centres), plus a
    sprinkle: the count at the first guess stays near the full count, so the reference has to double."""
    m = torch.zeros(shape, dtype=torch.bool)
    m[:, :, offset::period, offset::period] = True
    return m | _bernoulli(shape, extra, seed)


def _count_fn(mask, visited):
    B, S, H, W = mask.shape
    pre = mask.reshape(B * S, 1, H, W).float()

    def fn(f):
        visited.append(f)
        return (F.interpolate(pre, size=(H // f, W // f), mode="bilinear", align_corners=False) > 0.5).sum().item()
    return fn


SEARCH_MASKS = {
    "small": lambda: _bernoulli((2, 3, 37, 70), 0.7, 1),
    "wide": lambda: _bernoulli((1, 4, 154, 518), 0.7, 2),
    "small_lattice3": lambda: _lattice((2, 3, 37, 70), 3, 1, 0.02, 5),
    "small_lattice5": lambda: _lattice((2, 3, 37, 70), 5, 2, 0.02, 5),
    "wide_lattice7": lambda: _lattice((1, 4, 154, 518), 7, 3, 0.02, 5),
    "wide_lattice7_dense": lambda: _lattice((1, 4, 154, 518), 7, 3, 0.1, 5),
}
# (mask, max_points_icp, what the reference loop must be seen doing)
SEARCH_CASES = [
    ("small", 5000, "first"), ("small", 900, "first"), ("small", 300, "any"), ("small", 40, "any"),
    ("wide", 100_000, "first"), ("wide", 20_000, "any"), ("wide", 1500, "any"), ("wide", 97, "any"),
    ("small_lattice3", 276, "binary"), ("small_lattice3", 96, "binary"), ("small_lattice5", 52, "binary"),
    ("wide_lattice7", 320, "binary"), ("wide_lattice7_dense", 944, "binary"),
]


@pytest.mark.parametrize("name,max_points,expect", SEARCH_CASES)
def test_search_replays_the_reference_loop(name, max_points, expect):
    mask = SEARCH_MASKS[name]()
    H, W = mask.shape[-2:]
    want_f, want_v, want_visited = _reference_search(mask, max_points)
    visited = []
    f, v = search_subsample_factor(_count_fn(mask, visited), int(mask.sum()), max_points, H, W)
    assert (f, v) == (want_f, want_v)
    assert visited == want_visited
    assert v <= max_points
    if expect == "first":
        assert len(want_visited) == 1
    if expect == "binary":  # doubled at least once, then bisected
        assert len(want_visited) >= 3 and want_visited[1] == 2 * want_visited[0]
        assert any(a < want_visited[1] and a > want_visited[0] for a in want_visited[2:])


def test_search_cases_cover_every_branch():
    kinds = set()
    for name, max_points, _ in SEARCH_CASES:
        _, _, vis = _reference_search(SEARCH_MASKS[name](), max_points)
        if len(vis) == 1:
            kinds.add("first")
        elif vis[1] == 2 * vis[0]:
            kinds.add("doubling")
            if len(vis) > 2 and vis[-1] < max(vis):
                kinds.add("binary")
    assert kinds == {"first", "doubling", "binary"}


@pytest.mark.parametrize("seed", range(40))
def test_search_replays_the_reference_loop_on_count_tables(seed):
    """Counts from a table, not from an image: non-monotonic counts take the binary search down both of its
    branches (a middle factor that fails moves the lower bound), which subsampled Bernoulli masks rarely do."""
    g = np.random.default_rng(seed)
    H, W = int(g.integers(300, 600)), int(g.integers(300, 600))
    valid = int(g.integers(1000, 200_000))
    max_points = int(g.integers(50, valid))
    table = {f: int(valid / f ** 2 * g.uniform(0.3, 3.0)) for f in range(1, max(H, W) + 1)}
    want_visited, visited = [], []
    want = _reference_loop(lambda f: want_visited.append(f) or table[f], valid, max_points, H, W)
    got = search_subsample_factor(lambda f: visited.append(f) or table[f], valid, max_points, H, W)
    assert got == want and visited == want_visited
    assert all(H // f > 0 and W // f > 0 for f in visited)  # no case here ends in the ValueError


def test_search_is_a_no_op_under_the_limit():
    called = []
    assert search_subsample_factor(lambda f: called.append(f) or 0, 100, 100, 8, 8) == (1, 100)
    assert search_subsample_factor(lambda f: called.append(f) or 0, 100, None, 8, 8) == (1, 100)
    assert not called


def test_search_raises_where_interpolate_would_fail():
    # every pixel valid, one point allowed: the factor has to pass min(H, W), where H // f == 0
    mask = torch.ones(1, 1, 4, 64, dtype=torch.bool)
    with pytest.raises(ValueError, match="F.interpolate fails"):
        search_subsample_factor(_count_fn(mask, []), int(mask.sum()), 1, 4, 64)
    # the reference fails on the same input, in F.interpolate
    with pytest.raises(RuntimeError):
        _reference_search(mask, 1)
    # first guess already past max(H, W): the loop breaks before counting and the final subsample is empty
    with pytest.raises(ValueError, match="F.interpolate fails"):
        search_subsample_factor(lambda f: 0, 10_000, 1, 8, 8)


# ------------------------------------------------------------------ workspace sizes (host arithmetic)
def _native_or_skip():
    from aligned_vggt import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native


def test_kth_value_ws_bytes_without_a_device():
    N = _native_or_skip()
    assert N.kth_value_ws_bytes(0) == 0
    small, big = N.kth_value_ws_bytes(1), N.kth_value_ws_bytes(40_800_000)
    assert small >= 4 * 256 * 8 and small % 8 == 0   # four passes of 256 64-bit counters and the state
    assert big == small == N.kth_value_ws_bytes(1 << 40)


def test_prepare_clouds_ws_bytes_without_a_device():
    N = _native_or_skip()
    assert N.prepare_clouds_ws_bytes(0, 1, 1, 1) == 0
    for B, S, Ho, Wo in ((1, 1, 1, 1), (2, 3, 11, 23), (2, 5, 154, 518), (1, 512, 154, 518), (1, 512, 17, 57)):
        pixels = B * S * Ho * Wo
        for rpw in (0, 1, 7, 10_000_000):
            n = N.prepare_clouds_ws_bytes(B, S, Ho, Wo, rpw)
            assert n % 8 == 0
            assert n * 8 >= 2 * pixels + 2 * 32 * B  # two decision bits a pixel, two 32-bit totals a workgroup
        # the decision words grow with the pixels, not with their square: 16 bytes per 64 pixels, padded per row group
        assert N.prepare_clouds_ws_bytes(B, S, Ho, Wo, 0) <= pixels // 2 + 4096 * B + 64
    # one row a workgroup is the finest geometry and needs the most
    assert N.prepare_clouds_ws_bytes(2, 5, 154, 518, 1) >= N.prepare_clouds_ws_bytes(2, 5, 154, 518, 0)
