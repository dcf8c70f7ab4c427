"""GPU checks of the exact 1-nearest-neighbour kernel (vggt_nn1), the ICP sums
(vggt_nn1_pair_stats) and what is built on them (nearest_neighbors,
ChamferDistanceMetrics, iterative_closest_point).  Oracles, written here:
integer brute force on a lattice (every distance exact in fp32),
scipy.spatial.cKDTree and numpy in fp64 on the fp32-rounded inputs."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ exact lattice
LATTICE_PAIRS = [(1, 1), (2, 63), (63, 2), (64, 64), (65, 255), (255, 65), (257, 1023), (1023, 257), (1025, 1025),
                 (1, 4097), (4097, 1), (4097, 4097), (1025, 4097), (64, 1025)]


@pytest.fixture(scope="module")
def lattice():
    """4097 query and 4097 reference points with integer coordinates in [0, 8)^3: at most 512 distinct points, so
    duplicates and ties abound.  Smaller cases take prefixes."""
    g = np.random.default_rng(11)
    return g.integers(0, 8, (4097, 3)).astype(np.int32), g.integers(0, 8, (4097, 3)).astype(np.int32)


def _lattice_oracle(q, r, norm):
    d = np.empty((len(q), len(r)), np.int32)
    for a in range(0, len(q), 512):
        diff = q[a:a + 512, None, :] - r[None, :, :]
        d[a:a + 512] = (diff * diff).sum(-1) if norm == 2 else np.abs(diff).sum(-1)
    idx = d.argmin(1)  # first occurrence
    return d[np.arange(len(q)), idx].astype(np.float32), idx.astype(np.int64)


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("nq,nr", LATTICE_PAIRS)
def test_lattice_is_bitwise_exact(N, lattice, nq, nr, norm):
    q, r = lattice[0][:nq], lattice[1][:nr]
    want_d, want_i = _lattice_oracle(q, r, norm)
    qg, rg = (torch.from_numpy(a.astype(np.float32))[None].cuda() for a in (q, r))
    d, i = N.nn1(qg, rg, norm)
    assert np.array_equal(d[0].cpu().numpy().view(np.int32), want_d.view(np.int32))
    assert np.array_equal(i[0].cpu().numpy(), want_i)


# ------------------------------------------------------------------ float clouds far from the origin
@pytest.fixture(scope="module")
def far_clouds():
    """3,000 reference and 2,000 query points, uniform in a 10 m cube centred at (800, -650, 30); half of the
    queries are copies of reference points moved by less than 1 cm."""
    g = np.random.default_rng(7)
    c = np.array([800.0, -650.0, 30.0])
    r = (c + g.uniform(-5, 5, (3000, 3))).astype(np.float32)
    q = (c + g.uniform(-5, 5, (2000, 3))).astype(np.float32)
    pick = g.choice(3000, 1000, replace=False)
    off = g.normal(size=(1000, 3))
    off *= (g.uniform(0, 0.01, (1000, 1)) / np.linalg.norm(off, axis=1, keepdims=True))
    q[1000:] = (r[pick].astype(np.float64) + off).astype(np.float32)
    return q, r


@pytest.mark.parametrize("norm", [2, 1])
def test_far_clouds_keep_full_precision(N, far_clouds, norm):
    """dist is within 1e-6 relative of the fp64 distance to the returned index (one rounding per difference, doubled
    by the square, plus two for the sum: at most about 4 * 2^-24 = 2.4e-7), and that distance is the fp64 minimum
    to within the same factor, for every query.  |q|^2 + |r|^2 - 2 q.r misses both by orders of magnitude here."""
    q, r = far_clouds
    d, i = N.nn1(torch.from_numpy(q)[None].cuda(), torch.from_numpy(r)[None].cuda(), norm)
    d, i = d[0].cpu().numpy().astype(np.float64), i[0].cpu().numpy()
    assert i.min() >= 0 and i.max() < len(r)
    diff = q.astype(np.float64) - r[i].astype(np.float64)
    at_idx = (diff * diff).sum(1) if norm == 2 else np.abs(diff).sum(1)
    dmin, _ = cKDTree(r.astype(np.float64)).query(q.astype(np.float64), p=norm)
    dmin = dmin * dmin if norm == 2 else dmin
    rel = np.abs(d - at_idx) / np.maximum(at_idx, 1e-300)
    print(f"norm {norm}: max |dist - fp64 at idx| / fp64 = {rel.max():.3e}; max fp64 at idx / fp64 min - 1 = "
          f"{(at_idx / np.maximum(dmin, 1e-300)).max() - 1:.3e}")
    assert (np.abs(d - at_idx) <= 1e-6 * at_idx).all()
    assert (at_idx <= dmin * (1 + 1e-6)).all()


# ------------------------------------------------------------------ split invariance
def test_result_does_not_depend_on_split_or_run(N, lattice, far_clouds):
    for q, r in ((lattice[0].astype(np.float32), lattice[1].astype(np.float32)), far_clouds):
        qg, rg = torch.from_numpy(q)[None].cuda(), torch.from_numpy(r)[None].cuda()
        for norm in (2, 1):
            base_d, base_i = N.nn1(qg, rg, norm, split=1)
            for split in (1, 2, 7, 0):
                for _ in range(2):
                    d, i = N.nn1(qg, rg, norm, split=split)
                    assert torch.equal(_bits(d), _bits(base_d)), (norm, split)
                    assert torch.equal(i, base_i), (norm, split)
            d, none = N.nn1(qg, rg, norm, return_idx=False, split=2)
            assert none is None and torch.equal(_bits(d), _bits(base_d))


# ------------------------------------------------------------------ lengths, padding, NaN
def _brute64(q, r, norm):
    diff = q.astype(np.float64)[:, None, :] - r.astype(np.float64)[None, :, :]
    d = (diff * diff).sum(-1) if norm == 2 else np.abs(diff).sum(-1)
    return d.min(1), d.argmin(1)


@pytest.mark.parametrize("norm", [2, 1])
def test_lengths_and_nan_padding(N, norm):
    g = np.random.default_rng(19)
    q_len, r_len = [5, 0, 300], [257, 3, 1]
    q = np.full((3, 300, 3), np.nan, np.float32)
    r = np.full((3, 257, 3), np.nan, np.float32)
    for b in range(3):
        q[b, :q_len[b]] = g.uniform(-2, 2, (q_len[b], 3))
        r[b, :r_len[b]] = g.uniform(-2, 2, (r_len[b], 3))
    qg, rg = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    for split in (0, 1):
        d, i = N.nn1(qg, rg, norm, q_len=torch.tensor(q_len).cuda(), r_len=torch.tensor(r_len).cuda(), split=split)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        for b in range(3):
            n = q_len[b]
            assert (d[b, n:] == 0).all() and (i[b, n:] == -1).all()
            if n:
                want_d, want_i = _brute64(q[b, :n], r[b, :r_len[b]], norm)
                assert np.isfinite(d[b, :n]).all()
                assert np.array_equal(i[b, :n], want_i)
                assert (np.abs(d[b, :n] - want_d) <= 1e-6 * want_d).all()
    # an empty reference range: +inf / -1 on the valid query rows, the padding rows unchanged
    d, i = N.nn1(qg, rg, norm, q_len=torch.tensor(q_len).cuda(), r_len=torch.tensor([0, 3, 0]).cuda())
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert np.isposinf(d[0, :5]).all() and (i[0, :5] == -1).all()
    assert (d[0, 5:] == 0).all() and (i[0, 5:] == -1).all()
    assert np.isposinf(d[2]).all() and (i[2] == -1).all()
    assert (d[1] == 0).all() and (i[1] == -1).all()


@pytest.mark.parametrize("norm", [2, 1])
def test_lengths_under_a_split(N, norm):
    """Three reference tiles cut into parts, with lengths: the unpack pass writes the padding rows, a part that
    starts at or past r_len contributes nothing (r_len = 1000: every part but the first), and r_len = 0 under a
    split gives +inf / -1."""
    g = np.random.default_rng(29)
    q_len, r_len = [5, 0, 300, 300], [2500, 7, 1000, 0]
    q = np.full((4, 300, 3), np.nan, np.float32)
    r = np.full((4, 2500, 3), np.nan, np.float32)
    for b in range(4):
        q[b, :q_len[b]] = g.uniform(-2, 2, (q_len[b], 3))
        r[b, :r_len[b]] = g.uniform(-2, 2, (r_len[b], 3))
    qg, rg = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    ql, rl = torch.tensor(q_len).cuda(), torch.tensor(r_len).cuda()
    base_d, base_i = N.nn1(qg, rg, norm, q_len=ql, r_len=rl, split=1)
    for split in (2, 3, 0):
        d, i = N.nn1(qg, rg, norm, q_len=ql, r_len=rl, split=split)
        assert torch.equal(_bits(d), _bits(base_d)) and torch.equal(i, base_i), split
        d, i = d.cpu().numpy(), i.cpu().numpy()
        for b in range(4):
            n = q_len[b]
            assert (d[b, n:] == 0).all() and (i[b, n:] == -1).all()
            if n and r_len[b]:
                want_d, want_i = _brute64(q[b, :n], r[b, :r_len[b]], norm)
                assert np.array_equal(i[b, :n], want_i)
                assert (np.abs(d[b, :n] - want_d) <= 1e-6 * want_d).all()
        assert np.isposinf(d[3]).all() and (i[3] == -1).all()


def test_nan_points_are_never_selected(N):
    g = np.random.default_rng(23)
    q = g.uniform(-1, 1, (70, 3)).astype(np.float32)
    r = g.uniform(-1, 1, (1100, 3)).astype(np.float32)
    r[[0, 17, 1024, 1099]] = np.nan  # whole rows
    r[500, 1] = np.nan  # one coordinate
    q[3] = np.nan
    keep = np.ones(1100, bool)
    keep[[0, 17, 500, 1024, 1099]] = False
    d, i = N.nn1(torch.from_numpy(q)[None].cuda(), torch.from_numpy(r)[None].cuda(), 2, split=2)
    d, i = d[0].cpu().numpy(), i[0].cpu().numpy()
    assert np.isposinf(d[3]) and i[3] == -1
    ok = np.arange(70) != 3
    want_d, want_i = _brute64(q[ok], r[keep], 2)
    assert np.array_equal(i[ok], np.flatnonzero(keep)[want_i])
    assert np.isfinite(d[ok]).all()


def test_python_surface_shapes_and_errors(N):
    from aligned_vggt.eval import nearest_neighbors
    g = torch.Generator().manual_seed(2)
    q, r = torch.randn(40, 3, generator=g).cuda(), torch.randn(90, 3, generator=g).cuda()
    d, i = nearest_neighbors(q, r)
    assert d.shape == (40,) and i.shape == (40,) and i.dtype == torch.int64
    want_d, want_i = _brute64(q.cpu().numpy(), r.cpu().numpy(), 2)
    assert np.array_equal(i.cpu().numpy(), want_i)
    db, ib = nearest_neighbors(torch.stack([q, q]), torch.stack([r, r.flip(0)]), q_lengths=[40, 7], return_idx=False)
    assert ib is None and db.shape == (2, 40) and torch.equal(_bits(db[0]), _bits(d)) and (db[1, 7:] == 0).all()
    assert torch.equal(_bits(db[1, :7]), _bits(d[:7]))
    with pytest.raises(ValueError):
        nearest_neighbors(q, r[:0])
    with pytest.raises(ValueError):
        nearest_neighbors(torch.stack([q, q]), torch.stack([r, r]), r_lengths=[3, 0])
    with pytest.raises(ValueError):
        nearest_neighbors(q, r, norm=3)


# ------------------------------------------------------------------ pair_stats
def _stats64(x, y, idx, n, m):
    x, y, idx = x[:n].astype(np.float64), y.astype(np.float64), idx[:n]
    ok = (idx >= 0) & (idx < m)
    x, yy = x[ok], y[idx[ok]]
    return np.concatenate([[ok.sum()], x.sum(0), yy.sum(0), (x.T @ yy).reshape(-1), [((x - yy) ** 2).sum()]])


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_pair_stats_matches_fp64(N, n):
    """Positive coordinates, so that no sum cancels and a relative bar per value is meaningful."""
    g = np.random.default_rng(31 + n)
    m = 500
    x = g.uniform(1, 3, (2, n, 3)).astype(np.float32)
    y = g.uniform(1, 3, (2, m, 3)).astype(np.float32)
    idx = g.integers(0, m, (2, n)).astype(np.int64)
    idx[:, 3::7] = -1
    x_len, y_len = [n, n // 2], [m, m - 100]  # batch item 1: rows with idx >= 400 are skipped too
    out = [N.nn1_pair_stats(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(idx).cuda(),
                            x_len, y_len) for _ in range(2)]
    assert out[0].shape == (2, 17) and out[0].dtype == torch.float64
    assert torch.equal(out[0].view(torch.int64), out[1].view(torch.int64))
    got = out[0].cpu().numpy()
    for b in range(2):
        want = _stats64(x[b], y[b], idx[b], x_len[b], y_len[b])
        np.testing.assert_allclose(got[b], want, rtol=1e-12, atol=0)


# ------------------------------------------------------------------ ICP
def _icp_inputs(n, deg, shift):
    """Y: a 14^3 unit lattice jittered by U(-0.2, 0.2) (seed 5); X: n of its points rotated `deg` degrees about
    the z axis through Y's centroid, shifted by shift * (1, -0.5, 0.25) / 1.15, plus N(0, 0.02) noise."""
    g = np.random.default_rng(5)
    lat = np.stack(np.meshgrid(*[np.arange(14.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    Y = lat + g.uniform(-0.2, 0.2, lat.shape)
    sub = g.choice(len(Y), n, replace=False)
    c, a = Y.mean(0), np.deg2rad(deg)
    R = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    X = (Y[sub] - c) @ R + c + shift * np.array([1.0, -0.5, 0.25]) / 1.15 + g.normal(0, 0.02, (n, 3))
    return X.astype(np.float32), Y.astype(np.float32)


def _icp64(X, Y, max_iterations=30, thr=1e-6):
    """PyTorch3D's iteration restated in fp64 on the fp32-rounded inputs (SPEC_ASSUMPTIONS.md)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    tree = cKDTree(Y)
    Xt, prev, conv = X.copy(), None, False
    for it in range(max_iterations):
        Ynn = Y[tree.query(Xt)[1]]
        xm, ym = X.mean(0), Ynn.mean(0)
        U, _, Vt = np.linalg.svd((X - xm).T @ (Ynn - ym) / len(X))
        R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        T = ym - xm @ R
        Xt = X @ R + T
        rmse = np.sqrt(((Xt - Ynn) ** 2).sum(1).mean())
        if (1.0 if prev is None else (prev - rmse) / prev) <= thr:
            conv = True
            break
        prev = rmse
    return R, T, rmse, it + 1, conv


@pytest.fixture(scope="module")
def icp_cases():
    out = []
    for n, deg, shift in ((700, 3.0, 0.2), (1500, 5.0, 0.3)):
        X, Y = _icp_inputs(n, deg, shift)
        out.append((X, Y, _icp64(X, Y)))
    return out


def _check_icp(sol_R, sol_T, sol_rmse, ref, tag):
    R, T, rmse = ref[:3]
    dR = np.abs(sol_R.double().cpu().numpy() - R).max()
    dT = np.abs(sol_T.double().cpu().numpy() - T).max()
    dr = abs(float(sol_rmse) - rmse) / rmse
    print(f"icp {tag}: iterations {ref[3]}, |dR| {dR:.3e}, |dT| {dT:.3e}, rmse rel {dr:.3e}")
    assert dR <= 1e-5 and dT <= 1e-4 and dr <= 1e-4


@pytest.mark.parametrize("case", [0, 1])
def test_icp_matches_fp64_restatement(N, icp_cases, case):
    """Bars (about 10x the spread between an fp32 and an fp64 restatement, which share the fixed point): the same
    iteration count and convergence flag, |dR| <= 1e-5, |dT| <= 1e-4, rmse within 1e-4 relative."""
    from aligned_vggt.eval import iterative_closest_point
    X, Y, ref = icp_cases[case]
    sol = iterative_closest_point(torch.from_numpy(X)[None].cuda(), torch.from_numpy(Y)[None].cuda(),
                                  max_iterations=30)
    assert sol.iterations == ref[3] and sol.converged == ref[4] and ref[4]
    assert sol.rmse.shape == (1,) and sol.R.shape == (1, 3, 3) and sol.T.shape == (1, 3) and float(sol.s[0]) == 1.0
    _check_icp(sol.R[0], sol.T[0], sol.rmse[0], ref, f"case {case}")
    Xt = X.astype(np.float64) @ ref[0] + ref[1]
    assert np.abs(sol.Xt[0].double().cpu().numpy() - Xt).max() <= 5.2e-4  # the bars above: 3 * 14 * |dR| + |dT|


def test_icp_lists_of_unequal_clouds(N, icp_cases):
    """Lists as training_metrics.py:344-358 builds them; the batch iterates until every item has stopped, and an
    item that has reached its fixed point stays on it."""
    from aligned_vggt.eval import iterative_closest_point
    sol = iterative_closest_point([torch.from_numpy(c[0]).cuda() for c in icp_cases],
                                  [torch.from_numpy(c[1]).cuda() for c in icp_cases], max_iterations=30)
    assert sol.converged and sol.iterations == max(c[2][3] for c in icp_cases)
    assert isinstance(sol.Xt, list) and [tuple(x.shape) for x in sol.Xt] == [(700, 3), (1500, 3)]
    for b, c in enumerate(icp_cases):
        _check_icp(sol.R[b], sol.T[b], sol.rmse[b], c[2], f"list item {b}")


def test_icp_estimates_scale(N, icp_cases):
    """estimate_scale=True on a cloud shrunk by 2 % about its centroid recovers the factor."""
    from aligned_vggt.eval import iterative_closest_point
    X, Y, ref = icp_cases[0]
    Xt = (X.astype(np.float64) @ ref[0] + ref[1])
    c = Xt.mean(0)
    Xs = ((Xt - c) / 1.02 + c).astype(np.float32)
    sol = iterative_closest_point(torch.from_numpy(Xs)[None].cuda(), torch.from_numpy(Y)[None].cuda(),
                                  max_iterations=30, estimate_scale=True)
    assert sol.converged and abs(float(sol.s[0]) - 1.02) < 2e-3


# ------------------------------------------------------------------ Chamfer end to end
@pytest.mark.parametrize("norm,rmse,max_dist", [(2, True, None), (2, False, None), (1, True, None), (1, False, None),
                                                (2, True, 0.05), (1, False, 0.2)])
def test_chamfer_end_to_end(N, norm, rmse, max_dist):
    """Two updates, compute() against the fp64 oracle.  Bar 1e-5 relative: 1e-6 on each distance (above), the
    fp32 mean of at most 700 values and one square and root on top."""
    from aligned_vggt.eval import ChamferDistanceMetrics
    g = np.random.default_rng(41)
    clouds = [(g.uniform(-1, 1, (300, 3)).astype(np.float32), g.uniform(-1, 1, (400, 3)).astype(np.float32)),
              (g.uniform(-1, 1, (257, 3)).astype(np.float32), g.uniform(-1, 1, (123, 3)).astype(np.float32))]
    m = ChamferDistanceMetrics(norm=norm, max_dist=max_dist, rmse=rmse)
    p2g, g2p = [], []
    for p, t in clouds:
        m.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
        for a, b_, acc in ((p, t, p2g), (t, p, g2p)):
            d = cKDTree(b_.astype(np.float64)).query(a.astype(np.float64), p=norm)[0]
            d = d * d if norm == 2 else d
            acc.append(np.minimum(d, max_dist) if max_dist is not None else d)
    p2g, g2p = np.concatenate(p2g), np.concatenate(g2p)
    assert len(m.pred_to_gt) == 557 and len(m.gt_to_pred) == 523
    if rmse:
        want = {"accuracy_rmse": np.sqrt((p2g ** 2).mean()), "completion_rmse": np.sqrt((g2p ** 2).mean())}
        want["chamfer_distance_rmse"] = 0.5 * want["accuracy_rmse"] + 0.5 * want["completion_rmse"]
    else:
        want = {"accuracy": p2g.mean(), "completion": g2p.mean()}
        want["chamfer_distance"] = 0.5 * want["accuracy"] + 0.5 * want["completion"]
    got = m.compute()
    assert set(got) == set(want)
    for k in want:
        assert float(got[k]) == pytest.approx(want[k], rel=1e-5), k
    m.sync()  # world size 1: nothing changes
    again = m.compute()
    assert all(float(again[k]) == float(got[k]) for k in got)
