"""umeyama_alignment_from_points on the host (no GPU): numpy's fp32 percentile restated operation by
operation, the reference's outputs (tests/golden/points_alignment.npz, written by
tests/golden/gen_points_alignment.py from the reference's own code), the per-point layout, and the
C ABI's declarations.

Tolerances.  The fixture holds what the reference computes in fp32 numpy; the host function is held to
the fixture within 2 x the error of the fp32 model of edge_rules (_umeyama_torch in fp32 against its
fp64 form on the same samples): no fixed number."""
import os
import re

import numpy as np
import pytest
import torch

from edge_rules import F32, F64, _done
from points_alignment_rules import CASES, GOLDEN, host_rule, load_case, percentile32, samples, solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectors(P, g):
    """Confidence-like vectors of P floats: several binades, ties, adjacent floats."""
    out = [np.exp2(g.uniform(-12, 6, P)).astype(np.float32),
           (1.0 + np.floor(g.random(P) * 3.0)).astype(np.float32),
           np.nextafter(np.float32(1.5), np.float32(2.0)) * np.ones(P, np.float32)]
    adj = np.full(P, 1.5, np.float32)
    adj[g.random(P) < 0.5] = np.nextafter(np.float32(1.5), np.float32(2.0))
    out.append(adj)
    out.append((g.standard_normal(P) * 100.0).astype(np.float32))
    return out


def test_fp32_percentile_restatement_is_numpys_bit_for_bit():
    g = np.random.default_rng(0)
    checked = 0
    for P in range(1, 41):
        for v in _vectors(P, g):
            for q in (0, 10, 25, 37.5, 50, 90, 99.5, 100):
                want = np.percentile(v, float(q))
                got, a, c = percentile32(v, float(q))
                assert want.dtype == np.float32
                assert got.view(np.uint32) == want.view(np.uint32), (P, q, float(got), float(want), v.tolist())
                assert min(a, c) <= got <= max(a, c)
                checked += 1
    assert checked == 40 * 5 * 8


def test_fp32_percentile_restatement_with_a_nan():
    v = np.array([1.0, np.nan, 3.0, 2.0], np.float32)
    assert np.isnan(np.percentile(v, 50.0)) and np.isnan(percentile32(v, 50.0)[0])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", CASES)
def test_host_reference_layout_reproduces_the_fixture(golden, name):
    from aligned_vggt.utils.alignment import umeyama_alignment_from_points
    c = load_case(golden, name)
    q = float(c["q"])
    T, sc = umeyama_alignment_from_points(c["pred"], c["conf"], c["gt"], c["mask"], q)
    Tt, sct = umeyama_alignment_from_points(torch.from_numpy(c["pred"]), torch.from_numpy(c["conf"]),
                                            torch.from_numpy(c["gt"]), torch.from_numpy(c["mask"]), q,
                                            columns="reference")
    assert np.array_equal(T, Tt) and np.array_equal(sc, sct)  # host tensors take the same numpy code
    T64, c64, n, _ = solve_batch(c["pred"], c["conf"], c["gt"], c["mask"], q, "reference", F64)
    T32, c32, _, _ = solve_batch(c["pred"], c["conf"], c["gt"], c["mask"], q, "reference", F32)
    assert n == c["n"].tolist()
    errs = []
    B = T.shape[0]
    assert T.shape == (B, 4, 4) and sc.shape == (B,)
    assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)))
    host_rule(errs, f"{name} T", torch.from_numpy(T[:, :3]), torch.from_numpy(c["T"][:, :3]), T32[:, :3], T64[:, :3])
    host_rule(errs, f"{name} scale", torch.from_numpy(sc).reshape(B, 1), torch.from_numpy(c["scale"]).reshape(B, 1),
              c32.reshape(B, 1), c64.reshape(B, 1))
    # the fixture itself is the fp32 arithmetic of section 1: within the same rule of the fp64 restatement
    host_rule(errs, f"{name} fixture T", torch.from_numpy(c["T"][:, :3]), T64[:, :3], T32[:, :3], T64[:, :3])
    _done(errs)


@pytest.mark.parametrize("name", CASES)
def test_host_points_layout_is_the_per_point_fit(golden, name):
    from aligned_vggt.utils.alignment import umeyama_alignment_from_points
    c = load_case(golden, name)
    q = float(c["q"])
    T, sc = umeyama_alignment_from_points(c["pred"], c["conf"], c["gt"], c["mask"], q, columns="points")
    T64, c64, _, _ = solve_batch(c["pred"], c["conf"], c["gt"], c["mask"], q, "points", F64)
    T32, c32, _, _ = solve_batch(c["pred"], c["conf"], c["gt"], c["mask"], q, "points", F32)
    B = T.shape[0]
    errs = []
    host_rule(errs, f"{name} T", torch.from_numpy(T[:, :3]), T64[:, :3], T32[:, :3], T64[:, :3])
    host_rule(errs, f"{name} scale", torch.from_numpy(sc).reshape(B, 1), c64.reshape(B, 1), c32.reshape(B, 1),
              c64.reshape(B, 1))
    if name != "tiny":  # three points fit any similarity closely; the others recover the generator's 1.4
        assert np.all(np.abs(sc - 1.4) < 0.05), sc
    _done(errs)


def test_columns_argument_is_checked():
    from aligned_vggt.utils.alignment import umeyama_alignment_from_points
    z = np.zeros((1, 1, 1, 4, 3), np.float32)
    with pytest.raises(ValueError, match="columns"):
        umeyama_alignment_from_points(z, z[..., 0], z, z[..., 0] > -1, 50.0, columns="transpose")


def test_samples_layouts():
    rows = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert samples(rows, "points")[1].tolist() == [3.0, 4.0, 5.0]
    assert samples(rows, "reference")[1].tolist() == [1.0, 5.0, 9.0]  # (Xf[i], Xf[n + i], Xf[2n + i])


def test_header_and_signature_table_list_the_entry_points():
    from aligned_vggt import _native
    hdr = open(os.path.join(ROOT, "include", "vggt_mi355x.h")).read()
    for fn in ("vggt_gt_points_align", "vggt_gt_points_align_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
    assert "vggt_gt_points_align" in _native._SIGS
    assert "vggt_gt_points_align_ws_bytes" in _native._WS_FNS
    group = int(re.search(r"#define VGGT_GT_POINTS_GROUP (\d+)", hdr).group(1))
    words = int(re.search(r"#define VGGT_GT_POINTS_STATE_BYTES (\d+)", hdr).group(1)) // 8
    assert (group, words) == (_native.GT_POINTS_GROUP, _native.GT_POINTS_STATE_WORDS)
    assert (_native.GT_POINTS_REFERENCE, _native.GT_POINTS_POINTS) == (0, 1)
