"""Key-split tail of the global attention launch (vggt_attention_fwd_ws, knob
VGGT_TUNE_ATTN_TAIL_SPLIT forced): the last row blocks of the launch run as
2..4 workgroups over contiguous key ranges and a merge launch combines their
(m, l, O) partials.  All at H = 2, D = 64, nq = 4100 (17 row blocks of 256 per
head, the last holding 4 rows), 8-wave workgroups."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, NQ = 2, 64, 4100
C = H * D
NQB = (NQ + 255) // 256


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from aligned_vggt import _native
    _native.lib()
    return _native


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ref64(q, k, v):
    """fp64 host softmax attention of bf16-rounded [n, H*D] inputs."""
    qh = q.double().view(-1, H, D).permute(1, 0, 2)
    kh = k.double().view(-1, H, D).permute(1, 0, 2)
    vh = v.double().view(-1, H, D).permute(1, 0, 2)
    s = (qh @ kh.transpose(-1, -2)) * D ** -0.5
    return (torch.softmax(s, -1) @ vh).permute(1, 0, 2).reshape(-1, C)


def _run(N, q, k, v, knob):
    """One launch through _native.attention with the tail-split knob at `knob`."""
    nq, nk = q.shape[0], k.shape[0]
    prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
    prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
    try:
        o = torch.empty(nq, C, device="cuda", dtype=torch.bfloat16)
        N.attention(q.cuda(), k.cuda(), v.cuda(), o, 1, H, nq, nk, D, nq, nk, nq)
        torch.cuda.synchronize()
    finally:
        N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
        N.tune(N.TUNE_ATTN_WAVES, prev_w)
    return o.cpu()


_CASES = {}


def _case(N, nk):
    """Inputs, fp64 reference and the unsplit output for one key count, computed once."""
    if nk not in _CASES:
        g = torch.Generator().manual_seed(11 + nk)
        q = (torch.randn(NQ, C, generator=g) * 0.3).to(torch.bfloat16)
        k = (torch.randn(nk, C, generator=g) * 0.3).to(torch.bfloat16)
        v = torch.randn(nk, C, generator=g).to(torch.bfloat16)
        _CASES[nk] = (q, k, v, _ref64(q, k, v), _run(N, q, k, v, -1))
    return _CASES[nk]


def _tail_mask(tail_blocks):
    """[NQ, C] bool: the elements written by the last `tail_blocks` (head, row block) units."""
    m = torch.zeros(NQ, C, dtype=torch.bool)
    for u in range(H * NQB - tail_blocks, H * NQB):
        h, qb = divmod(u, NQB)
        m[qb * 256:(qb + 1) * 256, h * D:(h + 1) * D] = True
    return m


# What the split may add to the unsplit error: the parts' fp32 sums are
# re-associated over <= 4 parts, a relative change of <= 4 * 2^-24 = 2.4e-7 of
# a value before it is rounded to bf16 (the probabilities themselves are the
# same: these rows sit at offset 0 in every part).  That moves about
# 2.4e-7 / 2^-8 = 6e-5 of the elements across a bf16 rounding boundary, by one
# ulp (2^-8 relative) each: ||split - unsplit|| / ||ref|| <~ sqrt(6e-5) * 2^-8 =
# 3e-5, and by the triangle inequality the error grows by no more than that.
# (Measured on the first GPU run: see profiles/r12/ab_attn_tail_split.md.)
MARGIN = 5e-5
HARD_CAP = 6e-3


@pytest.mark.parametrize("parts,tail_blocks", [(2, 17), (3, 5), (4, 1)])
@pytest.mark.parametrize("nk", [65, 200, 1374])
def test_tail_split_accuracy(N, nk, parts, tail_blocks):
    """nk = 65 with 4 parts exercises the clamp to the tile count (2 parts run);
    nk = 200 with 4 parts gives one-tile parts, the last holding 8 keys."""
    q, k, v, ref, unsplit = _case(N, nk)
    # the forced launch does split: its workspace holds tail_blocks x (parts as run) partials
    nt = (nk + 63) // 64
    per = -(-nt // min(parts, nt))
    parts_run = -(-nt // per)
    assert parts_run >= 2
    prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
    prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, parts | tail_blocks << 8)
    try:
        need = N.lib().vggt_attention_ws_bytes(1, H, NQ, nk, D, None)
    finally:
        N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
        N.tune(N.TUNE_ATTN_WAVES, prev_w)
    assert need == tail_blocks * parts_run * (256 * D + 2 * 256) * 4
    got = _run(N, q, k, v, parts | tail_blocks << 8)
    assert torch.isfinite(got.float()).all()
    e_split, e_unsplit = _rel(got, ref), _rel(unsplit, ref)
    tail = _tail_mask(tail_blocks)
    e_split_t, e_unsplit_t = _rel(got[tail], ref[tail]), _rel(unsplit[tail], ref[tail])
    print(f"nk={nk} parts={parts} tail_blocks={tail_blocks}: rel-L2 vs fp64 split {e_split:.4e} unsplit "
          f"{e_unsplit:.4e}; tail rows only split {e_split_t:.4e} unsplit {e_unsplit_t:.4e}")
    assert e_split <= e_unsplit + MARGIN, (e_split, e_unsplit)
    assert e_split_t <= e_unsplit_t + MARGIN, (e_split_t, e_unsplit_t)
    assert e_split < HARD_CAP and e_split_t < HARD_CAP
    # every row outside the tail blocks is bitwise the unsplit launch's
    assert torch.equal(got.view(torch.int16)[~tail], unsplit.view(torch.int16)[~tail])


def test_tail_split_batched(N):
    """Two batches: the tail (40 units) covers all of batch 1 and the last 6 units of batch 0."""
    nk, B, tail_blocks = 200, 2, 40
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(B * NQ, C, generator=g) * 0.3).to(torch.bfloat16)
    k = (torch.randn(B * nk, C, generator=g) * 0.3).to(torch.bfloat16)
    v = torch.randn(B * nk, C, generator=g).to(torch.bfloat16)

    def run(knob):
        prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
        prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
        try:
            o = torch.empty(B * NQ, C, device="cuda", dtype=torch.bfloat16)
            N.attention(q.cuda(), k.cuda(), v.cuda(), o, B, H, NQ, nk, D, NQ, nk, NQ)
            torch.cuda.synchronize()
        finally:
            N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
            N.tune(N.TUNE_ATTN_WAVES, prev_w)
        return o.cpu()

    unsplit, got = run(-1), run(2 | tail_blocks << 8)
    ref = torch.cat([_ref64(q[b * NQ:(b + 1) * NQ], k[b * nk:(b + 1) * nk], v[b * nk:(b + 1) * nk]) for b in range(B)])
    tail = torch.cat([_tail_mask(tail_blocks - H * NQB), _tail_mask(H * NQB)])  # batch 0: 6 units, batch 1: all
    e_split, e_unsplit = _rel(got[tail], ref[tail]), _rel(unsplit[tail], ref[tail])
    print(f"batched: tail rows rel-L2 vs fp64 split {e_split:.4e} unsplit {e_unsplit:.4e}")
    assert e_split <= e_unsplit + MARGIN and e_split < HARD_CAP, (e_split, e_unsplit)
    assert torch.equal(got.view(torch.int16)[~tail], unsplit.view(torch.int16)[~tail])


NK_X = 1374  # 22 tiles; 4 parts of 6 tiles: keys [0, 384), [384, 768), [768, 1152), [1152, 1374)


@pytest.mark.parametrize("case", ["high_one_part", "low_one_part", "overflow_late_last_part", "mixed_rows"])
def test_tail_split_offsets_across_parts(N, case):
    """The offset-free softmax's extreme constructions placed so that the parts
    of one row end with different offsets m_i; every unit is split in 4."""
    g = torch.Generator().manual_seed(7)
    q = torch.randn(NQ, C, generator=g) * 0.3
    k = torch.randn(NK_X, C, generator=g) * 0.3
    v = torch.randn(NK_X, C, generator=g)
    if case == "high_one_part":
        # first tile of part 1 only: score 128 (log2 units +185 > 60); the other parts stay at
        # offset 0 and their weights 2^(0 - 185) underflow to 0
        q[:64] = 4.0
        k[384 + 3] = 4.0
    elif case == "low_one_part":
        # every score of part 2 ~ -112 (log2 units -161 < -60): that part carries offset -161
        q[:64] = 4.0
        k[768:1152] = -3.5 + 0.05 * torch.randn(384, C, generator=g)
    elif case == "overflow_late_last_part":
        # overflows 2^60 only in the third tile of the last part
        q[:40] = 4.0
        k[NK_X - 50] = 4.0
    else:
        # offset and zero-offset rows in one wave; +60 in part 0, larger still in part 3, -60 in part 2
        q[0:128:2] = 4.0
        q[NQ - 260:NQ - 132:2] = 4.0
        k[10] = 4.0
        k[NK_X - 100] = 4.5
        k[800:900] = -3.5
    q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
    got = _run(N, q, k, v, 4 | (H * NQB) << 8)
    ref = _ref64(q, k, v)
    assert torch.isfinite(got.float()).all()
    err = _rel(got, ref)
    row_err = ((got.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-6)).max().item()
    print(f"{case}: rel-L2 {err:.4e}, worst row {row_err:.4e}")
    assert err < 1e-2, err
    assert row_err < 5e-2, row_err


def test_tail_split_deterministic(N):
    q, k, v, _, _ = _case(N, 1374)
    a = _run(N, q, k, v, 3 | 20 << 8)
    b = _run(N, q, k, v, 3 | 20 << 8)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
