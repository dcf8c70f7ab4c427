"""Per-batch-element key-split tail of the global attention launch
(vggt_attention_fwd_ws, knob VGGT_TUNE_ATTN_TAIL_SPLIT with
ATTN_TAIL_SPLIT_PER_ELEMENT): the last `tail_blocks` (head, row block) units of
EVERY batch element run split over the keys, so an element's bits are the same
alone and inside any batch.  All at H = 2, D = 64, nq = 4100 (17 row blocks of
256 per head, the last holding 4 rows: 34 units per element), 8-wave workgroups,
B = 3.  q, k, v and o have batch strides larger than nq / nk rows (all four
different) with NaN in the gap rows, so a wrong (batch, unit, part) decode reads
or writes visibly."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, NQ, B = 2, 64, 4100, 3
C = H * D
NQB = (NQ + 255) // 256
UNITS = H * NQB  # per batch element
QS, OS = NQ + 16, NQ + 8  # batch strides in rows
SLAB_BYTES = (256 * D + 2 * 256) * 4
CASES = [(200, 2), (1374, 3)]  # (nk, parts): 4 tiles in 2 parts of 2; 22 tiles in 3 parts of 8, 8, 6
TAILS = [1, 5, 34]

# tests/test_gpu_attention_tail_split.py owns the fp64 bars of the split and derives this
# margin (what re-associating the fp32 sums over <= 4 parts may add to the unsplit error)
MARGIN = 5e-5


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


def _strided(x, n, stride):
    """[B * n, C] -> [B * stride, C] with NaN in the gap rows behind every element."""
    out = torch.full((B * stride, C), float("nan"), dtype=x.dtype)
    for b in range(B):
        out[b * stride:b * stride + n] = x[b * n:(b + 1) * n]
    return out


def _launch(N, dev, nk, knob, elems):
    """One launch over the batch elements `elems` (consecutive) with the tail-split knob at
    `knob`: [len(elems) * NQ, C] on the host.  o starts as NaN; its gap rows must stay NaN."""
    qd, kd, vd, ks, vs = dev
    b0, nb = elems[0], len(elems)
    prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
    prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
    try:
        o = torch.full((nb * OS, C), float("nan"), device="cuda", dtype=torch.bfloat16)
        N.attention(qd[b0 * QS:], kd[b0 * ks:], vd[b0 * vs:], o, nb, H, NQ, nk, D, QS, ks, OS, v_bstride=vs)
        torch.cuda.synchronize()
    finally:
        N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
        N.tune(N.TUNE_ATTN_WAVES, prev_w)
    o = o.cpu().view(nb, OS, C)
    assert torch.isnan(o[:, NQ:].float()).all(), "a gap row of o was written"
    return o[:, :NQ].reshape(nb * NQ, C).contiguous()


_INPUTS, _RUNS = {}, {}


def _inputs(N, nk):
    """Device inputs, the fp64 reference and the unsplit B = 3 launch for one key count, computed once."""
    if nk not in _INPUTS:
        g = torch.Generator().manual_seed(23 + nk)
        q = (torch.randn(B * NQ, C, generator=g) * 0.3).to(torch.bfloat16)
        k = (torch.randn(B * nk, C, generator=g) * 0.3).to(torch.bfloat16)
        v = torch.randn(B * nk, C, generator=g).to(torch.bfloat16)
        ks, vs = nk + 8, nk + 24
        dev = (_strided(q, NQ, QS).cuda(), _strided(k, nk, ks).cuda(), _strided(v, nk, vs).cuda(), ks, vs)
        ref = torch.cat([_ref64(q[b * NQ:(b + 1) * NQ], k[b * nk:(b + 1) * nk], v[b * nk:(b + 1) * nk])
                         for b in range(B)])
        _INPUTS[nk] = (dev, ref, _launch(N, dev, nk, -1, range(B)))
    return _INPUTS[nk]


def _batched(N, nk, parts, tail_blocks):
    """The B = 3 launch under the per-element forced knob, computed once per case."""
    key = (nk, parts, tail_blocks)
    if key not in _RUNS:
        dev, _, _ = _inputs(N, nk)
        _RUNS[key] = _launch(N, dev, nk, N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8, range(B))
    return _RUNS[key]


def _tail_mask(tail_blocks):
    """[B * NQ, C] bool: the elements written by the last `tail_blocks` (head, row block) units of every element."""
    m = torch.zeros(NQ, C, dtype=torch.bool)
    for u in range(UNITS - tail_blocks, UNITS):
        h, qb = divmod(u, NQB)
        m[qb * 256:(qb + 1) * 256, h * D:(h + 1) * D] = True
    return m.repeat(B, 1)


def _bits(x):
    return x.view(torch.int16)


@pytest.mark.parametrize("tail_blocks", TAILS)
@pytest.mark.parametrize("nk,parts", CASES)
def test_batched_element_is_bitwise_its_solo_launch(N, nk, parts, tail_blocks):
    dev, _, _ = _inputs(N, nk)
    got = _batched(N, nk, parts, tail_blocks)
    assert torch.isfinite(got.float()).all()
    knob = N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8
    for b in range(B):
        solo = _launch(N, dev, nk, knob, [b])
        assert torch.equal(_bits(got[b * NQ:(b + 1) * NQ]), _bits(solo)), f"batch element {b}"


@pytest.mark.parametrize("tail_blocks", TAILS)
@pytest.mark.parametrize("nk,parts", CASES)
def test_per_element_and_launch_global_layouts_agree_for_one_element(N, nk, parts, tail_blocks):
    dev, _, _ = _inputs(N, nk)
    per_elem = _launch(N, dev, nk, N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8, [0])
    launch_global = _launch(N, dev, nk, parts | tail_blocks << 8, [0])
    assert torch.equal(_bits(per_elem), _bits(launch_global))


@pytest.mark.parametrize("tail_blocks", TAILS)
@pytest.mark.parametrize("nk,parts", CASES)
def test_whole_units_are_bitwise_the_unsplit_launch(N, nk, parts, tail_blocks):
    _, _, unsplit = _inputs(N, nk)
    got = _batched(N, nk, parts, tail_blocks)
    whole = ~_tail_mask(tail_blocks)
    assert torch.equal(_bits(got)[whole], _bits(unsplit)[whole])


@pytest.mark.parametrize("tail_blocks", TAILS)
@pytest.mark.parametrize("nk,parts", CASES)
def test_tail_rows_stay_within_the_margin_of_the_unsplit_error(N, nk, parts, tail_blocks):
    _, ref, unsplit = _inputs(N, nk)
    got = _batched(N, nk, parts, tail_blocks)
    tail = _tail_mask(tail_blocks)
    for b in range(B):
        sl = slice(b * NQ, (b + 1) * NQ)
        t = tail[sl]
        e_split, e_unsplit = _rel(got[sl][t], ref[sl][t]), _rel(unsplit[sl][t], ref[sl][t])
        print(f"nk={nk} parts={parts} tail_blocks={tail_blocks} element {b}: tail rows rel-L2 vs fp64 "
              f"split {e_split:.4e} unsplit {e_unsplit:.4e}")
        assert e_split <= e_unsplit + MARGIN, (b, e_split, e_unsplit)


def _ws_bytes(N, batch, nk, knob):
    prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
    prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
    try:
        return N.lib().vggt_attention_ws_bytes(batch, H, NQ, nk, D, None)
    finally:
        N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
        N.tune(N.TUNE_ATTN_WAVES, prev_w)


@pytest.mark.parametrize("nk,parts", CASES)
def test_workspace_scales_with_batch(N, nk, parts):
    for tail_blocks in TAILS:
        knob = N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8
        one = _ws_bytes(N, 1, nk, knob)
        assert one == tail_blocks * parts * SLAB_BYTES
        assert _ws_bytes(N, B, nk, knob) == B * one
    # more tail blocks than an element has units: every unit of every element, no more
    assert _ws_bytes(N, B, nk, N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | 1000 << 8) == B * UNITS * parts * SLAB_BYTES


def test_short_workspace_is_an_error_and_launches_nothing(N):
    """The buffer handed over is full size (nothing could be written out of bounds);
    only the size the launch is told is one slab short."""
    nk, parts, tail_blocks = 200, 2, 5
    dev, _, _ = _inputs(N, nk)
    qd, kd, vd, ks, vs = dev
    knob = N.ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8
    need = _ws_bytes(N, B, nk, knob)
    assert need == B * tail_blocks * parts * SLAB_BYTES
    ws = torch.zeros(need // 4, device="cuda", dtype=torch.float32)
    o = torch.full((B * OS, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    prev_w = N.tune(N.TUNE_ATTN_WAVES, 8)
    prev_s = N.tune(N.TUNE_ATTN_TAIL_SPLIT, knob)
    try:
        rc = N.lib().vggt_attention_fwd_ws(
            N._p(qd), N._ld(qd), QS, N._p(kd), N._ld(kd), ks, N._p(vd), N._ld(vd), vs, N._p(o), N._ld(o), OS,
            B, H, NQ, nk, D, float(D ** -0.5), N._p(ws), ctypes.c_size_t(need - SLAB_BYTES), N._stream())
        torch.cuda.synchronize()
    finally:
        N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev_s)
        N.tune(N.TUNE_ATTN_WAVES, prev_w)
    assert rc == N.VGGT_ERR_SHAPE
    assert torch.isnan(o.float()).all() and not ws.any()
