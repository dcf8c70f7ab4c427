"""Which forward kernel vggt_attention_fwd launches (vggt_attention_fwd_form): host
arithmetic only, so it runs without a device.  `ladder` below restates the dispatch as
it stood before the library had one resolver -- a chain of special cases in
attention_fwd_impl, read off that code rule by rule, not off the resolver -- and the
library's answer must match it for every accepted variant, wave count, 16x16 setting,
head size and query count on either side of the 8-wave threshold."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest

ACCEPTED = (3, 7, 11, 15, 19, 23, 32, 33, 96, 97, 161, 289, 545, 2081, 4129)
WAVES = (2, 4, 8)
ATTN16 = (0, 1, 2)
HEAD = (64, 128)
NQ = (1, 4095, 4096)
TUNE_WAVES, TUNE_VARIANT, TUNE_ATTN16 = 2, 3, 5


def ladder(variant, waves, attn16, dma_half, D, nq):
    """(form16, waves per workgroup, kernel schedule bits); bits 0 for the 16x16 form."""
    if waves == 8 and nq >= 4096:
        nw = 8
    elif waves == 2 and (variant & 32) and (variant & 65) == 1:
        nw = 2
    else:
        nw = 4
    if D == 64 and nw != 2 and (variant == 161 or (variant == 33 and (attn16 == 1 or (attn16 == 2 and nw == 4)))):
        return 1, nw, 0
    if variant in (19, 23) and D == 64:  # (nw is never 2 here: 19 and 23 lack bit 5)
        return 0, nw, variant
    if dma_half and variant == 33 and D == 64 and nw == 8:
        return 0, nw, 2081
    if variant in (4129, 2081) and D == 64 and nw != 2:
        return 0, nw, variant if nw == 8 else 33
    if variant in (545, 289) and D == 64 and nw != 2:
        return 0, nw, variant
    if variant & 32:
        return 0, nw, 32 + (variant & 1) + (variant & 64)
    return 0, nw, variant & 15


def stamps_ladder(variant, waves, dma_half, nq):
    """(waves per workgroup, schedule bits) of vggt_attention_stamps, from the four branches it
    had: D = 64, the 16x16 setting ignored, 2 waves taken as 4, every result with the stamps bit."""
    nw = 8 if waves == 8 and nq >= 4096 else 4
    if nw == 8 and (variant == 2081 or (variant == 33 and dma_half)):
        return nw, 2081 | 1024
    if nw == 8 and variant == 4129:
        return nw, 4129 | 1024
    return nw, 33 | 1024


def sweep(lib):
    """{"variant,waves,attn16,D,nq": [form16, nw, var, launchable]} over the cross product, and
    {"stamps,variant,waves,attn16,nq": [nw, var, launchable]} for vggt_attention_stamps; leaves
    the three knobs as it found them."""
    tune = lib.vggt_tune
    prev = [(k, tune(k, v)) for k, v in ((TUNE_VARIANT, 33), (TUNE_WAVES, 8), (TUNE_ATTN16, 2))]
    out = {}
    try:
        for variant, waves, attn16 in itertools.product(ACCEPTED, WAVES, ATTN16):
            assert tune(TUNE_VARIANT, variant) >= 0 and tune(TUNE_WAVES, waves) >= 0 and tune(TUNE_ATTN16, attn16) >= 0
            for D, nq in itertools.product(HEAD, NQ):
                f, w, v = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
                rc = lib.vggt_attention_fwd_form(D, nq, ctypes.byref(f), ctypes.byref(w), ctypes.byref(v))
                out["%d,%d,%d,%d,%d" % (variant, waves, attn16, D, nq)] = [f.value, w.value, v.value, rc == 0]
            for nq in NQ:
                w, v = ctypes.c_int(-1), ctypes.c_int(-1)
                rc = lib.vggt_attention_stamps_form(nq, ctypes.byref(w), ctypes.byref(v))
                out["stamps,%d,%d,%d,%d" % (variant, waves, attn16, nq)] = [w.value, v.value, rc == 0]
    finally:
        for k, v in reversed(prev):
            tune(k, v)
    return out


def check(got, dma_half):
    assert len(got) == len(ACCEPTED) * len(WAVES) * len(ATTN16) * (len(HEAD) + 1) * len(NQ)
    wrong = []
    for key, val in got.items():
        if key.startswith("stamps,"):
            variant, waves, attn16, nq = map(int, key.split(",")[1:])
            if tuple(val) != stamps_ladder(variant, waves, dma_half, nq) + (True,):
                wrong.append((key, val, stamps_ladder(variant, waves, dma_half, nq)))
            continue
        f, w, v, ok = val
        variant, waves, attn16, D, nq = map(int, key.split(","))
        want = ladder(variant, waves, attn16, dma_half, D, nq)
        if (f, w, v) != want or not ok:
            wrong.append((key, (f, w, v, ok), want))
    assert not wrong, wrong[:10]


@pytest.fixture(scope="module")
def native():
    from aligned_vggt import _native
    _native.lib()
    return _native


def test_resolver_matches_the_ladder_and_every_form_is_launchable(native):
    lib = native.lib()

    def knobs():
        now = []
        for k, v in ((TUNE_VARIANT, 33), (TUNE_WAVES, 8), (TUNE_ATTN16, 2)):
            now.append(lib.vggt_tune(k, v))
            lib.vggt_tune(k, now[-1])
        return now

    before = knobs()
    dma_half = int(os.environ.get("VGGT_ATTN_DMA_HALF", "1")) != 0
    check(sweep(lib), dma_half)
    assert knobs() == before


def test_wrapper_and_unsupported_head_size(native):
    f, w, v, ok = native.attention_fwd_form(128, 4096)
    assert ok and f == 0 and w in (4, 8)
    assert native.attention_fwd_form(96, 4096)[3] is False
    w, v, ok = native.attention_stamps_form(4096)
    assert ok and w in (4, 8) and v & 1024


_CHILD = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[2])
import test_attention_fwd_form as T
print(json.dumps(T.sweep(ctypes.CDLL(sys.argv[1]))))
"""


def test_dma_half_off_in_a_fresh_process(native):
    """VGGT_ATTN_DMA_HALF is read once when the library loads: a child process that only
    loads the library and asks."""
    env = dict(os.environ, VGGT_ATTN_DMA_HALF="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, native.LIB_PATH, os.path.dirname(os.path.abspath(__file__))],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    check(got, False)
    assert got["33,8,0,64,4096"][:3] == [0, 8, 33]  # every wave issues its own DMA piece
    assert got["stamps,33,8,0,4096"][:2] == [8, 33 | 1024]
