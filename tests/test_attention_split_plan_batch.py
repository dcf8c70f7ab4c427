"""The key-split plan of a batched launch (vggt_attention_split_plan) is the plan
of one batch element, applied to every element: a chunk gets the same split
rows in the same parts alone or inside any batch.  Pure host arithmetic, so it
runs without a device."""
import pytest


@pytest.fixture(scope="module")
def N():
    from aligned_vggt import _native
    _native.lib()
    return _native


@pytest.mark.parametrize("b", [2, 3, 8])
def test_batched_plan_is_the_one_element_plan(N, b):
    one = N.attention_split_plan(1, 16, 21984, 21984, 64, 256)
    assert one is not None and one[0] == (86 * 16) % 512 == 352
    assert N.attention_split_plan(b, 16, 21984, 21984, 64, 256) == one


@pytest.mark.parametrize("n", [6592, 16384])
def test_unsplit_elements_stay_unsplit_in_a_batch(N, n):
    # 6592: 416 units per element, less than one round of 512 slots; 16384: whole rounds.  Two of
    # them together make a partial round (832, 2048 units), which no longer decides anything
    assert N.attention_split_plan(1, 16, n, n, 64, 256) is None
    assert N.attention_split_plan(2, 16, n, n, 64, 256) is None


def test_plan_is_the_default(N):
    # vggt_tune returns the previous value: set "off", read the default back, restore it
    prev = N.tune(N.TUNE_ATTN_TAIL_SPLIT, -1)
    N.tune(N.TUNE_ATTN_TAIL_SPLIT, prev)
    assert prev == 0
