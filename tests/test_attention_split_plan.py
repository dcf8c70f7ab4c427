"""Host policy of the key-split attention tail (vggt_attention_split_plan): pure
host arithmetic on the slot model -- two 8-wave workgroups per compute unit --,
so it runs without a device."""
import pytest

UNITS = 86 * 16  # 21,984 rows in 256-row blocks x 16 heads


@pytest.fixture(scope="module")
def plan():
    from aligned_vggt import _native
    _native.lib()
    return _native.attention_split_plan


def test_model_shape_splits_its_last_partial_round(plan):
    got = plan(1, 16, 21984, 21984, 64, 256)
    assert got is not None
    tail, parts = got
    assert tail == UNITS % 512 == 352  # the row blocks of the last, partial round of 512 slots
    assert parts in (2, 3, 4)


@pytest.mark.parametrize("n", [16384, 24576])
def test_whole_rounds_do_not_split(plan, n):
    assert plan(1, 16, n, n, 64, 256) is None


def test_less_than_one_round_does_not_split(plan):
    assert plan(1, 16, 6592, 6592, 64, 256) is None  # 26 x 16 = 416 units < 512 slots


def test_short_key_ranges_do_not_split(plan):
    # 2 x 16 x 26 = 832 units = 1.625 rounds, but 103 key tiles: parts would be shorter than any measured to pay
    assert plan(2, 16, 6592, 6592, 64, 256) is None


def test_short_launches_do_not_split(plan):
    # nq < 4096 never takes the 8-wave path, however many units the batch makes
    assert plan(64, 16, 4000, 4000, 64, 256) is None
    assert plan(1, 16, 21984, 21984, 128, 256) is None  # D = 64 only


def test_masked_stream_cu_count_changes_the_slots(plan):
    # 192 CUs: 384 slots, the last round holds 1376 % 384 = 224 units (32 CUs with two of them)
    got = plan(1, 16, 21984, 21984, 64, 192)
    assert got is not None and got[0] == UNITS % 384 == 224
    # 128 CUs: 256 slots, 96 units left, each alone on its CU (a lone workgroup has the
    # matrix pipe to itself): nothing to gain
    assert plan(1, 16, 21984, 21984, 64, 128) is None
    # 172 CUs: 344 slots, 1376 = 4 x 344, whole rounds
    assert plan(1, 16, 21984, 21984, 64, 172) is None
