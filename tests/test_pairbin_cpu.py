"""The band planner of the pair-binning engine (sx_pairbin.hpp) on the host, through sx_pair_bands_internal: whole rows
packed greedily under the pair cap, and the two refusals.  The 2^31 limit is out of reach of a GPU test of a few
seconds, so it is checked here."""
import pytest

import sphexa_amd as sx

DEFAULT_CAP = 1 << 27
MAX_BAND = 2 ** 31 - 1


def test_rows_without_pairs_make_one_band():
    assert sx.pair_bands([0, 0, 0, 0, 0]) == [(0, 5)]
    assert sx.pair_bands([0]) == [(0, 1)]
    assert sx.pair_bands([0, 0, 0], cap=1) == [(0, 3)]


def test_a_row_at_the_cap_is_accepted_and_one_above_is_refused():
    assert sx.pair_bands([1000], cap=1000) == [(0, 1)]
    assert sx.pair_bands([1, 1000, 1], cap=1000) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(sx.SxError, match=r"code 4: sx_map_render: one tile row holds 1001 pairs, more than the pair cap of "
                                         r"1000 \(sx_set_map_pair_cap\)$"):
        sx.pair_bands([1, 1001, 1], cap=1000)
    assert sx.SX_ERR_ARG == 4


def test_whole_rows_are_packed_greedily():
    assert sx.pair_bands([3, 3, 3, 3], cap=6) == [(0, 2), (2, 4)]
    assert sx.pair_bands([3, 3, 3, 3], cap=5) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert sx.pair_bands([3, 3, 3, 3], cap=0) == [(0, 4)]
    assert sx.pair_bands([5, 1, 1, 4, 2, 6], cap=6) == [(0, 2), (2, 4), (4, 5), (5, 6)]


def test_cap_zero_is_the_default_cap():
    assert sx.pair_bands([DEFAULT_CAP], cap=0) == [(0, 1)]
    assert sx.pair_bands([DEFAULT_CAP - 1, 1, 1], cap=0) == [(0, 2), (2, 3)]
    with pytest.raises(sx.SxError, match=r"code 4.*pair cap of %d " % DEFAULT_CAP):
        sx.pair_bands([DEFAULT_CAP + 1], cap=0)


@pytest.mark.parametrize("cap", [0, 1, 1 << 27, MAX_BAND, 1 << 40])
def test_a_row_of_2_to_the_31_is_refused_whatever_the_cap(cap):
    with pytest.raises(sx.SxError, match=r"code 4: sx_map_render: one tile row holds more than 2\^31 - 1 pairs "
                                         r"\(render a smaller window or fewer particles at a time\)$"):
        sx.pair_bands([1, 2 ** 31], cap=cap)


def test_a_cap_above_the_sort_limit_is_clamped_to_it():
    assert sx.pair_bands([MAX_BAND], cap=1 << 40) == [(0, 1)]
    # two rows that a cap of 2^40 would take as one band
    assert sx.pair_bands([MAX_BAND, 1], cap=1 << 40) == [(0, 1), (1, 2)]
    assert sx.pair_bands([MAX_BAND - 1, 1, 1], cap=2 ** 64 - 1) == [(0, 2), (2, 3)]
