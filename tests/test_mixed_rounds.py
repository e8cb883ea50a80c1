"""Side-window size of a mixed ADMM round (csrc/sqp_sched.cpp: qp_mix_split, through sco_debug_mix_split): host arithmetic only.

A mixed round runs k of the live problems on the row-local kernel (one per CU) beside the wavefront launch over the rest
(four per CU).  Workgroups are dealt to the XCDs in rotation, so the room is counted per XCD."""
import pytest

from sco_py_amd import _lib

PER_CU = 4
CHIPS = [(256, 8), (304, 8), (64, 1)]


def _up(a, b):
    return -(-a // b)


def _split(live, cus, xcds, slack):
    return _lib.load().sco_debug_mix_split(live, cus, xcds, slack, PER_CU)


def _fits(k, live, cus, xcds, slack):
    return _up(k, xcds) + slack + _up(_up(live - k, xcds), PER_CU) <= cus // xcds


def test_the_recorded_live_counts():
    assert [_split(live, 256, 8, 1) for live in (1001, 904, 776, 621)] == [0, 24, 72, 120]


@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("cus,xcds", CHIPS)
def test_split_over_every_live_count(cus, xcds, slack):
    ks = {live: _split(live, cus, xcds, slack) for live in range(1, 4 * cus + 1)}
    for live, k in ks.items():
        assert 0 <= k <= live
        if k:
            assert _fits(k, live, cus, xcds, slack), (live, k)                      # the per-XCD inequality
            # ... and k is the largest such count (no whole CU is free at live > 4 (cus - 1): see the next assertion)
            assert not any(_fits(j, live, cus, xcds, slack) for j in range(k + 1, min(live, cus) + 1)), (live, k)
        elif live <= PER_CU * (cus - 1):
            assert not any(_fits(j, live, cus, xcds, slack) for j in range(1, min(live, cus) + 1)), live
        assert k + _up(live - k, PER_CU)<= cus, (live, k)              # both launches fit the chip
        if live >= 4 * cus - 3:
            assert k == 0, live
        # k never falls when live falls -- until every live problem is in the side window (k = live, a count that can only
        # fall with live; the SQP loop runs row-local rounds long before)
        if live > 1:
            assert ks[live - 1] >= min(k, live - 1), (live, k, ks[live - 1])


def test_degenerate_arguments_give_no_side_window():
    assert _split(0, 256, 8, 1) == 0 and _split(-5, 256, 8, 1) == 0
    assert _split(500, 0, 8, 1) == 0 and _split(500, 256, 0, 1) == 0 and _split(500, 256, 8, -1) == 0
    assert _split(500, 250, 8, 1) == 0          # the XCDs do not divide the CUs: no per-XCD room to count
