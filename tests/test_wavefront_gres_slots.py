"""The slot mapping of the G-resident sweep of the wavefront ADMM tier (csrc/layout_wv.h: wv_gres_slot, through
sco_debug_wv_gres_slot), without a GPU: which DPP row pair runs which block position, in which register slot, and where the
position's right-hand side / x~ and couplings sit in LDS.  For every NSTEP the tier builds and every horizon it serves."""
import ctypes as C

import numpy as np
import pytest

from sco_py_amd import _lib

NSTEPS = (4, 8, 10)


def slot(nstep, pos):
    out = np.full(5, -7, dtype=np.int32)
    assert _lib.load().sco_debug_wv_gres_slot(nstep, pos, out.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return tuple(int(v) for v in out)          # pair, row, slot, vidx, eidx


def wv_vidx(npos, pos, k):
    """csrc/layout_wv.h: wv_vidx (block vectors are stored piece-major)."""
    return (k >> 1) * 2 * npos + 2 * pos + (k & 1)


def positions(nstep, nb):
    """Block positions of a horizon of nb blocks in the NSTEP-step kernel (wv_plan_build: both chains padded at their
    START with dummy blocks): chain A, chain B in sweep order, each as (position, real block or None)."""
    mid, len_b = nb // 2, nb - 1 - nb // 2
    assert mid <= nstep and len_b <= nstep
    a = [(p, p - (nstep - mid) if p >= nstep - mid else None) for p in range(nstep)]
    b = [(nstep + 1 + s, nb - 1 - (s - (nstep - len_b)) if s >= nstep - len_b else None) for s in range(nstep)]
    return a, b


@pytest.mark.parametrize("nstep", NSTEPS)
def test_every_position_has_one_row_pair_and_slot(nstep):
    hs = (nstep + 1) // 2
    seen = {}
    for pos in range(2 * nstep + 1):
        pair, row, s, vidx, eidx = slot(nstep, pos)
        assert pair in (0, 1) and row in (0, 1) and 0 <= s <= hs
        assert (pair, row, s) not in seen, (pos, seen[(pair, row, s)])      # no slot twice within a half of a chain
        seen[(pair, row, s)] = pos
        if pos == nstep:
            assert (pair, row, s) == (1, 0, hs)                  # the middle block: rows 2 and 3, the slot behind the halves
        else:
            assert s < hs and row == (1 if pos > nstep else 0)
    # the halves: rows 0 and 1 hold HS positions each, rows 2 and 3 the other NSTEP - HS, plus the middle block
    for row in (0, 1):
        assert sorted(s for (p, r, s) in seen if p == 0 and r == row) == list(range(hs))
        assert sorted(s for (p, r, s) in seen if p == 1 and r == row and s < hs) == list(range(nstep - hs))
    assert len(seen) == 2 * nstep + 1
    # no sweep lane holds the dummy block of the idle lanes, nor anything outside the layout
    for pos in (-1, 2 * nstep + 1, 2 * nstep + 2):
        assert slot(nstep, pos) == (-1,) * 5


@pytest.mark.parametrize("nstep", NSTEPS)
def test_addresses_are_those_of_the_position(nstep):
    npos = 2 * nstep + 2
    for pos in range(2 * nstep + 1):
        pair, row, s, vidx, eidx = slot(nstep, pos)
        assert vidx == wv_vidx(npos, pos, 0) and eidx == 8 * pos
        for k in range(8):                                       # component k: a fixed distance inside the block vector
            assert vidx + wv_vidx(npos, 0, k) == wv_vidx(npos, pos, k)
    # slot s + 1 of a lane is the next position: + 2 inside a block vector, + 8 inside the couplings (the kernel's strides)
    for pos in range(2 * nstep):
        a, b = slot(nstep, pos), slot(nstep, pos + 1)
        if a[:2] == b[:2] and pos != nstep and pos + 1 != nstep:
            assert b[2] == a[2] + 1 and b[3] == a[3] + 2 and b[4] == a[4] + 8


@pytest.mark.parametrize("nstep", NSTEPS)
def test_every_horizon_keeps_its_order_across_the_hand_over(nstep):
    hs = (nstep + 1) // 2
    all_dummy_first_half = 0
    for nb in range(1, 2 * nstep + 2):
        for chain in positions(nstep, nb):
            order = []                                           # (pair, slot) in sweep order
            real_first_half = 0
            for pos, blk in chain:
                pair, row, s, vidx, eidx = slot(nstep, pos)
                order.append((pair, s))
                real_first_half += blk is not None and pair == 0
            # the forward pass issues slots 0 .. HS-1 on pair 0, hands over, then slots 0 .. on pair 1
            assert order == sorted(order) and order == [(0, s) for s in range(hs)] + [(1, s) for s in range(nstep - hs)]
            # the real blocks are the chain's last: a half that holds only dummies is the FIRST one, and it is legal
            blks = [blk for _, blk in chain]
            n_real = sum(b is not None for b in blks)
            assert all(b is None for b in blks[:nstep - n_real]) and all(b is not None for b in blks[nstep - n_real:])
            if n_real and not real_first_half:
                all_dummy_first_half += 1
                assert n_real <= nstep - hs
        # every real block of the horizon sits on exactly one position
        a, b = positions(nstep, nb)
        real = sorted([blk for _, blk in a + b if blk is not None] + [nb // 2])
        assert real == list(range(nb))
    assert all_dummy_first_half > 0
