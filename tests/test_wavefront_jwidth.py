"""Jacobian widths of the wavefront ADMM tier, without a GPU: the hint the SQP layer derives from point_link for the
serial-arm families (csrc/sqp_layout.cpp: sqp_row_widths, through sco_debug_sqp_row_widths), the widths of the four hinge
slots and the width profile the planner picks for it (csrc/wv_plan.cpp: wv_plan_widths, through sco_debug_wv_widths), and
the SCO_WV_JW=0 switch.  The lane tables, the row assignment and the LDS request are wv_plan_build's and must not move."""
import ctypes as C

import numpy as np
import pytest

from sco_py_amd import _lib
from test_sqp_layout import ARM, JL, POINT, PROGRAM, QUADRATIC, REACH, VEL, _desc, _layout
from sco_py_amd.workloads import default_points

SPATIAL = 7
BENCH_LINKS = [1, 2, 4, 5, 6]                       # default_points(7, 5): the benchmark's link points
PROFILE_3577 = 3 | (5 << 4) | (7 << 8) | (7 << 12)


def _hint(desc, point_link):
    """(the family gives a hint, row_width[m]) and the layout of the descriptor."""
    rc, L = _layout(desc)
    assert rc == 0
    out = np.full(L.m, -9, dtype=np.int32)
    pl = np.ascontiguousarray(point_link, dtype=np.int32)
    got = _lib.load().sco_debug_sqp_row_widths(C.byref(desc), _lib.iptr(pl), _lib.iptr(out))
    assert got in (0, 1), got
    return bool(got), out, L


@pytest.fixture(autouse=True)
def _row_order(monkeypatch):
    """The tests below state the widths of rows dealt in ROW order (SCO_WV_JSORT=0) unless they say otherwise; the default,
    rows dealt by width, has its own test at the end."""
    monkeypatch.setenv("SCO_WV_JSORT", "0")


def _widths(L, row_width):
    """sco_debug_wv_widths for the penalty QP of layout L: fits, jw[4], profile, LDS bytes, <BS, NS, NV, NSTEP>, lanes per block."""
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    sizes = np.zeros(16, dtype=np.int32); info = np.full(12, -9, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    pat = [np.ascontiguousarray(a, dtype=np.int32) for a in (L.Pp1, L.Pi1, L.Ap1, L.Ai1)]
    assert lib.sco_debug_plan_build(L.n, L.m, *(ip(a) for a in pat), 1, ip(sizes)) == 0
    rw = None if row_width is None else np.ascontiguousarray(row_width, dtype=np.int32)
    assert lib.sco_debug_wv_widths(_lib.iptr(rw), ip(info)) == 0
    return [int(v) for v in info]


def _link_plan_lds():
    lib = _lib.load()
    info = np.zeros(16, dtype=np.int32)
    lib.sco_debug_wv_link_plan.argtypes = [C.POINTER(C.c_int)]
    assert lib.sco_debug_wv_link_plan(info.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return [int(v) for v in info]


@pytest.mark.parametrize("family", [ARM, REACH, SPATIAL, ARM | VEL, SPATIAL | JL])
def test_serial_arm_families_promise_point_link_plus_one_columns(family):
    d, T, K, O = 7, 20, 5, 2
    got, w, L = _hint(_desc(1, d, T, K, O, family), BENCH_LINKS)
    assert got
    want = np.zeros(L.m, dtype=np.int32)
    per_block = np.repeat(np.array(BENCH_LINKS) + 1, O)                        # row (k, o) of a block at k O + o
    assert list(per_block) == [2, 2, 3, 3, 5, 5, 6, 6, 7, 7]
    want[L.m_lin:L.m_lin + T * K * O] = np.tile(per_block, T)
    assert np.array_equal(w, want)                                             # linear, reach, bound and box rows: no promise
    assert L.m_nl == T * K * O + L.NE


@pytest.mark.parametrize("family,kw", [(POINT, dict(dof=2, n_points=1)), (QUADRATIC, dict(dof=3, n_points=1)),
                                       (PROGRAM, dict(dof=3, n_points=1)), (PROGRAM, dict(dof=3, n_points=1, span=2))])
def test_families_without_the_guarantee_give_no_hint(family, kw):
    desc = _desc(1, kw["dof"], 6, kw["n_points"], 2, family, span=kw.get("span", 0))
    got, w, L = _hint(desc, [0])
    assert not got and not w.any()


def test_bench_shape_has_widths_3_5_7_7_and_its_profile():
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), BENCH_LINKS)
    info = _widths(L, w)
    assert info[0] == 1 and info[7:12] == [7, 4, 3, 10, 3], info
    assert info[1:5] == [3, 5, 7, 7] and info[5] == PROFILE_3577, info
    # the spatial family's layout is the same pattern: same widths, same profile
    got, ws, Ls = _hint(_desc(1, 7, 20, 5, 2, SPATIAL), BENCH_LINKS)
    assert _widths(Ls, ws)[1:6] == [3, 5, 7, 7, PROFILE_3577]
    # 17 timesteps: the smallest horizon on <7,4,3,10,3>
    got, w17, L17 = _hint(_desc(1, 7, 17, 5, 2, ARM), BENCH_LINKS)
    i17 = _widths(L17, w17)
    assert i17[7:12] == [7, 4, 3, 10, 3] and i17[1:6] == [3, 5, 7, 7, PROFILE_3577], i17


def test_all_points_on_the_last_link_keep_the_generic_kernel():
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), [6] * 5)
    assert got and set(w[L.m_lin:L.m_lin + 200]) == {7}
    info = _widths(L, w)
    assert info[1:5] == [7, 7, 7, 7] and info[5] == 0, info


def test_no_hint_is_full_width_and_the_generic_kernel():
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), BENCH_LINKS)
    info = _widths(L, None)
    assert info[0] == 1 and info[1:5] == [7, 7, 7, 7] and info[5] == 0, info
    assert _widths(L, np.zeros(L.m, dtype=np.int32))[1:6] == [7, 7, 7, 7, 0]           # "no promise" for every row


@pytest.mark.parametrize("links", [[0, 0, 0, 0, 0], [0, 1, 2, 3, 4], [1, 2, 4, 5, 6], [2, 2, 4, 6, 6], [0, 4, 6, 6, 6],
                                   [6, 5, 4, 2, 1], [1, 2, 3, 6, 6], [2, 4, 6, 1, 0]])
def test_profile_dominates_the_widths_slot_by_slot(links):
    """Whatever point_link says, the profile the launch runs covers every slot's widest row -- or is the generic one; and the
    widths are the largest promise over the rows the plan deals to the slot (row r of a block: lane r % 3, slot r // 3)."""
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), links)
    info = _widths(L, w)
    per_block = np.repeat(np.array(links) + 1, 2)
    want = [int(per_block[3 * q:3 * q + 3].max()) for q in range(4)]
    assert info[1:5] == want, (info, want)
    prof = info[5]
    if prof:
        nib = [(prof >> (4 * q)) & 15 for q in range(4)]
        assert all(1 <= nib[q] <= 7 and nib[q] >= want[q] for q in range(4)), (nib, want)
    else:
        assert any(a > b for a, b in zip(want, [3, 5, 7, 7])), want       # the one compiled profile would have covered it


def test_switch_forces_the_generic_profile(monkeypatch):
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), BENCH_LINKS)
    monkeypatch.setenv("SCO_WV_JW", "0")
    info = _widths(L, w)
    assert info[1:5] == [3, 5, 7, 7] and info[5] == 0, info         # the widths are still recorded
    monkeypatch.setenv("SCO_WV_JW", "1")
    assert _widths(L, w)[5] == PROFILE_3577
    monkeypatch.delenv("SCO_WV_JW")
    assert _widths(L, w)[5] == PROFILE_3577


def test_layout_and_lds_request_do_not_move():
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), BENCH_LINKS)
    with_hint = _widths(L, w)
    base = _link_plan_lds()                                         # wv_plan_build alone, for the pattern just analysed
    without = _widths(L, None)
    assert with_hint[6] == without[6] == base[8] and base[8] <= 40 * 1024
    assert with_hint[7:12] == without[7:12] == [base[4], base[5], base[6], base[7], base[3]]


@pytest.mark.parametrize("shape", [(3, 7, 2, 2), (7, 14, 5, 2), (4, 21, 2, 2)])
def test_other_instantiations_stay_generic(shape):
    """Profiles exist for <7,4,3,10,3> only: every other plan records its widths and runs the generic kernel."""
    d, T, K, O = shape
    links, _ = default_points(d, K)
    got, w, L = _hint(_desc(1, d, T, K, O, ARM), links)
    info = _widths(L, w)
    assert got and info[0] == 1 and info[5] == 0 and info[7:12] != [7, 4, 3, 10, 3], info
    assert max(info[1:5]) == max(links) + 1


def test_rows_dealt_by_width_give_7_6_3_2(monkeypatch):
    """The default (no SCO_WV_JSORT, or 1): a timestep's rows go to the slots widest first -- 7, 7, 6 | 6, 5, 5 | 3, 3, 2 | 2 --
    same instantiation, same LDS bytes; without a hint, or with SCO_WV_JW=0, the rows stay in row order."""
    got, w, L = _hint(_desc(1, 7, 20, 5, 2, ARM), BENCH_LINKS)
    plain = _widths(L, w)
    assert plain[1:5] == [3, 5, 7, 7]
    monkeypatch.setenv("SCO_WV_JSORT", "1")
    assert _widths(L, w)[1:5] == [7, 6, 3, 2]
    monkeypatch.delenv("SCO_WV_JSORT")
    info = _widths(L, w)
    assert info[1:5] == [7, 6, 3, 2] and info[5] == 7 | (6 << 4) | (3 << 8) | (2 << 12), info
    assert info[6:] == plain[6:]
    assert _widths(L, None)[1:6] == [7, 7, 7, 7, 0]
    monkeypatch.setenv("SCO_WV_JW", "0")
    assert _widths(L, w)[1:6] == [3, 5, 7, 7, 0]
