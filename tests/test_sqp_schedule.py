"""Schedule of the SQP round loop (csrc/sqp_sched.cpp, through sco_debug_sqp_schedule / sco_debug_stage_sweep): host arithmetic only.

The numbers are those of the 256-CU, 8-XCD part: a wavefront round needs 704 live problems (2.75 per CU), the QPs run to
max_iter = 100000 at fixed rho unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from sco_py_amd import _lib

CUS, XCDS, WV_MIN, MAX_ITER = 256, 8, 704, 100000


@pytest.fixture(autouse=True)
def _no_schedule_environment(monkeypatch):
    for name in list(os.environ):
        if name.startswith("SCO_SQP_"):
            monkeypatch.delenv(name)


def _in(batch, admm_slice=0, adaptive=0, interval=100, max_qp_solves=0, n_active=None, groups_ok=True, wv=False, cus=CUS):
    n_active = batch if n_active is None else n_active
    return np.array([batch, cus, admm_slice, adaptive, MAX_ITER, interval, max_qp_solves, n_active, int(groups_ok), int(wv),
                     WV_MIN, XCDS], dtype=np.int32)


PLAN = ("slice", "G", "select", "has_wv", "mix_on", "mix_slack", "mix_slices", "mix_tail", "depth", "round_cap", "xcds", "trace")
ROUND = ("wv_round", "pass", "nwg", "mix_k", "side_off", "tier", "window", "counts_as_wv")


def plan(batch, **kw):
    out = np.zeros(20, dtype=np.int32)
    assert _lib.load().sco_debug_sqp_schedule(_lib.iptr(_in(batch, **kw)), _lib.iptr(out), None, None) == 0
    p = dict(zip(PLAN, (int(v) for v in out[:12])))
    p["windows"] = [(int(out[12 + 2 * g]), int(out[12 + 2 * g] + out[13 + 2 * g])) for g in range(p["G"])]
    return p


def round_(batch, live, index=0, group_nb=None, **kw):
    out = np.zeros(20, dtype=np.int32); r = np.zeros(8, dtype=np.int32)
    rin = np.array([batch if group_nb is None else group_nb, live, index], dtype=np.int32)
    assert _lib.load().sco_debug_sqp_schedule(_lib.iptr(_in(batch, **kw)), _lib.iptr(out), _lib.iptr(rin), _lib.iptr(r)) == 0
    return dict(zip(ROUND, (int(v) for v in r)))


# ---- the plan of a solve

def test_a_batch_that_fits_the_cus_runs_unsliced_one_round_ahead():
    p = plan(256)
    assert (p["slice"], p["select"], p["G"], p["depth"]) == (0, 0, 1, 1)


def test_a_batch_larger_than_the_chip_gets_slices_selection_and_two_rounds_ahead(monkeypatch):
    p = plan(1024)
    assert (p["slice"], p["select"], p["depth"], p["G"]) == (6250, 1, 2, 1)
    assert (p["has_wv"], p["mix_on"]) == (0, 0)                      # no wavefront tier on the handle
    p = plan(1024, wv=True)
    assert (p["has_wv"], p["mix_on"], p["mix_slack"], p["mix_slices"], p["mix_tail"], p["xcds"]) == (1, 1, 1, 2, 0, XCDS)
    monkeypatch.setenv("SCO_SQP_MIX", "0")
    p = plan(1024, wv=True)
    assert (p["has_wv"], p["mix_on"]) == (1, 0)


def test_adaptive_rho_or_a_tier_without_windows_has_no_selection_groups_or_mixed_rounds(monkeypatch):
    monkeypatch.setenv("SCO_SQP_GROUPS", "4")
    # (with adaptive rho no tier takes launch windows: sco_qp_supports_groups)
    p = plan(1024, adaptive=1, groups_ok=False, wv=True)
    assert (p["slice"], p["select"], p["G"], p["has_wv"], p["mix_on"], p["depth"]) == (2000, 0, 1, 0, 0, 2)
    p = plan(1024, groups_ok=False, wv=True)
    assert (p["slice"], p["select"], p["G"], p["has_wv"], p["mix_on"]) == (6250, 0, 1, 0, 0)
    # the planner's own dependence on adaptive rho, whatever the tier says about windows: the shorter slice, no mixed rounds
    monkeypatch.delenv("SCO_SQP_GROUPS")
    p = plan(1024, adaptive=1, groups_ok=True, wv=True)
    assert (p["slice"], p["select"], p["has_wv"], p["mix_on"]) == (2000, 1, 1, 0)


def test_the_slice_a_caller_asks_for_wins_over_the_environment(monkeypatch):
    assert plan(1024, admm_slice=-1)["slice"] == 0
    assert plan(1024, admm_slice=-1)["depth"] == 1
    monkeypatch.setenv("SCO_SQP_SLICE", "300")
    assert plan(1024, admm_slice=400)["slice"] == 400
    assert plan(200, admm_slice=400)["slice"] == 400                 # ... and over "the batch fits the CUs"
    assert plan(1024, admm_slice=-1)["slice"] == 0
    assert plan(1024, admm_slice=0)["slice"] == 300
    assert plan(256, admm_slice=0)["slice"] == 0
    monkeypatch.setenv("SCO_SQP_SLICE", "-5")
    assert plan(1024)["slice"] == 6250


def test_stream_groups(monkeypatch):
    monkeypatch.setenv("SCO_SQP_GROUPS", "3")
    p = plan(700, wv=True)
    assert (p["G"], p["windows"]) == (2, [(0, 350), (350, 700)])     # at least a chip's worth of problems per group
    assert (p["has_wv"], p["mix_on"]) == (1, 0)                      # mixed rounds need the side stream: one group only
    assert plan(300)["G"] == 1
    assert plan(300)["windows"] == [(0, 300)]
    monkeypatch.setenv("SCO_SQP_GROUPS", "9")
    p = plan(4096)
    assert (p["G"], p["windows"]) == (4, [(0, 1024), (1024, 2048), (2048, 3072), (3072, 4096)])
    monkeypatch.setenv("SCO_SQP_GROUPS", "0")
    assert plan(4096)["G"] == 1


def test_selection_can_be_switched_off_only_by_a_leading_zero(monkeypatch):
    monkeypatch.setenv("SCO_SQP_SELECT", "0")
    p = plan(1024, wv=True)
    assert (p["select"], p["has_wv"], p["mix_on"], p["depth"]) == (0, 0, 0, 2)
    monkeypatch.setenv("SCO_SQP_SELECT", "no")
    assert plan(1024)["select"] == 1


def test_mixed_round_settings_from_the_environment(monkeypatch):
    monkeypatch.setenv("SCO_SQP_MIX_SLACK", "-3"); monkeypatch.setenv("SCO_SQP_MIX_SLICES", "0")
    monkeypatch.setenv("SCO_SQP_MIX_PICK", "tail"); monkeypatch.setenv("SCO_SQP_XCDS", "4")
    p = plan(1024, wv=True)
    assert (p["mix_on"], p["mix_slack"], p["mix_slices"], p["mix_tail"], p["xcds"]) == (1, 0, 1, 1, 4)
    monkeypatch.setenv("SCO_SQP_MIX_PICK", "tails")
    assert plan(1024, wv=True)["mix_tail"] == 0
    assert plan(1024)["xcds"] == 1                                   # (the count matters to mixed rounds only)


@pytest.mark.parametrize("value,level", [(None, 0), ("", 1), ("0", 1), ("1", 1), ("2", 2), ("7", 2)])
def test_trace_level(monkeypatch, value, level):
    if value is not None:
        monkeypatch.setenv("SCO_SQP_TRACE_ROUNDS", value)
    assert plan(1024)["trace"] == level


def test_round_cap_is_two_launches_per_slice_of_every_qp_a_problem_may_solve():
    # 2 (max_qp_solves + 8) slices_per_qp with max_qp_solves = 0: 16 per slice of a QP
    assert plan(1024, admm_slice=0)["round_cap"] == 16 * 16                  # ceil(100000 / 6250) = 16
    assert plan(1024, admm_slice=400)["round_cap"] == 16 * 250
    assert plan(1024, admm_slice=175)["round_cap"] == 16 * 572
    assert plan(1024, admm_slice=-1)["round_cap"] == 16
    assert plan(1024, admm_slice=400, max_qp_solves=92)["round_cap"] == 200 * 250
    # adaptive rho: a launch per rho change at most on top, max_iter / interval + 1
    assert plan(1024, adaptive=1, interval=100, groups_ok=False)["round_cap"] == 16 * (50 + 1001)
    assert plan(200, admm_slice=-1, adaptive=1, interval=125, groups_ok=False)["round_cap"] == 16 * (1 + 801)


# ---- one round

@pytest.mark.parametrize("live,wv_round,nwg,mix_k,tier", [
    (2000, 1, 1024, 0, 2), (1001, 1, 1001, 0, 2), (904, 1, 904, 24, 3), (776, 1, 776, 72, 3), (704, 1, 704, 96, 3),
    (703, 0, 512, 0, 1), (200, 0, 200, 0, 1), (0, 0, 1, 0, 1)])
def test_rounds_with_selection_on_a_wavefront_handle(monkeypatch, live, wv_round, nwg, mix_k, tier):
    r = round_(2048, live, wv=True)
    assert (r["wv_round"], r["nwg"], r["mix_k"], r["tier"]) == (wv_round, nwg, mix_k, tier)
    assert r["pass"] == (4 * CUS if wv_round else CUS)
    assert (r["window"], r["counts_as_wv"], r["side_off"]) == (1, wv_round, 0)
    assert round_(2048, live, index=1, wv=True) == r
    # tail pick: the side window comes from the end of the list in odd rounds only
    monkeypatch.setenv("SCO_SQP_MIX_PICK", "tail")
    assert round_(2048, live, index=2, wv=True) == r
    assert round_(2048, live, index=1, wv=True) == dict(r, side_off=nwg - mix_k if mix_k else 0)
    # no mixed rounds: the same launches, all of a wavefront round on the wavefront tier
    monkeypatch.setenv("SCO_SQP_MIX", "0")
    assert round_(2048, live, index=1, wv=True) == dict(r, mix_k=0, tier=2 if wv_round else 1)


def test_a_side_window_that_would_take_the_whole_launch_is_dropped(monkeypatch):
    # 8 CUs in one XCD, wavefront rounds from 3 live problems on: with 3 live the split would move all of them
    monkeypatch.setenv("SCO_SQP_XCDS", "1")
    lib = _lib.load()
    assert lib.sco_debug_mix_split(3, 8, 1, 1, 4) >= 3
    inp = _in(64, wv=True, cus=8); inp[10] = 3
    out = np.zeros(20, dtype=np.int32); r = np.zeros(8, dtype=np.int32)
    assert lib.sco_debug_sqp_schedule(_lib.iptr(inp), _lib.iptr(out), _lib.iptr(np.array([64, 3, 0], dtype=np.int32)), _lib.iptr(r)) == 0
    r = dict(zip(ROUND, (int(v) for v in r)))
    assert out[4] == 1 and (r["wv_round"], r["nwg"], r["mix_k"], r["tier"]) == (1, 3, 0, 2)


def test_rounds_without_selection_go_by_the_size_of_the_launch():
    # a batch that fits the CUs: the whole group every round, no launch window; the launch picks the tier by its size and
    # a launch of at least wv_min problems on a wavefront handle is counted as a wavefront round
    r = round_(WV_MIN, 10, cus=1024, wv=True)
    assert (r["wv_round"], r["nwg"], r["mix_k"], r["tier"], r["window"], r["counts_as_wv"]) == (0, WV_MIN, 0, 0, 0, 1)
    r = round_(WV_MIN - 1, WV_MIN - 1, cus=1024, wv=True)
    assert (r["nwg"], r["tier"], r["window"], r["counts_as_wv"]) == (WV_MIN - 1, 0, 0, 0)
    r = round_(WV_MIN, WV_MIN, cus=1024, wv=False)
    assert (r["nwg"], r["tier"], r["window"], r["counts_as_wv"]) == (WV_MIN, 0, 0, 0)


def test_stream_groups_pass_their_window_and_size_rounds_by_their_own_live_count(monkeypatch):
    monkeypatch.setenv("SCO_SQP_GROUPS", "2")
    r = round_(1024, 300, group_nb=512)
    assert (r["nwg"], r["tier"], r["window"], r["mix_k"]) == (256, 0, 1, 0)
    monkeypatch.setenv("SCO_SQP_SELECT", "0")
    r = round_(1024, 300, group_nb=512)
    assert (r["nwg"], r["tier"], r["window"]) == (512, 0, 1)


@pytest.mark.parametrize("wv", [False, True])
def test_every_live_count_gets_whole_passes_or_exactly_its_problems(wv):
    for live in range(1, 4 * CUS + 1):
        r = round_(1024, live, wv=wv)
        assert 1 <= r["nwg"] <= max(live, 1), live
        assert r["nwg"] == live or r["nwg"] % r["pass"] == 0, live
        assert r["wv_round"] == (wv and live >= WV_MIN), live
        assert 0 <= r["mix_k"] < r["nwg"] and (r["tier"] == 3) == (r["mix_k"] > 0), live


def test_bad_arguments_are_refused():
    lib = _lib.load()
    out = np.zeros(20, dtype=np.int32)
    assert lib.sco_debug_sqp_schedule(None, _lib.iptr(out), None, None) != 0
    assert lib.sco_debug_sqp_schedule(_lib.iptr(_in(8)), _lib.iptr(out), _lib.iptr(np.zeros(3, dtype=np.int32)), None) != 0
    assert lib.sco_debug_sqp_schedule(_lib.iptr(_in(8, adaptive=1, interval=0)), _lib.iptr(out), None, None) != 0


# ---- stage times of overlapping stream groups

def sweep(intervals):
    b = np.array([i[0] for i in intervals], dtype=np.float64); e = np.array([i[1] for i in intervals], dtype=np.float64)
    s = np.array([i[2] for i in intervals], dtype=np.int32); ms = np.full(5, -1.0)
    assert _lib.load().sco_debug_stage_sweep(len(intervals), _lib.dptr(b), _lib.dptr(e), _lib.iptr(s), _lib.dptr(ms)) == 0
    return list(ms)


def test_disjoint_intervals_are_charged_their_own_length_and_a_gap_to_nobody():
    # (binary fractions: every sum below is exact)
    assert sweep([(0.0, 1.5, 0), (1.5, 2.0, 1), (2.0, 6.0, 2), (6.0, 6.25, 3)]) == [1.5, 0.5, 4.0, 0.25, 6.25]
    assert sweep([(6.0, 6.25, 3), (0.0, 1.5, 0), (2.0, 6.0, 2)]) == [1.5, 0.0, 4.0, 0.25, 5.75]          # 1.5 .. 2 is a gap
    assert sweep([]) == [0.0] * 5


@pytest.mark.parametrize("hi,lo", [(2, 1), (2, 0), (2, 3), (1, 0), (1, 3), (0, 3)])
def test_an_overlap_is_charged_to_the_stage_of_higher_priority_only(hi, lo):
    ms = sweep([(0.0, 4.0, lo), (3.0, 5.0, hi)])
    assert (ms[hi], ms[lo], ms[4]) == (2.0, 3.0, 5.0)
    ms = sweep([(0.0, 4.0, hi), (1.0, 2.0, lo)])                     # the lower stage entirely inside the higher one
    assert (ms[hi], ms[lo], ms[4]) == (4.0, 0.0, 4.0)


def test_two_groups_inside_the_same_stage_count_the_wall_time_once():
    ms = sweep([(0.0, 4.0, 2), (1.0, 6.0, 2), (6.0, 7.0, 3), (6.5, 8.0, 0)])
    assert ms == [1.5, 0.0, 6.0, 0.5, 8.0]


def test_empty_backward_and_unstaged_intervals_are_ignored():
    assert sweep([(1.0, 1.0, 2), (3.0, 2.0, 1), (0.0, 9.0, -1), (4.0, 5.0, 3)]) == [0.0, 0.0, 0.0, 1.0, 1.0]
    lib = _lib.load()
    assert lib.sco_debug_stage_sweep(-1, None, None, None, _lib.dptr(np.zeros(5))) != 0
    assert lib.sco_debug_stage_sweep(1, None, None, None, _lib.dptr(np.zeros(5))) != 0
