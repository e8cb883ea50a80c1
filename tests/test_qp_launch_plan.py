"""Tier choice and launch planning of the QP layer (csrc/qp_tier.cpp and qp_choose_tiers of csrc/qp_tier_choice.cpp, through
sco_debug_qp_launch_plan and sco_debug_plan_tiers): host arithmetic only.

The numbers are those of the 256-CU part: a wavefront launch needs 704 problems (2.75 per CU)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from sco_py_amd import _lib
from test_qp_plan import penalty_qp

INT_MAX = 2**31 - 1
CUS = 256
RL, REG, FAST, GENERIC = 0, 1, 2, 3                       # QpKernel
ERR_ARG, ERR_STATE, ERR_CAPACITY = -1, -4, -5
E_NONE, E_WINDOW, E_ADAPT_DENSE, E_ADAPT_SETTINGS, E_MIXED = range(5)
DENSE, BT, ONCHIP = 0, 1, 2                               # QpRoute
NEED_NONE, NEED_WINDOW, NEED_SIDE = 0, 1, 2
A_GENERIC, A_FAST, A_REG, A_RL, A_WV_RL, A_MIXED = range(6)
OUT = ("rc", "err", "slice", "nwg", "rho_init", "route", "wv_now", "mixed", "need", "cholesky", "sweep_nt", "admm", "ad_interval",
       "wv_min_live", "interval")

SWITCHES = ("FACTOR_CHOLESKY", "NO_ELIM", "FORCE_BIG", "NO_BT", "NO_RL", "NO_WV", "NO_REG", "NO_FAST")
ROUTES = {
    "none": (),
    "NO_RL": ("NO_RL",),
    "NO_RL+NO_REG": ("NO_RL", "NO_REG"),
    "NO_RL+NO_REG+NO_FAST": ("NO_RL", "NO_REG", "NO_FAST"),
    "FORCE_BIG": ("FORCE_BIG",),
    "FORCE_BIG+NO_BT": ("FORCE_BIG", "NO_BT"),
    "NO_WV": ("NO_WV",),
    "FACTOR_CHOLESKY": ("FACTOR_CHOLESKY",),
}


@pytest.fixture(autouse=True)
def _no_qp_environment(monkeypatch):
    for name in list(os.environ):
        if name.startswith("SCO_QP_") or name.startswith("SCO_WV_"):
            monkeypatch.delenv(name)


def plan(kern=RL, big=0, bt=0, wv=0, cholesky=0, batch=1024, n_c=140, cus=CUS, adaptive=0, interval=0, check=25, max_iter=100000,
         tol=5.0, slice=0, mask=0, wv_min=-1, window=None, tier=0, has_list=1, side=(0, 0), side_slices=2, side_ready=1):
    """window: (b0, nb) or None; side: (side_b0, side_nb)."""
    b0, nb = window if window else (0, 0)
    a = np.array([kern, big, bt, wv, cholesky, batch, n_c, cus, adaptive, interval, check, max_iter, slice, mask, wv_min,
                  1 if window else 0, b0, nb, tier, has_list, side[0], side[1], side_slices, side_ready], dtype=np.int32)
    out = np.full(15, -99, dtype=np.int32)
    assert _lib.load().sco_debug_qp_launch_plan(_lib.iptr(a), C.byref(C.c_double(tol)), _lib.iptr(out)) == 0
    return dict(zip(OUT, (int(v) for v in out)))


# ---- 1. the slice

def test_slices_end_on_a_termination_check():
    assert plan(slice=0)["slice"] == 0
    assert plan(slice=130)["slice"] == 150
    assert plan(slice=0, adaptive=1, max_iter=4010)["slice"] == 4025       # parks only when rho changes
    assert plan(slice=130, check=0)["slice"] == 0
    for asked in (0, 1, 130, 6250):
        assert plan(kern=GENERIC, big=1, slice=asked)["slice"] == 0             # the dense global-memory form cannot park
    assert plan(kern=GENERIC, big=1, bt=1, slice=130)["slice"] == 150


# ---- 2. / 3. the two numbers the SQP scheduler takes from here

def test_fewest_problems_of_a_wavefront_launch(monkeypatch):
    assert plan(cus=256)["wv_min_live"] == 704
    assert plan(cus=0)["wv_min_live"] == 704                                   # unknown: the 256-CU part
    assert plan(cus=256, adaptive=1)["wv_min_live"] == INT_MAX                 # adaptive rho: never, unless the variable says so
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    assert plan(cus=256)["wv_min_live"] == 0 and plan(cus=256, adaptive=1)["wv_min_live"] == 0
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "1e9")
    assert plan(cus=256)["wv_min_live"] == INT_MAX


@pytest.mark.parametrize("interval, check, want", [(0, 25, 100), (60, 25, 50), (10, 25, 25), (0, 0, 100), (70, 0, 70)])
def test_rho_estimate_interval_sits_on_termination_checks(interval, check, want):
    assert plan(interval=interval, check=check)["interval"] == want
    if check > 0:
        p = plan(interval=interval, check=check, adaptive=1)
        assert (p["rc"], p["ad_interval"]) == (0, want)
    assert plan(interval=interval, check=check)["ad_interval"] == 0           # fixed rho: no estimate


# ---- 4. tier of a launch

def test_a_launch_without_a_wish_goes_by_its_size():
    assert plan(wv=1, batch=704)["wv_now"] == 1 and plan(wv=1, batch=703)["wv_now"] == 0
    assert plan(wv=1, batch=1024, window=(10, 704))["wv_now"] == 1            # tier 0: by the window's nb
    assert plan(wv=1, batch=1024, window=(10, 703))["wv_now"] == 0
    p = plan(wv=1, batch=704)
    assert (p["admm"], p["need"], p["nwg"], p["route"]) == (A_WV_RL, NEED_NONE, 704, ONCHIP)


def test_the_windows_tier_overrides_the_size():
    assert plan(wv=1, batch=1024, window=(0, 1024), tier=1)["wv_now"] == 0    # row-local whatever the size
    assert plan(wv=1, batch=1024, window=(0, 3), tier=2)["wv_now"] == 1       # wavefront whatever the size
    for tier in (0, 1, 2):
        p = plan(wv=0, batch=1024, window=(0, 1024), tier=tier)               # a handle without the tier ignores the field
        assert (p["rc"], p["wv_now"], p["admm"]) == (0, 0, A_RL)


# ---- 5. which problems get the dense inverse besides those that start a QP

def test_extra_dense_inverses():
    assert plan(wv=0)["need"] == NEED_NONE
    assert plan(wv=1, batch=100)["need"] == NEED_WINDOW                        # row-local launch of a handle that holds the tier
    assert plan(wv=1, batch=1024, window=(0, 900), tier=1)["need"] == NEED_WINDOW
    assert plan(wv=1, batch=1024)["need"] == NEED_NONE                         # wavefront launch: the value test decides
    p = plan(wv=1, batch=1024, slice=100, window=(0, 900), tier=3, side=(0, 80))
    assert (p["rc"], p["mixed"], p["wv_now"], p["need"], p["admm"], p["nwg"]) == (0, 1, 1, NEED_SIDE, A_MIXED, 900)


# ---- 6. the factor kernel

@pytest.mark.parametrize("n_c, nt", [(1, 1), (176, 1), (177, 2), (252, 2), (253, 3), (256, 3)])
def test_sweep_instantiation(n_c, nt):
    p = plan(n_c=n_c)
    assert (p["cholesky"], p["sweep_nt"]) == (0, nt)
    assert plan(n_c=n_c, cholesky=1)["cholesky"] == 1


def test_admm_sequence_follows_the_handles_kernel():
    assert [plan(kern=k)["admm"] for k in (RL, REG, FAST, GENERIC)] == [A_RL, A_REG, A_FAST, A_GENERIC]
    assert plan(kern=GENERIC, big=1)["route"] == DENSE and plan(kern=GENERIC, big=1, bt=1)["route"] == BT
    assert plan(adaptive=1, mask=1)["rho_init"] == 1 and plan(adaptive=1, mask=0)["rho_init"] == 1
    assert plan(adaptive=1, mask=2)["rho_init"] == 0 and plan(adaptive=0, mask=1)["rho_init"] == 0


# ---- 7. errors: window, then adaptive rho, then the mixed round

def _err(p):
    return p["rc"], p["err"]


@pytest.mark.parametrize("handle", [dict(kern=REG), dict(kern=FAST), dict(kern=GENERIC), dict(kern=GENERIC, big=1),
                                    dict(kern=RL, cholesky=1), dict(kern=RL, adaptive=1), dict(kern=GENERIC, big=1, bt=1, adaptive=1)])
def test_windows_need_the_row_local_or_structured_tier_at_fixed_rho(handle):
    p = plan(window=(0, 64), **handle)
    assert _err(p) == (ERR_STATE, E_WINDOW) and p["slice"] == -1
    assert plan(**handle)["rc"] == 0


def test_windows_lie_inside_the_batch():
    assert plan(window=(0, 1024))["rc"] == 0 and plan(kern=GENERIC, big=1, bt=1, window=(1000, 24))["rc"] == 0
    for win in ((-1, 10), (0, 0), (5, -3), (1000, 25), (1024, 1)):
        assert _err(plan(window=win)) == (ERR_STATE, E_WINDOW), win


def test_adaptive_rho_errors():
    assert _err(plan(kern=GENERIC, big=1, adaptive=1)) == (ERR_CAPACITY, E_ADAPT_DENSE)
    assert plan(kern=GENERIC, big=1, bt=1, adaptive=1)["rc"] == 0
    assert _err(plan(adaptive=1, tol=1.0)) == (ERR_ARG, E_ADAPT_SETTINGS)
    assert _err(plan(adaptive=1, check=0)) == (ERR_ARG, E_ADAPT_SETTINGS)
    assert _err(plan(adaptive=1, tol=float("nan"))) == (ERR_ARG, E_ADAPT_SETTINGS)
    assert plan(adaptive=1, tol=1.0 + 1e-9)["rc"] == 0
    # the dense form's answer comes before the settings are looked at, the window's before both
    assert _err(plan(kern=GENERIC, big=1, adaptive=1, tol=1.0)) == (ERR_CAPACITY, E_ADAPT_DENSE)
    assert _err(plan(kern=GENERIC, big=1, adaptive=1, window=(0, 8))) == (ERR_STATE, E_WINDOW)


GOOD_MIX = dict(wv=1, batch=1024, slice=100, window=(100, 900), tier=3, side=(100, 80))


@pytest.mark.parametrize("change", [
    dict(side=(400, 80)),              # side window in the middle of the window
    dict(side=(100, 900)),             # side_nb == nb
    dict(side=(100, 0)),               # side_nb == 0
    dict(has_list=0),
    dict(slice=0),
    dict(wv=0),
    dict(side_ready=0),                # a side event (or the side stream) is missing
    dict(side_slices=0),
])
def test_a_malformed_mixed_round_is_refused(change):
    p = plan(**GOOD_MIX)
    assert (p["rc"], p["admm"], p["slice"]) == (0, A_MIXED, 100)
    assert plan(**dict(GOOD_MIX, side=(920, 80)))["rc"] == 0                   # at the tail of the window
    p = plan(**dict(GOOD_MIX, **change))
    assert _err(p) == (ERR_STATE, E_MIXED)
    assert p["slice"] == (0 if change.get("slice") == 0 else 100)              # the slice is reported before this check


# ---- 8. the tiers of a handle, from its pattern

def _pattern(P, A):
    Pu = sp.triu(sp.csc_matrix(P), format="csc"); Pu.sort_indices()
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    return (A.shape[1], A.shape[0], Pu.indptr.astype(np.int32), Pu.indices.astype(np.int32),
            Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32))


def penalty_pattern(T, d, r):
    P, q, A, l, u = penalty_qp(np.random.default_rng(T), T, d, r)
    return _pattern(P, A)


def dense_row_pattern():
    """14 variables, six dense rows and a box: the pattern of test_wide_rows_fall_back_to_the_looping_kernels."""
    n, m_c = 14, 6
    return _pattern(np.eye(n), np.vstack([np.ones((m_c, n)), np.eye(n)]))


PATTERNS = {"3x6": lambda: penalty_pattern(6, 3, 4), "7x20": lambda: penalty_pattern(20, 7, 10),
            "12x50": lambda: penalty_pattern(50, 12, 10), "dense rows": dense_row_pattern}

# sco_debug_qp_tiers of handles created on an MI355X by the library of the commit before the planner existed, reduced so that
# of bits 0 - 2 only the lowest set one remains (profiles/qp_tier_refactor.md)
TIERS = {     # routes in the order of ROUTES
    "3x6": (33, 2, 4, 0, 24, 8, 1, 1),
    "7x20": (33, 2, 4, 0, 24, 8, 1, 1),
    "12x50": (88, 88, 88, 88, 88, 8, 88, 88),
    "dense rows": (4, 4, 4, 0, 24, 8, 4, 4),
}


def set_route(monkeypatch, route):
    for s in SWITCHES:
        monkeypatch.delenv("SCO_QP_" + s, raising=False)
    for s in ROUTES[route]:
        monkeypatch.setenv("SCO_QP_" + s, "1")


def plan_tiers(pattern):
    n, m, Pp, Pi, Ap, Ai = pattern
    lib = _lib.load()
    ip = C.POINTER(C.c_int)
    lib.sco_debug_plan_build.restype = C.c_int
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [ip] * 4 + [C.c_int, ip]
    sizes = np.zeros(16, dtype=np.int32)
    assert lib.sco_debug_plan_build(n, m, _lib.iptr(Pp), _lib.iptr(Pi), _lib.iptr(Ap), _lib.iptr(Ai), 1, _lib.iptr(sizes)) == 0
    mask = C.c_int(-1)
    assert lib.sco_debug_plan_tiers(C.byref(mask)) == 0
    return mask.value


@pytest.mark.parametrize("name", list(PATTERNS))
def test_tiers_of_a_handle_follow_from_its_pattern_and_the_switches(monkeypatch, name):
    pattern = PATTERNS[name]()
    for route in ROUTES:
        set_route(monkeypatch, route)
        assert plan_tiers(pattern) == TIERS[name][list(ROUTES).index(route)], route
