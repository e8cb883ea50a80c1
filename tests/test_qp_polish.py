"""Polish (include/sco_hip.h: sco_qp_polish) without a GPU: the ABI, the restatement tests/qp_polish_ref.py against the
ADMM-free optima of the golden QPs, row multiplicities, a rejected polish, and the host-only launch plan
(csrc/qp_polish_plan.cpp through sco_debug_polish_plan)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
import qp_polish_ref as R                     # noqa: E402
from make_qp_exact import golden_qp           # noqa: E402
from oracle import osqp_ref as o              # noqa: E402
from sco_py_amd import _lib                   # noqa: E402
from sco_py_amd.sco_osqp import osqp_utils, prob, solver   # noqa: E402
from test_qp_plan import penalty_qp           # noqa: E402
REF_SETTINGS = dict(rho=0.1, sigma=5e-10, eps_abs=1e-6, eps_rel=1e-9, max_iter=100000)    # osqp_utils.py:10-15

# The rejected polish: penalty_qp(default_rng(3), 3, 3, 4) solved to eps_abs = eps_rel = 0.1 stops after 25 iterations with
# residuals (0.108, 0.036); the active sets guessed from that pair (13 low, 8 upp rows) are wrong and the polished point has
# a primal residual of 0.67 > 0.108, so OSQP's rule keeps the ADMM answer.  Also the input of tests/test_qp_polish_gpu.py.
REJECT_SEED, REJECT_SHAPE, REJECT_EPS = 3, (3, 3, 4), 0.1


def reject_case():
    P, q, A, l, u = penalty_qp(np.random.default_rng(REJECT_SEED), *REJECT_SHAPE)
    return P, q, A, l, u, dict(eps_abs=REJECT_EPS, eps_rel=REJECT_EPS)


def oracle_polish(P, q, A, l, u, w=None, okw=None, **pkw):
    res = o.solve(P, q, A, l, u, w=w, **(okw or {}))
    return res, R.polish(P, q, A, l, u, res.x, res.y, (res.info.pri_res, res.info.dua_res), res.info.status_val, w=w, **pkw)


# ------------------------------------------------------------------ ABI
def test_header_and_binding_declare_polish():
    text = open(os.path.join(os.path.dirname(HERE), "include", "sco_hip.h")).read()
    for name in ("sco_qp_polish", "sco_qp_default_polish_settings"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.ABI
    for name, val in (("SCO_QP_POLISH_OK", 1), ("SCO_QP_POLISH_FAILED", -1), ("SCO_QP_POLISH_NOT_RUN", 0)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), text), name
    assert C.sizeof(_lib.PolishSettings) == 16
    s = _lib.default_polish_settings()
    assert (s.delta, s.refine_iter) == (1e-6, 3)                  # OSQP 0.6: delta, polish_refine_iter
    assert _lib.default_polish_settings(refine_iter=5).refine_iter == 5
    with pytest.raises(TypeError):
        _lib.default_polish_settings(nope=1)


def test_mirror_api_accepts_polish():
    for fn in (osqp_utils.optimize, osqp_utils._solve_qp, prob.Prob.optimize, solver.Solver.solve):
        p = inspect.signature(fn).parameters
        assert "polish" in p and p["polish"].default is False, fn
    assert "host loop" in solver.Solver.solve.__doc__


def test_polish_flag_travels_down_the_seam_and_splits_the_batches(monkeypatch):
    """optimize(polish=True) -> a seventh settings entry (requests with and without polish never share a launch) and
    info.status_polish from the fourth entry of the result; without the flag the request is what it always was."""
    seen = []

    def fake(requests):
        seen.extend(r["settings"] for r in requests)
        n = requests[0]["A"].shape[1]
        return [(np.full(n, 3.0), 1, 25) + ((1,) if len(r["settings"]) > 6 else ()) for r in requests]

    monkeypatch.setattr(osqp_utils, "_solve_qp_batch", fake)
    v = osqp_utils.OSQPVar("x")
    args = ([v], [], [osqp_utils.OSQPQuadraticObj(np.array([v]), np.array([v]), np.array([2.0]))], [osqp_utils.OSQPLinearObj(v, -4.0)], [])
    res, _ = osqp_utils.optimize(*args)
    assert res.info.status_polish == 0 and len(seen[-1]) == 6
    res, _ = osqp_utils.optimize(*args, polish=True)
    assert res.info.status_polish == 1 and len(seen[-1]) == 7 and seen[-1][6] == 1.0 and res.x[0] == 3.0


# ------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "trajopt_7x20.npz")), np.load(os.path.join(GOLD, "qp_exact_7x20.npz"))


@pytest.mark.parametrize("k", [0, 1])
def test_polished_golden_qps_land_on_the_exact_optimum(golden, k):
    g, ex = golden
    pre = "p0_qp%d" % k
    P, q, A, l, u = golden_qp(g, pre)
    res, pol = oracle_polish(P, q, A, l, u, okw=REF_SETTINGS if k else {})
    assert res.info.status_val == 1 and pol.status == R.OK
    err = np.abs(pol.x - ex[pre + "_x"]).max()
    print(pre, "admm", np.abs(res.x - ex[pre + "_x"]).max(), "polished", err, "active", len(pol.low), len(pol.upp))
    assert err < 1e-12
    assert (len(pol.low), len(pol.upp)) == ((9, 5), (208, 13))[k]
    assert pol.resid[0] < res.info.pri_res and pol.resid[1] < res.info.dua_res


def test_unsolved_golden_qp_is_not_polished(golden):
    g, _ = golden
    P, q, A, l, u = golden_qp(g, "p0_qp2")
    res, pol = oracle_polish(P, q, A, l, u, okw=REF_SETTINGS)
    assert res.info.status_val == -2 and pol.status == R.NOT_RUN
    assert np.array_equal(pol.x, res.x) and np.array_equal(pol.y, res.y)


def test_weighted_rows_match_physically_duplicated_rows():
    rng = np.random.default_rng(5)
    T, d, r = 5, 3, 4
    for mult in (1, 2, 3, 4, 5):
        P, q, A, l, u = penalty_qp(rng, T, d, r)
        m = len(l)
        w = np.ones(m, dtype=np.int32); w[d:d + T * r] = mult
        _, pol = oracle_polish(P, q, A, l, u, w=w)
        order = np.repeat(np.arange(m), w)
        _, dup = oracle_polish(P, q, A[order], l[order], u[order])
        assert pol.status == R.OK and dup.status == R.OK
        assert np.abs(pol.x - dup.x).max() < 1e-10
        # y is the multiplier of the logical row: the sum over its physical copies
        assert np.abs(np.add.reduceat(dup.y, np.cumsum(w) - w) - pol.y).max() < 1e-8 * (1 + np.abs(pol.y).max())


def test_wrong_active_set_is_rejected():
    P, q, A, l, u, okw = reject_case()
    res, pol = oracle_polish(P, q, A, l, u, okw=okw)
    assert res.info.status_val == 1 and res.info.iter == 25
    assert pol.status == R.FAILED
    assert np.array_equal(pol.x, res.x) and np.array_equal(pol.y, res.y)
    assert tuple(pol.resid) == (res.info.pri_res, res.info.dua_res)
    assert pol.resid_try[0] > 2 * res.info.pri_res                  # 0.67 against 0.108: not a borderline rejection
    # the same QP at the reference's tolerances polishes fine
    _, good = oracle_polish(P, q, A, l, u)
    assert good.status == R.OK


# ------------------------------------------------------------------ the launch plan
def _plan(n, m, batch, k, budget=0):
    lib = _lib.load()
    lib.sco_debug_polish_plan.restype = C.c_int
    lib.sco_debug_polish_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 7)()
    rc = lib.sco_debug_polish_plan(n, m, batch, k, budget, out)
    assert rc == out[0]
    return dict(rc=rc, err=out[1], ld=out[2], per_chunk=out[3], chunks=out[4], lds=out[5], ws=out[6])


def test_plan_tile_edges():
    assert _plan(16, 8, 4, 0)["ld"] == 16 and _plan(5, 8, 4, 0)["ld"] == 16            # k = 0: the order is n
    for N, ld in ((15, 16), (16, 16), (17, 32), (33, 48)):
        p = _plan(10, 40, 3, N - 10)
        assert (p["rc"], p["ld"], p["per_chunk"], p["chunks"]) == (0, ld, 3, 1)
        assert p["lds"] == (16 * ld + 32) * 8 and p["ws"] == 3 * ld * ld * 8


def test_plan_capacity_and_budget(monkeypatch):
    monkeypatch.delenv("SCO_QP_POLISH_WS_MB", raising=False)
    p = _plan(340, 764, 1024, 764)                                  # N = 1104, the capacity constant
    assert p["rc"] == 0 and p["ld"] == 1104 and p["lds"] <= 160 * 1024
    assert p["per_chunk"] == (1 << 30) // (1104 * 1104 * 8) == 110 and p["chunks"] == 10
    assert _plan(340, 754, 1, 754)["ld"] == 1104                    # the 7-DOF x 20 penalty QP with every row active: 1094
    p = _plan(340, 765, 1024, 765)                                  # one beyond it
    assert p["rc"] == -5 and p["err"] == 2 and p["ld"] == 0
    # a budget that holds exactly one image: one problem per chunk; one byte less: refused
    img = 576 * 576 * 8
    p = _plan(340, 554, 5, 221, img)
    assert (p["rc"], p["ld"], p["per_chunk"], p["chunks"], p["ws"]) == (0, 576, 1, 5, img)
    assert _plan(340, 554, 5, 221, 2 * img - 1)["per_chunk"] == 1
    assert _plan(340, 554, 5, 221, 2 * img)["chunks"] == 3
    p = _plan(340, 554, 5, 221, img - 1)
    assert p["rc"] == -5 and p["err"] == 3
    monkeypatch.setenv("SCO_QP_POLISH_WS_MB", "3")                  # the environment's budget when the call gives none
    assert _plan(340, 554, 5, 221)["per_chunk"] == 1
    for bad in ((0, 5, 1, 0), (5, -1, 1, 0), (5, 5, 0, 0), (5, 5, 1, 6), (5, 5, 1, -1)):
        assert _plan(*bad)["rc"] == -1
