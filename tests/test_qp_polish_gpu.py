"""sco_qp_polish on the device against the restatement tests/qp_polish_ref.py.

The restatement is always fed the DEVICE's ADMM (x, y, resid), so ADMM drift plays no part: what is compared is the polish
step alone -- active sets (through y's support), polish_status, x, y, resid.

Tolerance of the device's polished x against the restatement's:  |x_dev - x_ref|_inf <= 1e3 (e_ref + 2.2e-16 |x*|_inf), where
e_ref is the restatement's own distance from x* (tests/golden/qp_exact_7x20.npz; where there is no x*, the distance between
the restatement at 3 and at 6 refinement steps, and x* is the latter).  The 1e3 is for a different summation order through an
unpivoted LDL' whose pivots span twelve orders of magnitude.  y is held to the same rule on its own scale.  The residuals the
device reports are checked against residuals recomputed in NumPy from the x, y it returned: 100 eps times the largest sum of
absolute terms of a row (two summation orders of rows of at most ~40 terms).  The ratios reached are in profiles/qp_polish.md."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
import qp_polish_ref as R                     # noqa: E402
import wv_stack_cases as sc                   # noqa: E402
from make_qp_exact import golden_qp           # noqa: E402
from sco_py_amd import _lib                   # noqa: E402
from sco_py_amd.sco_osqp import osqp_utils    # noqa: E402
from test_qp_gpu import _stack                # noqa: E402
from test_qp_plan import penalty_qp           # noqa: E402
from test_qp_polish import REF_SETTINGS, reject_case   # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.2e-16
MARGIN = 1e3


class Run(object):
    """One handle: load, solve, polish; keeps what both calls returned."""

    def __init__(self, probs, w=None, settings=None, psettings=None, polish=True):
        self.probs, self.w = probs, w
        n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
        self.qp = _lib.BatchedQP(len(probs), n, m, Pp, Pi, Ap, Ai)
        try:
            self.qp.load(Pval, q, Aval, l, u, w)
            self.solve(settings)
            if polish:
                self.polish(psettings)
        except Exception:
            self.qp.close()
            raise

    def solve(self, settings=None):
        self.x, self.y, self.st, self.it, self.res = self.qp.solve(settings)

    def polish(self, psettings=None):
        self.xp, self.yp, self.ps, self.rp = self.qp.polish(psettings)
        self.ms, self.k = self.qp.polish_info()

    def close(self):
        self.qp.close()


def residuals(P, q, A, l, u, w, x, y):
    """(pri, dua, rounding scale of pri, of dua) of a point, as the device defines them."""
    z = A @ x
    pri = np.max(np.abs(z - np.clip(z, l, u)), initial=0.0)
    wy = y                                       # (y is the multiplier of the whole row, copies included)
    dua = np.max(np.abs(P @ x + q + A.T @ wy), initial=0.0)
    fin_l, fin_u = np.where(np.isfinite(l), np.abs(l), 0.0), np.where(np.isfinite(u), np.abs(u), 0.0)
    s_pri = np.max(np.abs(A) @ np.abs(x) + np.maximum(fin_l, fin_u), initial=0.0)
    s_dua = np.max(np.abs(P) @ np.abs(x) + np.abs(q) + np.abs(A.T) @ np.abs(wy), initial=0.0)
    return pri, dua, s_pri, s_dua


def compare(run, xstar=None, refine=3, tag=""):
    """Every problem of the run against the restatement; returns the largest ratio |x_dev - x_ref| / bound."""
    worst = 0.0
    for b, (P, q, A, l, u) in enumerate(run.probs):
        w = np.ones(len(l)) if run.w is None else run.w[b].astype(np.float64)
        args = (P, q, A, l, u, run.x[b], run.y[b], run.res[b], int(run.st[b]))
        ref = R.polish(*args, w=w, refine_iter=refine)
        assert run.ps[b] == ref.status, (tag, b, run.ps[b], ref.status)
        if ref.status != R.OK:
            assert np.array_equal(run.xp[b], run.x[b]) and np.array_equal(run.yp[b], run.y[b]) and np.array_equal(run.rp[b], run.res[b])
            assert run.k[b] == (-1 if ref.status == R.NOT_RUN else len(ref.low) + len(ref.upp))
            continue
        act = np.sort(np.concatenate([ref.low, ref.upp]))
        assert run.k[b] == act.size
        assert np.array_equal(np.flatnonzero(run.yp[b]), act[ref.y[act] != 0.0]), (tag, b)      # the same active sets
        far = R.polish(*args, w=w, refine_iter=2 * refine)
        xs, ys = (far.x if xstar is None else xstar[b]), far.y
        e_x, e_y = np.abs(ref.x - xs).max(), np.abs(ref.y - ys).max()
        bx = MARGIN * (e_x + EPS * np.abs(xs).max())
        by = MARGIN * (e_y + EPS * np.abs(ys).max())
        dy = np.abs(run.yp[b] - ref.y).max(initial=0.0)
        rx, ry = np.abs(run.xp[b] - ref.x).max() / bx, (dy / by if by > 0 else float(dy > 0))    # (no active row: y = 0 on both sides)
        pri, dua, s_pri, s_dua = residuals(P, q, A, l, u, w, run.xp[b], run.yp[b])
        print("%s b=%d N=%d |x_dev-x_ref|=%.2e ratio_x=%.3g ratio_y=%.3g e_ref=%.2e x*_err=%.2e resid dev (%.2e, %.2e) ref (%.2e, %.2e) admm (%.2e, %.2e)"
              % (tag, b, len(q) + act.size, np.abs(run.xp[b] - ref.x).max(), rx, ry, e_x,
                 np.abs(run.xp[b] - xs).max(), run.rp[b, 0], run.rp[b, 1], ref.resid[0], ref.resid[1], run.res[b, 0], run.res[b, 1]))
        assert rx <= 1.0, (tag, b, rx)
        assert ry <= 1.0, (tag, b, ry)
        assert abs(run.rp[b, 0] - pri) <= 100 * EPS * s_pri and abs(run.rp[b, 1] - dua) <= 100 * EPS * s_dua, (tag, b, run.rp[b], pri, dua)
        worst = max(worst, rx)
    return worst


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "trajopt_7x20.npz")), np.load(os.path.join(GOLD, "qp_exact_7x20.npz"))


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("k", [0, 1])
def test_golden_qps_polish_to_the_exact_optimum(gpu, golden, k):
    g, ex = golden
    pre = "p0_qp%d" % k
    run = Run([golden_qp(g, pre)], settings=_lib.default_qp_settings(**REF_SETTINGS) if k else None)
    try:
        assert run.st[0] == 1 and run.ps[0] == 1
        assert (len(np.flatnonzero(run.yp[0])) <= (14, 221)[k]) and run.k[0] == (14, 221)[k]
        compare(run, xstar=[ex[pre + "_x"]], tag=pre)
        err_admm, err = np.abs(run.x[0] - ex[pre + "_x"]).max(), np.abs(run.xp[0] - ex[pre + "_x"]).max()
        print(pre, "admm error", err_admm, "polished", err)
        assert err < 1e-12 and err <= err_admm                     # what the restatement reaches on the CPU (test_qp_polish.py)
        assert run.rp[0, 0] < run.res[0, 0] and run.rp[0, 1] < run.res[0, 1]
    finally:
        run.close()


# ------------------------------------------------------------------ small orders, row weights
@pytest.mark.parametrize("shape", [(3, 3, 4), (6, 3, 4), (20, 7, 10)])
def test_penalty_qps_with_row_weights(gpu, shape):
    T, d, r = shape
    rng = np.random.default_rng(40 + T)
    probs = [penalty_qp(rng, *shape) for _ in range(4)]
    w = np.ones((4, len(probs[0][3])), dtype=np.int32)
    w[:, d:d + T * r] = np.array([1, 2, 3, 5])[:, None]
    run = Run(probs, w=w)
    try:
        assert np.all(run.st == 1) and np.all(run.ps == 1)
        compare(run, tag="penalty %dx%dx%d" % shape)
    finally:
        run.close()


# ------------------------------------------------------------------ tile edges
def hand_qp(rng, n, k):
    """Tridiagonal SPD P, A = I; the first k variables are pushed against an upper bound half a unit under their free optimum."""
    P = np.diag(4.0 + rng.random(n)) + np.diag(np.full(n - 1, -0.5), 1) + np.diag(np.full(n - 1, -0.5), -1)
    x0 = rng.standard_normal(n)
    q = -P @ x0
    l = x0 - 5.0; u = x0 + 5.0
    u[:k] = x0[:k] - 0.5
    return P, q, np.eye(n), l, u


@pytest.mark.parametrize("n,k", [(7, 0), (10, 5), (10, 6), (10, 7), (20, 13)], ids=["N7_k0", "N15", "N16", "N17", "N33"])
def test_hand_built_orders_around_the_tile(gpu, n, k):
    rng = np.random.default_rng(n + k)
    run = Run([hand_qp(rng, n, k) for _ in range(3)])
    try:
        assert np.all(run.st == 1) and np.all(run.k == k) and np.all(run.ps == 1)
        compare(run, tag="hand n=%d k=%d" % (n, k))
    finally:
        run.close()


def test_all_rows_equalities(gpu):
    rng = np.random.default_rng(12)
    n, m = 12, 5
    probs = []
    for _ in range(3):
        M = rng.standard_normal((n, n))
        A = rng.standard_normal((m, n))
        b = rng.standard_normal(m)
        probs.append((M @ M.T + np.eye(n), rng.standard_normal(n), A, b, b.copy()))
    run = Run(probs)
    try:
        assert np.all(run.st == 1) and np.all(run.k == m) and np.all(run.ps == 1)      # N = n + m = 17
        compare(run, tag="equalities")
    finally:
        run.close()


# ------------------------------------------------------------------ no-ops and rejection
def _assert_untouched(run, status, pstatus):
    assert np.all(run.st == status) and np.all(run.ps == pstatus)
    assert np.array_equal(run.xp, run.x) and np.array_equal(run.yp, run.y) and np.array_equal(run.rp, run.res)
    x2, y2, *_ = run.qp.polish()                                   # and the handle still holds them
    assert np.array_equal(x2, run.x) and np.array_equal(y2, run.y)


def test_unsolved_qp_is_not_polished(gpu, golden):
    g, _ = golden
    run = Run([golden_qp(g, "p0_qp1")], settings=_lib.default_qp_settings(**dict(REF_SETTINGS, max_iter=50)))
    try:
        _assert_untouched(run, -2, 0)
        assert run.k[0] == -1
    finally:
        run.close()


def test_infeasible_qp_is_not_polished(gpu):
    probs, w = sc.StackCase("one", (3, 3, 4), -0.05, -3).build()
    run = Run(probs, w=w)
    try:
        _assert_untouched(run, -3, 0)
    finally:
        run.close()


def test_wrong_active_set_is_rejected(gpu):
    P, q, A, l, u, okw = reject_case()
    run = Run([(P, q, A, l, u)] * 2, settings=_lib.default_qp_settings(**okw))
    try:
        _assert_untouched(run, 1, -1)
        compare(run, tag="rejected")                                # the restatement rejects it too, same active rows
    finally:
        run.close()


# ------------------------------------------------------------------ call order, capacity
def test_call_order_and_capacity(gpu):
    rng = np.random.default_rng(3)
    probs = [penalty_qp(rng, 3, 3, 4) for _ in range(2)]
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    qp = _lib.BatchedQP(2, n, m, Pp, Pi, Ap, Ai)
    try:
        qp.load(Pval, q, Aval, l, u)
        with pytest.raises(_lib.ScoHipError) as e:
            qp.polish()
        assert e.value.code == -4
        qp.solve()
        assert np.all(qp.polish()[2] == 1)
        qp.solve()
        qp.set_bounds(l, u)
        with pytest.raises(_lib.ScoHipError) as e:
            qp.polish()
        assert e.value.code == -4
        qp.solve()
        qp.load(Pval, q, Aval, l, u)
        with pytest.raises(_lib.ScoHipError) as e:
            qp.polish()
        assert e.value.code == -4
        with pytest.raises(_lib.ScoHipError) as e:
            qp.solve(); qp.polish(_lib.default_polish_settings(delta=0.0))
        assert e.value.code == -1
    finally:
        qp.close()
    n = 600                                                         # n + m = 1200 > 1104: refused before anything is launched
    eye = sp.identity(n, format="csc")
    qp = _lib.BatchedQP(1, n, n, eye.indptr, eye.indices, eye.indptr, eye.indices)
    try:
        qp.load(np.ones((1, n)), np.zeros((1, n)), np.ones((1, n)), -np.ones((1, n)), np.ones((1, n)))
        with pytest.raises(_lib.ScoHipError) as e:
            qp.polish()
        assert e.value.code == -5
    finally:
        qp.close()


# ------------------------------------------------------------------ after polish
@pytest.fixture(scope="module")
def batch_20x7():
    rng = np.random.default_rng(77)
    probs = [penalty_qp(rng, 20, 7, 10) for _ in range(4)]
    w = np.ones((4, len(probs[0][3])), dtype=np.int32); w[:, 7:207] = 2
    return probs, w


def test_two_runs_are_bit_identical_and_chunks_do_not_matter(gpu, batch_20x7, monkeypatch):
    probs, w = batch_20x7
    run = Run(probs, w=w)
    try:
        first = (run.xp.copy(), run.yp.copy(), run.ps.copy(), run.rp.copy())
        assert np.all(run.ps == 1)
        run.solve(); run.polish()
        for a, b in zip(first, (run.xp, run.yp, run.ps, run.rp)):
            assert np.array_equal(a, b)
        # a 4 MiB workspace holds one image of this batch (order n + k between 513 and 720): four chunks, same bits
        ld = (340 + int(run.k.max()) + 15) // 16 * 16
        assert ld * ld * 8 <= 4 << 20 < 2 * ld * ld * 8
        monkeypatch.setenv("SCO_QP_POLISH_WS_MB", "4")
        run.solve(); run.polish()
        for a, b in zip(first, (run.xp, run.yp, run.ps, run.rp)):
            assert np.array_equal(a, b)
    finally:
        run.close()


def test_warm_start_begins_at_the_polished_point(gpu, batch_20x7):
    probs, w = batch_20x7
    run = Run(probs, w=w)
    try:
        cold = run.it.copy()
        xp = run.xp.copy()
        run.solve(_lib.default_qp_settings(warm_start=1))
        print("iterations cold", cold, "warm after polish", run.it)
        assert np.all(run.st == 1) and np.all(run.it <= cold)
        assert np.abs(run.x - xp).max() < 1e-4                      # (it stays there: the QP tolerances)
    finally:
        run.close()


@pytest.mark.parametrize("which", ["p0_qp1", "20x7x10"])
def test_mfma_and_vector_trailing_updates_agree(gpu, golden, batch_20x7, monkeypatch, which):
    if which == "p0_qp1":
        g, ex = golden
        probs, w, xstar, st = [golden_qp(g, "p0_qp1")], None, [ex["p0_qp1_x"]], _lib.default_qp_settings(**REF_SETTINGS)
    else:
        (probs, w), xstar, st = batch_20x7, None, None
    run = Run(probs, w=w, settings=st)
    try:
        x_mfma = run.xp.copy()
        monkeypatch.setenv("SCO_QP_POLISH_NO_MFMA", "1")
        run.solve(st); run.polish()
        compare(run, xstar=xstar, tag=which + " vector")           # the vector build against the restatement
        for b, (P, q, A, l, u) in enumerate(probs):                # and against the MFMA build, by the same rule
            args = (P, q, A, l, u, run.x[b], run.y[b], run.res[b], 1)
            ww = None if w is None else w[b]
            ref = R.polish(*args, w=ww)
            xs = xstar[b] if xstar is not None else R.polish(*args, w=ww, refine_iter=6).x
            bound = MARGIN * (np.abs(ref.x - xs).max() + EPS * np.abs(xs).max())
            print(which, b, "|x_mfma - x_vector|", np.abs(x_mfma[b] - run.xp[b]).max(), "bound", bound)
            assert np.abs(x_mfma[b] - run.xp[b]).max() <= bound
    finally:
        run.close()


# ------------------------------------------------------------------ Python path
def test_optimize_with_polish_returns_the_polished_point(gpu):
    """The mirror API's small known answer: min x^2 - 4 x inside the trust box [3, 5] -> 3, the lower bound active."""
    P, q, A, l, u = np.array([[2.0]]), np.array([-4.0]), np.array([[1.0]]), np.array([3.0]), np.array([5.0])
    run = Run([(P, q, A, l, u)], settings=_lib.default_qp_settings(**REF_SETTINGS), polish=False)
    try:
        ref = R.polish(P, q, A, l, u, run.x[0], run.y[0], run.res[0], int(run.st[0]))
    finally:
        run.close()
    assert ref.status == R.OK
    v = osqp_utils.OSQPVar("x", 3.0, 5.0)
    args = ([v], [], [osqp_utils.OSQPQuadraticObj(np.array([v]), np.array([v]), np.array([2.0]))], [osqp_utils.OSQPLinearObj(v, -4.0)], [])
    try:
        plain, _ = osqp_utils.optimize(*args)
        out, _ = osqp_utils.optimize(*args, polish=True)
    finally:
        osqp_utils.clear_handle_cache()
    assert plain.info.status_polish == 0 and plain.info.status_val == 1
    assert out.info.status_val == 1 and out.info.status_polish == 1
    assert abs(out.x[0] - ref.x[0]) <= MARGIN * (abs(ref.x[0] - 3.0) + EPS * 3.0)
    assert abs(out.x[0] - 3.0) <= abs(plain.x[0] - 3.0)
