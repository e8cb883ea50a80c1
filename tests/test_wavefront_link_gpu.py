"""Link rows on the wavefront ADMM kernel (csrc/sco_admm_wv.hip, LNK = 2: rows on one in-block index of two neighbouring
timesteps, i.e. velocity limits): every batch of tests/wv_link_cases.py on the tier against the oracle ADMM (status,
iteration count, x, y, residuals: test_qp_gpu._check) and against the row-local kernel (same statuses and counts,
|dx| < 1e-10), with the tier's own iteration counter as the proof that the wavefront kernel did the work; warm start, a
mixed batch, run-to-run determinism, and the device SQP loop with velocity limits (time slices: park and resume).
tests/test_wavefront_link.py holds the plan of each pattern and the oracle's verdict on each batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import wv_link_cases as lc
from oracle import arm_family as af
from sco_py_amd import _lib, batch as sb
from test_qp_gpu import _check, _stack, _tiers
from test_wavefront_edges_gpu import _wv_iters, wv_counted      # noqa: F401  (wv_counted: a fixture)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def on_tier(monkeypatch):
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    return monkeypatch


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_link_rows_on_the_wavefront_kernel(gpu, on_tier, wv_counted, case):
    probs, w = case.build()
    n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
    assert _tiers(n, m, Pp, Pi, Ap, Ai) & 32, "pattern did not land on the wavefront tier"
    _, x_wv, st_wv, it_wv = _check(probs, w=w, check=case.check)
    assert len(wv_counted) == 1
    assert wv_counted[0] == int(it_wv.sum()), ("iterations run by the wavefront kernel", wv_counted[0], it_wv)
    assert list(st_wv) == case.status, st_wv
    on_tier.setenv("SCO_QP_NO_WV", "1")
    assert not _tiers(n, m, Pp, Pi, Ap, Ai) & 32
    _, x_rl, st_rl, it_rl = _check(probs, w=w, check=[])
    assert wv_counted[1] == 0
    assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
    ok = np.isin(st_wv, (1, 2, -2))                     # (the iterate of a certified-infeasible problem is a ray, not an answer)
    assert np.abs(x_wv[ok] - x_rl[ok]).max(initial=0.0) < 1e-10, np.abs(x_wv[ok] - x_rl[ok]).max()


def _warm_sequence(probs, w, counted):
    """Cold, warm from the solution, a perturbed q cold, the perturbed q warm from the old QP's solution."""
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    q2 = q + 0.05 * np.random.default_rng(11).standard_normal(q.shape)
    warm = _lib.default_qp_settings(warm_start=1)
    k0 = len(counted)
    qp = _lib.BatchedQP(len(probs), n, m, Pp, Pi, Ap, Ai)
    try:
        qp.load(Pval, q, Aval, l, u, w)
        outs = [qp.solve(), qp.solve(warm)]
        qp.load(Pval, q2, Aval, l, u, w)
        outs.append(qp.solve())
        qp.load(Pval, q, Aval, l, u, w); qp.solve()
        qp.load(Pval, q2, Aval, l, u, w)
        outs.append(qp.solve(warm))
    finally:
        qp.close()
    cnt = counted[k0:]
    return [(o[0], o[2], o[3]) for o in outs], [cnt[0], cnt[1], cnt[2], cnt[4]]


@pytest.mark.parametrize("shape", [(3, 3, 4), (17, 5, 5), (14, 7, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_warm_start_with_link_rows_agrees_with_the_row_local_kernel(gpu, on_tier, wv_counted, shape):
    """EXT = 1 with link rows (z = A x over both ends, y = c y / E): the warm solves run on the wavefront kernel and give
    what the row-local kernel gives from the same start."""
    probs, w = lc.batch(lc.one_sided, shape, 0.15)
    wv, cnt = _warm_sequence(probs, w, wv_counted)
    for (x, st, it), c in zip(wv, cnt):
        assert c == int(it.sum()), ("iterations run by the wavefront kernel", c, it)
    (x0, st0, it0), (xw, stw, itw), (xc, stc, itc), (xw2, stw2, itw2) = wv
    ok = st0 == 1                                       # (problem 2 of the 17 x 5 batch is primal infeasible: wv_link_cases)
    assert ok.sum() >= 3 and np.all(stw[ok] == 1) and np.all(itw[ok] <= it0[ok]), (st0, stw, it0, itw)
    assert np.abs(xw[ok] - x0[ok]).max() < 1e-5
    on_tier.setenv("SCO_QP_NO_WV", "1")
    rl, cnt = _warm_sequence(probs, w, wv_counted)
    assert cnt == [0, 0, 0, 0]
    for (x_wv, st_wv, it_wv), (x_rl, st_rl, it_rl) in zip(wv, rl):
        assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
        fin = np.isin(st_wv, (1, 2, -2))                # (the iterate of a certified-infeasible problem is a ray, not an answer)
        assert np.abs(x_wv[fin] - x_rl[fin]).max() < 1e-10, np.abs(x_wv[fin] - x_rl[fin]).max()


@pytest.mark.parametrize("shape", [(3, 3, 4), (14, 7, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_equality_link_rows_send_a_problem_to_the_row_local_kernel(gpu, on_tier, wv_counted, shape):
    """Problem 1 of the batch has its link rows made equalities (two-sided rows with l = u): they take rho_eq, the problem
    fails the value test and the row-local kernel solves it behind the wavefront launch; the counter holds the others."""
    T, d, r = shape
    probs, w = lc.batch(lc.two_sided, shape, 0.15, B=5)
    P, q, A, l, u = probs[1]
    l, u = l.copy(), u.copy()
    lo = d + T * r; nl = lc.n_links(lc.two_sided, T, d)
    l[lo:lo + nl] = 0.01; u[lo:lo + nl] = 0.01
    probs[1] = (P, q, A, l, u)
    others = [0, 2, 3, 4]
    _, x_wv, st_wv, it_wv = _check(probs, w=w)           # (every status is the oracle's: a draw may be primal infeasible)
    assert wv_counted == [int(it_wv[others].sum())], (wv_counted, it_wv)
    assert (st_wv[others] == 1).sum() >= 3, st_wv
    on_tier.setenv("SCO_QP_NO_WV", "1")
    _, x_rl, st_rl, it_rl = _check(probs, w=w, check=[])
    assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl)
    ok = np.isin(st_wv, (1, 2, -2))
    assert np.abs(x_wv[ok] - x_rl[ok]).max() < 1e-10


@pytest.mark.parametrize("shape", [(20, 7, 10), (14, 7, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_link_rows_are_run_to_run_deterministic(gpu, on_tier, shape):
    probs, w = lc.batch(lc.one_sided, shape, 0.15, B=6)
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    outs = []
    for _ in range(2):
        qp = _lib.BatchedQP(6, n, m, Pp, Pi, Ap, Ai)
        try:
            qp.load(Pval, q, Aval, l, u, w)
            outs.append(qp.solve())
            assert _wv_iters(qp) == int(outs[-1][3].sum())
        finally:
            qp.close()
    (x0, y0, s0, i0, _), (x1, y1, s1, i1, _) = outs
    assert np.all(np.isin(s0, (1, -3))) and (s0 == 1).sum() >= 4, s0      # (a draw may be primal infeasible: wv_link_cases)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)


# ---- the device loop ------------------------------------------------------------------------------------------------------
def _sqp(arrays, params=None):
    res = None
    a = arrays
    with sb.TrajOptBatch(a["B"], a["d"], a["T"], a["K"], a["O"], reach=bool(a.get("reach")), vel_limits=a.get("vmax") is not None) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"],
                target=a.get("target"), vmax=a.get("vmax"))
        tb.solve(params)
        res = tb.fetch(); res.trace = tb.trace(); res.timing = tb.last_timing()
        lib = _lib.load()
        lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
        res.wv_rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    return res


@pytest.mark.parametrize("nb,kw,which,slice_", [(12, dict(d=3, T=6, K=2, O=2, vel_limit=0.6), range(0, 12, 2), 300),
                                                (4, dict(vel_limit=0.3), range(2), 0)], ids=["3x6 slices of 300", "7x20"])
def test_velocity_limits_through_the_device_loop_on_the_wavefront_tier(gpu, on_tier, nb, kw, which, slice_):
    """Every round of the SQP loop on the wavefront tier; with admm_slice = 300 a QP parks at slice ends and resumes through
    sz / sy.  Decisions, QP statuses, iteration counts and trajectories of the flat oracle."""
    from test_sqp_gpu import _compare
    arrays, probs = af.make_batch(nb, **kw)
    res = _sqp(arrays, _lib.default_sqp_params(admm_slice=slice_) if slice_ else None)
    assert res.wv_rounds > 0 and res.timing["wv_iters"] > 0, res.timing
    _compare(res, probs, which)


def test_velocity_limit_golden_runs_on_the_wavefront_tier(gpu, on_tier):
    """The v*_ and t*_ cases of tests/golden/trajopt_vel.npz (recorded from the reference's own code), asserts of
    test_sqp_gpu.test_velocity_limits_match_reference_golden_runs_incl_infeasible_projection."""
    sys.path.insert(0, GOLD)
    from vel_cases import CASES
    g = np.load(os.path.join(GOLD, "trajopt_vel.npz"))
    for prefix, kw, i in CASES:
        if not (prefix.startswith("v") and not prefix.startswith("vr")) and not prefix.startswith("t"):
            continue
        arrays, _ = af.make_batch(1, first=i, **kw)
        res = _sqp(arrays)
        assert res.wv_rounds > 0, prefix
        assert np.abs(res.x[0] - g[prefix + "x"]).max() < 1e-6, prefix
        assert bool(res.success[0]) == bool(g[prefix + "success"]), prefix
        nq = int(g[prefix + "n_qp"])
        assert [int(v) for v in res.trace[0][:, 6]] == [int(g["%sqp%d_status" % (prefix, k)]) for k in range(nq)], prefix
        assert [int(v) for v in res.trace[0][:, 7]] == [int(g["%sqp%d_iters" % (prefix, k)]) for k in range(nq)], prefix


def test_reach_with_velocity_limits_stays_off_the_wavefront_tier(gpu, on_tier):
    arrays, _ = af.make_batch(4, d=3, T=6, K=2, O=2, vel_limit=0.6, reach=True)
    res = _sqp(arrays)
    assert res.wv_rounds == 0
