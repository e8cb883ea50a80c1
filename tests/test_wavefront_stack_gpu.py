"""Stacked rows on the wavefront ADMM kernel (csrc/sco_admm_wv.hip, LNK = 2 with an empty partner: single rows of a core
variable other than its last one, i.e. joint limits): every batch of tests/wv_stack_cases.py on the tier against the oracle
ADMM (status, iteration count, x, y, residuals: test_qp_gpu._check) and against the row-local kernel (same statuses and
counts, |dx| < 1e-10), with the tier's own iteration counter as the proof that the wavefront kernel did the work; warm
start, equalities in a stacked slot, run-to-run determinism, the device SQP loop with joint limits, the reference's golden
runs and the object API.  tests/test_wavefront_stack.py holds the plan of each pattern and the oracle's verdict on each
batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import wv_stack_cases as sc
from oracle import arm_family as af
from sco_py_amd import _lib, batch as sb
from test_qp_gpu import _check, _stack, _tiers
from test_wavefront_edges_gpu import _wv_iters, wv_counted      # noqa: F401  (wv_counted: a fixture)
from test_wavefront_link_gpu import _warm_sequence

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def on_tier(monkeypatch):
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    return monkeypatch


def _both_kernels(probs, w, on_tier, counted, check=None):
    """The batch on the tier against the oracle, then on the row-local kernel alone: x, statuses, counts of the tier's run."""
    n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
    assert _tiers(n, m, Pp, Pi, Ap, Ai) & 32, "pattern did not land on the wavefront tier"
    k0 = len(counted)
    _, x_wv, st_wv, it_wv = _check(probs, w=w, check=check)
    assert len(counted) == k0 + 1
    on_tier.setenv("SCO_QP_NO_WV", "1")
    assert not _tiers(n, m, Pp, Pi, Ap, Ai) & 32
    _, x_rl, st_rl, it_rl = _check(probs, w=w, check=[])
    assert counted[k0 + 1] == 0
    assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
    ok = np.isin(st_wv, (1, 2, -2))                     # (the iterate of a certified-infeasible problem is a ray, not an answer)
    assert np.abs(x_wv[ok] - x_rl[ok]).max(initial=0.0) < 1e-10, np.abs(x_wv[ok] - x_rl[ok]).max()
    return x_wv, st_wv, it_wv, counted[k0]


# ---- a. every case on the tier -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_stacked_rows_on_the_wavefront_kernel(gpu, on_tier, wv_counted, case):
    probs, w = case.build()
    x, st, it, count = _both_kernels(probs, w, on_tier, wv_counted, check=case.check)
    assert count == int(it[case.tier].sum()), ("iterations run by the wavefront kernel", count, it)
    assert list(st) == case.status, st


# ---- b. warm start ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 4), (17, 5, 5), (14, 7, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_warm_start_with_stacked_rows_agrees_with_the_row_local_kernel(gpu, on_tier, wv_counted, shape):
    """EXT = 1 with stacked rows (z = A x over the own end alone, y = c y / E): the warm solves run on the wavefront kernel
    and give what the row-local kernel gives from the same start."""
    probs, w = sc.batch(shape)
    wv, cnt = _warm_sequence(probs, w, wv_counted)
    for (x, st, it), c in zip(wv, cnt):
        assert c == int(it.sum()), ("iterations run by the wavefront kernel", c, it)
    (x0, st0, it0), (xw, stw, itw), (xc, stc, itc), (xw2, stw2, itw2) = wv
    assert np.all(st0 == 1) and np.all(stw == 1) and np.all(itw <= it0), (st0, stw, it0, itw)
    assert np.abs(xw - x0).max() < 1e-5
    on_tier.setenv("SCO_QP_NO_WV", "1")
    rl, cnt = _warm_sequence(probs, w, wv_counted)
    assert cnt == [0, 0, 0, 0]
    for (x_wv, st_wv, it_wv), (x_rl, st_rl, it_rl) in zip(wv, rl):
        assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
        fin = np.isin(st_wv, (1, 2, -2))
        assert np.abs(x_wv[fin] - x_rl[fin]).max() < 1e-10, np.abs(x_wv[fin] - x_rl[fin]).max()


# ---- c. equalities in a stacked slot -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.EQ_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_equality_limit_rows_send_a_problem_to_the_row_local_kernel(gpu, on_tier, wv_counted, shape):
    """Problem 1 of the batch has its limit rows made equalities (l = u = mid): they take rho_eq, the problem fails the value
    test and the row-local kernel solves it behind the wavefront launch; the counter holds the others.  (The start pins of
    this batch are narrow boxes: an equality pin next to a two-sided limit row is stacked itself, the test below.)"""
    probs, w = sc.equality_batch(shape)
    x, st, it, count = _both_kernels(probs, w, on_tier, wv_counted)      # (every status is the oracle's)
    assert count == int(it[sc.EQ_OTHERS].sum()), (count, it)
    assert (st[sc.EQ_OTHERS] == 1).sum() >= 3, st


def test_a_pin_in_a_stacked_slot_sends_every_problem_to_the_row_local_kernel(gpu, on_tier, wv_counted):
    """Two-sided limits next to the start pins: a pinned variable has three single rows and both slots free, so pin and limit
    row are stacked.  A slot runs on the base rho and a pin sits on rho_eq: every problem fails the value test, the results
    are the row-local kernel's and the counter stays 0.  (One-sided limits leave the pin over for an extra-row lane.)"""
    probs, w = sc.batch((3, 3, 4), two=True)
    x, st, it, count = _both_kernels(probs, w, on_tier, wv_counted)
    assert count == 0 and np.all(st == 1), (count, st)


# ---- d. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(20, 7, 10), (14, 7, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_stacked_rows_are_run_to_run_deterministic(gpu, on_tier, shape):
    probs, w = sc.batch(shape, B=6)
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
    assert np.all(s0 == 1), s0
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)


# ---- e. the device loop ------------------------------------------------------------------------------------------------------
def _sqp(arrays, params=None):
    a = arrays
    with sb.TrajOptBatch(a["B"], a["d"], a["T"], a["K"], a["O"], reach=bool(a.get("reach")), vel_limits=a.get("vmax") is not None,
                         joint_limits=a.get("jlo") is not None) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"],
                target=a.get("target"), vmax=a.get("vmax"), jlo=a.get("jlo"), jhi=a.get("jhi"))
        tb.solve(params)
        res = tb.fetch(); res.trace = tb.trace(); res.timing = tb.last_timing()
        lib = _lib.load()
        lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
        res.wv_rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    return res


@pytest.mark.parametrize("nb,kw,which,slice_", [(12, dict(d=3, T=6, K=2, O=2, joint_limit=0.3), range(0, 12, 2), 300),
                                                (4, dict(joint_limit=0.2), range(2), 0)], ids=["3x6 slices of 300", "7x20"])
def test_joint_limits_through_the_device_loop_on_the_wavefront_tier(gpu, on_tier, nb, kw, which, slice_):
    """Every round of the SQP loop on the wavefront tier; with admm_slice = 300 a QP parks at slice ends and resumes through
    sz / sy.  Decisions, QP statuses, iteration counts and trajectories of the flat oracle."""
    from test_sqp_gpu import _compare
    arrays, probs = af.make_batch(nb, **kw)
    res = _sqp(arrays, _lib.default_sqp_params(admm_slice=slice_) if slice_ else None)
    assert res.wv_rounds > 0 and res.timing["wv_iters"] > 0, res.timing
    _compare(res, probs, which)


# ---- f. goldens on the tier --------------------------------------------------------------------------------------------------
def test_joint_limit_goldens_run_on_the_wavefront_tier(gpu, on_tier):
    """The j*_ and jt*_ cases of tests/golden/trajopt_jl.npz (recorded from the reference's own code), asserts of
    test_sqp_gpu.test_joint_limits_match_reference_golden_runs; with velocity limits as well (jv*_: four slots per variable)
    and on the reach family (jr*_) the loop stays on the row-local kernel."""
    sys.path.insert(0, GOLD)
    from jl_cases import CASES
    g = np.load(os.path.join(GOLD, "trajopt_jl.npz"))
    for prefix, kw, i in CASES:
        arrays, _ = af.make_batch(1, first=i, **kw)
        res = _sqp(arrays)
        if prefix.startswith("jv") or prefix.startswith("jr"):
            assert res.wv_rounds == 0, prefix
            continue
        assert res.wv_rounds > 0, prefix
        assert np.abs(res.x[0] - g[prefix + "x"]).max() < 1e-6, prefix
        assert bool(res.success[0]) == bool(g[prefix + "success"]), prefix
        nq = int(g[prefix + "n_qp"])
        assert [int(v) for v in res.trace[0][:, 6]] == [int(g["%sqp%d_status" % (prefix, k)]) for k in range(nq)], prefix
        assert [int(v) for v in res.trace[0][:, 7]] == [int(g["%sqp%d_iters" % (prefix, k)]) for k in range(nq)], prefix


# ---- g. the object API -------------------------------------------------------------------------------------------------------
def test_a_prob_with_joint_limits_through_solver_solve_on_the_tier(gpu, on_tier):
    """One Prob with joint limits through Solver().solve(prob), the resident loop on the wavefront tier: the golden run of
    the reference's modules, and Python evaluated nothing (test_object_api_gpu._solve: host_evals == 0)."""
    from test_object_api_gpu import _against_golden, _solve
    sys.path.insert(0, GOLD)
    from jl_cases import CASES
    prefix, kw, i = CASES[0]
    g = np.load(os.path.join(GOLD, "trajopt_jl.npz"))
    ok, prob, traj, step_vars, solver = _solve(af.make_problem(i, **kw))
    assert solver.last_device["wv_iters"] > 0, solver.last_device
    _against_golden(g, prefix, ok, traj, solver)
