"""Width profiles of the wavefront ADMM kernel on the device (csrc/sco_admm_wv.hip: the JW argument of qp_admm_wv_kernel,
the value test of qp_wv_factor_kernel; csrc/wv_plan.cpp: wv_plan_widths).  A hinge slot whose rows are promised to be zero
from some column on skips those columns; skipping fma(0.0, x, s) leaves s, so against the generic kernel (SCO_WV_JW=0)
NOTHING may differ: x, y, statuses and iteration counts under np.array_equal (which takes +0 and -0 as equal, the one
deviation there can be).  Against the row-local kernel (SCO_QP_NO_WV=1), which shares no code with either: equal statuses
and counts, |dx| <= 1e-9, the bar of tests/test_wavefront_sweep_slots_gpu.py.

QP layer, 7 joints, 10 hinge rows per timestep with the benchmark's widths 2, 2, 3, 3, 5, 5, 6, 6, 7, 7 (slots: 3, 5, 7, 7),
8 problems at 17 timesteps -- the shortest horizon on <7,4,3,10,3> -- and at 20.  The pattern keeps every Jacobian entry, as
the SQP layer's does; the values beyond a row's width are 0.0.  max_iter 600, check_termination 25.  In every batch
problem 7 is primal infeasible (a pin 20 outside its variable's box: the certificate branch, status -3 well before
max_iter), the others converge or end at max_iter; all three ends are asserted for the cold cases.  The warm case solves, perturbs q and solves again from the solution (the
instantiation that may start warm, <7,4,3,10,3,1,0,JW>).

A wrong hint costs speed, never a result: with a non-zero written beyond its width into ONE problem's values, that problem
must leave the tier (the iterations the tier's counter reports are exactly the other problems') and match the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_gpu import TOL as ORACLE_TOL
from test_qp_plan import penalty_qp
from test_wavefront_edges_gpu import _wv_iters

pytestmark = pytest.mark.gpu

B, D, R = 8, 7, 10
WIDTHS = [2, 2, 3, 3, 5, 5, 6, 6, 7, 7]
MAX_ITER, CHECK = 600, 25
TOL = 1e-9


def _batch(T, seed):
    """(dense pattern problem, problems with the width structure, hinge weights, row_width[m])."""
    rng = np.random.default_rng(seed)
    dense = penalty_qp(rng, T, D, R)
    probs = []
    for b in range(B):
        P, q, A, l, u = penalty_qp(rng, T, D, R)
        A = A.copy()
        for t in range(T):
            for k in range(R):
                A[D + t * R + k, t * D + WIDTHS[k]:(t + 1) * D] = 0.0
        probs.append((P, q, A, l, u))
    # problem 7: the pin of joint 0 moved 20 outside the joint's box of +-1 -- primal infeasible
    P, q, A, l, u = probs[7]
    l = l.copy(); u = u.copy(); l[0] += 20.0; u[0] += 20.0
    probs[7] = (P, q, A, l, u)
    m = len(l)
    w = np.ones((B, m), dtype=np.int32); w[:, D:D + T * R] = rng.integers(1, 4, size=(B, 1))
    rw = np.zeros(m, dtype=np.int32); rw[D:D + T * R] = np.tile(WIDTHS, T)
    return dense, probs, w, rw


def _stack(dense, probs):
    """The pattern of the dense problem (every Jacobian entry present), the values of `probs`."""
    P0, q0, A0, l0, u0 = dense
    n, m = len(q0), len(l0)
    Pu = sp.triu(sp.csc_matrix(P0), format="csc"); Pu.sort_indices()
    Ac = sp.csc_matrix((A0 != 0).astype(float)); Ac.sort_indices()
    pr, pc = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    ar, ac = Ac.indices, np.repeat(np.arange(n), np.diff(Ac.indptr))
    for p in probs:
        assert not np.any((p[2] != 0) & (A0 == 0)) and not np.any((np.triu(p[0]) != 0) & (np.triu(P0) == 0))
    Pval = np.stack([p[0][pr, pc] for p in probs]); Aval = np.stack([p[2][ar, ac] for p in probs])
    q = np.stack([p[1] for p in probs]); l = np.stack([p[3] for p in probs]); u = np.stack([p[4] for p in probs])
    return n, m, Pu.indptr, Pu.indices, Ac.indptr, Ac.indices, Pval, q, Aval, l, u


def _profile(qp):
    """The width profile the handle's next launch runs (0: generic), from the handle's own plan."""
    import ctypes as C
    lib = _lib.load()
    lib.sco_debug_qp_wv_profile.restype = C.c_int; lib.sco_debug_qp_wv_profile.argtypes = [C.c_void_p]
    return lib.sco_debug_qp_wv_profile(qp._h)


def _solve(stacked, w, rw, warm, want_profile):
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = stacked
    qp = _lib.BatchedQP(Pval.shape[0], n, m, Pp, Pi, Ap, Ai)
    try:
        qp.set_row_widths(rw)
        if want_profile is not None:
            assert _profile(qp) == want_profile, (_profile(qp), want_profile)
        qp.load(Pval, q, Aval, l, u, w)
        st = _lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK)
        if warm:
            qp.solve(st)
            seen = _wv_iters(qp)
            q2 = q + 0.05 * np.random.default_rng(11).standard_normal(q.shape)
            qp.load(Pval, q2, Aval, l, u, w)
            x, y, s, it, _ = qp.solve(_lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK, warm_start=1))
            return x, y, s, it, _wv_iters(qp) - seen
        x, y, s, it, _ = qp.solve(st)
        return x, y, s, it, _wv_iters(qp)
    finally:
        qp.close()


PROFILE_3577 = 3 | (5 << 4) | (7 << 8) | (7 << 12)
_memo = {}


def _three_ways(monkeypatch, T, seed, warm):
    """Profiled kernel, generic kernel (SCO_WV_JW=0), row-local kernel (SCO_QP_NO_WV=1): computed once per case."""
    key = (T, seed, warm)
    if key not in _memo:
        dense, probs, w, rw = _batch(T, seed)
        stacked = _stack(dense, probs)
        monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
        monkeypatch.setenv("SCO_WV_JSORT", "0")                 # rows in row order: the profiled kernel adds what the generic one adds
        outs = []
        for env, prof in (({}, PROFILE_3577), ({"SCO_WV_JW": "0"}, 0), ({"SCO_QP_NO_WV": "1"}, 0)):
            for k in ("SCO_WV_JW", "SCO_QP_NO_WV"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            outs.append(_solve(stacked, w, rw, warm, prof))
        _memo[key] = outs
    return _memo[key]


CASES = [(17, 9301, False), (20, 9302, False), (20, 9303, True)]
# how the problems 0 .. 6 of the cold batches end on the CPU oracle (problem 7: the certificate): converged below max_iter,
# or at max_iter with status -2
ENDS = {9301: ([0, 3, 4, 5], [1, 2, 6]), 9302: ([0, 1, 2], [3, 4, 5, 6])}
IDS = ["7x17", "7x20", "7x20 warm"]


@pytest.mark.parametrize("T,seed,warm", CASES, ids=IDS)
def test_profiled_kernel_equals_the_generic_kernel(gpu, monkeypatch, T, seed, warm):
    (x0, y0, s0, i0, t0), (x1, y1, s1, i1, t1), _ = _three_ways(monkeypatch, T, seed, warm)
    print("statuses", s0, "iterations", i0)
    assert t0 == int(i0.sum()) and t1 == int(i1.sum())                       # the tier ran every iteration, both times
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)


@pytest.mark.parametrize("T,seed,warm", CASES, ids=IDS)
def test_profiled_kernel_against_the_row_local_kernel(gpu, monkeypatch, T, seed, warm):
    (x0, y0, s0, i0, t0), _, (xr, yr, sr_, ir, tr) = _three_ways(monkeypatch, T, seed, warm)
    assert tr == 0 and t0 == int(i0.sum())
    assert np.array_equal(s0, sr_) and np.array_equal(i0, ir), (s0, sr_, i0, ir)
    if not warm:
        # every end of the loop: converged, max_iter (-2, or 2 when the ten times wider test passes), a certificate
        assert sr_[7] == -3 and ir[7] < MAX_ITER, (sr_, ir)
        conv, capped = ENDS[seed]
        assert np.all(sr_[conv] == 1) and np.all(ir[conv] < MAX_ITER), (sr_, ir)
        assert np.all(sr_[capped] == -2) and np.all(ir[capped] == MAX_ITER), (sr_, ir)
    fin = np.isin(sr_, (1, 2, -2))
    err = float(np.abs(x0[fin] - xr[fin]).max())
    print("max |dx| = %.3e" % err)
    assert err <= TOL, err


def test_a_nonzero_beyond_its_width_sends_the_problem_to_the_row_local_kernel(gpu, monkeypatch):
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.setenv("SCO_WV_JSORT", "0")
    dense, probs, w, rw = _batch(17, 9304)
    bad = 3
    P, q, A, l, u = probs[bad]
    A = A.copy(); A[D + 5 * R + 0, 5 * D + 4] = 0.37                 # row 0 of timestep 5 (width 2, slot 0: 3 columns), column 4
    probs[bad] = (P, q, A, l, u)
    stacked = _stack(dense, probs)
    x, y, s, it, on_tier = _solve(stacked, w, rw, False, PROFILE_3577)
    print("statuses", s, "iterations", it, "on the tier", on_tier)
    assert on_tier == int(it.sum()) - int(it[bad]), (on_tier, it)     # the others stayed, this one left
    for b in (bad, 0):
        ref = o.solve(*probs[b], w=w[b], max_iter=MAX_ITER, check_termination=CHECK)
        assert s[b] == ref.info.status_val and it[b] == ref.info.iter, (b, s[b], it[b], ref.info.status_val, ref.info.iter)
        assert np.abs(x[b] - ref.x).max() < ORACLE_TOL
    # without the profile the same values are the tier's: the generic kernel multiplies every column
    monkeypatch.setenv("SCO_WV_JW", "0")
    x2, y2, s2, it2, on2 = _solve(stacked, w, rw, False, 0)
    assert on2 == int(it2.sum()) and np.array_equal(s, s2) and np.array_equal(it, it2)
    assert np.abs(x - x2).max() <= TOL


PROFILE_7632 = 7 | (6 << 4) | (3 << 8) | (2 << 12)


@pytest.mark.parametrize("T,seed,warm", CASES, ids=IDS)
def test_rows_dealt_by_width_against_the_row_local_kernel(gpu, monkeypatch, T, seed, warm):
    """The default, SCO_WV_JSORT unset: the widest rows of a timestep in slot 0, widths 7, 6, 3, 2.  The partial sums of a block add in
    another order, so the generic kernel is no referee to the bit; the row-local kernel is, at its usual bar."""
    _, _, (xr, yr, sr_, ir, tr) = _three_ways(monkeypatch, T, seed, warm)
    dense, probs, w, rw = _batch(T, seed)
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_WV_JSORT", raising=False)
    x, y, s_, it, on_tier = _solve(_stack(dense, probs), w, rw, warm, PROFILE_7632)
    assert on_tier == int(it.sum())
    assert np.array_equal(s_, sr_) and np.array_equal(it, ir), (s_, sr_, it, ir)
    fin = np.isin(sr_, (1, 2, -2))
    err = float(np.abs(x[fin] - xr[fin]).max())
    print("max |dx| = %.3e" % err)
    assert err <= TOL, err
