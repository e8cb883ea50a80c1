"""Dense NumPy restatement of the polish step (include/sco_hip.h: sco_qp_polish), the reference of tests/test_qp_polish*.py.

Written from OSQP's published description (Stellato et al., "OSQP: an operator splitting solver for quadratic programs",
section 4 "Solution polishing", and the acceptance test of OSQP 0.6's polish.c):

  * active rows from the ADMM pair (x, y):  low = {i : (A x)_i - l_i < -y_i / w_i},  upp = {i : u_i - (A x)_i < y_i / w_i};
  * reduced KKT system of order n + |low| + |upp| with the rows ordered [low; upp],
        [[P + delta I, Ar'], [Ar, -delta I]] [x; s] = [-q; l_low; u_upp],
    solved by an LDL' WITHOUT pivoting in float64, then `refine_iter` steps of iterative refinement against the
    unregularised matrix [[P, Ar'], [Ar, 0]];
  * a row of multiplicity w_i enters once.  y_i is the multiplier of the logical row -- the sum over its w_i copies, which
    is what sco_qp_solve and the oracle return -- so one copy carries y_i / w_i (the tests above are OSQP's on a copy) and
    the unknown of the reduced system is y_i itself;
  * residuals of the polished point, unscaled:  pri = |A x - clip(A x, l, u)|_inf,  dua = |P x + q + A' y|_inf;
  * accepted (status OK) when both are smaller than the solve's, or one is smaller while the solve's other one is already
    under 1e-10; otherwise status FAILED and (x, y, resid) stay the solve's.  A solve whose status is not 1: NOT_RUN.
"""
from collections import namedtuple

import numpy as np

OK, FAILED, NOT_RUN = 1, -1, 0
Polished = namedtuple("Polished", "x y status resid low upp x_try y_try resid_try")


def active_sets(A, l, u, x, y, w):
    z = A @ x
    yc = y / w
    low = np.where(z - l < -yc)[0]
    upp = np.where(u - z < yc)[0]
    return low, upp


def ldl_nopivot(K):
    """Unit lower L and diagonal d with K = L diag(d) L', columns left to right, no pivoting."""
    K = np.array(K, dtype=np.float64)
    N = K.shape[0]
    L = np.eye(N); d = np.zeros(N)
    for k in range(N):
        d[k] = K[k, k]
        col = K[k + 1:, k] / d[k]
        L[k + 1:, k] = col
        K[k + 1:, k + 1:] -= np.outer(col, K[k + 1:, k])
    return L, d


def _ldl_solve(L, d, r):
    from scipy.linalg import solve_triangular
    v = solve_triangular(L, r, lower=True, unit_diagonal=True)
    return solve_triangular(L.T, v / d, lower=False, unit_diagonal=True)


def polish(P, q, A, l, u, x, y, resid, status=1, w=None, delta=1e-6, refine_iter=3):
    """P full symmetric (n x n), A (m x n) dense; (x, y, resid) what the solve returned, resid = (primal, dual)."""
    P = np.asarray(P, dtype=np.float64); A = np.asarray(A, dtype=np.float64)
    n, m = P.shape[0], A.shape[0]
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64); resid = np.asarray(resid, dtype=np.float64)
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    none = np.zeros(0, dtype=np.int64)
    if status != 1:
        return Polished(x, y, NOT_RUN, resid, none, none, x, y, resid)
    low, upp = active_sets(A, l, u, x, y, w)
    act = np.concatenate([low, upp])
    k = act.size
    Ar = A[act]
    Kreg = np.block([[P + delta * np.eye(n), Ar.T], [Ar, -delta * np.eye(k)]])
    Kun = np.block([[P, Ar.T], [Ar, np.zeros((k, k))]])
    rhs = np.concatenate([-q, l[low], u[upp]])
    with np.errstate(all="ignore"):
        L, d = ldl_nopivot(Kreg)
        sol = _ldl_solve(L, d, rhs)
        for _ in range(refine_iter):
            sol = sol + _ldl_solve(L, d, rhs - Kun @ sol)
        xp = sol[:n]
        yp = np.zeros(m); yp[act] = sol[n:]
        z = A @ xp
        pri = np.max(np.abs(z - np.clip(z, l, u)), initial=0.0)
        dua = np.max(np.abs(P @ xp + q + A.T @ yp), initial=0.0)
    rp = np.array([pri, dua])
    good = bool((pri < resid[0] and dua < resid[1]) or (pri < resid[0] and resid[1] < 1e-10) or
                (dua < resid[1] and resid[0] < 1e-10))
    if good:
        return Polished(xp, yp, OK, rp, low, upp, xp, yp, rp)
    return Polished(x, y, FAILED, resid, low, upp, xp, yp, rp)
