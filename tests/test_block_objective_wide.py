"""Wide objective terms (SCO_FAM_FLAG_OBJ_WIDE: 17 to 32 numbers), host side: the eigenvalue sweep the device restates at
orders 17, 24 and 32 and the finite-difference Hessians of the wide terms, against mpmath at 50 digits; compile_rows and
compile_prob on wide programs; the flat oracle and the mirror API's host loop against runs of the reference's own modules
(tests/golden/make_golden_blockobj32.py); the ADMM tier plans of the 24- to 32-number bands.  No GPU here."""
import ctypes as C
import os
import sys

import mpmath
import numpy as np
import pytest
import scipy.sparse as sp

import blockobj_build as bb
import conftest as ct
from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib, devexpr as dx, rowexpr as rx, workloads as wl
from sco_py_amd.rowexpr import X, P, compile_rows
from sco_py_amd.sco_osqp import compile as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from blockobj32_cases import CASES as GOLDEN32        # noqa: E402

mp = mpmath.mp


def _rotated(lam, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(lam), len(lam))))
    h = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return 0.5 * (h + h.T)


def _near_diagonal(n, off):
    h = np.diag(np.concatenate([np.linspace(-1.0, 1.0, n - 4), [0.25] * 4]))
    for i in range(n):
        j = (i + 1) % n
        h[i, j] = h[j, i] = off * (1 + i % 3)
    return h


def _spectra(n):
    return {
        "cluster at the bottom": lambda: _rotated([1e-3] * 4 + [0.5] * 3 + list(np.linspace(1, 8, n - 7)), 10 + n),
        "all repeated": lambda: _rotated([3.0] * (n - 1) + [3.0 + 1e-9], 20 + n),
        "graded 1e-8 .. 1e4": lambda: _rotated(np.logspace(-8, 4, n), 30 + n),
        "one negative": lambda: _rotated(np.concatenate([[-1e2], np.logspace(-2, 4, n - 1)]), 40 + n),
        "near diagonal, 1e-299": lambda: _near_diagonal(n, 1e-299),
        "near diagonal, below the skip": lambda: _near_diagonal(n, 5e-301),
    }


@pytest.mark.parametrize("n", [17, 24, 32])
@pytest.mark.parametrize("name", sorted(_spectra(17)))
def test_jacobi_sweep_matches_mpmath_at_wide_orders(n, name):
    """sco_ref.min_eig_jacobi (the device's 12 cyclic sweeps, in the per-thread and the wavefront form alike) finds the smallest
    eigenvalue of designed spectra at orders 17, 24 and 32 to 1e-12 max |lambda|."""
    h = _spectra(n)[name]()
    assert h.shape == (n, n) and np.array_equal(h, h.T)
    mp.dps = 50
    eigs = [mpmath.mpf(v) for v in mpmath.eigsy(mpmath.matrix(h.tolist()), eigvals_only=True)]
    lam, norm = min(eigs), max(abs(e) for e in eigs)
    assert abs(mpmath.mpf(sr.min_eig_jacobi(h)) - lam) <= 1e-12 * norm, (n, name, sr.min_eig_jacobi(h), lam)


def _smooth_mp(x, p, d, span):
    if span == 3:
        ax, ay = x[0] - 2 * x[d] + x[2 * d], x[1] - 2 * x[d + 1] + x[2 * d + 1]
        g = (x[d], x[d + 1])
    else:
        ax = x[3 * d] - 3 * x[2 * d] + 3 * x[d] - x[0]
        ay = x[3 * d + 1] - 3 * x[2 * d + 1] + 3 * x[d + 1] - x[1]
        g = (x[2 * d], x[2 * d + 1])
    return p[8] * mpmath.sqrt(1 + p[9] * (ax ** 2 + ay ** 2)) - \
        p[10] * mpmath.exp(-((g[0] - p[11]) ** 2 + (g[1] - p[12]) ** 2) / mpmath.mpf("0.08"))


@pytest.mark.parametrize("kind,d,span", [("smooth3", 8, 3), ("smooth4", 8, 4)])
def test_fd_hessian_matches_mpmath_on_wide_terms(kind, d, span):
    """sco_ref.fd_hessian (the device's ladder) against the exact Hessian of the smooth3 (24 numbers) and smooth4 (32) terms,
    to 2e-9 max(1, |H|) as at 16 numbers."""
    pr = wl.make_block_obj_problem(1, kind, d=d, T=6, wide=True)
    par = pr["row_params"]
    f = pr["row_program"].block_objective_fn(par)
    n = span * d
    x = pr["x0"][:n].copy()
    mp.dps = 50
    pm = [mpmath.mpf(float(v)) for v in par]
    assert abs(f(x) - float(_smooth_mp([mpmath.mpf(float(v)) for v in x], pm, d, span))) <= 1e-14 * max(1.0, abs(f(x)))
    xm = [mpmath.mpf(float(v)) for v in x]
    exact = np.zeros((n, n))
    # the terms read x, y of the points only: the other entries are exactly zero
    live = [k for k in range(n) if k % d < 2]
    for a, i in enumerate(live):
        for j in live[a:]:
            order = [0] * n
            order[i] += 1; order[j] += 1
            exact[i, j] = exact[j, i] = float(mpmath.diff(lambda *v: _smooth_mp(list(v), pm, d, span), xm, tuple(order)))
    fd = sr.fd_hessian(f, x)
    assert np.abs(fd - exact).max() <= 2e-9 * max(1.0, np.abs(exact).max()), np.abs(fd - exact).max()


def test_compile_rows_wide_keyword_and_limits():
    term = X(0) ** 2
    for span, dof in ((2, 16), (3, 10), (4, 8)):
        prog = compile_rows([X(0)], block_objective=term, span=span, dof=dof, wide=True)
        assert prog.wide and prog.block_objective
        with pytest.raises(ValueError):
            compile_rows([X(0)], block_objective=term, span=span, dof=dof)          # without wide= the 16-number limit holds
    assert compile_rows([X(0)], block_objective=X(31), span=2, wide=True).wide       # the term's own state: 32 numbers
    with pytest.raises(ValueError):
        compile_rows([X(0)], block_objective=X(32), span=2, wide=True)               # 33
    with pytest.raises(ValueError):
        compile_rows([X(0)], block_objective=term, span=4, dof=9, wide=True)         # 36
    prog = compile_rows([X(0)], objective=X(0) ** 2, dof=32, wide=True)
    assert prog.wide and prog.objective
    with pytest.raises(ValueError):
        compile_rows([X(0)], objective=X(0) ** 2, dof=33, wide=True)
    with pytest.raises(ValueError):
        compile_rows([X(0)], wide=True)                                                # wide needs a term
    assert not compile_rows([X(0)], block_objective=term, span=2).wide
    assert rx.OBJ_DMAX == 16 and rx.OBJ_WIDE_DMAX == 32


def test_workloads_keep_their_programs_and_problems():
    """wide= changes the flag of a program, not its words; the seeded problems are those without it."""
    for kind, d in (("effort", 3), ("ee-path", 7), ("smooth3", 2), ("smooth4", 2)):
        a, b = wl.block_obj_program(kind, d), wl.block_obj_program(kind, d, wide=True)
        assert a is not b and not a.wide and b.wide
        assert np.array_equal(a.words, b.words) and np.array_equal(a.consts, b.consts) and np.array_equal(a.row_ptr, b.row_ptr)
        p, q = wl.make_block_obj_problem(0, kind), wl.make_block_obj_problem(0, kind, wide=True)
        for k in ("x0", "start", "goal", "row_params"):
            assert np.array_equal(p[k], q[k])
    for kind, d in (("ee-path", 16), ("smooth3", 10), ("smooth4", 8)):
        assert wl.block_obj_program(kind, d, wide=True).wide
    with pytest.raises(ValueError):
        wl.block_obj_program("ee-path", 9)
    with pytest.raises(ValueError):
        wl.block_obj_program("smooth4", 9, wide=True)
    pr = wl.make_block_obj_problem(0, "attract", wide=True)
    ref = wl.make_problem(0, program=True, variant="attract", d=20, T=12)
    assert pr["row_program"].wide and pr["row_program"].objective and np.array_equal(pr["x0"], ref["x0"])
    assert np.array_equal(pr["row_program"].words, wl.variant_program("attract", 20).words)


def _refused(prob, reason):
    assert cc.compile_prob(prob) is None
    assert cc._reason[0] == reason, cc._reason[0]


def test_compile_prob_accepts_wide_terms_and_refuses_beyond_32():
    mods = ct.mirror_mods()
    pr = wl.make_block_obj_problem(2, "smooth4", d=8, T=6, wide=True)
    prob, _, _, _ = bb.build_prob(mods, pr, device_exprs=True)
    cp = cc.compile_prob(prob)
    assert cp is not None, cc._reason[0]
    assert cp.key[4] == ("program", id(pr["row_program"]), False, 0, "block_obj", "wide")
    # rows on one coordinate, the term on one number, blocks of 32 (dof 8) and 36 (dof 9) numbers: without the flag today's
    # reason, with it accepted up to 32 and a reason of its own beyond
    for dof, wide, reason in ((8, False, "block objective terms on more than 16 numbers (span * dof)"), (8, True, None),
                              (9, True, "wide block objective terms on more than 32 numbers (span * dof)")):
        big = dict(wl.make_problem(0, program=True, variant="jerk", d=dof, T=6))
        big["row_program"] = compile_rows([X(0) - 5.0], block_objective=X(0) ** 2, span=4, wide=wide)
        big["row_params"] = np.zeros(0); big["O"] = 1; big["obstacles"] = np.zeros((1, 3))
        prob, _, _, _ = bb.build_prob(mods, big, device_exprs=True)
        if reason is None:
            assert cc.compile_prob(prob) is not None, cc._reason[0]
        else:
            _refused(prob, reason)
    # the span-1 term of a timestep at dof 20
    pa = wl.make_block_obj_problem(0, "attract", T=6, wide=True)
    import trajopt_build as tb
    prob, _, _, _ = tb.build_prob(mods, pa, device_exprs=True)
    cp = cc.compile_prob(prob)
    assert cp is not None and cp.key[4][-1] == "wide", cc._reason[0]


def _flat(pr, analytic_jac=False):
    return bb.flat(pr, analytic_jac=analytic_jac) if pr["row_program"].block_objective else sr.trajopt_flat(pr, analytic_jac=analytic_jac)


@pytest.mark.parametrize("case", range(len(GOLDEN32)))
def test_flat_oracle_reproduces_wide_golden_runs(case):
    prefix, kw, i, aj = GOLDEN32[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj32.npz"))
    ref = sr.penalty_sqp(_flat(af.make_problem(i, **kw), analytic_jac=aj), None, emulate_memo=True)
    n = int(g[prefix + "n_qp"])
    assert ref.qp_solves == n and [int(v) for v in ref.trace[:, 6]] == [int(g["%sqp%d_status" % (prefix, k)]) for k in range(n)]
    assert ref.success == bool(g[prefix + "success"])
    assert np.abs(ref.x - g[prefix + "x"]).max() < 1e-7
    bb.check_merit_log(g[prefix + "merit_log"], ref.trace, tol=1e-6)


@pytest.mark.parametrize("case", range(len(GOLDEN32)))
def test_mirror_host_loop_reproduces_wide_golden_qps(case, oracle_qp_backend):
    import trajopt_build as tb
    prefix, kw, i, aj = GOLDEN32[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj32.npz"))
    pr = af.make_problem(i, **kw)
    mods = ct.mirror_mods()
    build = bb.build_prob if pr["row_program"].block_objective else tb.build_prob
    prob, traj, _, _ = build(mods, pr, analytic_jac=aj)
    solver = mods.Solver()
    solver.device_loop = False
    ok = solver.solve(prob, method="penalty_sqp")
    gold = ct.load_golden_qps(g, prefix, sparse=True)
    assert len(gold) == len(oracle_qp_backend) and ok == bool(g[prefix + "success"])
    n_x = pr["d"] * pr["T"]
    for k, (a, rec) in enumerate(zip(gold, oracle_qp_backend)):
        _, _, Ae, le, ue = ct.expand_weighted_qp(rec)
        P2, q2, A2, l2, u2, perm = tb.canonical_qp(rec["P"], rec["q"], Ae, le, ue, n_x)
        ct.assert_qp_close(a, P2, q2, A2, l2, u2, ("mirror", prefix, k), tol=1e-7)
        assert a["status"] == rec["status"]
    assert np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < 1e-7


def _plan_info(pr, which):
    out = sr.penalty_sqp(_flat(pr), sr.SolverParams(max_qp_solves=2), record_qps=True)
    q = out.qps[1]
    Pm = sp.triu(sp.csc_matrix(q["P"] != 0), format="csc"); A = sp.csc_matrix(q["A"] != 0)
    Pm.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    sizes = np.zeros(16, dtype=np.int32); info = np.zeros(10, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    fn = getattr(lib, "sco_debug_%s_plan" % which)
    fn.argtypes = [C.POINTER(C.c_int)]
    assert lib.sco_debug_plan_build(len(q["q"]), len(q["l"]), ip(Pm.indptr), ip(Pm.indices), ip(A.indptr), ip(A.indices), 1, ip(sizes)) == 0
    assert fn(ip(info)) == 0
    return info


@pytest.mark.parametrize("case", range(len(GOLDEN32)))
def test_wide_band_plans(case):
    """Host plans of the penalty QP with a band 24 to 32 numbers wide (and the dof-20 diagonal blocks of "attract"): never the
    wavefront tier, always the row-local tier at column width 12 (so every shape of the goldens runs on the device)."""
    _, kw, i, _ = GOLDEN32[case]
    pr = af.make_problem(i, **kw)
    assert _plan_info(pr, "wv")[0] == 0
    rl = _plan_info(pr, "rl")
    assert rl[0] == 1 and rl[1] == 12, rl.tolist()
