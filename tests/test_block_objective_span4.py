"""Block objective terms (SCO_FAM_FLAG_OBJ_BLOCK) at span 4 and on the widest block states (16 numbers), host side: the
eigenvalue sweep and the finite-difference Hessian the device restates, checked against mpmath at 50 digits; compile_prob
on span-4 terms; the flat oracle and the mirror API's host loop against runs of the reference's own modules
(tests/golden/make_golden_blockobj4.py); the ADMM tier plans of the span-4 band.  No GPU here."""
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
from sco_py_amd import _lib, devexpr as dx, workloads as wl
from sco_py_amd.sco_osqp import compile as cc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from blockobj4_cases import CASES as GOLDEN4        # noqa: E402

mp = mpmath.mp


def _rotated(lam, seed):
    """Q diag(lam) Q' for a seeded orthogonal Q of order len(lam), symmetrised after rounding."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(lam), len(lam))))
    h = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return 0.5 * (h + h.T)


def _near_diagonal(off):
    """Distinct (and some equal) diagonal entries, off-diagonals of size `off` on a ring: the sweep's 1e-300 skip and,
    above it, rotations with |theta| far beyond 1e150 (theta^2 would overflow)."""
    h = np.diag(np.concatenate([np.linspace(-1.0, 1.0, 12), [0.25, 0.25, 0.25, 0.25]]))
    for i in range(16):
        j = (i + 1) % 16
        h[i, j] = h[j, i] = off * (1 + i % 3)
    return h


SPECTRA = {
    "cluster of four at the bottom": lambda: _rotated([1e-3] * 4 + [0.5] * 3 + [1.0, 1.0 + 1e-12] + list(np.linspace(2, 8, 7)), 1),
    "all sixteen repeated": lambda: _rotated([3.0] * 15 + [3.0 + 1e-9], 2),
    "graded 1e-8 .. 1e4": lambda: _rotated(np.logspace(-8, 4, 16), 3),
    "graded, shuffled": lambda: _rotated(np.random.default_rng(9).permutation(np.logspace(-8, 4, 16)), 4),
    "one negative": lambda: _rotated(np.concatenate([[-1e2], np.logspace(-2, 4, 15)]), 5),
    "one small negative under large ones": lambda: _rotated(np.concatenate([[-1e-2 * 1e4], np.linspace(1.0, 1e4, 15)]), 6),
    "near diagonal, 1e-299": lambda: _near_diagonal(1e-299),
    "near diagonal, at the 1e-300 skip": lambda: _near_diagonal(1e-300),
    "near diagonal, below the skip": lambda: _near_diagonal(5e-301),
}


def _exact_eigs(h):
    mp.dps = 50
    return [mpmath.mpf(v) for v in mpmath.eigsy(mpmath.matrix(h.tolist()), eigvals_only=True)]


@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_jacobi_sweep_matches_mpmath_at_order_16(name):
    """sco_ref.min_eig_jacobi restates the device sweep op for op (12 cyclic sweeps, no convergence test): at order 16 it
    finds the smallest eigenvalue of the float64 matrix to 1e-12 |H| on clustered, repeated, graded and negative spectra and
    on matrices whose off-diagonals sit at the skip threshold."""
    h = _SPECTRUM_CACHE.setdefault(name, SPECTRA[name]())
    assert h.shape == (16, 16) and np.array_equal(h, h.T)
    eigs = _exact_eigs(h)
    lam, norm = min(eigs), max(abs(e) for e in eigs)
    assert abs(mpmath.mpf(sr.min_eig_jacobi(h)) - lam) <= 1e-12 * norm, (name, sr.min_eig_jacobi(h), lam)
    assert abs(mpmath.mpf(float(np.linalg.eigvalsh(h)[0])) - lam) <= 1e-12 * norm      # what the reference calls


_SPECTRUM_CACHE = {}


def test_twelve_sweeps_are_needed_at_order_16():
    """The spectra above tell a short sweep from the device's: 3 sweeps miss 1e-12 |H| on most of them."""
    missed = []
    for name in sorted(SPECTRA):
        h = _SPECTRUM_CACHE.setdefault(name, SPECTRA[name]())
        eigs = _exact_eigs(h)
        if abs(mpmath.mpf(sr.min_eig_jacobi(h, sweeps=3)) - min(eigs)) > 1e-12 * max(abs(e) for e in eigs):
            missed.append(name)
    assert len(missed) >= 3, missed


def _smooth4_mp(x, p, d):
    """The smooth4 term of workloads.block_obj_program("smooth4", d) in mpmath (parameters from index 8)."""
    jx = x[3 * d] - 3 * x[2 * d] + 3 * x[d] - x[0]
    jy = x[3 * d + 1] - 3 * x[2 * d + 1] + 3 * x[d + 1] - x[1]
    return p[8] * mpmath.sqrt(1 + p[9] * (jx ** 2 + jy ** 2)) - \
        p[10] * mpmath.exp(-((x[2 * d] - p[11]) ** 2 + (x[2 * d + 1] - p[12]) ** 2) / mpmath.mpf("0.08"))


def _ee_path_mp(x, p, d):
    """The ee-path term of workloads.block_obj_program("ee-path", d) in mpmath (parameter index 9)."""
    def ee(off):
        phi, ex, ey = 0, 0, 0
        for k in range(d):
            phi = phi + x[off + k]
            ex, ey = ex + mpmath.cos(phi) / d, ey + mpmath.sin(phi) / d
        return ex, ey
    (ax, ay), (bx, by) = ee(0), ee(d)
    return p[9] * ((bx - ax) ** 2 + (by - ay) ** 2)


def _exact_hessian(f, x):
    mp.dps = 50
    xm = [mpmath.mpf(float(v)) for v in x]
    n = len(xm)
    h = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            order = [0] * n
            order[i] += 1; order[j] += 1
            h[i, j] = h[j, i] = float(mpmath.diff(lambda *a: f(list(a)), xm, tuple(order)))
    return h


@pytest.mark.parametrize("kind,d,scale", [("smooth4", 4, 0.0), ("smooth4", 4, 30.0), ("ee-path", 8, 0.0), ("ee-path", 8, 30.0)])
def test_fd_hessian_matches_mpmath_on_16_numbers(kind, d, scale):
    """sco_ref.fd_hessian (the device's ladder: steps 2^-6 max(1, |x_i|) halved three times, Richardson) against the exact
    Hessian of the smooth4 and ee-path terms on 16 numbers, at the problem's start and at points whose coordinates are about
    30 (steps scale with |x|).  Tolerance 2e-9 max(1, |H|): at |x| <= 1 the floor is rounding, about 16 eps |f| / h^2 with
    h = 2^-9 (observed 1.7e-10); at |x| ~ 30 the finest step is 0.06 and the extrapolated truncation is below 1e-11."""
    pr = wl.make_block_obj_problem(1, kind, d=d, T=6)
    par = pr["row_params"]
    f = pr["row_program"].block_objective_fn(par)
    fm = _smooth4_mp if kind == "smooth4" else _ee_path_mp
    pm = [mpmath.mpf(float(v)) for v in par]
    ds = pr["row_program"].span * d
    assert ds == 16
    x = pr["x0"][:ds].copy()
    if scale:
        rng = np.random.default_rng(11)
        x = x + scale * rng.uniform(0.5, 1.0, size=ds) * rng.choice([-1.0, 1.0], size=ds)
    mp.dps = 50
    assert abs(f(x) - float(fm([mpmath.mpf(float(v)) for v in x], pm, d))) <= 1e-14 * max(1.0, abs(f(x)))
    exact = _exact_hessian(lambda a: fm(a, pm, d), x)
    fd = sr.fd_hessian(f, x)
    assert np.abs(fd - exact).max() <= 2e-9 * max(1.0, np.abs(exact).max()), np.abs(fd - exact).max()


def test_smooth4_program_and_seeded_parameters():
    for d in (2, 3, 4):
        prog = wl.block_obj_program("smooth4", d)
        base = wl.variant_program("jerk", d)
        assert prog.block_objective and prog.span == 4 and prog.n_state == 3 * d + 2      # x, y of the last point
        assert prog.n_rows == base.n_rows and prog.n_params == base.n_params + 5
        pr = wl.make_block_obj_problem(0, "smooth4", d=d, T=6)
        ref = wl.make_problem(0, program=True, variant="jerk", d=d, T=6)
        assert np.array_equal(pr["x0"], ref["x0"]) and np.array_equal(pr["row_params"][:8], ref["row_params"])
        x = np.random.default_rng(d).uniform(-1, 1, 4 * d)
        assert np.array_equal(prog.evaluate(x, pr["row_params"]), base.evaluate(x, ref["row_params"]))
        pm = [mpmath.mpf(float(v)) for v in pr["row_params"]]
        assert abs(prog.block_objective_fn(pr["row_params"])(x) - float(_smooth4_mp(list(map(mpmath.mpf, x)), pm, d))) < 1e-14
    with pytest.raises(ValueError):
        wl.block_obj_program("smooth4", 5)                  # span 4 x dof 5 = 20 numbers
    assert wl.make_problem(3, block_obj="smooth4")["row_program"] is wl.block_obj_program("smooth4", 2)


@pytest.mark.parametrize("kind,d,T", [("smooth4", 2, 8), ("smooth4", 4, 5), ("ee-path", 8, 4)])
def test_compile_prob_accepts_span4_and_16_number_terms(kind, d, T):
    pr = wl.make_block_obj_problem(2, kind, d=d, T=T)
    mods = ct.mirror_mods()
    prob, _, sv, _ = bb.build_prob(mods, pr, device_exprs=True)
    assert len(sv) == T - pr["row_program"].span + 1
    cp = cc.compile_prob(prob)
    assert cp is not None, cc._reason[0]
    assert cp.key[4] == ("program", id(pr["row_program"]), False, 0, "block_obj")
    assert cp.pr["row_program"] is pr["row_program"] and cp.pr["d"] == d and cp.pr["T"] == T
    # the refusal reasons stay what they are at span 4
    del prob._nonquad_obj_exprs[-1]
    assert cc.compile_prob(prob) is None and cc._reason[0] == "block objective terms: one per constraint block"
    prob, _, _, _ = bb.build_prob(mods, pr, device_exprs=True)
    be = prob._nonquad_obj_exprs[0]
    prob._nonquad_obj_exprs[0] = mods.BoundExpr(dx.ProgramBlockObjExpr(pr["row_program"], pr["row_params"] * 1.5), be.var)
    assert cc.compile_prob(prob) is None
    assert cc._reason[0] == "a block objective term has another program than the rows, or other parameters than its block's"


@pytest.mark.parametrize("case", range(len(GOLDEN4)))
def test_flat_oracle_reproduces_span4_golden_runs(case):
    """The flat oracle (four overlapping ObjBlocks per entry at span 4; 16-number blocks) against the reference's runs."""
    prefix, kw, i, aj = GOLDEN4[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj4.npz"))
    ref = sr.penalty_sqp(bb.flat(af.make_problem(i, **kw), analytic_jac=aj), None, emulate_memo=True)
    n = int(g[prefix + "n_qp"])
    assert ref.qp_solves == n and [int(v) for v in ref.trace[:, 6]] == [int(g["%sqp%d_status" % (prefix, k)]) for k in range(n)]
    assert ref.success == bool(g[prefix + "success"])
    assert np.abs(ref.x - g[prefix + "x"]).max() < 1e-7
    bb.check_merit_log(g[prefix + "merit_log"], ref.trace, tol=1e-6)


@pytest.mark.parametrize("case", range(len(GOLDEN4)))
def test_mirror_host_loop_reproduces_span4_golden_qps(case, oracle_qp_backend):
    """The mirror API's host loop builds every QP the reference built at span 4 and on 16-number blocks."""
    import trajopt_build as tb
    prefix, kw, i, aj = GOLDEN4[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj4.npz"))
    pr = af.make_problem(i, **kw)
    mods = ct.mirror_mods()
    prob, traj, _, _ = bb.build_prob(mods, pr, analytic_jac=aj)
    solver = mods.Solver()
    solver.device_loop = False
    ok = solver.solve(prob, method="penalty_sqp")
    gold = ct.load_golden_qps(g, prefix)
    assert len(gold) == len(oracle_qp_backend) and ok == bool(g[prefix + "success"])
    n_x = pr["d"] * pr["T"]
    for k, (a, rec) in enumerate(zip(gold, oracle_qp_backend)):
        _, _, Ae, le, ue = ct.expand_weighted_qp(rec)
        P2, q2, A2, l2, u2, perm = tb.canonical_qp(rec["P"], rec["q"], Ae, le, ue, n_x)
        ct.assert_qp_close(a, P2, q2, A2, l2, u2, ("mirror", prefix, k), tol=1e-7)
        assert a["status"] == rec["status"]
        if k:
            # the band: an entry couples timesteps up to span - 1 apart (three at span 4), and no further
            gap = np.abs(np.subtract.outer(np.arange(n_x) // pr["d"], np.arange(n_x) // pr["d"]))
            w = pr["row_program"].span - 1
            assert not np.any(a["P"][:n_x, :n_x][gap > w]) and np.any(a["P"][:n_x, :n_x][gap == w])
    assert np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < 1e-7


def _plan_info(kind, d, T, which):
    out = sr.penalty_sqp(bb.flat(wl.make_block_obj_problem(0, kind, d=d, T=T)), sr.SolverParams(max_qp_solves=2), record_qps=True)
    q = out.qps[1]
    P = sp.triu(sp.csc_matrix(q["P"] != 0), format="csc"); A = sp.csc_matrix(q["A"] != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); info = np.zeros(10, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    fn = getattr(lib, "sco_debug_%s_plan" % which)
    fn.argtypes = [C.POINTER(C.c_int)]
    assert lib.sco_debug_plan_build(len(q["q"]), len(q["l"]), ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert fn(ip(info)) == 0
    return info


PLAN_SHAPES = [("smooth4", 2, 10), ("smooth4", 4, 5), ("smooth4", 4, 8), ("ee-path", 8, 4)]


@pytest.mark.parametrize("kind,d,T", PLAN_SHAPES)
def test_span4_band_plans(kind, d, T):
    """Host-side plans of the penalty QP with a band three blocks wide (span 4) or 16 numbers wide (ee-path at dof 8): never
    the wavefront tier (its core is block-tridiagonal), always the row-local tier at the default column width 12, as at
    span 2 (profiles/r05_blockobj_speed.txt)."""
    assert _plan_info(kind, d, T, "wv")[0] == 0
    rl = _plan_info(kind, d, T, "rl")
    assert rl[0] == 1 and rl[1] == 12, rl.tolist()
