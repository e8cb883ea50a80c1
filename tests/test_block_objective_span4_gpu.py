"""Block objective terms (SCO_FAM_FLAG_OBJ_BLOCK) on the device at span 4 and on 16-number block states: the band lowering
where four blocks cover an entry, the eigenvalue shift on designed 16 x 16 spectra, every ADMM tier on the span-4 band,
program rows on 32-number states, the longest horizon and a batch wider than the CU count -- against the reference's runs
(tests/golden/make_golden_blockobj4.py) and the flat oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import blockobj_build as bb
import conftest as ct
from oracle import sco_ref as sr
from sco_py_amd import _lib, batch as sb, workloads as wl
from sco_py_amd.rowexpr import X, compile_rows

pytestmark = pytest.mark.gpu
TOL = 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from blockobj4_cases import CASES as GOLDEN4        # noqa: E402


def _check(res, b, ref):
    """Decisions, QP statuses, merits, x and success of problem b against an oracle run."""
    tr, rt = res.trace[b], ref.trace[:64]
    assert tr.shape == rt.shape and np.array_equal(tr[:, 0], rt[:, 0]), (b, tr[:, 0], rt[:, 0])
    assert np.array_equal(tr[:, 6], rt[:, 6]), b
    assert np.abs(tr[:, 1:4] - rt[:, 1:4]).max() < 1e-6 * (1 + np.abs(rt[:, 1:4]).max()), b
    assert np.abs(res.x[b] - ref.x).max() < TOL, (b, np.abs(res.x[b] - ref.x).max())
    assert bool(res.success[b]) == ref.success


def _smooth4_numpy(p, d):
    """The smooth4 term of workloads.block_obj_program("smooth4", d) in NumPy (the same function up to rounding)."""
    def f(x):
        jx = x[3 * d] - 3.0 * x[2 * d] + 3.0 * x[d] - x[0]
        jy = x[3 * d + 1] - 3.0 * x[2 * d + 1] + 3.0 * x[d + 1] - x[1]
        return p[8] * np.sqrt(1.0 + p[9] * (jx * jx + jy * jy)) - \
            p[10] * np.exp(-((x[2 * d] - p[11]) ** 2 + (x[2 * d + 1] - p[12]) ** 2) / 0.08)
    return f


def _flat(pr, term):
    """bb.flat with the block terms given as NumPy functions, term(params of block t): the oracle's numeric Hessians of
    16-number blocks stay affordable (the program evaluator in Python is the slow part of the oracle here)."""
    fp = sr.trajopt_flat(pr)
    d, S = pr["d"], pr["row_program"].span
    for t in range(pr["T"] - S + 1):
        par = pr["row_params"][t] if np.ndim(pr["row_params"]) == 2 else pr["row_params"]
        fp.obj_blocks.append(sr.ObjBlock(term(par), np.arange(t * d, (t + S) * d)))
    return sr.penalty_sqp(fp, None, emulate_memo=True)


@pytest.mark.parametrize("case", range(len(GOLDEN4)))
def test_span4_golden_runs_through_the_batch_and_the_object_api(gpu, case):
    """The reference's runs at span 4 (dof 2 and 4, weights, limits with groups, the analytic row Jacobian) and ee-path at
    dof 8: through TrajOptBatch and plain Solver().solve(prob) -- x to 1e-6, success, every QP's status, the merit log."""
    prefix, kw, i, aj = GOLDEN4[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj4.npz"))
    n = int(g[prefix + "n_qp"])
    status = [int(g["%sqp%d_status" % (prefix, k)]) for k in range(n)]
    arrays, probs = wl.make_batch(1, first=i, **kw)
    res = sb.solve_batch(arrays, analytic_jac=aj)
    assert res.qp_solves[0] == n and [int(v) for v in res.trace[0][:, 6]] == status
    assert bool(res.success[0]) == bool(g[prefix + "success"])
    assert np.abs(res.x[0] - g[prefix + "x"]).max() < TOL
    bb.check_merit_log(g[prefix + "merit_log"], res.trace[0], tol=1e-6)
    mods = ct.mirror_mods()
    prob, traj, _, _ = bb.build_prob(mods, probs[0], analytic_jac=aj, device_exprs=True)
    solver = mods.Solver()
    ok = solver.solve(prob, method="penalty_sqp")
    assert solver.last_path == "device" and solver.last_device["rounds"] > 0
    assert ok == bool(g[prefix + "success"]) and np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < TOL
    assert [int(v) for v in solver.last_device["traces"][0][:, 6]] == status


def _quadratic_problem(lam, seed, d=4, T=6):
    """The jerk rows at dof 4 (span 4: 16 numbers per block) with the block term f = 1/2 sum_k lam_k (u_k . (x - c))^2, u
    orthonormal: its Hessian is Q diag(lam) Q', which the ladder of second differences reproduces up to rounding."""
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((16, 16)))
    arrays, (pr,) = wl.make_batch(1, first=seed, program=True, variant="jerk", d=d, T=T)
    c = pr["x0"][:16] + 0.05 * rng.standard_normal(16)
    term = None
    for k in range(16):
        s = None
        for i in range(16):
            e = float(u[i, k]) * (X(i) - float(c[i]))
            s = e if s is None else s + e
        e = (0.5 * float(lam[k])) * s ** 2
        term = e if term is None else term + e
    v = wl.variant_rows("jerk", d)
    pr["row_program"] = arrays["row_program"] = compile_rows(v["rows"], eq_rows=v["eq_rows"], span=4, block_objective=term, dof=d)
    lam = np.asarray(lam, dtype=np.float64)
    return arrays, pr, lambda par: (lambda x: 0.5 * float(np.sum(lam * (u.T @ (np.asarray(x) - c)) ** 2)))


SPECTRA = {
    "one negative": np.concatenate([[-1e-2 * 10.0], np.linspace(0.5, 10.0, 15)]),
    "four equal at the bottom": np.concatenate([[0.02] * 4, np.linspace(0.5, 10.0, 12)]),
    "graded 1e-6 .. 1e4": np.logspace(-6, 4, 16),
    "singular, positive semi-definite": np.concatenate([[0.0] * 3, np.linspace(0.1, 5.0, 13)]),
}


@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_designed_spectra_follow_the_oracle(gpu, name):
    """A quadratic block term on 16 numbers with a designed spectrum: only the eigenvalue shift (the device's 12 Jacobi sweeps
    against the reference's eigvalsh) and the band assembly are under test.  Decisions identical, x to 1e-6."""
    arrays, pr, term = _quadratic_problem(SPECTRA[name], 3 + sorted(SPECTRA).index(name))
    f = pr["row_program"].block_objective_fn(pr["row_params"])
    x = pr["x0"][:16] + 0.1
    assert abs(f(x) - term(None)(x)) <= 1e-13 * max(1.0, abs(f(x)))
    h = sr.fd_hessian(f, x)
    assert np.allclose(np.linalg.eigvalsh(h), np.sort(SPECTRA[name]), rtol=0, atol=1e-7 * np.abs(SPECTRA[name]).max())
    res = sb.solve_batch(arrays)
    assert res.qp_solves[0] > 1
    _check(res, 0, _flat(pr, term))


ROUTES = [("default", {}), ("register", dict(SCO_QP_NO_RL="1")),
          ("generic", dict(SCO_QP_NO_RL="1", SCO_QP_NO_REG="1", SCO_QP_NO_FAST="1")),
          ("structured", dict(SCO_QP_FORCE_BIG="1", SCO_QP_NO_BT="0")), ("big generic", dict(SCO_QP_FORCE_BIG="1", SCO_QP_NO_BT="1"))]


def test_every_admm_tier_solves_the_span4_band(gpu, monkeypatch):
    """The span-4 batch at dof 4 (16-number blocks) once per reachable ADMM route: the same statuses and ADMM iteration
    counts everywhere, x within 1e-6 of the oracle.  The default route is not the wavefront tier (the host plan puts the band
    on the row-local tier, tests/test_block_objective_span4.py)."""
    arrays, probs = wl.make_batch(4, first=40, block_obj="smooth4", d=4, T=7)
    refs = [_flat(pr, lambda p: _smooth4_numpy(p, 4)) for pr in probs]
    outs = []
    for name, env in ROUTES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res = sb.solve_batch(arrays)
        for k in env:
            monkeypatch.delenv(k)
        if name == "default":
            assert res.timing["wv_launches"] == 0 and res.timing["other_launches"] > 0
        for b in range(4):
            _check(res, b, refs[b])
        outs.append((name, res))
    base = outs[0][1]
    for name, res in outs[1:]:
        assert np.array_equal(res.qp_solves, base.qp_solves), name
        assert all(np.array_equal(res.trace[b][:, 6], base.trace[b][:, 6]) for b in range(4)), name
        assert all(np.array_equal(res.trace[b][:, 7], base.trace[b][:, 7]) for b in range(4)), name
        assert np.array_equal(res.admm_iters, base.admm_iters), name


def test_span4_batch_wider_than_the_cu_count(gpu):
    """300 span-4 problems at dof 4 (more than the 256 CUs: compact rounds), four of them against the oracle."""
    arrays, probs = wl.make_batch(300, block_obj="smooth4", d=4, T=6)
    res = sb.solve_batch(arrays)
    assert np.all(res.qp_solves >= 1) and np.all(np.isfinite(res.x))
    for b in (0, 101, 202, 299):
        _check(res, b, _flat(probs[b], lambda p: _smooth4_numpy(p, 4)))


def test_longest_horizon_at_span4(gpu):
    """dof 4, span 4 at the longest horizon sco_sqp_create accepts (256: 253 blocks, 1024 numbers) against the flat oracle."""
    lib = _lib.load()
    for T, want in ((256, 0), (257, -1)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, 4, T, 1, 3, sb.SCO_FAM_STATE_PROGRAM | sb.SCO_FAM_FLAG_OBJ_BLOCK, 0, 2, 4, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == want, T
        if want == 0:
            assert lib.sco_sqp_destroy(h) == 0
    arrays, probs = wl.make_batch(1, block_obj="smooth4", d=4, T=256)
    res = sb.solve_batch(arrays)
    _check(res, 0, _flat(probs[0], lambda p: _smooth4_numpy(p, 4)))


@pytest.mark.parametrize("analytic", [False, True])
def test_jerk_rows_on_32_numbers(gpu, analytic):
    """Program rows at the widest state: "jerk" at dof 8 (span 4 x dof 8 = SCO_STATE_MAX = 32 numbers), numeric and analytic
    row Jacobians, against the flat oracle; dof 8 is accepted at span 4 and dof 9 refused."""
    lib = _lib.load()
    for dof, want in ((8, 0), (9, -1)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 3, sb.SCO_FAM_STATE_PROGRAM, 0, 2, 4, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == want, dof
        if want == 0:
            assert lib.sco_sqp_destroy(h) == 0
    arrays, probs = wl.make_batch(2, first=5, program=True, variant="jerk", d=8, T=7)
    assert arrays["row_program"].span * arrays["d"] == 32
    res = sb.solve_batch(arrays, analytic_jac=analytic)
    assert np.all(res.qp_solves > 1)
    for b in range(2):
        _check(res, b, sr.penalty_sqp(sr.trajopt_flat(probs[b], analytic_jac=analytic), None, emulate_memo=True))


def test_span4_refusals(gpu):
    lib = _lib.load()
    P, OB = sb.SCO_FAM_STATE_PROGRAM, sb.SCO_FAM_FLAG_OBJ_BLOCK
    for fam, dof in ((P | OB, 5), (P | OB | sb.SCO_FAM_FLAG_OBJ_PROGRAM, 4), (P | OB | sb.SCO_FAM_FLAG_OBJ_PROGRAM, 2)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 2, fam, 0, 2, 4, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == -1, (fam, dof)      # SCO_ERR_ARG
