"""Wide objective terms (SCO_FAM_FLAG_OBJ_WIDE) on the device: the wavefront-cooperative eigenvalue sweep in LDS and the
lane-parallel model on terms of 17 to 32 numbers, against the reference's runs (tests/golden/make_golden_blockobj32.py) and the
flat oracle; the terms of 16 numbers or fewer with and without the flag; the refusals of sco_sqp_create."""
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
from blockobj32_cases import CASES as GOLDEN32        # noqa: E402
from blockobj_cases import CASES as GOLDEN            # noqa: E402
from blockobj4_cases import CASES as GOLDEN4          # noqa: E402


def _check(res, b, ref):
    tr, rt = res.trace[b], ref.trace[:64]
    assert tr.shape == rt.shape and np.array_equal(tr[:, 0], rt[:, 0]), (b, tr[:, 0], rt[:, 0])
    assert np.array_equal(tr[:, 6], rt[:, 6]), b
    assert np.abs(tr[:, 1:4] - rt[:, 1:4]).max() < 1e-6 * (1 + np.abs(rt[:, 1:4]).max()), b
    assert np.abs(res.x[b] - ref.x).max() < TOL, (b, np.abs(res.x[b] - ref.x).max())
    assert bool(res.success[b]) == ref.success


@pytest.mark.parametrize("case", range(len(GOLDEN32)))
def test_wide_golden_runs_through_the_batch_and_the_object_api(gpu, case):
    import trajopt_build as tb
    prefix, kw, i, aj = GOLDEN32[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj32.npz"))
    n = int(g[prefix + "n_qp"])
    status = [int(g["%sqp%d_status" % (prefix, k)]) for k in range(n)]
    arrays, probs = wl.make_batch(1, first=i, **kw)
    assert arrays["row_program"].wide
    res = sb.solve_batch(arrays, analytic_jac=aj)
    assert res.qp_solves[0] == n and [int(v) for v in res.trace[0][:, 6]] == status
    assert bool(res.success[0]) == bool(g[prefix + "success"])
    assert np.abs(res.x[0] - g[prefix + "x"]).max() < TOL
    bb.check_merit_log(g[prefix + "merit_log"], res.trace[0], tol=1e-6)
    mods = ct.mirror_mods()
    build = bb.build_prob if probs[0]["row_program"].block_objective else tb.build_prob
    prob, traj, _, _ = build(mods, probs[0], analytic_jac=aj, device_exprs=True)
    solver = mods.Solver()
    ok = solver.solve(prob, method="penalty_sqp")
    assert solver.last_path == "device" and solver.last_device["rounds"] > 0
    exprs = [be.expr.expr for be in prob._nonlin_cnt_exprs] + [be.expr for be in prob._nonquad_obj_exprs]
    assert sum(e.host_evals for e in exprs) == 0
    assert ok == bool(g[prefix + "success"]) and np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < TOL
    assert [int(v) for v in solver.last_device["traces"][0][:, 6]] == status


def _quadratic_problem(lam, seed, variant, d, T):
    """Rows of `variant` at dof d with the block term f = 1/2 sum_k lam_k (u_k . (x - c))^2, u orthonormal: its Hessian is
    Q diag(lam) Q'."""
    n = len(lam)
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((n, n)))
    arrays, (pr,) = wl.make_batch(1, first=seed, program=True, variant=variant, d=d, T=T)
    c = pr["x0"][:n] + 0.05 * rng.standard_normal(n)
    term = None
    for k in range(n):
        s = None
        for i in range(n):
            e = float(u[i, k]) * (X(i) - float(c[i]))
            s = e if s is None else s + e
        e = (0.5 * float(lam[k])) * s ** 2
        term = e if term is None else term + e
    v = wl.variant_rows(variant, d)
    pr["row_program"] = arrays["row_program"] = compile_rows(v["rows"], eq_rows=v["eq_rows"], span=v["span"], block_objective=term,
                                                             dof=d, wide=True)
    lam = np.asarray(lam, dtype=np.float64)
    f = lambda x: 0.5 * float(np.sum(lam * (u.T @ (np.asarray(x) - c)) ** 2))
    fp = sr.trajopt_flat(pr)
    S = v["span"]
    for t in range(T - S + 1):
        fp.obj_blocks.append(sr.ObjBlock(f, np.arange(t * d, (t + S) * d)))
    return arrays, sr.penalty_sqp(fp, None, emulate_memo=True)


SPECTRA = {
    "one negative": lambda n: np.concatenate([[-0.1], np.linspace(0.5, 10.0, n - 1)]),
    "four equal at the bottom": lambda n: np.concatenate([[0.02] * 4, np.linspace(0.5, 10.0, n - 4)]),
    "graded 1e-6 .. 1e4": lambda n: np.logspace(-6, 4, n),
}


@pytest.mark.parametrize("variant,d", [("accel", 8), ("jerk", 8)])
@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_designed_wide_spectra_follow_the_oracle(gpu, variant, d, name):
    """Quadratic block terms on 24 (span 3 x dof 8) and 32 (span 4 x dof 8) numbers with designed spectra: the wavefront
    sweep against the oracle's eigvalsh.  Decisions identical, x to 1e-6."""
    n = (3 if variant == "accel" else 4) * d
    arrays, ref = _quadratic_problem(SPECTRA[name](n), 3 + sorted(SPECTRA).index(name), variant, d, 6)
    res = sb.solve_batch(arrays)
    assert res.qp_solves[0] > 1
    _check(res, 0, ref)


def _narrow_cases():
    out = []
    for gname, cases in (("blockobj", GOLDEN), ("blockobj4", GOLDEN4)):
        out += [(gname, c) for c in cases]
    return out


@pytest.mark.parametrize("case", range(len(_narrow_cases())))
def test_terms_of_16_numbers_give_the_same_bits_with_the_flag(gpu, case):
    """The goldens of 16 numbers or fewer, once without and once with SCO_FAM_FLAG_OBJ_WIDE: the wavefront sweep does the
    per-thread sweep's operations in its order, so x, the traces and the ADMM iteration counts agree bit for bit."""
    _, (prefix, kw, i, aj) = _narrow_cases()[case]
    a, _ = wl.make_batch(1, first=i, **kw)
    b, _ = wl.make_batch(1, first=i, wide=True, **kw)
    assert not a["row_program"].wide and b["row_program"].wide
    ra, rb = sb.solve_batch(a, analytic_jac=aj), sb.solve_batch(b, analytic_jac=aj)
    assert np.array_equal(ra.x, rb.x), np.abs(ra.x - rb.x).max()
    assert np.array_equal(ra.trace[0], rb.trace[0]) and np.array_equal(ra.admm_iters, rb.admm_iters)
    assert np.array_equal(ra.success, rb.success) and np.array_equal(ra.qp_solves, rb.qp_solves)


ROUTES = [("default", {}), ("register", dict(SCO_QP_NO_RL="1")),
          ("generic", dict(SCO_QP_NO_RL="1", SCO_QP_NO_REG="1", SCO_QP_NO_FAST="1")),
          ("structured", dict(SCO_QP_FORCE_BIG="1", SCO_QP_NO_BT="0")), ("big generic", dict(SCO_QP_FORCE_BIG="1", SCO_QP_NO_BT="1"))]


def test_every_admm_route_solves_the_wide_band(gpu, monkeypatch):
    """smooth3 at dof 8 (24-number blocks), four problems, once per ADMM route: the same statuses and ADMM iteration counts
    everywhere, x within 1e-6 of the oracle; the default route is not the wavefront tier."""
    arrays, probs = wl.make_batch(4, first=40, block_obj="smooth3", d=8, T=6, wide=True)
    refs = [sr.penalty_sqp(bb.flat(pr), None, emulate_memo=True) for pr in probs]
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


def test_wide_batch_wider_than_the_cu_count(gpu):
    """300 ee-path problems at dof 12 (24-number blocks): compact rounds, four of them against the oracle."""
    arrays, probs = wl.make_batch(300, block_obj="ee-path", d=12, T=4, wide=True)
    res = sb.solve_batch(arrays)
    assert np.all(res.qp_solves >= 1) and np.all(np.isfinite(res.x))
    for b in (0, 101, 202, 299):
        _check(res, b, sr.penalty_sqp(bb.flat(probs[b]), None, emulate_memo=True))


def test_longest_horizon_at_32_numbers(gpu):
    """Horizon 256 with 32-number terms fits no ADMM tier -- neither the span-4 band of smooth4 at dof 8 nor the dof-32
    diagonal blocks of a per-timestep term (a core of 2048 / 8192 variables; the global-memory tier takes 1024): sco_sqp_create
    refuses both with SCO_ERR_CAPACITY and a message, 257 stays SCO_ERR_ARG.  A 32-number per-timestep term at horizon 24
    (768 variables) is solved, and the run repeats bit for bit."""
    lib = _lib.load()
    P, OB, OP, W = sb.SCO_FAM_STATE_PROGRAM, sb.SCO_FAM_FLAG_OBJ_BLOCK, sb.SCO_FAM_FLAG_OBJ_PROGRAM, sb.SCO_FAM_FLAG_OBJ_WIDE
    for dof, span, fam in ((8, 4, P | OB | W), (32, 1, P | OP | W)):
        for T, want in ((256, -5), (257, -1)):
            h = C.c_void_p()
            desc = _lib.TrajoptDesc(1, dof, T, 1, 3, fam, 0, 2, span, 0)
            assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == want, (dof, T)
            if want == -5:
                assert b"pattern not supported" in lib.sco_last_error()
    arrays, _ = wl.make_batch(1, block_obj="attract", d=32, T=24, wide=True)
    assert arrays["row_program"].wide and arrays["d"] == 32
    res = sb.solve_batch(arrays)
    again = sb.solve_batch(arrays)
    assert res.qp_solves[0] > 1 and np.all(np.isfinite(res.x))
    assert np.array_equal(res.x, again.x) and np.array_equal(res.trace[0], again.trace[0])


def test_wide_refusals(gpu):
    lib = _lib.load()
    P, OB, OP, W = sb.SCO_FAM_STATE_PROGRAM, sb.SCO_FAM_FLAG_OBJ_BLOCK, sb.SCO_FAM_FLAG_OBJ_PROGRAM, sb.SCO_FAM_FLAG_OBJ_WIDE
    for fam, dof, span in ((P | W, 3, 2), (P | W, 3, 1), (P | OB | OP | W, 3, 2), (P | OB | W | sb.SCO_FAM_FLAG_EE_COST, 3, 2),
                           (sb.SCO_FAM_ARM_CIRCLES | W, 3, 1), (sb.SCO_FAM_STATE_QUADRATIC | OP | W, 3, 1),
                           (P | OB | W, 9, 4), (P | OB | W, 17, 2), (P | OP | W, 33, 1),
                           (P | OB, 9, 2), (P | OP, 17, 1)):                    # without the flag: the limits of today
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 2, fam, 0, 2, span, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == -1, (fam, dof, span)      # SCO_ERR_ARG
    for fam, dof, span in ((P | OB | W, 16, 2), (P | OB | W, 10, 3), (P | OB | W, 8, 4), (P | OP | W, 32, 1), (P | OB | W, 3, 2)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 2, fam, 0, 2, span, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == 0, (fam, dof, span)
        assert lib.sco_sqp_destroy(h) == 0
    # the term's operands address the block's state: an X index >= span * dof is refused at load time
    arrays, _ = wl.make_batch(1, block_obj="ee-path", d=12, T=4, wide=True)
    bad = compile_rows([X(0) - 5.0, X(1) - 5.0], block_objective=X(24), span=2, wide=True)
    ok = compile_rows([X(0) - 5.0, X(1) - 5.0], block_objective=X(23), span=2, wide=True)
    with sb.TrajOptBatch(1, 12, 4, 1, 2, program=ok) as tbh:
        tbh.load(arrays["x0"], arrays["start"], arrays["goal"], arrays["link_len"], arrays["point_link"],
                 arrays["point_frac"], np.zeros((1, 2, 3)), row_program=ok)
        for prog, want in ((bad, -1), (ok, 0)):
            words = np.ascontiguousarray(prog.words.ravel())
            rc = lib.sco_sqp_load_program(tbh._h, len(prog.words), _lib.iptr(words), _lib.iptr(prog.row_ptr), len(prog.consts),
                                          _lib.dptr(prog.consts), 0, None)
            assert rc == want, (prog.n_state, rc)
