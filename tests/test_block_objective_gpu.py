"""Objective programs per constraint block (SCO_FAM_FLAG_OBJ_BLOCK) on the device: the degree-2 model of a term over two or
more timesteps (its Hessian fills off-diagonal blocks of P, overlapping blocks add up in block order), the merits on the
block state, through TrajOptBatch, plain Solver().solve(prob) and solve_many -- against the flat oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import blockobj_build as bb
import conftest as ct
from oracle import sco_ref as sr
from sco_py_amd import _lib, batch as sb, workloads as wl
from sco_py_amd.sco_osqp import batching

pytestmark = pytest.mark.gpu
TOL = 1e-6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from blockobj_cases import CASES as GOLDEN        # noqa: E402

CASES = [("effort", dict(T=6)), ("effort", dict(T=6, per_step=True)), ("effort", dict(T=6, obj_weights=True, acc_weights=True)),
         ("effort", dict(T=6, vel_limit=0.6, groups="halves")), ("ee-path", dict(T=5)), ("effort", dict(T=8, analytic=True)),
         ("smooth3", dict(T=8)), ("smooth3", dict(acc_weights=True)), ("smooth3", dict(d=3, T=9, per_step=True, obj_weights=True)),
         ("smooth4", dict(T=8)), ("smooth4", dict(d=4, T=6, acc_weights=True))]       # span 4; 16-number blocks


@pytest.mark.parametrize("case", range(len(GOLDEN)))
def test_golden_runs_through_the_batch_and_the_object_api(gpu, case):
    """Every run of the reference's own modules (tests/golden/make_golden_blockobj.py): span 2 and 3, per-step parameters,
    velocity limits with groups, weights and the acceleration term, the analytic row Jacobian -- through TrajOptBatch and
    through plain Solver().solve(prob): trajectory to 1e-6, success, every QP's status, the merit log."""
    prefix, kw, i, aj = GOLDEN[case]
    g = np.load(os.path.join(GOLD, "trajopt_blockobj.npz"))
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
    exprs = [be.expr.expr for be in prob._nonlin_cnt_exprs] + [be.expr for be in prob._nonquad_obj_exprs]
    assert sum(e.host_evals for e in exprs) == 0
    assert ok == bool(g[prefix + "success"]) and np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < TOL
    assert [int(v) for v in solver.last_device["traces"][0][:, 6]] == status


def _check(res, b, pr, analytic=False):
    """Decisions, QP statuses, merits, x and success of problem b against the flat oracle (ADMM iteration counts are not
    compared where an objective term is in play: numeric Hessians)."""
    ref = sr.penalty_sqp(bb.flat(pr, analytic_jac=analytic), None, emulate_memo=True)
    tr, rt = res.trace[b], ref.trace[:64]
    assert tr.shape == rt.shape and np.array_equal(tr[:, 0], rt[:, 0]), (b, tr[:, 0], rt[:, 0])
    assert np.array_equal(tr[:, 6], rt[:, 6]), b
    assert np.abs(tr[:, 1:4] - rt[:, 1:4]).max() < 1e-6 * (1 + np.abs(rt[:, 1:4]).max()), b
    assert np.abs(res.x[b] - ref.x).max() < TOL, (b, np.abs(res.x[b] - ref.x).max())
    assert bool(res.success[b]) == ref.success
    return ref


@pytest.mark.parametrize("case", range(len(CASES)))
def test_batch_follows_the_flat_oracle(gpu, case):
    kind, kw = CASES[case]
    kw = dict(kw); analytic = kw.pop("analytic", False)
    arrays, probs = wl.make_batch(4, first=10 * case, block_obj=kind, **kw)
    assert arrays["row_program"].span == {"smooth3": 3, "smooth4": 4}.get(kind, 2)
    res = sb.solve_batch(arrays, analytic_jac=analytic)
    assert np.all(res.qp_solves > 1)
    for b in range(4):
        _check(res, b, probs[b], analytic)


def test_object_api_runs_the_resident_loop(gpu):
    """Plain Solver().solve(prob) on a Prob built the reference's way: the device loop ran, Python evaluated nothing, and
    the answer is the batch's."""
    for kind, kw in CASES[:5]:
        pr = wl.make_block_obj_problem(3, kind, **kw)
        mods = ct.mirror_mods()
        prob, traj, _, _ = bb.build_prob(mods, pr, device_exprs=True)
        solver = mods.Solver()
        ok = solver.solve(prob, method="penalty_sqp")
        assert solver.last_path == "device" and solver.last_device["rounds"] > 0
        exprs = [be.expr.expr for be in prob._nonlin_cnt_exprs] + [be.expr for be in prob._nonquad_obj_exprs]
        assert sum(e.host_evals for e in exprs) == 0
        arrays, _ = wl.make_batch(1, first=3, block_obj=kind, **kw)
        res = sb.solve_batch(arrays)
        assert np.array_equal(traj.get_value().ravel(), res.x[0]) and ok == bool(res.success[0])
        assert [int(v) for v in solver.last_device["traces"][0][:, 6]] == [int(v) for v in res.trace[0][:, 6]]


def test_ee_path_7x20_batch(gpu):
    """The 7-DOF x 20 sweep rows with the end-effector step length (ds = 14): a batch of 64, every 8th problem checked."""
    arrays, probs = wl.make_batch(64, block_obj="ee-path")
    res = sb.solve_batch(arrays)
    assert np.all(res.qp_solves >= 1) and np.all(np.isfinite(res.x))
    for b in range(0, 64, 8):
        _check(res, b, probs[b])


def test_effort_batch_above_the_cu_count_and_scheduling(gpu, monkeypatch):
    """256 effort problems, every 16th against the oracle; repeat solves are bit-identical, and time slices and round
    selection change the schedule, not the results."""
    arrays, probs = wl.make_batch(256, block_obj="effort")
    res = sb.solve_batch(arrays)
    for b in range(0, 256, 16):
        _check(res, b, probs[b])
    again = sb.solve_batch(arrays)
    assert np.array_equal(res.x, again.x) and np.array_equal(res.trace[0], again.trace[0])
    for env in (dict(SCO_SQP_SLICE="40"), dict(SCO_SQP_SELECT="0", SCO_SQP_GROUPS="1")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = sb.solve_batch(arrays)
        assert np.array_equal(res.x, other.x) and np.array_equal(res.success, other.success), env
        assert all(np.array_equal(res.trace[b], other.trace[b]) for b in range(256)), env
        for k in env:
            monkeypatch.delenv(k)


def test_solve_many_mixes_block_objective_and_plain_problems(gpu):
    mods = ct.mirror_mods()
    import trajopt_build as tb
    probs, trajs, singles = [], [], []
    for i in range(6):
        if i % 2:
            pr = wl.make_problem(i, program=True, variant="dynamics", d=3, T=6)
            prob, traj, _, _ = tb.build_prob(mods, pr, device_exprs=True)
        else:
            pr = wl.make_block_obj_problem(i, "effort", T=6)
            prob, traj, _, _ = bb.build_prob(mods, pr, device_exprs=True)
        probs.append(prob); trajs.append(traj); singles.append(pr)
    oks, stats = batching.solve_many(probs)
    for i, pr in enumerate(singles):
        arrays, _ = wl.make_batch(1, first=i, block_obj="effort", T=6) if i % 2 == 0 else \
            wl.make_batch(1, first=i, program=True, variant="dynamics", d=3, T=6)
        res = sb.solve_batch(arrays)
        assert np.array_equal(trajs[i].get_value().ravel(), res.x[0]) and oks[i] == bool(res.success[0]), i


def test_descriptor_refusals(gpu):
    lib = _lib.load()
    P, OB = sb.SCO_FAM_STATE_PROGRAM, sb.SCO_FAM_FLAG_OBJ_BLOCK
    for fam, dof, span in ((P | OB, 3, 1), (P | OB, 9, 2), (P | OB, 5, 4), (P | OB | sb.SCO_FAM_FLAG_OBJ_PROGRAM, 3, 2),
                           (P | OB | sb.SCO_FAM_FLAG_EE_COST, 3, 2), (sb.SCO_FAM_ARM_CIRCLES | OB, 3, 2),
                           (sb.SCO_FAM_STATE_QUADRATIC | OB, 3, 2), (sb.SCO_FAM_POINT_CIRCLES | OB, 3, 1)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 2, fam, 0, 2, span, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == -1, (fam, dof, span)      # SCO_ERR_ARG
    # accepted: span 2 .. 4 with span * dof <= 16
    for dof, span in ((3, 2), (8, 2), (4, 4)):
        h = C.c_void_p()
        desc = _lib.TrajoptDesc(1, dof, 8, 1, 2, P | OB, 0, 2, span, 0)
        assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == 0
        assert lib.sco_sqp_destroy(h) == 0
    # the term's operands address the block's state: an X index >= span * dof is refused at load time
    from sco_py_amd.rowexpr import X, compile_rows
    arrays, _ = wl.make_batch(1, block_obj="effort", T=6)
    bad = compile_rows([X(0) - 5.0, X(1) - 5.0], block_objective=X(6), span=2)
    ok = compile_rows([X(0) - 5.0, X(1) - 5.0], block_objective=X(5), span=2)
    with sb.TrajOptBatch(1, 3, 6, 1, 2, program=ok) as tbh:
        tbh.load(arrays["x0"], arrays["start"], arrays["goal"], arrays["link_len"], arrays["point_link"],
                 arrays["point_frac"], np.zeros((1, 2, 3)), row_program=ok)
        for prog, want in ((bad, -1), (ok, 0)):
            words = np.ascontiguousarray(prog.words.ravel())
            rc = lib.sco_sqp_load_program(tbh._h, len(prog.words), _lib.iptr(words), _lib.iptr(prog.row_ptr), len(prog.consts),
                                          _lib.dptr(prog.consts), 0, None)
            assert rc == want
