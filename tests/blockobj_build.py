"""Block objective terms (SCO_FAM_FLAG_OBJ_BLOCK) on top of the shared problem builders.

``trajopt_build.build_prob`` and ``oracle.sco_ref.trajopt_flat`` see a block-objective program as a constraint-only program
(``Program.objective`` is False); the helpers below append the terms themselves: one ``Expr`` per constraint block, on that
block's own Variable (prob.py:88-104), or one ``ObjBlock`` per block on the flat oracle."""
import numpy as np

import trajopt_build as tb
from oracle import arm_family as af
from oracle import sco_ref as sr

_base_build = tb.build_prob          # (tests/golden/make_golden_blockobj.py routes tb.build_prob through build_prob below)


def build_prob(mods, pr, analytic_jac=False, device_exprs=False):
    """``trajopt_build.build_prob`` plus the block terms; returns the same tuple."""
    prob, traj, step_vars, atoms = _base_build(mods, pr, analytic_jac=analytic_jac, device_exprs=device_exprs)
    prog = pr["row_program"]
    assert prog.block_objective and len(step_vars) == pr["T"] - prog.span + 1
    for t, sv in enumerate(step_vars):
        par = af.step_params(pr, t)
        if device_exprs:
            from sco_py_amd import devexpr as dx
            e = dx.ProgramBlockObjExpr(prog, par)
        else:
            f = prog.block_objective_fn(par)
            e = mods.Expr(lambda x, f=f: np.array([[f(x.ravel())]]))
        prob.add_obj_expr(mods.BoundExpr(e, sv))
    return prob, traj, step_vars, atoms


def flat(pr, analytic_jac=False):
    """``sco_ref.trajopt_flat`` on the constraint part, then one ObjBlock per constraint block."""
    fp = sr.trajopt_flat(pr, analytic_jac=analytic_jac)
    prog, d = pr["row_program"], pr["d"]
    for t in range(pr["T"] - prog.span + 1):
        fp.obj_blocks.append(sr.ObjBlock(prog.block_objective_fn(af.step_params(pr, t)), np.arange(t * d, (t + prog.span) * d)))
    return fp


def check_merit_log(log, trace, tol=1e-9):
    """The reference's scalar get_value / get_approx_value log (rows: is_approx, vectorize, penalty, value) against a decision
    trace (oracle or device; row 0 = the projection).  Call order (solver.py:130-149): one get_value at every convexification
    point, then per trust-region trial one get_approx_value (model) and one get_value (new point); a convexification follows
    an accepted step and every return of the minimisation (penalty escalation)."""
    exact = log[(log[:, 0] == 0) & (log[:, 1] == 0)][:, 3]
    model = log[(log[:, 0] == 1) & (log[:, 1] == 0)][:, 3]
    tr = trace[1:]
    expected, new_iter = [], True
    for row in tr:
        if new_iter:
            expected.append(row[1])
        expected.append(row[3])
        new_iter = row[0] != sr.STEP_SHRINK
    assert len(model) == len(tr) and np.allclose(model, tr[:, 2], rtol=tol, atol=tol), (model, tr[:, 2])
    assert len(exact) >= len(expected) and np.allclose(exact[:len(expected)], expected, rtol=tol, atol=tol), (exact, expected)
