"""Golden vectors for the spatial-arm family (SCO_FAM_ARM_SPATIAL: per timestep one LEqExpr block on an Expr with
g[k O + o](theta) = r_o + rad_k - ||p_k(theta) - c_o||, three-dimensional forward kinematics; the same lowering as the
planar arm's obstacle rows, prob.py:251-278) recorded from the REFERENCE's own modules, with the same stand-ins as
make_golden.py:
    python tests/golden/make_golden_spatial.py  ->  tests/golden/trajopt_spatial.npz
The problems are built by tests/spatial_build.py (tests/trajopt_build.py does not know the family), the cases are GOLDEN of
tests/spatial_cases.py.  The fixture holds numbers only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402
from oracle import arm_family as af           # noqa: E402
import spatial_build as sbd                   # noqa: E402
import trajopt_build as tb                    # noqa: E402
from spatial_cases import GOLDEN              # noqa: E402


def run_spatial(mods, pr, analytic_jac=False):
    """make_golden.run_trajopt for a problem of tests/spatial_build.py (without the merit-call log)."""
    del mg.QP_LOG[:]
    n_x = pr["d"] * pr["T"]
    mg.CANON_NX[0] = n_x
    prob, traj, _, _ = sbd.build_prob(mods, pr, analytic_jac=analytic_jac)
    ok = mods.Solver().solve(prob, method="penalty_sqp")
    qps = []
    for rec in mg.QP_LOG:
        P2, q2, A2, l2, u2, perm = tb.canonical_qp(rec["P"], rec["q"], rec["A"], rec["l"], rec["u"], n_x)
        qps.append(dict(P=P2, q=q2, A=A2, l=l2, u=u2, x=rec["x"][perm], status=rec["status"], iters=rec["iters"]))
    return dict(success=bool(ok), x=traj.get_value().ravel(), qps=qps, merit_log=np.zeros((0, 4)),
                max_violation=float(prob.get_max_cnt_violation()), nonconverged=sorted(set(prob.nonconverged_groups)))


def main():
    mg.install_standins()
    mods = mg.import_reference()
    out = {}
    for prefix, kw, i, analytic in GOLDEN:
        mg.pack(prefix, run_spatial(mods, af.make_problem(i, **kw), analytic_jac=analytic), out, sparse=True)
    path = os.path.join(HERE, "trajopt_spatial.npz")
    np.savez_compressed(path, **out)
    print("trajopt_spatial.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
