"""Golden vectors for objective programs per constraint block (SCO_FAM_FLAG_OBJ_BLOCK) at span 4 and on block states of 16
numbers, recorded from the REFERENCE's own modules, with the same stand-ins as make_golden.py:
    python tests/golden/make_golden_blockobj4.py  ->  tests/golden/trajopt_blockobj4.npz
Every block Variable of trajopt_build.build_prob gets one plain ``Expr(f_t)`` with ``add_obj_expr`` (f_t = the program's block
objective term with block t's parameters): the reference convexifies it to degree 2 on the block's span * dof numbers and
lowers the model, off-diagonal blocks included, into P (expr.py:143-153, prob.py:88-104, osqp_utils.py:150-163)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402
import blockobj_build as bb                   # noqa: E402
import trajopt_build as tb                    # noqa: E402
from blockobj4_cases import CASES             # noqa: E402
from oracle import arm_family as af           # noqa: E402


def main():
    mg.install_standins()
    mods = mg.import_reference()
    tb.build_prob = bb.build_prob             # run_trajopt builds through trajopt_build: add the block terms there
    out = {}
    for prefix, kw, i, aj in CASES:
        mg.pack(prefix, mg.run_trajopt(mods, af.make_problem(i, **kw), analytic_jac=aj), out)
    np.savez_compressed(os.path.join(HERE, "trajopt_blockobj4.npz"), **out)
    print("trajopt_blockobj4.npz", os.path.getsize(os.path.join(HERE, "trajopt_blockobj4.npz")), "bytes")


if __name__ == "__main__":
    main()
