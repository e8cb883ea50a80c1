"""Golden vectors for WIDE objective terms (SCO_FAM_FLAG_OBJ_WIDE: 17 to 32 numbers), recorded from the REFERENCE's own
modules with the same stand-ins as make_golden.py:
    python tests/golden/make_golden_blockobj32.py  ->  tests/golden/trajopt_blockobj32.npz
Block terms go through blockobj_build.build_prob (one plain Expr per block Variable, as make_golden_blockobj.py); the span-1
"attract" term through trajopt_build.build_prob (one plain Expr per timestep Variable).  T stays small: the reference's numeric
Hessian of a 32-number term is 528 pairs of four-point stencils on four levels, in Python."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                      # noqa: E402
import blockobj_build as bb                   # noqa: E402
import trajopt_build as tb                    # noqa: E402
from blockobj32_cases import CASES            # noqa: E402
from oracle import arm_family as af           # noqa: E402


def main():
    mg.install_standins()
    mods = mg.import_reference()
    base = tb.build_prob

    def build(mods_, pr, **kw):
        return (bb.build_prob if pr["row_program"].block_objective else base)(mods_, pr, **kw)
    tb.build_prob = build
    out = {}
    for prefix, kw, i, aj in CASES:
        res = mg.run_trajopt(mods, af.make_problem(i, **kw), analytic_jac=aj)
        print(prefix, "success", res["success"], [(q["status"], q["iters"]) for q in res["qps"]], flush=True)
        mg.pack(prefix, res, out, sparse=True)
    np.savez_compressed(os.path.join(HERE, "trajopt_blockobj32.npz"), **out)
    print("trajopt_blockobj32.npz", os.path.getsize(os.path.join(HERE, "trajopt_blockobj32.npz")), "bytes")


if __name__ == "__main__":
    main()
