"""Screen the seeds of the spatial-arm parity runs (tests/spatial_cases.py) on the CPU.

For every configuration and each of its first 8 seeds the flat oracle runs twice: forward kinematics in float64, and in
numpy.longdouble rounded to float64.  A seed is kept when both runs take the same decisions (kinds, QP statuses, iteration
counts) and end within 1e-9 of the same trajectory.  Prints the SEEDS table and, per run, the number of QPs and |dx|.

    python scripts/spatial_screen_seeds.py [configuration ...]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import arm_family as af          # noqa: E402
from oracle import sco_ref as sr             # noqa: E402
import spatial_build as sbd                  # noqa: E402
import spatial_cases as sc                   # noqa: E402


def same_run(a, b):
    return a.trace.shape == b.trace.shape and np.array_equal(a.trace[:, 0], b.trace[:, 0]) and \
        np.array_equal(a.trace[:, 6:8], b.trace[:, 6:8]) and float(np.abs(a.x - b.x).max()) < 1e-9


def main():
    names = sys.argv[1:] or list(sc.CONFIGS)
    table = {}
    for name in names:
        kw, params, analytic = sc.CONFIGS[name]
        keep = []
        for i in range(8):
            pr = af.make_problem(i, **kw)
            t0 = time.time()
            runs = [sr.penalty_sqp(sbd.flat_problem(pr, analytic_jac=analytic, dtype=dt), sr.SolverParams(**params))
                    for dt in (np.float64, np.longdouble)]
            ok = same_run(*runs)
            print("%-16s seed %d: %2d QPs, success %d, |dx| %.1e, %s (%.1f s)" % (
                name, i, runs[0].qp_solves, runs[0].success, float(np.abs(runs[0].x - runs[1].x).max()),
                "kept" if ok else "DROPPED", time.time() - t0), flush=True)
            if ok:
                keep.append(i)
        table[name] = keep
    print("SEEDS = {")
    for name, keep in table.items():
        print('    "%s": %r,' % (name, keep))
    print("}")


if __name__ == "__main__":
    main()
