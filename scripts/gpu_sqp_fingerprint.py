"""Bit fingerprint of the device SQP loop: B = 8 problems of every family feature set the GPU tests build
(tests/test_sqp_gpu.py::test_round_selection_with_every_family_feature, the block-objective tests: per timestep, per block at
span 2, 3 and 4, wide; plus the point, quadratic, program, circle-row and general-row families), at those tests' small
shapes, each solved once with finite-difference Jacobians and the rounded-point memo on and once with analytic Jacobians
and the memo off.  Prints one SHA-256 per run over the bytes of x, every trace, admm_iters, qp_solves, sqp_iters, success,
merit, max_violation and the flags.  Two builds compute the same numbers exactly when their outputs are identical."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sco_py_amd import _lib, batch as sb, workloads as wl          # noqa: E402

B = 8
ARM = dict(d=3, T=6, K=2, O=2)
SETS = [
    ("arm", dict(**ARM)),
    ("reach+vel+groups", dict(reach=True, vel_limit=0.6, groups="halves", **ARM)),
    ("jl+vel", dict(joint_limit=0.3, vel_limit=0.6, **ARM)),
    ("objective terms", dict(ee_cost_weight=0.5, **ARM)),
    ("acc+weights", dict(acc_weights=True, obj_weights=True, **ARM)),
    ("point", dict(point=True, d=2, T=8, O=3)),
    ("quadratic, 1 eq", dict(quadratic=True, d=2, T=8, O=3, n_eq=1)),
    ("program", dict(program=True, d=2, T=8)),
    ("program per step+general rows", dict(program=True, d=2, T=8, per_step=True, lin_rows=True)),
    ("program+circles", dict(program=True, d=2, T=8, circles=2)),
    ("program dynamics (span 2, 2 eq)", dict(program=True, variant="dynamics", d=3, T=6)),
    ("objective per timestep", dict(program=True, variant="attract", d=2, T=6)),
    ("objective per block, span 2", dict(block_obj="effort", T=6)),
    ("objective per block, span 2, acc+vel+groups", dict(block_obj="effort", T=6, obj_weights=True, acc_weights=True, vel_limit=0.6, groups="halves")),
    ("objective per block, span 2, ee-path", dict(block_obj="ee-path", T=5)),
    ("objective per block, span 3", dict(block_obj="smooth3", T=6)),
    ("objective per block, span 4", dict(block_obj="smooth4", d=4, T=7)),
    ("wide, span 3", dict(block_obj="smooth3", d=8, T=6, wide=True)),
    ("wide, span 2", dict(block_obj="ee-path", d=12, T=4, wide=True)),
    ("wide, per timestep", dict(block_obj="attract", d=20, T=5, wide=True)),
]


def fingerprint(res):
    h = hashlib.sha256()
    for a in [res.x] + list(res.trace) + [res.admm_iters, res.qp_solves, res.sqp_iters, res.success, res.merit, res.max_violation, res.flags]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    for name, kw in SETS:
        arrays, _ = wl.make_batch(B, **kw)
        for mode, analytic, memo in (("fd+memo", False, 1), ("analytic", True, 0)):
            res = sb.solve_batch(arrays, params=_lib.default_sqp_params(memoize_rounded=memo), analytic_jac=analytic)
            print("%-46s %-9s %s  qps %4d  ok %d" % (name, mode, fingerprint(res), int(res.qp_solves.sum()), int(res.success.sum())), flush=True)


if __name__ == "__main__":
    main()
