"""Host loop vs resident loop for Probs with block objective terms (SCO_FAM_FLAG_OBJ_BLOCK): the same problems built the
reference's way, once with plain Expr objects (Python in every SQP iteration, one QP launch per Prob.optimize) and once with
devexpr objects (solve_many: one device batch), wall time of each."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import blockobj_build as bb          # noqa: E402
import conftest as ct                # noqa: E402
from sco_py_amd import workloads as wl            # noqa: E402
from sco_py_amd.sco_osqp import batching          # noqa: E402

for kind, B in (("effort", int(os.environ.get("B_EFFORT", 4))), ("ee-path", int(os.environ.get("B_EE", 1)))):
    mods = ct.mirror_mods()
    prs = [wl.make_block_obj_problem(i, kind) for i in range(B)]
    host = [bb.build_prob(mods, pr)[:2] for pr in prs]
    t = time.time(); oks_h, st_h = batching.solve_many([p for p, _ in host]); th = time.time() - t
    dev = [bb.build_prob(mods, pr, device_exprs=True)[:2] for pr in prs]
    batching.solve_many([p for p, _ in dev])                    # (handle creation, first launch)
    dev = [bb.build_prob(mods, pr, device_exprs=True)[:2] for pr in prs]
    t = time.time(); oks_d, st_d = batching.solve_many([p for p, _ in dev]); td = time.time() - t
    dx = max(float(np.abs(a.get_value() - b.get_value()).max()) for (_, a), (_, b) in zip(host, dev))
    print("%-8s B=%d host loop %.2f s (%.2f s per problem), resident loop %.3f s -> x%.0f; success host %s device %s; max |x_host - x_dev| %.1e"
          % (kind, B, th, th / B, td, th / td, list(oks_h), list(oks_d), dx), flush=True)
