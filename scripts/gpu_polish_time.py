"""What polish costs next to the ADMM it follows (results: profiles/qp_polish.md).

    python scripts/gpu_polish_time.py [batch] [rounds]

`batch` (1024) penalty QPs of the 7-DOF x 20 shape, penalty_qp(rng, 20, 7, 10).  Alternating, `rounds` (3) times:
  A  sco_qp_solve at the reference's tolerances (eps_abs 1e-6, eps_rel 1e-9) + sco_qp_polish
  B  sco_qp_solve alone at eps_abs = 1e-9: what that accuracy costs without polish
Per round: sco_qp_last_timing of the solves, HIP-event time of polish by kernel, polish statuses, residuals before and after,
and the distance of each answer from run A's polished x."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sco_py_amd import _lib                    # noqa: E402
from test_qp_gpu import _stack                 # noqa: E402
from test_qp_plan import penalty_qp            # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rng = np.random.default_rng(2024)
    probs = [penalty_qp(rng, 20, 7, 10) for _ in range(B)]
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    qp = _lib.BatchedQP(B, n, m, Pp, Pi, Ap, Ai)
    print(json.dumps(dict(batch=B, n=n, m=m)))
    try:
        qp.load(Pval, q, Aval, l, u)
        for r in range(rounds):
            t0 = time.perf_counter()
            x, y, st, it, res = qp.solve(_lib.default_qp_settings())
            t1 = time.perf_counter()
            ta = qp.last_timing()
            xp, yp, ps, rp = qp.polish()
            t2 = time.perf_counter()
            ms, k = qp.polish_info()
            xt, yt, st_t, it_t, res_t = qp.solve(_lib.default_qp_settings(eps_abs=1e-9))
            tb = qp.last_timing()
            ok = ps == 1
            row = dict(
                solve=ta, solve_wall_ms=1e3 * (t1 - t0), polish=ms, polish_ms=sum(ms.values()), polish_wall_ms=1e3 * (t2 - t1),
                status=dict(OK=int((ps == 1).sum()), FAILED=int((ps == -1).sum()), NOT_RUN=int((ps == 0).sum())),
                solve_status={str(s): int((st == s).sum()) for s in np.unique(st)},
                iters_median=float(np.median(it)), iters_max=int(it.max()),
                k_median=float(np.median(k[k >= 0])) if (k >= 0).any() else -1, k_max=int(k.max()),
                resid_admm_max=[float(res[ok, 0].max(initial=0)), float(res[ok, 1].max(initial=0))],
                resid_polished_max=[float(rp[ok, 0].max(initial=0)), float(rp[ok, 1].max(initial=0))],
                admm_vs_polished_x_max=float(np.abs(x[ok] - xp[ok]).max(initial=0)),
                tight=tb, tight_status={str(s): int((st_t == s).sum()) for s in np.unique(st_t)},
                tight_iters_median=float(np.median(it_t)), tight_iters_max=int(it_t.max()),
                tight_resid_max=[float(res_t[:, 0].max()), float(res_t[:, 1].max())],
                tight_vs_polished_x_max=float(np.abs(xt[ok] - xp[ok]).max(initial=0)))
            print(json.dumps(row))
    finally:
        qp.close()


if __name__ == "__main__":
    main()
