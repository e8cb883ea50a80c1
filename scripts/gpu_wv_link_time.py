"""Per-iteration time of the wavefront ADMM tier with link rows (velocity limits) next to the link-free kernel and to the
row-local kernel, 7 x 20 with 10 hinge rows per timestep (dev script, shipped library).

eps_abs = eps_rel = 0: no solve ends before max_iter, every launch runs `iters` iterations with a termination test every 25.
Usage: python scripts/gpu_wv_link_time.py [B]"""
import os, sys
import numpy as np, scipy.sparse as sp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sco_py_amd import _lib as L
import wv_link_cases as lc

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
ITERS = 5000


def timeit(builder, no_wv):
    os.environ["SCO_WV_MIN_PER_CU"] = "0"
    os.environ["SCO_QP_NO_WV"] = "1" if no_wv else "0"
    rng = np.random.default_rng(7)
    T, d, r = 20, 7, 10
    probs = [builder(rng, T, d, r) for _ in range(min(B, 32))]
    probs = [probs[i % len(probs)] for i in range(B)]
    P0, q0, A0, l0, u0 = probs[0]
    n, m = len(q0), len(l0)
    Pu = sp.triu(sp.csc_matrix(P0), format="csc"); Pu.sort_indices(); Ac = sp.csc_matrix(A0 != 0, dtype=float); Ac.sort_indices()
    pr, pc = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr)); ar, ac = Ac.indices, np.repeat(np.arange(n), np.diff(Ac.indptr))
    Pval = np.stack([p[0][pr, pc] for p in probs]); Aval = np.stack([p[2][ar, ac] for p in probs])
    q = np.stack([p[1] for p in probs]); l = np.stack([p[3] for p in probs]); u = np.stack([p[4] for p in probs])
    qp = L.BatchedQP(B, n, m, Pu.indptr, Pu.indices, Ac.indptr, Ac.indices)
    qp.load(Pval, q, Aval, l, u, None)
    st = L.default_qp_settings(max_iter=ITERS, eps_abs=0.0, eps_rel=0.0)
    qp.solve(st); out = qp.solve(st)
    tm = qp.last_timing(); qp.close()
    if not np.all(out[3] == ITERS):                     # (a certified-infeasible draw ends early: the launch still runs ITERS)
        print("  %d of %d problems ended before %d iterations" % (int((out[3] != ITERS).sum()), B, ITERS))
    return 1e3 * tm["admm_ms"] / ITERS


for name, builder in (("link-free", lambda rng, T, d, r: lc.penalty_qp(rng, T, d, r)),
                      ("one-sided link rows, vmax 0.15", lambda rng, T, d, r: lc.one_sided(rng, T, d, r, 0.15)),
                      ("two-sided link rows, vmax 0.15", lambda rng, T, d, r: lc.two_sided(rng, T, d, r, 0.15))):
    for no_wv in (False, True):
        print("B=%5d %-32s %-10s %.3f us per iteration of the batch" % (B, name, "row-local" if no_wv else "wavefront", timeit(builder, no_wv)), flush=True)
