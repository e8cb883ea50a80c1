"""Per-iteration time of the wavefront ADMM tier with phases switched off (dev script; SCO_WV_ABLATE: results wrong, timing only).

The shipped kernel does not test SCO_WV_ABLATE: this script loads the variant library that does
(`python scripts/build_ablate.py wv:WV_ABLATE` -> csrc/variants/libsco_ablate_wv_WV_ABLATE.so), or SCO_LIB_OVERRIDE."""
import os, sys
import numpy as np, scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.argv = [sys.argv[0], "noop"]
from sco_py_amd import _lib as L, _build
if os.environ.get("SCO_LIB_OVERRIDE"):
    _build.LIB = os.environ["SCO_LIB_OVERRIDE"]; print("library", _build.LIB)
else:
    _build.LIB = os.path.join(_build.CSRC, "variants", "libsco_ablate_wv_WV_ABLATE.so"); print("library", _build.LIB)
    if not os.path.exists(_build.LIB):
        sys.exit("build the variant first: python scripts/build_ablate.py wv:WV_ABLATE")
os.environ["SCO_WV_MIN_PER_CU"] = "0"     # every launch on the wavefront tier (default: > 3.3 problems per CU)
import importlib.util
spec = importlib.util.spec_from_file_location("wvc", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_wv_check.py"))
src = open(spec.origin).read().split("quick = len(sys.argv)")[0]
ns = {"__file__": spec.origin, "__name__": "wvc"}
exec(compile(src, spec.origin, "exec"), ns)
penalty_qp = ns["penalty_qp"]

def timeit(B, ablate, iters=20000):
    rng = np.random.default_rng(7)
    T, d, r = 20, 7, 10
    probs = [penalty_qp(rng, T, d, r, pc=1e6) for _ in range(min(B, 64))]
    # SCO_WV_TIME_WIDTHS=1: hinge row k of a timestep is zero from column WIDTHS[k] on (the pattern keeps every entry) and the
    # handle gets the width hint, so that the launch runs the width profile (profiles/wv_jwidth.md); SCO_WV_JW=0 for the generic one
    widths = [2, 2, 3, 3, 5, 5, 6, 6, 7, 7] if os.environ.get("SCO_WV_TIME_WIDTHS") == "1" else None
    pattern = probs[0][2] != 0
    h0 = pattern.shape[0] - pattern.shape[1] - T * r          # first hinge row: behind the pins, in front of the n bound rows
    if widths:
        for p in probs:
            for t in range(T):
                for k in range(r):
                    p[2][h0 + t * r + k, t * d + widths[k]:(t + 1) * d] = 0.0
    probs = [probs[i % len(probs)] for i in range(B)]
    P0, q0, A0, l0, u0 = probs[0]
    n = len(q0); m = len(l0)
    Pu = sp.triu(sp.csc_matrix(P0), format='csc'); Pu.sort_indices(); Ac = sp.csc_matrix(pattern, dtype=float); Ac.sort_indices()
    Pp, Pi, Ap, Ai = Pu.indptr, Pu.indices, Ac.indptr, Ac.indices
    rows_of = np.asarray(Ai); cols_of = np.repeat(np.arange(n), np.diff(Ap)); prow = np.asarray(Pi); pcol = np.repeat(np.arange(n), np.diff(Pp))
    Pval = np.stack([p[0][prow, pcol] for p in probs]); Aval = np.stack([p[2][rows_of, cols_of] for p in probs])
    q = np.stack([p[1] for p in probs]); l = np.stack([p[3] for p in probs]); u = np.stack([p[4] for p in probs])
    os.environ["SCO_WV_ABLATE"] = str(ablate)
    qp = L.BatchedQP(B, n, m, Pp, Pi, Ap, Ai)
    if widths and hasattr(qp, "set_row_widths"):
        rw = np.zeros(m, dtype=np.int32); rw[h0:h0 + T * r] = np.tile(widths, T)
        qp.set_row_widths(rw)
    qp.load(Pval, q, Aval, l, u, None)
    st = L.default_qp_settings(max_iter=iters, check_termination=0 if ablate in (1, 2, 3, 4) else 25)
    qp.solve(st); qp.solve(st)
    tm = qp.last_timing(); qp.close()
    return 1e3 * tm["admm_ms"] / iters

for B in ((1024,) if os.environ.get("SCO_LIB_OVERRIDE") else (64, 1024)):
    for ab, name in ((0, "full (with termination tests)"), (4, "full, no termination tests"), (64, "tests without infeasibility certificates"),
                     (16, "checked iterations, no test pass"), (1, "no sweeps"), (2, "no row passes")):
        print("B=%5d %-32s %.3f us per iteration" % (B, name, timeit(B, ab)))
