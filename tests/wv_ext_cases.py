"""The four seeded batches on which the wavefront ADMM tier's opt-in extensions (warm start, adaptive rho) are tested,
shared by tests/test_wavefront_extensions.py (oracle only, no GPU) and tests/test_wavefront_extensions_gpu.py.

One batch per kind of instantiation of qp_admm_wv_kernel: the small-block kernel <8,1,1,4>, order 8 on <8,2,2,8>, the
run-time lanes-per-block kernel <7,4,3,10,0> and <7,4,3,10,3> of the 7-DOF x 20 shape.  Four penalty QPs each, every hinge
row with multiplicity 2 (taken as a weight: expand_dups=0)."""
import functools

import numpy as np

from test_qp_plan import penalty_qp

# (T, d, r) -> seed
BATCHES = [((7, 3, 4), 31), ((9, 8, 8), 33), ((14, 7, 10), 34), ((20, 7, 10), 35)]
IDS = ["%dx%dx%d" % s for s, _ in BATCHES]
B = 4


@functools.lru_cache(maxsize=None)
def build(shape, seed):
    T, d, r = shape
    rng = np.random.default_rng(seed)
    probs = [penalty_qp(rng, T, d, r) for _ in range(B)]
    w = np.ones((B, len(probs[0][3])), dtype=np.int32)
    w[:, d:d + T * r] = 2
    return probs, w


@functools.lru_cache(maxsize=None)
def oracle_adaptive(shape, seed):
    """(status, iterations, rho updates) per problem of the batch from the CPU oracle with adaptive_rho=1."""
    from oracle import osqp_ref as o
    probs, w = build(shape, seed)
    out = []
    for b in range(B):
        ref = o.solve(*probs[b], w=w[b], adaptive_rho=1, expand_dups=0)
        out.append((ref.info.status_val, ref.info.iter, ref.info.rho_updates))
    return np.array(out)
