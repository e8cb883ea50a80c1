"""Penalty QPs at the edges of the wavefront ADMM tier's lane and block layout (csrc/sco_admm_wv.hip), shared by
tests/test_wavefront_edges.py (host plan + oracle, no GPU) and tests/test_wavefront_edges_gpu.py (the kernel).

Builders are plain functions of an `rng` that return (P, q, A, l, u) in the row order of test_qp_plan.penalty_qp:
[pins of block 0 | further pins | hinge rows by timestep | one bound row per variable].  CASES lists every batch the GPU
file compares with the oracle; the CPU file asserts for the same batches that the oracle alone ends where the GPU test
expects it to."""
import numpy as np

from test_qp_plan import penalty_qp

# ---- the plan table: (T, d, r) -> info[:8] = fits, block order, blocks, lanes per block, instantiation <BS, NS, NV, NSTEP>
ACCEPTED = [
    ((1, 3, 4), (1, 3, 1, 8, 8, 1, 1, 4), "T=1: no chain"),
    ((2, 3, 4), (1, 3, 2, 8, 8, 1, 1, 4), "T=2: chain B empty"),
    ((3, 3, 4), (1, 3, 3, 8, 8, 1, 1, 4), "T=3: shortest two-sided"),
    ((1, 8, 3), (1, 8, 1, 8, 8, 1, 1, 4), "order 8, T=1"),
    ((4, 8, 8), (1, 8, 4, 8, 8, 1, 1, 4), "order 8, r = NS*lpb"),
    ((8, 8, 8), (1, 8, 8, 8, 8, 1, 1, 4), "order 8, r = NS*lpb, T=8"),
    ((8, 8, 7), (1, 8, 8, 8, 8, 1, 1, 4), "order 8, r = NS*lpb - 1"),
    ((3, 1, 1), (1, 1, 3, 8, 8, 1, 1, 4), "order 1"),
    ((5, 1, 2), (1, 1, 5, 8, 8, 1, 1, 4), "order 1, two rows"),
    ((9, 8, 8), (1, 8, 9, 5, 8, 2, 2, 8), "order 8, T=9 leaves lpb 8"),
    ((9, 3, 8), (1, 3, 9, 5, 8, 2, 2, 8), "T=9 leaves lpb 8"),
    ((12, 8, 10), (1, 8, 12, 5, 8, 2, 2, 8), "order 8, r = NS*lpb at lpb 5"),
    ((16, 8, 8), (1, 8, 16, 4, 8, 2, 2, 8), "order 8, NS edge at lpb 4"),
    ((17, 6, 6), (1, 6, 17, 3, 8, 2, 2, 8), "order 6, T=17 = 2 NSTEP + 1"),
    ((17, 5, 5), (1, 5, 17, 3, 8, 2, 2, 8), "T=17 = 2 NSTEP + 1, r = NS*lpb - 1"),
    ((20, 6, 6), (1, 6, 20, 3, 8, 2, 2, 10), "order 6, r = NS*lpb on NSTEP 10"),
    ((21, 4, 4), (1, 4, 21, 2, 8, 2, 2, 10), "order 4, lpb 2, T=21 = 2 NSTEP + 1"),
    ((21, 2, 3), (1, 2, 21, 2, 8, 2, 2, 10), "lpb 2, T=21, r = NS*lpb - 1"),
    ((17, 7, 10), (1, 7, 17, 3, 7, 4, 3, 10), "7-DOF T=17: padded, odd"),
    ((19, 7, 10), (1, 7, 19, 3, 7, 4, 3, 10), "7-DOF T=19: padded, odd"),
    ((18, 7, 12), (1, 7, 18, 3, 7, 4, 3, 10), "7-DOF T=18, every row slot full"),
    ((20, 7, 12), (1, 7, 20, 3, 7, 4, 3, 10), "7-DOF T=20, every row slot full"),
    ((20, 7, 11), (1, 7, 20, 3, 7, 4, 3, 10), "7-DOF T=20, r = NS*lpb - 1"),
    ((14, 7, 10), (1, 7, 14, 4, 7, 4, 3, 10), "LPB=0 kernel T=14"),
    ((16, 7, 10), (1, 7, 16, 4, 7, 4, 3, 10), "LPB=0 kernel T=16"),
    ((13, 7, 16), (1, 7, 13, 4, 7, 4, 3, 10), "LPB=0 kernel T=13, every row slot full"),
    ((16, 7, 8), (1, 7, 16, 4, 8, 2, 2, 8), "7-DOF on the BS=8 kernel, lpb 4"),
    ((12, 7, 10), (1, 7, 12, 5, 8, 2, 2, 8), "7-DOF on the BS=8 kernel, lpb 5"),
]
# the refusal next to each edge, and why
REFUSED = [
    ((16, 8, 9), "three row slots at lpb 4"), ((20, 6, 7), "three row slots at lpb 3"), ((22, 2, 3), "mid 11 > NSTEP 10"),
    ((20, 7, 13), "five row slots at lpb 3"), ((21, 7, 8), "7 variables on 2 lanes: four variable slots"),
    ((9, 7, 20), "LDS 41152 B > 40 KB"), ((8, 7, 30), "LDS 45376 B > 40 KB"),
]


def hinge_rows(A):
    """Mask of the hinge rows: the only rows with more than one entry (core columns of one timestep + their slack)."""
    return np.count_nonzero(A, axis=1) >= 2


def hinge_weights(rng, probs, lo=1, hi=4):
    """One multiplicity per problem on all its hinge rows, 1 elsewhere (as test_qp_gpu draws them)."""
    h = hinge_rows(probs[0][2])
    w = np.ones((len(probs), len(h)), dtype=np.int32)
    w[:, h] = rng.integers(lo, hi, size=(len(probs), 1))
    return w


def _insert_rows(prob, at, rows, vals):
    P, q, A, l, u = prob
    vals = np.asarray(vals, dtype=float)
    return (P, q, np.vstack([A[:at], rows, A[at:]]), np.concatenate([l[:at], vals, l[at:]]), np.concatenate([u[:at], vals, u[at:]]))


def _box_mid(prob, T, d, r, c):
    box0 = d + T * r
    return 0.5 * (prob[3][box0 + c] + prob[4][box0 + c])


def goal_pins(rng, T, d, r):
    """Start AND goal pins: one equality row per joint of the last block, behind the start pins and in front of the hinge
    rows, so that every variable's box row stays its last single row (the order osqp_utils.py builds)."""
    prob = penalty_qp(rng, T, d, r)
    n = len(prob[1])
    rows = np.zeros((d, n)); vals = []
    for j in range(d):
        c = (T - 1) * d + j
        rows[j, c] = 1.0; vals.append(_box_mid(prob, T, d, r, c) + 0.05 * rng.standard_normal())
    return _insert_rows(prob, d, rows, vals)


def middle_pin(rng, T, d, r, blk, k=1):
    """One equality row on component k of block blk (a way point)."""
    prob = penalty_qp(rng, T, d, r)
    c = blk * d + k
    row = np.zeros((1, len(prob[1]))); row[0, c] = 1.0
    return _insert_rows(prob, d, row, [_box_mid(prob, T, d, r, c) + 0.2])


def no_box_row(rng, T, d, r, var):
    """Core variable `var` loses its box row."""
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    keep = np.ones(len(l), dtype=bool); keep[d + T * r + var] = False
    return P, q, A[keep], l[keep], u[keep]


def ragged_hinge_rows(rng, T, d, r):
    """Every other hinge row misses every other core column (the pattern is taken from A != 0)."""
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    nx = T * d
    A = A.copy(); blk = A[d:d + T * r, :nx]; blk[::2, ::2] = 0.0; A[d:d + T * r, :nx] = blk
    return P, q, A, l, u


def empty_timestep(rng, T, d, r, t):
    """Timestep t has no hinge row and no slack variable at all."""
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    nx = T * d; n = len(q); box0 = d + T * r
    rows = np.ones(len(l), dtype=bool); cols = np.ones(n, dtype=bool)
    rows[d + t * r:d + (t + 1) * r] = False; cols[nx + t * r:nx + (t + 1) * r] = False
    rows[box0 + nx + t * r:box0 + nx + (t + 1) * r] = False
    return P[np.ix_(cols, cols)], q[cols], A[np.ix_(rows, cols)], l[rows], u[rows]


def dense_p_blocks(rng, T, d, r, pins="start"):
    """A random symmetric positive semidefinite d x d block on every diagonal block of P."""
    P, q, A, l, u = goal_pins(rng, T, d, r) if pins == "both" else penalty_qp(rng, T, d, r)
    P = P.copy()
    for t in range(T):
        M = rng.standard_normal((d, d)); P[t * d:(t + 1) * d, t * d:(t + 1) * d] += M @ M.T
    return P, q, A, l, u


def dual_infeasible_dense_p(rng, T, d, r):
    """Boxes open below, no pins, q = 1000 on the joints; P's added blocks are N N' with the columns of N summing to zero:
    the all-ones direction stays in P's null space, but P dx = 0 holds only through cancellation of off-diagonal entries."""
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    nx = T * d; box0 = d + T * r
    P = P.copy(); q = q.copy(); l = l.copy(); u = u.copy()
    for t in range(T):
        N = rng.standard_normal((d, d)); N -= N.mean(axis=0)
        P[t * d:(t + 1) * d, t * d:(t + 1) * d] += N @ N.T
    q[:nx] = 1000.0; l[:d] = -np.inf; u[:d] = np.inf; l[box0:box0 + nx] = -np.inf
    return P, q, A, l, u


def odd_values(rng, T, d, r, ordinary):
    """Six + problems of one pattern: 1 .. 4 break the value structure of a penalty QP (two-sided hinge row, slack with an
    upper bound, a box narrow enough for the equality rho, unequal hinge weights), the ones in `ordinary` do not."""
    B = max(ordinary) + 1
    probs = [list(penalty_qp(rng, T, d, r)) for _ in range(B)]
    nx = T * d; m = len(probs[0][3])
    probs[1][3] = probs[1][3].copy(); probs[1][3][d + 2] = -3.0
    probs[2][4] = probs[2][4].copy(); probs[2][4][d + T * r + nx + 1] = 5.0
    lo, hi = probs[3][3].copy(), probs[3][4].copy()
    nb = d + T * r + d + 1                                     # box row of a variable of block 1 (not pinned)
    mid = 0.5 * (lo[nb] + hi[nb]); lo[nb] = mid - 2e-5; hi[nb] = mid + 2e-5
    probs[3][3], probs[3][4] = lo, hi
    w = np.ones((B, m), dtype=np.int32); w[:, d:d + T * r] = 2; w[4, d + 1] = 3
    return [tuple(p) for p in probs], w


# ---- the batches of the GPU file ------------------------------------------------------------------------------------
class Case(object):
    """make(rng) -> (probs, w or None).  check: problems compared with the oracle (None = all).  okw: settings, given to the
    oracle and to the device alike.  status: what the oracle returns for every checked problem (1), or a list per checked
    problem; "max_iter": -2 after exactly max_iter iterations.  tier: problems the wavefront kernel itself has to solve
    (None = all; the others fail its value test and go to the row-local kernel)."""

    def __init__(self, name, seed, make, check=None, okw=None, status=1, tier=None, plan=None, n_extra=None):
        self.name, self.seed, self.make, self.check, self.okw = name, seed, make, check, dict(okw or {})
        self.status, self.tier, self.plan, self.n_extra = status, tier, plan, n_extra

    def build(self):
        rng = np.random.default_rng(self.seed)
        probs, w = self.make(rng)
        check = list(range(len(probs))) if self.check is None else list(self.check)
        tier = list(range(len(probs))) if self.tier is None else list(self.tier)
        return probs, w, check, tier

    def __repr__(self):
        return self.name


def _batch(builder, B, *args, weights=True, **kw):
    def make(rng):
        probs = [builder(rng, *args, **kw) for _ in range(B)]
        return probs, (hinge_weights(rng, probs) if weights else None)
    return make


def _batch_pin_weights(builder, B, *args):
    """As _batch, and every pin (the rows in front of the hinge rows: the extra-row lanes) with a multiplicity of 2 or 3."""
    def make(rng):
        probs = [builder(rng, *args) for _ in range(B)]
        w = hinge_weights(rng, probs)
        w[:, :int(np.argmax(hinge_rows(probs[0][2])))] = rng.integers(2, 4, size=(B, 1))
        return probs, w
    return make


SMALL = (1, 3, None, 8, 8, 1, 1, 4)       # plan of every variant of a (6 | 7, 3, 4) pattern: info[2] = T is filled in


def _cases():
    out = []
    # a. shape sweep: batch of 5, weights 1 .. 3; every problem against the oracle where T d <= 64, else the first three
    for k, (shape, plan, note) in enumerate(ACCEPTED):
        T, d, r = shape
        out.append(Case("sweep %dx%dx%d [%s]" % (T, d, r, note), 1000 + k, _batch(penalty_qp, 5, T, d, r),
                        check=None if T * d <= 64 else range(3), plan=plan))
    # b. pins elsewhere
    out.append(Case("goal pins 7x3", 2001, _batch(goal_pins, 5, 7, 3, 4), plan=SMALL, n_extra=6))
    for blk, side in ((2, "chain A"), (3, "the middle block"), (5, "chain B")):
        out.append(Case("middle pin on block %d of 7 (%s)" % (blk, side), 2010 + blk, _batch(middle_pin, 5, 7, 3, 4, blk), plan=SMALL, n_extra=4))
    out.append(Case("goal pins 7x3 with row multiplicities on the pins", 2002, _batch_pin_weights(goal_pins, 5, 7, 3, 4), plan=SMALL, n_extra=6))
    out.append(Case("middle pin on block 5 of 7 with row multiplicities on the pins", 2003, _batch_pin_weights(middle_pin, 5, 7, 3, 4, 5), plan=SMALL, n_extra=4))
    out.append(Case("start + goal pins 20x7x10", 2020, _batch(goal_pins, 5, 20, 7, 10), check=range(3), plan=(1, 7, 20, 3, 7, 4, 3, 10), n_extra=14))
    out.append(Case("start + goal pins 14x7x10 (LPB=0 kernel)", 2021, _batch(goal_pins, 5, 14, 7, 10), check=range(3), plan=(1, 7, 14, 4, 7, 4, 3, 10), n_extra=14))
    # c. missing pieces
    out.append(Case("missing box row in the middle block", 3001, _batch(no_box_row, 5, 7, 3, 4, 10), plan=SMALL, n_extra=3))
    out.append(Case("missing box row in the last block", 3002, _batch(no_box_row, 5, 7, 3, 4, 20), plan=SMALL, n_extra=3))
    out.append(Case("missing box row in block 0: pin on rho_eq, row-local kernel", 3003, _batch(no_box_row, 5, 7, 3, 4, 1), plan=SMALL, n_extra=2, tier=[]))
    out.append(Case("hinge rows missing alternate columns 6x3", 3004, _batch(ragged_hinge_rows, 5, 6, 3, 4), plan=SMALL, n_extra=3))
    out.append(Case("hinge rows missing alternate columns 16x7x10 (LPB=0 kernel)", 3005, _batch(ragged_hinge_rows, 5, 16, 7, 10), check=range(3), plan=(1, 7, 16, 4, 7, 4, 3, 10), n_extra=7))
    for t, where in ((0, "first"), (3, "middle"), (6, "last")):
        out.append(Case("empty timestep: %s block of 7" % where, 3010 + t, _batch(empty_timestep, 5, 7, 3, 4, t), plan=SMALL, n_extra=3))
    # d. dense P blocks
    out.append(Case("dense P blocks 6x3", 4001, _batch(dense_p_blocks, 5, 6, 3, 4), plan=SMALL, n_extra=3))
    out.append(Case("dense P blocks 9x8 (order 8)", 4002, _batch(dense_p_blocks, 5, 9, 8, 8), check=range(3), plan=(1, 8, 9, 5, 8, 2, 2, 8), n_extra=8))
    out.append(Case("dense P blocks 20x7x10", 4003, _batch(dense_p_blocks, 5, 20, 7, 10), check=range(3), plan=(1, 7, 20, 3, 7, 4, 3, 10), n_extra=7))
    out.append(Case("dense P blocks with goal pins 14x7x10 (LPB=0 kernel)", 4004, _batch(dense_p_blocks, 5, 14, 7, 10, pins="both"), check=range(3), plan=(1, 7, 14, 4, 7, 4, 3, 10), n_extra=14))
    for shape, seed in (((6, 3, 4), 4010), ((7, 3, 4), 4011)):
        out.append(Case("dual infeasible on dense P blocks %dx%d" % shape[:2], seed, _batch(dual_infeasible_dense_p, 3, *shape, weights=False),
                        status=-4, plan=SMALL, n_extra=3))      # (the open pin rows stay in the pattern)
    # e. settings on the tier
    lines = [("max_iter=40", dict(max_iter=40), "max_iter"),
             ("rho sigma eps alpha check_termination=10", dict(rho=0.5, sigma=1e-6, eps_abs=1e-5, eps_rel=1e-5, alpha=1.2, check_termination=10), 1),
             ("alpha=1.0", dict(alpha=1.0), 1), ("check_termination=1", dict(check_termination=1), 1),
             ("max_iter=25 on a check", dict(max_iter=25), "max_iter"), ("max_iter=26 one past a check", dict(max_iter=26), "max_iter"),
             ("max_iter=49 one before a check", dict(max_iter=49), "max_iter")]
    for shape in ((6, 3, 4), (20, 7, 10)):
        for k, (nm, okw, status) in enumerate(lines):
            out.append(Case("settings %s at %dx%d" % (nm, shape[0], shape[1]), 5000 + shape[0], _batch(penalty_qp, 3, *shape), okw=okw, status=status))
    # f. batch sizes
    out.append(Case("batch of 1", 6001, _batch(penalty_qp, 1, 6, 3, 4)))
    out.append(Case("batch of 1027", 6002, _batch(penalty_qp, 1027, 6, 3, 4), check=[int(v) for v in np.linspace(0, 1026, 8)]))
    # g. mixed batch at (14, 7, 10): problems 1 .. 4 fail the value test
    out.append(Case("mixed batch 14x7x10: odd value structure between ordinary problems", 7001,
                    lambda rng: odd_values(rng, 14, 7, 10, ordinary=(0, 5, 6)), tier=[0, 5, 6]))
    return out


CASES = _cases()
# two solves of one batch must give identical bits: the shapes, and the seed of their batch of 6
REPEAT = [((20, 7, 10), 8001), ((14, 7, 10), 8002)]
# the default arm family on the LPB = 0 kernel, through the SQP loop
ARM_HORIZONS = [13, 14, 16]
