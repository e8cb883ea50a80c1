"""Penalty QPs with rows that link neighbouring timesteps (velocity limits), for the link-row class of the wavefront ADMM
tier (csrc/sco_admm_wv.hip), shared by tests/test_wavefront_link.py (host plan + oracle, no GPU) and
tests/test_wavefront_link_gpu.py (the kernel).

Builders are plain functions of an `rng` that return (P, q, A, l, u) in the row order
[pins of block 0 | hinge rows by timestep | link rows by transition and joint | one bound row per variable]: the link rows sit
behind the hinge rows and in front of the bound rows, so every variable's box row stays its last single row."""
import numpy as np

import wv_cases as wc
from test_qp_plan import penalty_qp

# (T, d, r) and what each covers; the plan of each is the one of its link-free pattern (wv_cases.ACCEPTED)
SHAPES = [
    ((2, 3, 4), "one transition, chain B empty"),
    ((3, 3, 4), "links into and out of the middle block"),
    ((4, 8, 8), "order 8"),
    ((9, 3, 8), "lpb 5"),
    ((17, 5, 5), "lpb 3, two variable slots"),
    ((21, 2, 3), "lpb 2, T = 2 NSTEP + 1"),
    ((14, 7, 10), "run-time lanes-per-block kernel"),
    ((20, 7, 10), "full 7-wide instantiation"),
]
PLAN = {shape: plan for shape, plan, _ in wc.ACCEPTED}
PLAN[(20, 7, 10)] = (1, 7, 20, 3, 7, 4, 3, 10)       # (wv_cases lists 7 x 20 with 11 and 12 rows: the same plan)
TIGHT = [(2, 3, 4), (3, 3, 4), (4, 8, 8)]            # vmax = 0.02: many rows at their bound (53 625 iterations at 7 x 20: left off)
CONTRA = [(3, 3, 4), (9, 3, 8), (20, 7, 10)]         # vmax = -0.05: the two rows of a pair contradict each other, status -3
BATCH = 4


def _insert(prob, at, rows, lo, hi):
    P, q, A, l, u = prob
    return (P, q, np.vstack([A[:at], rows, A[at:]]), np.concatenate([l[:at], np.asarray(lo, float), l[at:]]),
            np.concatenate([u[:at], np.asarray(hi, float), u[at:]]))


def one_sided(rng, T, d, r, vmax):
    """The 2 d (T - 1) rows  +(x[t+1, k] - x[t, k]) <= vmax,  -(x[t+1, k] - x[t, k]) <= vmax  (the device family's form)."""
    prob = penalty_qp(rng, T, d, r)
    n = len(prob[1]); rows = []
    for t in range(T - 1):
        for k in range(d):
            for sgn in (1.0, -1.0):
                e = np.zeros(n); e[(t + 1) * d + k] = sgn; e[t * d + k] = -sgn; rows.append(e)
    return _insert(prob, d + T * r, np.array(rows), [-np.inf] * len(rows), [vmax] * len(rows))


def two_sided(rng, T, d, r, vmax):
    """One row  -vmax <= x[t+1, k] - x[t, k] <= vmax  per pair."""
    prob = penalty_qp(rng, T, d, r)
    n = len(prob[1]); rows = []
    for t in range(T - 1):
        for k in range(d):
            e = np.zeros(n); e[(t + 1) * d + k] = 1.0; e[t * d + k] = -1.0; rows.append(e)
    return _insert(prob, d + T * r, np.array(rows), [-vmax] * len(rows), [vmax] * len(rows))


def n_links(builder, T, d):
    return (2 if builder is one_sided else 1) * d * (T - 1)


def weights(rng, probs, T, d, r):
    """One multiplicity 1 .. 3 per problem on its hinge rows, 1 elsewhere (link rows: the value test wants 1)."""
    w = np.ones((len(probs), len(probs[0][3])), dtype=np.int32)
    w[:, d:d + T * r] = rng.integers(1, 4, size=(len(probs), 1))
    return w


def batch(builder, shape, vmax, B=BATCH):
    """B problems of one pattern from default_rng(100 + T), and their row multiplicities."""
    T, d, r = shape
    rng = np.random.default_rng(100 + T)
    probs = [builder(rng, T, d, r, vmax) for _ in range(B)]
    return probs, weights(rng, probs, T, d, r)


class LinkCase(object):
    """status: what the oracle returns for every problem of the batch (one value, or one per problem)."""

    def __init__(self, builder, shape, vmax, status):
        self.builder, self.shape, self.vmax = builder, shape, vmax
        self.status = list(status) if isinstance(status, (list, tuple)) else [status] * BATCH
        self.check = list(range(BATCH))

    def build(self):
        return batch(self.builder, self.shape, self.vmax)

    def __repr__(self):
        return "%s %dx%dx%d vmax=%g" % ((self.builder.__name__,) + self.shape + (self.vmax,))


def _cases():
    out = []
    # (problem 2 of the 17 x 5 batch draws two neighbouring boxes more than vmax apart: the oracle certifies it primal
    # infeasible, with feasible-looking link rows -- kept, as one more certificate through the link rows)
    odd = {(17, 5, 5): [1, 1, -3, 1]}
    for shape, _ in SHAPES:
        out.append(LinkCase(one_sided, shape, 0.15, odd.get(shape, 1)))
    for shape in ((3, 3, 4), (17, 5, 5), (20, 7, 10)):
        out.append(LinkCase(two_sided, shape, 0.15, odd.get(shape, 1)))
    for shape in TIGHT:
        out.append(LinkCase(one_sided, shape, 0.02, 1))
    for shape in CONTRA:
        out.append(LinkCase(one_sided, shape, -0.05, -3))
    return out


CASES = _cases()


# ---- patterns the plan refuses: (name, builder of (P, A), reason = WvWhy of csrc/sco_internal.h) ----------------------
WHY_THIRD_LINK, WHY_SAME_BLOCK, WHY_FAR_BLOCKS, WHY_INDEX, WHY_THREE_CORE = 3, 4, 5, 6, 7


def _with_row(T, d, r, cols, base=None):
    prob = base if base is not None else penalty_qp(np.random.default_rng(0), T, d, r)
    e = np.zeros((1, len(prob[1])))
    for c in cols:
        e[0, c] = 1.0
    return _insert(prob, d + T * r, e, [-1.0], [1.0])


def refused():
    T, d, r = 3, 3, 4
    links = two_sided(np.random.default_rng(0), T, d, r, 0.15)
    two = _with_row(T, d, r, (d + 1, 1), base=links)
    return [
        ("a third link row on one pair", _with_row(T, d, r, (d + 1, 1), base=two), WHY_THIRD_LINK),
        ("two core variables inside one block without a slack", _with_row(T, d, r, (d, d + 1)), WHY_SAME_BLOCK),
        ("blocks t, t + 2", _with_row(T, d, r, (1, 2 * d + 1)), WHY_FAR_BLOCKS),
        ("different in-block indices", _with_row(T, d, r, (0, d + 1)), WHY_INDEX),
        ("three core variables", _with_row(T, d, r, (1, d + 1, 2 * d + 1)), WHY_THREE_CORE),
        ("three core variables of two blocks", _with_row(T, d, r, (0, 1, d + 1)), WHY_THREE_CORE),
    ]
