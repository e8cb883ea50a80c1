"""Penalty QPs with more than two single rows on a core variable (joint limits), for the stacked-row class of the wavefront
ADMM tier (csrc/sco_admm_wv.hip), shared by tests/test_wavefront_stack.py (host plan + oracle, no GPU) and
tests/test_wavefront_stack_gpu.py (the kernel).

Builders are plain functions of an `rng` that return (P, q, A, l, u).  The limit rows sit behind the hinge rows (and behind
the link rows, where there are any) and in front of the bound rows, so every variable's box row stays its last single row:
the order csrc/sco_sqp.hip builds (linear_entries)."""
import numpy as np

import wv_cases as wc
import wv_link_cases as lc
from test_qp_plan import penalty_qp

BATCH = 4
H = 0.35                                                  # half width of the limits around the centre of the box row
ONE_SIDED = [(1, 3, 4), (2, 3, 4), (3, 3, 4), (4, 8, 8), (9, 3, 8), (17, 5, 5), (21, 2, 3), (14, 7, 10), (20, 7, 10)]
TWO_SIDED = [(3, 3, 4), (17, 5, 5), (20, 7, 10)]
CONTRA = [(3, 3, 4), (9, 3, 8), (20, 7, 10)]              # h = -0.05: the two rows of a variable contradict each other, status -3
GOAL = [(7, 3, 4), (14, 7, 10), (20, 7, 10)]
LINK = [(3, 3, 4), (17, 5, 5), (14, 7, 10)]
# the plan of each shape is the one of its limit-free pattern
PLAN = dict(lc.PLAN)
PLAN[(1, 3, 4)] = (1, 3, 1, 8, 8, 1, 1, 4)
PLAN[(7, 3, 4)] = wc.SMALL[:2] + (7,) + wc.SMALL[3:]


def add_limits(prob, T, d, at, box0, h, two=False):
    """Limit rows on every core variable of `prob`, inserted in front of row `at`; `box0` is the first box row of `prob`.
    One-sided (the device family's form): the T d rows +e_c <= mid + h, then the T d rows -e_c <= h - mid; two-sided: the rows
    mid - h <= e_c <= mid + h.  mid is the centre of the variable's box row."""
    P, q, A, l, u = prob
    nx = T * d
    mid = 0.5 * (l[box0:box0 + nx] + u[box0:box0 + nx])
    eye = np.zeros((nx, len(q))); eye[np.arange(nx), np.arange(nx)] = 1.0
    if two:
        rows, lo, hi = eye, mid - h, mid + h
    else:
        rows, lo, hi = np.vstack([eye, -eye]), np.full(2 * nx, -np.inf), np.concatenate([mid + h, h - mid])
    return lc._insert(prob, at, rows, lo, hi)


def limits(rng, T, d, r, h, two=False):
    """[pins of block 0 | hinge rows | limit rows | box rows]"""
    return add_limits(penalty_qp(rng, T, d, r), T, d, d + T * r, d + T * r, h, two)


def goal_limits(rng, T, d, r, h=H):
    """[start pins | goal pins | hinge rows | one-sided limit rows | box rows]: four single rows on the variables of the first
    and of the last block."""
    return add_limits(wc.goal_pins(rng, T, d, r), T, d, 2 * d + T * r, 2 * d + T * r, h)


def link_limits(rng, T, d, r, vmax=0.25, h=0.8):
    """[pins | hinge rows | two-sided link rows | two-sided limit rows | box rows]: a link row and a limit row share the link
    slots of every variable but the last block's."""
    nl = d * (T - 1)
    return add_limits(lc.two_sided(rng, T, d, r, vmax), T, d, d + T * r + nl, d + T * r + nl, h, two=True)


def n_limit_rows(two, T, d):
    return (1 if two else 2) * T * d


class StackCase(object):
    """kind: "one" / "two" (limits with half width h), "goal", "link".  status: what the oracle returns for every problem of
    the batch (one value, or one per problem); max_iters: a bound on the oracle's iteration counts where one was recorded.
    tier: the problems the wavefront kernel itself has to solve.  With two-sided limits a pinned variable has three single rows
    and both link slots free, so its pin is stacked next to its limit row: a slot runs on the base rho, the pin sits on
    rho_eq, every problem of such a batch fails the kernel's value test and the row-local kernel behind the launch solves it."""

    def __init__(self, kind, shape, h, status, max_iters=None):
        self.kind, self.shape, self.h, self.max_iters = kind, shape, h, max_iters
        self.status = list(status) if isinstance(status, (list, tuple)) else [status] * BATCH
        self.check = list(range(BATCH))
        self.tier = [] if kind == "two" else list(range(BATCH))

    def build(self, B=BATCH):
        T, d, r = self.shape
        if self.kind in ("one", "two"):
            rng = np.random.default_rng(200 + T)
            probs = [limits(rng, T, d, r, self.h, two=self.kind == "two") for _ in range(B)]
            return probs, lc.weights(rng, probs, T, d, r)
        rng = np.random.default_rng(300 + T)
        probs = [(goal_limits if self.kind == "goal" else link_limits)(rng, T, d, r) for _ in range(B)]
        return probs, np.ones((B, len(probs[0][3])), dtype=np.int32)

    def __repr__(self):
        return "%s %dx%dx%d h=%g" % ((self.kind,) + self.shape + (self.h,))


def _cases():
    out = [StackCase("one", s, H, 1, 2600) for s in ONE_SIDED]
    out += [StackCase("two", s, H, 1) for s in TWO_SIDED]
    out += [StackCase("one", s, -0.05, -3, 2125) for s in CONTRA]
    out += [StackCase("goal", s, H, 1, 5950) for s in GOAL]
    # (problem 2 of the 17 x 5 and of the 14 x 7 batch draws neighbouring boxes more than vmax apart: primal infeasible)
    odd = {(17, 5, 5): [1, 1, -3, 1], (14, 7, 10): [1, 1, -3, 1]}
    out += [StackCase("link", s, 0.8, odd.get(s, 1)) for s in LINK]
    return out


CASES = _cases()


def batch(shape, B=BATCH, two=False, h=H):
    """B problems with limits from default_rng(200 + T), and their row multiplicities."""
    return StackCase("two" if two else "one", shape, h, 1).build(B)


EQ_SHAPES = [(3, 3, 4), (14, 7, 10)]
EQ_OTHERS = [0, 2, 3, 4]


def equality_batch(shape):
    """Five two-sided problems whose start pins are boxes of half width 0.01 instead of equalities -- inequality rows on the
    base rho, so that the stacked slots of the pinned variables pass the value test -- and in problem 1 the limit rows are
    equalities (l = u = mid): rho_eq in a stacked slot."""
    T, d, r = shape
    probs, w = batch(shape, B=5, two=True)
    lo = d + T * r; nl = n_limit_rows(True, T, d)
    out = []
    for b, (P, q, A, l, u) in enumerate(probs):
        l, u = l.copy(), u.copy()
        l[:d] -= 0.01; u[:d] += 0.01
        if b == 1:
            mid = 0.5 * (l[lo:lo + nl] + u[lo:lo + nl])
            l[lo:lo + nl] = mid; u[lo:lo + nl] = mid
        out.append((P, q, A, l, u))
    return out, w
