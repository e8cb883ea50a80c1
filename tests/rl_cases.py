"""Penalty QPs at the edges of the row-local ADMM tier's thread and tile plan (csrc/rl_plan.cpp, csrc/sco_admm_rl.hip),
shared by tests/test_row_local_edges.py (host plan + oracle, no GPU) and tests/test_row_local_edges_gpu.py (the kernel).

A case is a batch of 3 or 4 QPs on one pattern, from test_qp_plan.penalty_qp with a fixed seed (rows: [start pins | hinge
rows by timestep | one bound row per variable]) plus a structural edit, with what the host must decide about the pattern
while SCO_QP_NO_WV=1 keeps the wavefront tier off:
  plan    (fits, CW, TR, TC, NS) of sco_debug_rl_plan: fields 0, 1, 2, 3, 7 -- the instantiation <TR, TC, CW, NS> of
          qp_admm_rl_kernel; (0,) where the planner refuses the pattern;
  unsplit, unsplit_mask  the same under SCO_QP_RL_SPLIT=0 (one lane per column, no helper lane) where they differ: all of
          a column's operand pairs on one lane can need a wider instantiation, or one that does not exist;
  mask    of sco_debug_plan_tiers (1 row-local, 2 register-offset, 4 sliced-ELL, 0 generic kernel, 8 | 16 global memory);
  status  the oracle's status of every problem.
Seeds are chosen so that every problem meant to converge does so within MAX_ORACLE_ITER oracle iterations (a condition on
the cases that keeps a GPU test to seconds; tests/test_row_local_edges.py asserts it).

The thread layout behind the "shared lanes" cases: thread e owns eliminated variable e (the slacks: n_e = T r), core column
c sits on the lanes 510 - 2c (owner) and 511 - 2c (helper), so with n_e + 2 n_c > 512 the lanes 512 - 2 n_c .. n_e - 1 hold
both.

CW 20 (LCW_MAX3: ten operand pairs per column, three row slots): no penalty_qp shape with n <= 1024 reaches it with the
default plan -- of all (T, d, r) with 129 <= T d <= 156, T r <= 512 and T (d + r) <= 1024, the ones that need three row
slots and stay on chip have at most 12 operand pairs in a column, 6 + 6 on owner and helper.  The one-lane-per-column plan
does reach it: (43, 3, 11) and (37, 4, 12) below run <5,9,20,3> and <5,10,20,3> in their SCO_QP_RL_SPLIT=0 solve."""
import numpy as np

from test_qp_plan import penalty_qp
from wv_cases import empty_timestep, hinge_weights

MAX_ORACLE_ITER = 20000

# the on-chip kernels by mask, for the record of which one a case ran
RL, REG, FAST, GENERIC, STRUCTURED = 1, 2, 4, 0, 24


def pin_outside_its_box(prob, T, d, r, j=0):
    """Start pin of joint j four above the trust box of its variable: primal infeasible."""
    P, q, A, l, u = prob
    l, u = l.copy(), u.copy()
    l[j] = u[j] = u[d + T * r + j] + 4.0
    return P, q, A, l, u


def no_box_rows_at(rng, T, d, r, t):
    """The core variables of timestep t lose their box rows."""
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    keep = np.ones(len(l), dtype=bool); keep[d + T * r + t * d:d + T * r + (t + 1) * d] = False
    return P, q, A[keep], l[keep], u[keep]


def rowless_variable(rng, T, d, r, var):
    """Core variable `var` (not of timestep 0: no pin) has no row at all: no box row, and a structural zero in the hinge rows
    of its timestep.  Its column of A is empty; the smoothing terms of P still hold it."""
    assert var >= d
    P, q, A, l, u = penalty_qp(rng, T, d, r)
    keep = np.ones(len(l), dtype=bool); keep[d + T * r + var] = False
    A = A[keep].copy(); A[:, var] = 0.0
    return P, q, A, l[keep], u[keep]


class Case(object):
    """make(rng) -> list of (P, q, A, l, u).  okw: settings, given to the oracle and to the device alike.  build() -> (probs,
    w): one row multiplicity of 1 .. 3 per problem on all its hinge rows (wv_cases.hinge_weights), none with adaptive rho."""

    def __init__(self, name, seed, make, plan, mask, status=1, okw=None, unsplit=None, unsplit_mask=None):
        self.name, self.seed, self.make, self.plan, self.mask, self.okw = name, seed, make, tuple(plan), mask, dict(okw or {})
        self._status, self.unsplit = status, self.plan if unsplit is None else tuple(unsplit)
        self.unsplit_mask = mask if unsplit_mask is None else unsplit_mask

    def build(self):
        rng = np.random.default_rng(self.seed)
        probs = self.make(rng)
        return probs, (None if self.okw.get("adaptive_rho") else hinge_weights(rng, probs))

    def status(self, B):
        return list(self._status) if isinstance(self._status, (list, tuple)) else [self._status] * B

    def __repr__(self):
        return self.name


def _batch(builder, B, *args, infeasible=None):
    def make(rng):
        probs = [builder(rng, *args) for _ in range(B)]
        if infeasible is not None:
            probs[infeasible] = pin_outside_its_box(probs[infeasible], *args[:3])
        return probs
    return make


def _tile(TR, TC, CW=12, NS=2):
    return (1, CW, TR, TC, NS)


REFUSED = (0,)

# every W tile at its first and last core order, then the neighbours that leave the tier
TILES = [
    (32, (16, 2, 1), _tile(1, 2), "last order of <1,2>"), (33, (11, 3, 1), _tile(2, 4), "first order of <2,4>"),
    (64, (8, 8, 1), _tile(2, 4), "last order of <2,4>"), (65, (13, 5, 1), _tile(3, 6), "first order of <3,6>"),
    (96, (12, 8, 1), _tile(3, 6), "last order of <3,6>"), (97, (97, 1, 1), _tile(4, 8), "first order of <4,8>"),
    (128, (16, 8, 1), _tile(4, 8), "last order of <4,8>"), (129, (43, 3, 1), _tile(5, 9), "first order of <5,9>"),
    (144, (18, 8, 1), _tile(5, 9), "last order of <5,9>"), (145, (29, 5, 1), _tile(5, 10), "first order of <5,10>"),
    (156, (26, 6, 1), _tile(5, 10), "last order of <5,10>, the largest core the plan takes"),
]
LEAVING = [
    (157, (157, 1, 1), REG, "register-offset kernel"), (160, (20, 8, 1), FAST, "sliced-ELL kernel"), (161, (161, 1, 0), GENERIC, "generic kernel"),
]


def _cases():
    out = []

    def add(name, seed, *a, **kw):
        out.append(Case(name, seed, *a, **kw))

    # a. tile boundaries
    for k, (order, shape, plan, note) in enumerate(TILES):
        add("tile: core order %d at %dx%dx%d [%s]" % ((order,) + shape + (note,)), 1000 + k, _batch(penalty_qp, 3, *shape), plan, RL)
    for k, (order, shape, mask, note) in enumerate(LEAVING):
        add("past the tier: core order %d at %dx%dx%d [%s]" % ((order,) + shape + (note,)), 1100 + k, _batch(penalty_qp, 3, *shape), REFUSED, mask)
    # b. wide columns and rows: five operand pairs in a row take the wide instantiation, which exists for the 5-row tiles
    add("wide rows: 15x9x1 on <5,9> CW 16", 2001, _batch(penalty_qp, 3, 15, 9, 1), _tile(5, 9, 16), RL)
    add("wide rows: 15x10x1 on <5,10> CW 16", 2002, _batch(penalty_qp, 3, 15, 10, 1), _tile(5, 10, 16), RL)
    add("wide rows refused: 13x11x1, six operand pairs in a row", 2003, _batch(penalty_qp, 3, 13, 11, 1), REFUSED, FAST)
    add("wide rows refused: 4x9x2, five operand pairs on a small tile", 2004, _batch(penalty_qp, 3, 4, 9, 2), REFUSED, FAST)
    # c. three row slots: 2 (512 - n_e) < d + n_c free rows; only the 5-row tiles have the instantiation
    add("three row slots: 65x2x7 on <5,9> NS 3", 3021, _batch(penalty_qp, 3, 65, 2, 7), _tile(5, 9, 12, 3), RL)
    add("three row slots: 75x2x6 on <5,10> NS 3", 3002, _batch(penalty_qp, 3, 75, 2, 6), _tile(5, 10, 12, 3), RL)
    add("three row slots: 43x3x11 on <5,9> NS 3, CW 20 without the helper lanes", 3003, _batch(penalty_qp, 3, 43, 3, 11), _tile(5, 9, 12, 3), RL,
        unsplit=_tile(5, 9, 20, 3))
    add("three row slots: 37x4x12 on <5,10> NS 3, CW 20 without the helper lanes", 3004, _batch(penalty_qp, 3, 37, 4, 12), _tile(5, 10, 12, 3), RL,
        unsplit=_tile(5, 10, 20, 3))
    add("three row slots without a kernel: 100x1x5 would be <4,8> NS 3", 3025, _batch(penalty_qp, 3, 100, 1, 5), REFUSED, GENERIC)
    add("three row slots without a kernel: 50x1x10 would be <2,4> NS 3", 3006, _batch(penalty_qp, 3, 50, 1, 10), REFUSED, GENERIC)
    # d. shared lanes, one problem of four primal infeasible: its certificate runs on them next to problems that converge
    add("shared lanes: 20x7x12, lanes 232..239, one problem infeasible", 4001, _batch(penalty_qp, 4, 20, 7, 12, infeasible=2), _tile(5, 9), RL,
        status=[1, 1, -3, 1], unsplit=_tile(5, 9, 16))
    add("shared lanes: 20x7x20, lanes 232..399, one problem infeasible", 4002, _batch(penalty_qp, 4, 20, 7, 20, infeasible=2), _tile(5, 9), RL,
        status=[1, 1, -3, 1], unsplit=REFUSED, unsplit_mask=GENERIC)
    add("shared lanes: 32x1x15 on <1,2>, lanes 448..479, one problem infeasible", 4003, _batch(penalty_qp, 4, 32, 1, 15, infeasible=2), _tile(1, 2), RL,
        status=[1, 1, -3, 1], unsplit=REFUSED, unsplit_mask=FAST)
    # e. structure, on a pattern without and one with shared lanes
    for k, (shape, t, var) in enumerate((((29, 5, 1), 14, 72), ((20, 7, 12), 19, 139))):
        T, d, r = shape
        tile = _tile(5, 10) if shape == (29, 5, 1) else _tile(5, 9)
        un = dict(unsplit=_tile(5, 9, 16)) if shape == (20, 7, 12) else {}         # 6 + 1 operand pairs on one lane
        nm = "%dx%dx%d" % shape
        add("structure: no hinge rows at timestep %d of %s" % (t, nm), 5001 + 10 * k, _batch(empty_timestep, 3, T, d, r, t), tile, RL, **un)
        add("structure: no box rows at timestep %d of %s" % (t, nm), 5002 + 10 * k, _batch(no_box_rows_at, 3, T, d, r, t), tile, RL, **un)
        add("structure: variable %d of %s without a row" % (var, nm), 5003 + 10 * k, _batch(rowless_variable, 3, T, d, r, var), tile, RL, **un)
    # r = 0: no hinge row and no slack.  At 1x2 there is no smoothing term either: both variables are eliminated and the
    # core is empty; at 8x4 nothing is eliminated
    add("structure: r = 0 at 1x2, no core variable", 5021, _batch(penalty_qp, 3, 1, 2, 0), _tile(1, 2), RL)
    add("structure: r = 0 at 8x4, no eliminated variable", 5022, _batch(penalty_qp, 3, 8, 4, 0), _tile(1, 2), RL)
    # f. adaptive rho: the ADAPT twins
    ad = dict(adaptive_rho=1)
    add("adaptive rho: 32x1x15 on <1,2>", 6001, _batch(penalty_qp, 3, 32, 1, 15), _tile(1, 2), RL, okw=ad, unsplit=REFUSED, unsplit_mask=FAST)
    add("adaptive rho: 26x6x1 on <5,10>", 6002, _batch(penalty_qp, 3, 26, 6, 1), _tile(5, 10), RL, okw=ad)
    add("adaptive rho: 65x2x7 on <5,9> NS 3", 6003, _batch(penalty_qp, 3, 65, 2, 7), _tile(5, 9, 12, 3), RL, okw=ad)
    return out


CASES = _cases()

# Every instantiation rl_launch has (each also with ADAPT): (TR, TC, CW, NS, layout), layout 0 open, 1 = SCO_QP_RL_LAY8,
# 2 = SCO_QP_RL_ALIGNED.  Spelled out here, not read from csrc/layout_rl.h: the test is the second opinion.
SIX_TILES = [(1, 2), (2, 4), (3, 6), (4, 8), (5, 9), (5, 10)]
INSTANTIATIONS = set(
    [(TR, TC, 12, 2, 0) for TR, TC in SIX_TILES] + [(5, TC, 16, 2, 0) for TC in (9, 10)] +
    [(5, TC, CW, 3, 0) for TC in (9, 10) for CW in (12, 20)] + [(3, 18, CW, 2, lay) for CW in (12, 16) for lay in (1, 2)])



def ns3_sweep():
    """penalty_qp shapes with 400 <= n_e <= 512 at every TR (core orders 24, 56, 88, 120, 152) and d = 1, 2, 3, 5, 8, n_e in
    steps of 16, and the two shapes the planner used to accept without a kernel.  In a penalty_qp pattern the free rows
    (d pins and n_c box rows) sit two to a thread on the 512 - n_e threads without an eliminated variable, so the plan needs a
    third row slot when d + n_c > 2 (512 - n_e): needs_three_slots."""
    out = [(100, 1, 5), (50, 1, 10)]
    for d in (1, 2, 3, 5, 8):
        for TR in range(1, 6):
            T = (32 * TR - 8) // d
            for n_e in range(400, 513, 16):
                r = n_e // T
                if r >= 1 and 400 <= T * r <= 512 and (T, d, r) not in out:
                    out.append((T, d, r))
    return out


def needs_three_slots(T, d, r):
    return d + T * d > 2 * (512 - T * r)
