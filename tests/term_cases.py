"""QPs that end on every branch of the OSQP termination test, under every setting that feeds it, shared by
tests/test_termination_tiers.py (oracle + host planners, no GPU) and tests/test_termination_tiers_gpu.py (every ADMM kernel).

A batch is a list of (P, q, A, l, u) on one pattern; problem 0 holds every structural non-zero (test_qp_gpu._stack takes
the pattern from it), the others may carry explicit zeros.  Four patterns:
  P1  penalty_qp 6x3x4             -- every on-chip kernel, the wavefront tier and both global-memory forms can run it
  P2  penalty_qp 6x3x20            -- dense row chunks on the structured tier
  P3  14 variables, 6 dense rows above an identity, diagonal P (test_wide_rows_fall_back_to_the_looping_kernels): the
      sliced-ELL kernel's looping dots, two rows per thread
  P4  40 variables, `mr` rows of 3 entries above an identity: m = mr + 40 > 1024 takes the sliced-ELL kernel's
      three-rows-per-thread instantiation; mr = 984 (m = 1024) is the last two-row shape, mr = 985 the first three-row one
P1 / P2 batches hold, for each of two seeds, [base, prim, dual, twin]: as generated; start pin of joint 0 four above its
variable's box (primal infeasible); no pins, boxes open below and q = +1000 on the joints (dual infeasible); the same with
q = -1000, which the upper boxes bound -- it must converge, so the cone test has to say "no".
P3 / P4 batches hold [base, second set of values, prim, dual]: one multi-entry row at l = u = 1e3; variable j without
curvature (explicit zeros in P), every row that holds it unbounded, q_j = 1.  P4 holds a second dual problem with q_j = 1e-3,
whose certificate takes several checks and moves with eps_dual_inf.

SETTINGS names the settings sets, each applied to the whole batch on the device and on the oracle alike; Batch.sets lists the
ones a batch runs and Batch.want the oracle's (status, iteration count) of every problem under each of them, as literals
that tests/test_termination_tiers.py reproduces -- with the float64 oracle and with its x87 extended-precision build, which
have to agree: no count here hinges on rounding.  ROUTES names the kernels: the switches that select one, and the
sco_debug_plan_tiers mask per pattern."""
import numpy as np
import scipy.sparse as sp

from rl_cases import pin_outside_its_box
from test_qp_plan import penalty_qp

MAX_ORACLE_ITER = 30000


# ---- problems --------------------------------------------------------------------------------------------------------------
def open_below(prob, T, d, r, push):
    """No pins, boxes open below, q = push on the joints (test_wavefront_tier_infeasibility_certificates): with push > 0
    every joint runs down a direction P does not see -- dual infeasible; with push < 0 the upper boxes hold."""
    P, q, A, l, u = prob
    q, l, u = q.copy(), l.copy(), u.copy()
    nx = T * d; box0 = d + T * r
    l[:d] = -np.inf; u[:d] = np.inf
    l[box0:box0 + nx] = -np.inf
    q[:nx] = push
    return P, q, A, l, u


def penalty_batch(T, d, r, seeds):
    probs, kinds = [], []
    for seed in seeds:
        base = penalty_qp(np.random.default_rng(seed), T, d, r)
        probs += [base, pin_outside_its_box(base, T, d, r), open_below(base, T, d, r, 1000.0), open_below(base, T, d, r, -1000.0)]
        kinds += ["base", "prim", "dual", "twin"]
    return probs, kinds


def row_far_outside(prob, row):
    P, q, A, l, u = prob
    assert np.count_nonzero(A[row]) > 1
    l, u = l.copy(), u.copy()
    l[row] = u[row] = 1e3
    return P, q, A, l, u


def free_direction(prob, j, cost=1.0):
    """Variable j: no curvature (its P values become explicit zeros), no bound on any row that holds it, q_j = cost."""
    P, q, A, l, u = prob
    P, q, l, u = P.copy(), q.copy(), l.copy(), u.copy()
    P[j, :] = 0.0; P[:, j] = 0.0
    rows = np.nonzero(A[:, j])[0]
    l[rows] = -np.inf; u[rows] = np.inf
    q[j] = cost
    return P, q, A, l, u


def wide_batch():
    """The pattern and the first two problems of test_wide_rows_fall_back_to_the_looping_kernels."""
    rng = np.random.default_rng(23)
    n, m_c = 14, 6
    P = np.diag(rng.random(n) + 0.5)
    A = np.vstack([rng.standard_normal((m_c, n)), np.eye(n)])
    probs = []
    for _ in range(2):
        l = np.concatenate([-rng.random(m_c) - 0.5, -np.ones(n)]); u = np.concatenate([rng.random(m_c) + 0.5, np.ones(n)])
        probs.append((P, rng.standard_normal(n), A, l, u))
    return probs + [row_far_outside(probs[0], 2), free_direction(probs[0], 5)], ["base", "base", "prim", "dual"]


def tall_pattern(rng, mr, n=40):
    """Where M (10 % density) and the mr rows of 3 entries hold their non-zeros."""
    Mm = sp.random(n, n, density=0.1, random_state=np.random.RandomState(int(rng.integers(1 << 30)))).toarray() != 0
    return Mm, np.array([rng.choice(n, 3, replace=False) for _ in range(mr)])


def tall_qp(rng, pattern):
    """mr rows of 3 random entries above an identity; P = sparse M'M + a positive diagonal; bounds A x0 +- U(0, 1); q = -P x0
    + 0.3 N(0, 1): the unconstrained optimum lies near x0, so that few of the thousand rows are active and ADMM ends in
    hundreds of iterations (thousands with scaling = 0), not in tens of thousands."""
    Mm, cols = pattern
    n, mr = Mm.shape[0], len(cols)
    M = np.where(Mm, rng.random((n, n)), 0.0)
    P = M.T @ M + np.diag(rng.uniform(0.5, 1.5, n))
    A = np.zeros((mr, n)); A[np.arange(mr)[:, None], cols] = rng.standard_normal((mr, 3))
    A = np.vstack([A, np.eye(n)])
    x0 = rng.standard_normal(n)
    ax = A @ x0
    return P, -P @ x0 + 0.3 * rng.standard_normal(n), A, ax - rng.uniform(0.0, 1.0, mr + n), ax + rng.uniform(0.0, 1.0, mr + n)


def tall_batch(mr, seed=2):
    rng = np.random.default_rng(seed)
    pattern = tall_pattern(rng, mr)
    base, second = tall_qp(rng, pattern), tall_qp(rng, pattern)
    # (with q_j = 1 the free direction is certified at the first check whatever eps_dual_inf is; with q_j = 1e-3 it takes five
    # checks at the default tolerance and one at 1e-2)
    return ([base, second, row_far_outside(base, 7), free_direction(base, 11), free_direction(base, 11, cost=1e-3)],
            ["base", "base", "prim", "dual", "dual"])


# ---- settings --------------------------------------------------------------------------------------------------------------
SETTINGS = {
    "default": {},
    "check_termination=1": dict(check_termination=1),
    "eps_inf=1e-2": dict(eps_prim_inf=1e-2, eps_dual_inf=1e-2),
    "eps_inf=1e-6": dict(eps_prim_inf=1e-6, eps_dual_inf=1e-6),
    # the two apart: with equal values a kernel that read one tolerance in the other's place would pass
    "eps_prim_inf=1e-2 eps_dual_inf=1e-6": dict(eps_prim_inf=1e-2, eps_dual_inf=1e-6),
    "eps_prim_inf=1e-6 eps_dual_inf=1e-2": dict(eps_prim_inf=1e-6, eps_dual_inf=1e-2),
    "scaling=0": dict(scaling=0),
    "scaling=3": dict(scaling=3),
    "alpha=1.0": dict(alpha=1.0),
    "check_termination=0 max_iter=150": dict(check_termination=0, max_iter=150),     # one test, at the cap
    "max_iter=213": dict(max_iter=213),                                               # no multiple of 25: ends between two checks
}
# max_iter cuts taken from the oracle's counts: the `approximate` branch at the cap (statuses 2, 3, 4) next to -2.  P1 shows
# all four at 60 (3, -2), 200 (2) and 6400 (4); P2 shows 3 and -2 at 150 and 300, 4 at 27000 and 2 at 3625 under scaling = 0.
# The rule behind the choice: a dual problem that a cut stops is on its way down its ray, |x| growing by about ten per
# iteration, and x there can be compared at 1e-10 only while the oracle's own two precisions agree that far -- they differ by
# 3e-11 after 200 iterations, 1.1e-10 after 575 and 1e-8 after 4000.  So a cut either stops the dual problems within 300
# iterations or comes after they are certified (test_iterates_that_a_cut_stops_are_still_comparable).  With the default
# scaling P2's first status 2 is at 575 iterations (its first twin converges at 625) with both dual problems on their rays;
# under scaling = 0 they are certified at 1200 and 50 and the twin of seed 300 converges at 3650: status 2 at 3625.  P4 m = 1140
# adds a cut at 450, where both its base problems stop with status 2 on the three-rows-per-thread kernel.
for _cut in (60, 200, 6400, 150, 300, 27000, 450):
    SETTINGS["max_iter=%d" % _cut] = dict(max_iter=_cut)
SETTINGS["scaling=0 max_iter=3625"] = dict(scaling=0, max_iter=3625)
FEW = ["default", "check_termination=1", "scaling=0", "eps_inf=1e-2"]

# ---- routes: the switches that select a kernel, and the sco_debug_plan_tiers mask of each pattern under them ----------------
# (bit 0 row-local, 1 register-offset, 2 sliced-ELL, none of them: the generic kernel, 3 global memory, 4 its structured form,
# 5 wavefront tier beside the row-local kernel)
_NO_RL, _NO_REG, _NO_FAST = {"SCO_QP_NO_RL": "1"}, {"SCO_QP_NO_REG": "1"}, {"SCO_QP_NO_FAST": "1"}
ROUTES = {
    "row-local": ({"SCO_QP_NO_WV": "1"}, {"P1": 1, "P2": 1}),
    "wavefront": ({"SCO_WV_MIN_PER_CU": "0"}, {"P1": 33}),
    "register-offset": (_NO_RL, {"P1": 2}),
    # (the mask says 4 for all three forms of qp_admm_fast_kernel; FAST_PLAN below tells them apart: capped dots on P1, the
    # looping form on P2 -- a core column holds 20 hinge entries -- and P3, three rows per thread on P4 past m = 1024)
    "sliced-ELL": ({**_NO_RL, **_NO_REG}, {"P1": 4, "P2": 4}),
    "sliced-ELL by default": ({}, {"P3": 4, "P4": 4}),
    "generic": ({**_NO_RL, **_NO_REG, **_NO_FAST}, {"P1": 0, "P2": 0, "P3": 0, "P4": 0}),
    "global memory, dense": ({"SCO_QP_FORCE_BIG": "1", "SCO_QP_NO_BT": "1"}, {"P1": 8, "P3": 8}),
    "structured": ({"SCO_QP_FORCE_BIG": "1"}, {"P1": 24, "P2": 24}),
}
# a pattern's own route: the other routes are compared with it (statuses and counts equal, |dx| < 1e-10)
HOME = {"P1": "row-local", "P2": "row-local", "P3": "sliced-ELL by default", "P4": "sliced-ELL by default"}
# where a switch set does NOT select the kernel of its name: P2 is past the wavefront plan (20 hinge rows per timestep) and
# past the register-offset caps
NOT_A_ROUTE = {("P2", "wavefront"): 1, ("P2", "register-offset"): 4}
# every switch a route sets: a test clears them all before it sets its own
SWITCHES = sorted({k for sw, _ in ROUTES.values() for k in sw} | {"SCO_QP_NO_ELIM", "SCO_QP_FACTOR_CHOLESKY", "SCO_QP_NO_MFMA"})

# sco_debug_fast_plan (fits, TR, TC, capped dots, rows per thread, LDS bytes) and sco_debug_reg_plan (fits, TR, TC, CW, RW, PX,
# dynamic LDS bytes) of the batches that run those kernels: the instantiation <TR, TC, 12, 8, 12, 8, 2> / <TR, TC, 0, 0, 0, 0,
# rows per thread> of qp_admm_fast_kernel and <TR, TC, CW, RW, PX> of qp_admm_reg_kernel, and the LDS each launch asks for
FAST_PLAN = {"P1": (1, 1, 2, 1, 2, 19400), "P2": (1, 1, 2, 0, 2, 53432), "P3": (1, 1, 2, 0, 2, 29480), "P4 m=1140": (1, 2, 4, 0, 3, 129968),
             "P4 m=1024": (1, 2, 4, 0, 2, 116944), "P4 m=1025": (1, 2, 4, 0, 3, 118248)}
REG_PLAN = {"P1": (1, 1, 2, 12, 8, 10, 17408)}
# sco_debug_rl_plan of the patterns on the row-local route: (fits, CW, TR, TC, dynamic LDS bytes, closed, layout, NS)
RL_PLAN = {"P1": (1, 12, 1, 2, 56832, 0, 0, 2), "P2": (1, 12, 1, 2, 64000, 0, 0, 2)}
# Every instantiation fast_launch / reg_launch has.  Spelled out here, not read from the kernel files: the second opinion.
TILES = [(1, 2), (2, 4), (3, 6), (4, 8), (5, 9), (5, 10)]
FAST_INSTANTIATIONS = {(TR, TC, capped, nq) for TR, TC in TILES for capped, nq in ((1, 2), (0, 2), (0, 3))}
REG_INSTANTIATIONS = {(TR, TC, 12, 8, PX) for TR, TC in TILES for PX in (10, 12)}


# ---- the table -------------------------------------------------------------------------------------------------------------
class Batch(object):
    """make() -> (probs, kinds).  sets: the settings sets it runs.  routes: the kernels that solve it.  want[set]: the oracle's
    (status, iteration count) per problem.  wv_kept: the problems the wavefront tier's value test keeps (the kernel certifies
    or solves them itself; the others it hands to the row-local kernel) -- None where the batch does not run that route.
    resid_parity: residuals compared at the parity tolerance (test_qp_gpu.TOL), for the reason in the docstring of
    test_random_sparsity_patterns_match_oracle."""

    def __init__(self, name, pattern, make, routes, want, resid_parity=False, wv_kept=None):
        self.name, self.pattern, self.make, self.routes, self.want = name, pattern, make, list(routes), want
        self.sets, self.resid_parity, self.wv_kept, self._built = list(want), resid_parity, wv_kept, None

    def build(self):
        if self._built is None:
            self._built = self.make()
        return self._built

    def status(self, s):
        return [st for st, _ in self.want[s]]

    def __repr__(self):
        return self.name


# (status, iteration count) of the oracle, float64 and x87 alike.  P1 / P2: [base, prim, dual, twin] of seed 300, then of seed
# 302 (seed 301 is not used: its dual problem on P2 creeps down its ray to max_iter = 100 000).  P3 / P4: [base, second set of
# values, prim, dual], P4 with a second dual problem (q_j = 1e-3)
WANT = {
    'P1': {
        'default': [(1, 225), (-3, 100), (-4, 5350), (1, 375), (1, 125), (-3, 75), (-4, 6475), (1, 275)],
        'check_termination=1': [(1, 211), (-3, 92), (-4, 5345), (1, 277), (1, 113), (-3, 48), (-4, 6454), (1, 252)],
        'eps_inf=1e-2': [(1, 225), (-3, 50), (-4, 3875), (1, 375), (1, 125), (-3, 25), (-4, 775), (1, 275)],
        'eps_inf=1e-6': [(1, 225), (-3, 200), (-4, 7750), (1, 375), (1, 125), (-3, 75), (-4, 8725), (1, 275)],
        'eps_prim_inf=1e-2 eps_dual_inf=1e-6': [(1, 225), (-3, 50), (-4, 7750), (1, 375), (1, 125), (-3, 25), (-4, 8725), (1, 275)],
        'eps_prim_inf=1e-6 eps_dual_inf=1e-2': [(1, 225), (-3, 200), (-4, 3875), (1, 375), (1, 125), (-3, 75), (-4, 775), (1, 275)],
        'scaling=0': [(1, 2500), (-3, 1200), (-4, 50), (1, 1575), (1, 375), (-3, 375), (-4, 50), (1, 1600)],
        'scaling=3': [(1, 225), (-3, 100), (-4, 5700), (1, 375), (1, 125), (-3, 75), (-4, 3075), (1, 275)],
        'alpha=1.0': [(1, 350), (-3, 175), (-4, 8575), (1, 275), (1, 125), (-3, 75), (-4, 10325), (1, 200)],
        'check_termination=0 max_iter=150': [(-2, 150), (-3, 150), (-2, 150), (-2, 150), (1, 150), (-3, 150), (-2, 150), (-2, 150)],
        'max_iter=213': [(1, 213), (-3, 100), (-2, 213), (-2, 213), (1, 125), (-3, 75), (-2, 213), (-2, 213)],
        'max_iter=60': [(-2, 60), (3, 60), (-2, 60), (-2, 60), (-2, 60), (-3, 60), (-2, 60), (-2, 60)],
        'max_iter=200': [(2, 200), (-3, 100), (-2, 200), (-2, 200), (1, 125), (-3, 75), (-2, 200), (-2, 200)],
        'max_iter=6400': [(1, 225), (-3, 100), (-4, 5350), (1, 375), (1, 125), (-3, 75), (4, 6400), (1, 275)],
    },
    'P2': {
        'default': [(1, 1950), (-3, 1825), (-4, 27975), (1, 625), (1, 1750), (-3, 200), (-4, 9250), (1, 725)],
        'eps_inf=1e-2': [(1, 1950), (-3, 75), (-4, 4325), (1, 625), (1, 1750), (-3, 75), (-4, 1300), (1, 725)],
        'scaling=0': [(1, 18650), (-3, 18150), (-4, 1200), (1, 3650), (1, 16925), (-3, 2150), (-4, 50), (1, 14350)],
        'max_iter=150': [(-2, 150), (-2, 150), (-2, 150), (-2, 150), (-2, 150), (3, 150), (-2, 150), (-2, 150)],
        'max_iter=300': [(-2, 300), (-2, 300), (-2, 300), (-2, 300), (-2, 300), (-3, 200), (-2, 300), (-2, 300)],
        'max_iter=27000': [(1, 1950), (-3, 1825), (4, 27000), (1, 625), (1, 1750), (-3, 200), (-4, 9250), (1, 725)],
        'scaling=0 max_iter=3625': [(-2, 3625), (-2, 3625), (-4, 1200), (2, 3625), (-2, 3625), (-3, 2150), (-4, 50), (-2, 3625)],
    },
    'P3': {
        'default': [(1, 75), (1, 75), (-3, 50), (-4, 25)],
        'check_termination=1': [(1, 52), (1, 75), (-3, 37), (-4, 1)],
        'scaling=0': [(1, 125), (1, 175), (-3, 75), (-4, 25)],
        'eps_inf=1e-2': [(1, 75), (1, 75), (-3, 50), (-4, 25)],
    },
    'P4 m=1140': {
        'default': [(1, 600), (1, 475), (-3, 50), (-4, 25), (-4, 125)],
        'check_termination=1': [(1, 588), (1, 463), (-3, 27), (-4, 10), (-4, 122)],
        'scaling=0': [(1, 6150), (1, 2600), (-3, 25), (-4, 25), (-4, 75)],
        'eps_inf=1e-2': [(1, 600), (1, 475), (-3, 25), (-4, 25), (-4, 25)],
        'max_iter=450': [(2, 450), (2, 450), (-3, 50), (-4, 25), (-4, 125)],
    },
    'P4 m=1024': {
        'default': [(1, 1375), (1, 550), (-3, 50), (-4, 25), (-4, 125)],
    },
    'P4 m=1025': {
        'default': [(1, 325), (1, 1050), (-3, 50), (-4, 25), (-4, 125)],
    },
}
# settings sets by pattern: P2's long solves (28 000 iterations on its dual problems, 19 000 at scaling = 0) run the sets
# that matter most; P3 / P4 run FEW; the two shapes at the edge of the rows-per-thread rule run the default alone
assert list(WANT["P3"]) == FEW and list(WANT["P4 m=1140"]) == FEW + ["max_iter=450"]

_P1_ROUTES = ["row-local", "wavefront", "register-offset", "sliced-ELL", "generic", "global memory, dense", "structured"]
BATCHES = [
    # (the pin of a prim problem and the open rows of a dual / twin problem keep the values of a penalty QP: the wavefront
    # tier's value test keeps all eight, and its kernel forms both certificates itself)
    Batch("P1 6x3x4", "P1", lambda: penalty_batch(6, 3, 4, (300, 302)), _P1_ROUTES, WANT["P1"], wv_kept=list(range(8))),
    Batch("P2 6x3x20", "P2", lambda: penalty_batch(6, 3, 20, (300, 302)), ["row-local", "sliced-ELL", "generic", "structured"], WANT["P2"]),
    Batch("P3 wide rows", "P3", wide_batch, ["sliced-ELL by default", "generic", "global memory, dense"], WANT["P3"], resid_parity=True),
    Batch("P4 m=1140", "P4", lambda: tall_batch(1100), ["sliced-ELL by default", "generic"], WANT["P4 m=1140"], resid_parity=True),
    Batch("P4 m=1024", "P4", lambda: tall_batch(984), ["sliced-ELL by default", "generic"], WANT["P4 m=1024"], resid_parity=True),
    Batch("P4 m=1025", "P4", lambda: tall_batch(985), ["sliced-ELL by default", "generic"], WANT["P4 m=1025"], resid_parity=True),
]
# every (batch, route, settings set) the GPU file solves
RUNS = [(b, r, s) for b in BATCHES for r in b.routes for s in b.sets]
