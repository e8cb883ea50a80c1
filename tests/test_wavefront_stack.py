"""Stacked rows of the wavefront ADMM tier (csrc/sco_admm_wv.hip, plan: csrc/wv_plan.cpp; single rows of a core variable other than its last one,
held in the variable slot's free link slots with an empty partner, i.e. joint limits), without a GPU: the host plan of the
patterns of tests/wv_stack_cases.py through sco_debug_wv_stack_plan, the counts of stacked and extra-lane rows worked out
from the assignment rule, the plans of the patterns the tier took before, the refusals, the launch planner's rule for
adaptive rho, and the oracle's own verdict on every batch that tests/test_wavefront_stack_gpu.py solves on the device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import wv_cases as wc
import wv_link_cases as lc
import wv_stack_cases as sc
from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_launch_plan import A_RL, A_WV_RL, INT_MAX, NEED_NONE, NEED_WINDOW, _no_qp_environment, plan      # noqa: F401  (a fixture)
from test_qp_plan import penalty_qp
from test_wavefront_edges import wv_plan
from test_wavefront_link import link_plan

WHY_STACKED = 10
NL, LANES = 2, 64                   # link slots per variable slot, extra-row lanes (WV_NL, WV_T of csrc/sco_internal.h)


def stack_plan(Pm, Am):
    """info = the fourteen fields of test_wavefront_link.link_plan, then the stacked rows."""
    P = sp.triu(sp.csc_matrix(np.asarray(Pm) != 0), format="csc"); A = sp.csc_matrix(np.asarray(Am) != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); info = np.full(15, -99, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    lib.sco_debug_wv_stack_plan.argtypes = [C.POINTER(C.c_int)]; lib.sco_debug_wv_stack_plan.restype = C.c_int
    assert lib.sco_debug_plan_build(P.shape[0], A.shape[0], ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert lib.sco_debug_wv_stack_plan(ip(info)) == 0
    return [int(v) for v in info]


def by_the_rule(A, nx):
    """(stacked rows, extra-lane rows) of the pattern of A (core columns: the first nx), or None where the rule refuses."""
    single = [0] * nx; links = [0] * nx
    for row in np.asarray(A) != 0:
        cols = np.flatnonzero(row)
        if cols[-1] >= nx:
            continue                                     # a hinge row or a slack's bound row
        if len(cols) == 1:
            single[cols[0]] += 1
        else:
            links[cols[0]] += 1                          # a link row belongs to the variable of the earlier block
    if max(single) <= 2 and sum(k == 2 for k in single) <= LANES:
        return 0, sum(k == 2 for k in single)            # the assignment the tier had: nothing stacked
    n_stack = n_extra = 0
    for k, nl in zip(single, links):                     # the rows in front of the last one: free slots first, one may be left over
        if k >= 3:
            if k - 1 > NL - nl + 1:
                return None
            n_stack += min(NL - nl, k - 1); n_extra += k - 1 > NL - nl
    if n_extra > LANES:
        return None
    for k, nl in zip(single, links):                     # pairs, in column order: a lane while lanes last, then a slot
        if k == 2:
            if n_extra < LANES:
                n_extra += 1
            elif nl < NL:
                n_stack += 1
            else:
                return None
    return n_stack, n_extra


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_stacked_patterns_are_accepted_on_the_instantiation_of_their_limit_free_pattern(case):
    T, d, r = case.shape
    probs, _ = case.build(1)
    P, q, A, l, u = probs[0]
    info = stack_plan(P, A)
    assert tuple(info[:8]) == sc.PLAN[case.shape], info
    assert info[11] == 2 and info[13] == 0, info
    assert info[12] == 4 and info[8] <= 40 * 1024, info          # four problems per CU
    want = by_the_rule(A, T * d)
    assert want is not None and want[0] > 0 and (info[14], info[9]) == want, (info, want)
    assert info[10] == (d * (T - 1) if case.kind == "link" else 0), info
    assert link_plan(P, A) == info[:14]                    # the handle's plan, through the older export
    assert wv_plan(P, A)[0] == 0                           # the link-free plan still refuses the pattern


def test_the_counts_of_the_worked_examples():
    """One-sided limits at 20 x 7: two stacked rows per variable, the start pins on lanes.  Goal pins as well: 14 lanes.
    Two-sided links and limits at 17 x 5: the 5 pins and 59 limit rows fill the lanes, the pinned variables' limit rows and
    the 21 limit rows without a lane are stacked.  Two-sided limits at 20 x 7: pin and limit row of the pinned variables are
    stacked (both slots are free), 64 of the other 133 limit rows have a lane."""
    rng = np.random.default_rng(0)
    for prob, want in ((sc.limits(rng, 20, 7, 10, sc.H), (280, 7)), (sc.goal_limits(rng, 20, 7, 10), (280, 14)),
                       (sc.link_limits(rng, 17, 5, 5), (26, 64)), (sc.limits(rng, 20, 7, 10, sc.H, two=True), (14 + 69, 64))):
        info = stack_plan(prob[0], prob[2])
        assert info[0] == 1 and (info[14], info[9]) == want, (info, want)
        assert by_the_rule(prob[2], info[1] * info[2]) == want


def _taken_before():
    rng = np.random.default_rng(0)
    out = [("penalty_qp %dx%dx%d" % s, penalty_qp(rng, *s), lc.PLAN[s], s[1], 0) for s in ((3, 3, 4), (17, 5, 5), (20, 7, 10))]
    out += [("goal_pins 7x3x4", wc.goal_pins(rng, 7, 3, 4), sc.PLAN[(7, 3, 4)], 6, 0),
            ("goal_pins 20x7x10", wc.goal_pins(rng, 20, 7, 10), lc.PLAN[(20, 7, 10)], 14, 0),
            ("middle_pin 7x3x4", wc.middle_pin(rng, 7, 3, 4, 5), sc.PLAN[(7, 3, 4)], 4, 0)]
    for builder in (lc.one_sided, lc.two_sided):
        for s in ((3, 3, 4), (17, 5, 5), (14, 7, 10), (20, 7, 10)):
            out.append(("%s %dx%dx%d" % ((builder.__name__,) + s), builder(rng, *s, 0.15), lc.PLAN[s], s[1], lc.n_links(builder, s[0], s[1])))
    return out


@pytest.mark.parametrize("name,prob,plan8,n_extra,n_link", _taken_before(), ids=[c[0] for c in _taken_before()])
def test_a_pattern_the_tier_took_before_has_the_plan_it_had(name, prob, plan8, n_extra, n_link):
    """At most two single rows per variable and at most 64 second rows: nothing is stacked, and instantiation, lanes, LDS
    bytes, extra-lane rows and link slots are those of the plan without stacked rows."""
    info = stack_plan(prob[0], prob[2])
    assert tuple(info[:8]) == plan8 and info[9] == n_extra, info
    assert info[10:] == [n_link, 2 if n_link else 0, 4, 0, 0], info
    assert info[:14] == link_plan(prob[0], prob[2])
    if not n_link:
        assert info[:10] == wv_plan(prob[0], prob[2])
    if name.endswith("sided 20x7x10"):
        assert info[8] == 37696, info                      # the LDS bytes of a 7 x 20 link plan (profiles/wv_link_rows.md)
    if name.endswith("sided 14x7x10"):
        assert info[8] == 39104, info                      # ... and with four lanes per block


def _family_qp(**kw):
    from oracle import arm_family as af
    from oracle import sco_ref as sr
    out = sr.penalty_sqp(sr.trajopt_flat(af.make_problem(0, **kw)), sr.SolverParams(max_qp_solves=2), record_qps=True)
    return out.qps[1]


def _refused():
    T, d, r = 3, 3, 4
    one = sc.limits(np.random.default_rng(0), T, d, r, sc.H)
    # 9 x 8: 72 variables.  One-sided limits and one more single row on every variable behind block 0: four single rows on
    # each of them, five on none -- 72 left-over rows for 64 lanes
    T9, d9, r9 = 9, 8, 8
    wide = sc.limits(np.random.default_rng(0), T9, d9, r9, sc.H)
    more = np.zeros((T9 * d9 - d9, len(wide[1]))); more[np.arange(len(more)), d9 + np.arange(len(more))] = 1.0
    wide = lc._insert(wide, d9 + T9 * r9, more, [-1.0] * len(more), [1.0] * len(more))
    return [
        ("a fifth single row on one variable", lambda: lc._with_row(T, d, r, (0,), base=one)),
        ("a third stacked row on a variable that has no extra lane left", lambda: wide),
        ("velocity and joint limits of the device family", lambda: tuple(_family_qp(vel_limit=0.3, joint_limit=0.2)[k] for k in ("P", "q", "A", "l", "u"))),
    ]


@pytest.mark.parametrize("name,make", _refused(), ids=[c[0] for c in _refused()])
def test_refusals_carry_the_reason_of_stacked_rows(name, make):
    prob = make()
    info = stack_plan(prob[0], prob[2])
    assert info[0] == 0 and info[13] == WHY_STACKED, (name, info)
    assert wv_plan(prob[0], prob[2])[0] == 0
    nx = info[1] * info[2] if info[1] > 0 else None
    if nx:
        assert by_the_rule(np.asarray(prob[2]), nx) is None


def test_four_single_rows_next_to_the_refusals_are_accepted():
    """The 9 x 8 pattern of the refusal with its additional row on 56 variables only: 64 left-over rows, every lane taken."""
    T, d, r = 9, 8, 8
    prob = sc.limits(np.random.default_rng(0), T, d, r, sc.H)
    more = np.zeros((56, len(prob[1]))); more[np.arange(56), d + np.arange(56)] = 1.0
    prob = lc._insert(prob, d + T * r, more, [-1.0] * 56, [1.0] * 56)
    info = stack_plan(prob[0], prob[2])
    assert info[0] == 1 and (info[14], info[9]) == (2 * T * d, 64) and by_the_rule(prob[2], T * d) == (2 * T * d, 64), info


@pytest.mark.parametrize("kw,want", [(dict(joint_limit=0.2), (1, 7, 20, 3, 7, 4, 3, 10)), (dict(d=3, T=6, K=2, O=2, joint_limit=0.3), (1, 3, 6, 8, 8, 1, 1, 4))],
                         ids=["7x20", "3x6"])
def test_joint_limits_of_the_device_family_are_stacked_rows(kw, want):
    """Two one-sided rows per joint and timestep (csrc/sco_sqp.hip linear_entries) next to the trust-box row: the pattern
    lands on the instantiation of the family without them, and a handle created for it holds the tier."""
    q = _family_qp(**kw)
    info = stack_plan(q["P"], q["A"])
    T, d = want[2], want[1]
    assert tuple(info[:8]) == want and info[14] == 2 * d * T and info[10] == 0 and info[11] == 2 and info[13] == 0, info
    assert info[12] == 4 and info[8] <= 40 * 1024, info
    mask = C.c_int(0)
    assert _lib.load().sco_debug_plan_tiers(C.byref(mask)) == 0 and mask.value & 32


def test_adaptive_rho_on_a_stacked_plan_stays_on_the_row_local_kernel():
    """wv = 2: the handle's wavefront plan holds link slots in use (NL > 0), which have no adaptive-rho instantiation."""
    big = dict(batch=1024, wv_min=0)
    p = plan(wv=2, **big)
    assert (p["wv_now"], p["admm"], p["need"]) == (1, A_WV_RL, NEED_NONE)
    p = plan(wv=2, adaptive=1, **big)
    assert (p["rc"], p["wv_now"], p["admm"], p["need"]) == (0, 0, A_RL, NEED_WINDOW)
    assert plan(wv=2, adaptive=1)["wv_min_live"] == INT_MAX


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_oracle_ends_where_the_gpu_test_expects(case):
    """The recorded status for every problem, within the recorded iteration count."""
    probs, w = case.build()
    for b in case.check:
        ref = o.solve(*probs[b], w=w[b])
        assert ref.info.status_val == case.status[b], (b, ref.info.status_val, ref.info.iter)
        assert ref.info.iter <= (case.max_iters or 99999), (b, ref.info.iter)


@pytest.mark.parametrize("shape", sc.EQ_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_oracle_finishes_the_batch_with_equality_limit_rows(shape):
    """tests/test_wavefront_stack_gpu.py compares every problem of this batch with the oracle: it has to end below max_iter,
    at least three of the four problems beside the one with equalities solved.  Pins as boxes keep the plan: the pattern is
    the one of the two-sided case."""
    probs, w = sc.equality_batch(shape)
    st = []
    for b in range(5):
        ref = o.solve(*probs[b], w=w[b])
        assert ref.info.status_val in (1, -3) and ref.info.iter < 100000, (b, ref.info.status_val, ref.info.iter)
        st.append(ref.info.status_val)
    assert sum(st[b] == 1 for b in sc.EQ_OTHERS) >= 3, st
    T, d, r = shape
    info = stack_plan(probs[0][0], probs[0][2])
    assert info[0] == 1 and info[14] >= 2 * d, info          # pin (box) and limit row of every variable of block 0
