"""Link rows of the wavefront ADMM tier (csrc/sco_admm_wv.hip, plan: csrc/wv_plan.cpp; rows on one in-block index of two neighbouring timesteps,
i.e. velocity limits), without a GPU: the host plan of the patterns of tests/wv_link_cases.py through
sco_debug_wv_link_plan, the refusals and their reasons, the launch planner's rule for adaptive rho, and the oracle's own
verdict on every batch that tests/test_wavefront_link_gpu.py solves on the device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import wv_link_cases as lc
from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_launch_plan import A_RL, A_WV_RL, INT_MAX, NEED_NONE, NEED_WINDOW, _no_qp_environment, plan      # noqa: F401  (a fixture)
from test_wavefront_edges import wv_plan


def link_plan(Pm, Am):
    """info = the ten fields of wv_plan (link rows allowed), then link rows, link slots per variable slot, problems per CU,
    reason of a refusal."""
    P = sp.triu(sp.csc_matrix(np.asarray(Pm) != 0), format="csc"); A = sp.csc_matrix(np.asarray(Am) != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); info = np.full(14, -99, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    lib.sco_debug_wv_link_plan.argtypes = [C.POINTER(C.c_int)]; lib.sco_debug_wv_link_plan.restype = C.c_int
    assert lib.sco_debug_plan_build(P.shape[0], A.shape[0], ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert lib.sco_debug_wv_link_plan(ip(info)) == 0
    return [int(v) for v in info]


@pytest.mark.parametrize("builder", [lc.one_sided, lc.two_sided], ids=["one-sided", "two-sided"])
@pytest.mark.parametrize("shape,note", lc.SHAPES, ids=["%dx%dx%d %s" % (s + (n,)) for s, n in lc.SHAPES])
def test_link_patterns_are_accepted_on_the_instantiation_of_their_link_free_pattern(shape, note, builder):
    T, d, r = shape
    P, q, A, l, u = builder(np.random.default_rng(0), T, d, r, 0.15)
    info = link_plan(P, A)
    assert tuple(info[:8]) == lc.PLAN[shape], info
    assert info[9] == d and info[10] == lc.n_links(builder, T, d) and info[11] == 2 and info[13] == 0, info
    assert info[12] == 4 and info[8] <= 40 * 1024, info          # four problems per CU
    old = wv_plan(P, A)
    assert old[0] == 0, old                              # the link-free plan still refuses the pattern


@pytest.mark.parametrize("shape", [(3, 3, 4), (20, 7, 10)])
def test_a_link_free_pattern_has_the_plan_it_had(shape):
    P, q, A, l, u = lc.penalty_qp(np.random.default_rng(0), *shape)
    info, old = link_plan(P, A), wv_plan(P, A)
    assert info[:10] == old and info[10:] == [0, 0, 4, 0], (info, old)


@pytest.mark.parametrize("name,prob,why", lc.refused(), ids=[c[0] for c in lc.refused()])
def test_refusals_name_their_reason(name, prob, why):
    info = link_plan(prob[0], prob[2])
    assert info[0] == 0 and info[13] == why, (name, info)
    assert wv_plan(prob[0], prob[2])[0] == 0


def test_two_rows_on_a_pair_fill_both_link_slots():
    """One two-sided row and one further row on the same pair: accepted (NL = 2); the third is the refusal above."""
    T, d, r = 3, 3, 4
    two = lc._with_row(T, d, r, (d + 1, 1), base=lc.two_sided(np.random.default_rng(0), T, d, r, 0.15))
    info = link_plan(two[0], two[2])
    assert info[0] == 1 and info[10] == d * (T - 1) + 1 and info[13] == 0, info


@pytest.mark.parametrize("kw,want", [(dict(vel_limit=0.3), (1, 7, 20, 3, 7, 4, 3, 10)), (dict(d=3, T=6, K=2, O=2, vel_limit=0.6), (1, 3, 6, 8, 8, 1, 1, 4))],
                         ids=["7x20", "3x6"])
def test_velocity_limits_of_the_device_family_are_link_rows(kw, want):
    """Two one-sided rows per joint and transition (csrc/sco_sqp.hip linear_entries): the pattern lands on the instantiation
    of the family without them, and a handle created for it holds the tier."""
    from oracle import arm_family as af
    from oracle import sco_ref as sr
    out = sr.penalty_sqp(sr.trajopt_flat(af.make_problem(0, **kw)), sr.SolverParams(max_qp_solves=2), record_qps=True)
    q = out.qps[1]
    info = link_plan(q["P"], q["A"])
    T, d = want[2], want[1]
    assert tuple(info[:8]) == want and info[10] == 2 * d * (T - 1) and info[13] == 0, info
    mask = C.c_int(0)
    assert _lib.load().sco_debug_plan_tiers(C.byref(mask)) == 0 and mask.value & 32


def test_adaptive_rho_on_a_link_plan_stays_on_the_row_local_kernel(monkeypatch):
    """wv = 2: the handle's wavefront plan holds link rows, which have no adaptive-rho instantiation."""
    big = dict(batch=1024, wv_min=0)
    p = plan(wv=2, **big)
    assert (p["wv_now"], p["admm"], p["need"]) == (1, A_WV_RL, NEED_NONE)
    p = plan(wv=2, adaptive=1, **big)
    assert (p["rc"], p["wv_now"], p["admm"], p["need"]) == (0, 0, A_RL, NEED_WINDOW)
    p = plan(wv=1, adaptive=1, **big)
    assert (p["wv_now"], p["admm"]) == (1, A_WV_RL)                               # link-free: as before
    # the default: a link plan goes to the tier by the rule of a link-free one (704 problems on 256 CUs)
    assert plan(wv=2)["wv_min_live"] == 704 and plan(wv=2)["wv_now"] == 1 and plan(wv=2, batch=703)["wv_now"] == 0
    assert plan(wv=2, adaptive=1)["wv_min_live"] == INT_MAX
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    assert plan(wv=2, adaptive=1)["wv_now"] == 0 and plan(wv=1, adaptive=1)["wv_now"] == 1


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_oracle_ends_where_the_gpu_test_expects(case):
    """Status 1, or -3 for the contradicting rows, strictly below max_iter."""
    probs, w = case.build()
    for b in case.check:
        ref = o.solve(*probs[b], w=w[b])
        assert ref.info.status_val == case.status[b] and ref.info.iter < 100000, (b, ref.info.status_val, ref.info.iter)
        if case.status[b] == 1:
            T, d, r = case.shape
            nl = lc.n_links(case.builder, T, d)
            z = probs[b][2][d + T * r:d + T * r + nl] @ ref.x
            assert np.all(z <= case.vmax + 1e-3) and (case.builder is lc.one_sided or np.all(z >= -case.vmax - 1e-3))
