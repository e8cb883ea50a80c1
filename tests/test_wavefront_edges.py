"""The wavefront ADMM tier at the edges of its lane and block layout, without a GPU: the host plan
(csrc/wv_plan.cpp: wv_plan_build -- which instantiation, how many lanes per block, which shapes are refused) for the
patterns of tests/wv_cases.py, and the oracle's own verdict on every batch that tests/test_wavefront_edges_gpu.py solves
on the device: a comparison on a problem that stops on max_iter without being meant to would pin much less."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import wv_cases as wc
from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_plan import penalty_qp


def wv_plan(Pm, Am):
    """info = fits, block order, blocks, lanes per block, BS, NS, NV, NSTEP, LDS bytes, second single rows."""
    P = sp.triu(sp.csc_matrix(np.asarray(Pm) != 0), format="csc"); A = sp.csc_matrix(np.asarray(Am) != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); info = np.zeros(10, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int)]
    lib.sco_debug_wv_plan.argtypes = [C.POINTER(C.c_int)]
    assert lib.sco_debug_plan_build(P.shape[0], A.shape[0], ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert lib.sco_debug_wv_plan(ip(info)) == 0
    return [int(v) for v in info]


@pytest.mark.parametrize("shape,want,note", wc.ACCEPTED, ids=["%dx%dx%d %s" % (s + (n,)) for s, _, n in wc.ACCEPTED])
def test_plan_of_the_accepted_shapes(shape, want, note):
    T, d, r = shape
    P, q, A, l, u = penalty_qp(np.random.default_rng(0), T, d, r)
    info = wv_plan(P, A)
    assert tuple(info[:8]) == want, info
    assert info[8] <= 40 * 1024                         # four problems per CU
    assert info[9] == d                                 # the start pins are the second single rows
    # the lanes hold what the plan says they hold
    fits, bs, nb, lpb, BS, NS, NV, NSTEP = want
    assert nb <= 4 * (16 // lpb) and (lpb == 8 or nb > 4 * (16 // (lpb + 1)))
    assert NS * lpb >= r and NV * lpb >= bs and bs <= BS and nb // 2 <= NSTEP


@pytest.mark.parametrize("shape,why", wc.REFUSED, ids=["%dx%dx%d %s" % (s + (w,)) for s, w in wc.REFUSED])
def test_plan_refuses_the_shapes_next_to_each_edge(shape, why):
    P, q, A, l, u = penalty_qp(np.random.default_rng(0), *shape)
    info = wv_plan(P, A)
    assert info[0] == 0, info
    if "LDS" in why:
        assert info[8] == int(why.split()[1]) and info[8] > 40 * 1024


@pytest.mark.parametrize("T", wc.ARM_HORIZONS)
def test_default_arm_family_at_13_to_16_steps_lands_on_the_LPB0_kernel(T):
    """The benchmark's family with a shorter horizon: <7, 4, 3, 10> with four lanes per block -- the instantiation with
    run-time lanes per block (wv_launch)."""
    from oracle import arm_family as af
    from oracle import sco_ref as sr
    out = sr.penalty_sqp(sr.trajopt_flat(af.make_problem(0, T=T)), sr.SolverParams(max_qp_solves=2), record_qps=True)
    q = out.qps[1]
    info = wv_plan(q["P"], q["A"])
    assert tuple(info[:8]) == (1, 7, T, 4, 7, 4, 3, 10) and info[8] == 39744 and info[9] == 14, info


@pytest.mark.parametrize("case", [c for c in wc.CASES if c.plan is not None and not c.name.startswith("sweep")], ids=repr)
def test_plan_of_the_structural_variants(case):
    """Goal and middle pins, missing box rows, ragged hinge rows, an emptied timestep and dense P blocks are all accepted,
    on the instantiation of the plain pattern; only the count of second single rows (extra-row lanes) changes."""
    probs, w, check, tier = case.build()
    info = wv_plan(probs[0][0], probs[0][2])
    want = tuple(case.plan)
    if want[2] is None:
        want = want[:2] + (info[2],) + want[3:]
        assert info[2] in (6, 7)
    assert tuple(info[:8]) == want and info[8] <= 40 * 1024 and info[9] == case.n_extra, info
    for p in probs[1:]:                                  # one pattern per batch
        assert np.array_equal(p[2] != 0, probs[0][2] != 0) and np.array_equal(np.triu(p[0]) != 0, np.triu(probs[0][0]) != 0)


@pytest.mark.parametrize("case", wc.CASES, ids=repr)
def test_oracle_ends_where_the_gpu_test_expects(case):
    """Status 1 strictly below max_iter unless the case says otherwise (a certificate, or max_iter on purpose)."""
    probs, w, check, tier = case.build()
    max_iter = case.okw.get("max_iter", 100000)
    for k, b in enumerate(check):
        ref = o.solve(*probs[b], w=None if w is None else w[b], **case.okw)
        if case.status == "max_iter":
            assert (ref.info.status_val, ref.info.iter) == (-2, max_iter), (b, ref.info.status_val, ref.info.iter)
        else:
            want = case.status[k] if isinstance(case.status, (list, tuple)) else case.status
            assert ref.info.status_val == want and ref.info.iter < max_iter, (b, ref.info.status_val, ref.info.iter)


def test_every_edge_is_named_in_a_case():
    names = " | ".join(c.name for c in wc.CASES)
    for edge in ("LPB=0 kernel", "order 1", "order 8", "T=1:", "T=2:", "T=3:", "T=9 ", "T=17", "T=21", "goal pins", "middle pin",
                 "missing box row", "empty timestep", "dense P blocks", "settings", "batch of 1027", "mixed batch"):
        assert edge in names, edge
