"""The row-local ADMM tier at the edges of its thread and tile plan, without a GPU: the host plan (csrc/rl_plan.cpp:
rl_plan_build -- which instantiation of qp_admm_rl_kernel, which patterns are refused) and the tier choice
(csrc/qp_tier_choice.cpp) for the patterns of tests/rl_cases.py, that every plan the planner accepts names an instantiation
the launcher has, and the oracle's own verdict on every batch that tests/test_row_local_edges_gpu.py solves on the device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import rl_cases as rc
from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_plan import penalty_qp

_IP = C.POINTER(C.c_int)


def rl_plan(Pm, Am):
    """(info, mask): info = fits, CW, TR, TC, dynamic LDS bytes, closed, layout (1 aligned, 2 lay8), NS of sco_debug_rl_plan,
    mask of sco_debug_plan_tiers, both under the SCO_QP_* switches as they stand."""
    P = sp.triu(sp.csc_matrix(np.asarray(Pm) != 0), format="csc"); A = sp.csc_matrix(np.asarray(Am) != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(_IP)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); info = np.zeros(8, dtype=np.int32); mask = np.zeros(1, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [_IP] * 4 + [C.c_int, _IP]
    lib.sco_debug_rl_plan.argtypes = [_IP]
    assert lib.sco_debug_plan_build(P.shape[0], A.shape[0], ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert lib.sco_debug_rl_plan(ip(info)) == 0
    assert lib.sco_debug_plan_tiers(ip(mask)) == 0
    return [int(v) for v in info], int(mask[0])


def _tuple(info):
    return (info[0], info[1], info[2], info[3], info[7]) if info[0] else (0,)


def _instantiation(info):
    """(TR, TC, CW, NS, layout as the kernel's LAY: 0 open, 1 lay8, 2 aligned)."""
    return info[2], info[3], info[1], info[7], {0: 0, 1: 2, 2: 1}[info[6]]


@pytest.fixture
def switches(monkeypatch):
    """The wavefront tier off (the GPU file's setting), every other switch of the tier choice unset."""
    for name in ("SCO_QP_NO_RL", "SCO_QP_NO_REG", "SCO_QP_NO_FAST", "SCO_QP_NO_ELIM", "SCO_QP_FORCE_BIG", "SCO_QP_NO_BT", "SCO_QP_FACTOR_CHOLESKY",
                 "SCO_QP_RL_SPLIT", "SCO_QP_RL_ALIGNED", "SCO_QP_RL_CLOSED", "SCO_QP_RL_LAY8"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SCO_QP_NO_WV", "1")
    return monkeypatch


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_plan_and_tier_of_every_case(switches, case):
    probs, w = case.build()
    assert 3 <= len(probs) <= 4
    for p in probs[1:]:                                  # one pattern per batch
        assert np.array_equal(p[2] != 0, probs[0][2] != 0) and np.array_equal(np.triu(p[0]) != 0, np.triu(probs[0][0]) != 0)
    info, mask = rl_plan(probs[0][0], probs[0][2])
    assert _tuple(info) == case.plan and mask == case.mask, (info, mask)
    assert bool(mask & 1) == bool(info[0])               # the tier choice takes the row-local plan whenever there is one
    if info[0]:
        assert _instantiation(info) in rc.INSTANTIATIONS and info[4] + 40 * 1024 <= 160 * 1024
    switches.setenv("SCO_QP_RL_SPLIT", "0")
    info0, mask0 = rl_plan(probs[0][0], probs[0][2])
    assert mask0 == case.unsplit_mask and _tuple(info0) == case.unsplit, (info0, mask0)
    switches.setenv("SCO_QP_NO_RL", "1")
    assert not rl_plan(probs[0][0], probs[0][2])[1] & 1


def test_shared_lanes_are_where_the_cases_say(switches):
    """Eliminated variables on the threads 0 .. n_e - 1, core columns on 512 - 2 n_c .. 511: the lanes in the case's name."""
    import re
    seen = 0
    for case in rc.CASES:
        m = re.match(r"shared lanes: (\d+)x(\d+)x(\d+).* lanes (\d+)\.\.(\d+)", case.name)
        if not m:
            continue
        T, d, r, lo, hi = (int(v) for v in m.groups())
        assert (lo, hi) == (512 - 2 * T * d, T * r - 1) and lo <= hi
        seen += 1
    assert seen == 3
    # ... and r = 21 at 7 x 20 is past the on-chip tiers (the setup's LDS request): r = 20 is the largest with shared lanes
    P, q, A, l, u = penalty_qp(np.random.default_rng(0), 20, 7, 21)
    assert rl_plan(P, A)[1] == rc.STRUCTURED


def test_every_accepted_plan_has_an_instantiation(switches):
    """rl_launch dispatches on (TR, TC, CW, NS, layout); a plan outside rc.INSTANTIATIONS would be created and then fail
    every solve with "rl_launch: unsupported tile".  Over the cases and over a sweep of penalty_qp shapes that need a third row
    slot at every TR, under the default plan and the three opt-in ones.  (The planner once fell back to three row slots at
    any tile: (100, 1, 5) gave <4,8> NS 3 and (50, 1, 10) <2,4> NS 3, both with mask 1.)"""
    patterns = [(c.name, c.build()[0][0]) for c in rc.CASES]
    three = {}
    for shape in rc.ns3_sweep():
        T, d, r = shape
        assert 400 <= T * r <= 512
        patterns.append((shape, penalty_qp(np.random.default_rng(0), T, d, r)))
        if rc.needs_three_slots(T, d, r):
            three.setdefault((T * d + 31) // 32, []).append(shape)
    assert sorted(three) == [1, 2, 3, 4, 5], three             # the sweep asks for a third row slot at every TR
    bad, ran, ns3 = [], set(), set()
    for switch in (None, "SCO_QP_RL_SPLIT", "SCO_QP_RL_ALIGNED", "SCO_QP_RL_LAY8"):
        with switches.context() as mp:
            if switch:
                mp.setenv(switch, "0" if switch.endswith("SPLIT") else "1")
            for name, prob in patterns:
                info, mask = rl_plan(prob[0], prob[2])
                if not info[0]:
                    assert not mask & 1
                    continue
                ran.add(_instantiation(info))
                if info[7] == 3 and not switch:
                    ns3.add(name)
                if _instantiation(info) not in rc.INSTANTIATIONS:
                    bad.append((name, switch, info, mask))
    assert not bad, bad
    # the sweep is not vacuous: three-slot plans are accepted where the kernel exists, and the opt-in layouts were built
    assert ns3 & set(three[5]) and not ns3 & set(sum((three[k] for k in (1, 2, 3, 4)), []))
    assert {(3, 18, 12, 2, 1), (3, 18, 12, 2, 2), (5, 9, 20, 3, 0), (5, 10, 20, 3, 0), (5, 9, 16, 2, 0), (5, 10, 16, 2, 0)} <= ran
    assert {(TR, TC, 12, 2, 0) for TR, TC in rc.SIX_TILES} | {(5, 9, 12, 3, 0), (5, 10, 12, 3, 0)} <= ran


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_oracle_ends_where_the_gpu_test_expects(case):
    """Every problem gets the status the case names, within MAX_ORACLE_ITER iterations: a comparison on a problem that stops
    on max_iter without being meant to would pin much less, and would take the GPU test long."""
    probs, w = case.build()
    want = case.status(len(probs))
    for b, prob in enumerate(probs):
        ref = o.solve(*prob, w=None if w is None else w[b], **case.okw)
        assert ref.info.status_val == want[b] and ref.info.iter <= rc.MAX_ORACLE_ITER, (b, ref.info.status_val, ref.info.iter)
    if "infeasible" in case.name:
        assert sorted(want) == [-3, 1, 1, 1]


def test_every_edge_is_named_in_a_case():
    names = " | ".join(c.name for c in rc.CASES)
    for edge in ["order of <%d,%d>" % t for t in rc.SIX_TILES] + [
            "core order 157", "core order 160", "core order 161", "CW 16", "wide rows refused", "<5,9> NS 3", "<5,10> NS 3", "CW 20",
            "100x1x5", "50x1x10", "shared lanes: 20x7x12", "shared lanes: 20x7x20", "shared lanes: 32x1x15 on <1,2>", "no hinge rows",
            "no box rows", "without a row", "no core variable", "no eliminated variable", "adaptive rho: 32x1x15 on <1,2>",
            "adaptive rho: 26x6x1 on <5,10>", "adaptive rho: 65x2x7 on <5,9> NS 3"]:
        assert edge in names, edge
    for tile in rc.SIX_TILES:                            # first and last order of every tile
        assert "first order of <%d,%d>" % tile in names or tile == (1, 2)
        assert "last order of <%d,%d>" % tile in names
    assert len({c.name for c in rc.CASES}) == len(rc.CASES)
