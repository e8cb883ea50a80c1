"""The table of tests/term_cases.py without a GPU: the oracle's (status, iteration count) of every problem under every settings
set, in float64 and in x87 extended precision; the conditions that make the table worth solving on the device (every status
occurs, every setting changes a count, the cone test has to say "no" somewhere); and which kernel -- which instantiation -- each
(pattern, route) pair runs: the sco_debug_plan_tiers mask, sco_debug_fast_plan and sco_debug_reg_plan under the route's
switches.  tests/test_termination_tiers_gpu.py solves the same table on every kernel."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import term_cases as tc
from oracle import osqp_ref as o
from sco_py_amd import _lib

_IP = C.POINTER(C.c_int)


def plans(Pm, Am, with_rl=False):
    """(mask, fast, reg[, rl]) of a pattern under the switches as they stand: sco_debug_plan_tiers, sco_debug_fast_plan (fits, TR,
    TC, capped dots, rows per thread, LDS bytes), sco_debug_reg_plan (fits, TR, TC, CW, RW, PX, dynamic LDS bytes) and, with
    with_rl, the eight fields of sco_debug_rl_plan."""
    P = sp.triu(sp.csc_matrix(np.asarray(Pm) != 0), format="csc"); A = sp.csc_matrix(np.asarray(Am) != 0)
    P.sort_indices(); A.sort_indices()
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(_IP)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (P.indptr, P.indices, A.indptr, A.indices))
    sizes = np.zeros(16, dtype=np.int32); fast = np.zeros(8, dtype=np.int32); reg = np.zeros(8, dtype=np.int32); mask = np.zeros(1, dtype=np.int32)
    lib.sco_debug_plan_build.argtypes = [C.c_int, C.c_int] + [_IP] * 4 + [C.c_int, _IP]
    lib.sco_debug_fast_plan.argtypes = [_IP]; lib.sco_debug_reg_plan.argtypes = [_IP]
    assert lib.sco_debug_plan_build(P.shape[0], A.shape[0], ip(Pp), ip(Pi), ip(Ap), ip(Ai), 1, ip(sizes)) == 0
    assert lib.sco_debug_fast_plan(ip(fast)) == 0 and lib.sco_debug_reg_plan(ip(reg)) == 0
    assert lib.sco_debug_plan_tiers(ip(mask)) == 0
    out = int(mask[0]), tuple(int(v) for v in fast[:6]), tuple(int(v) for v in reg[:7])
    if with_rl:                                          # sco_debug_rl_plan: fits, CW, TR, TC, dynamic LDS bytes, closed, layout, NS
        rl = np.zeros(8, dtype=np.int32)
        lib.sco_debug_rl_plan.argtypes = [_IP]
        assert lib.sco_debug_rl_plan(ip(rl)) == 0
        out += (tuple(int(v) for v in rl),)
    return out


@pytest.fixture
def switches(monkeypatch):
    for name in tc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _pattern(P, A):
    return np.triu(P) != 0, A != 0


@pytest.mark.parametrize("batch", tc.BATCHES, ids=repr)
def test_one_pattern_per_batch_and_problem_0_holds_it(batch):
    probs, kinds = batch.build()
    assert len(probs) == len(kinds) and all(len(w) == len(probs) for w in batch.want.values())
    P0, A0 = _pattern(probs[0][0], probs[0][2])
    for P, q, A, l, u in probs[1:]:
        Pk, Ak = _pattern(P, A)
        assert not (Pk & ~P0).any() and not (Ak & ~A0).any()          # (explicit zeros are fine, new non-zeros are not)
        assert np.all(l <= u)
    m = len(probs[0][3])
    assert m == {"P1 6x3x4": 69, "P2 6x3x20": 261, "P3 wide rows": 20, "P4 m=1140": 1140, "P4 m=1024": 1024, "P4 m=1025": 1025}[batch.name]


@pytest.mark.parametrize("batch,name", [(b, s) for b in tc.BATCHES for s in b.sets], ids=lambda v: v if isinstance(v, str) else repr(v))
def test_oracle_reproduces_the_table_in_both_precisions(batch, name):
    """A seed for which the float64 and the x87 route differ would make a device count a matter of rounding: there is none."""
    probs, _ = batch.build()
    okw = tc.SETTINGS[name]
    cap = min(okw.get("max_iter", tc.MAX_ORACLE_ITER), tc.MAX_ORACLE_ITER)
    for extended in (False, True):
        got = [(r.info.status_val, r.info.iter) for r in (o.solve(*p, extended=extended, **okw) for p in probs)]
        assert got == batch.want[name], (extended, got)
    assert all(it <= cap for _, it in batch.want[name])


def _uncapped(batch):
    return [s for s in batch.sets if "max_iter" not in tc.SETTINGS[s]]


def test_every_status_occurs_and_every_twin_converges():
    seen = {st for b in tc.BATCHES for s in b.sets for st in b.status(s)}
    assert seen == {1, 2, 3, 4, -2, -3, -4}
    for b, n_cuts in zip(tc.BATCHES[:2], (3, 4)):                              # the `approximate` branch at the cuts: all four
        cuts = [s for s in b.sets if "max_iter=" in s and s != "max_iter=213" and "check_termination" not in s]
        assert len(cuts) == n_cuts and {2, 3, 4, -2} <= {st for s in cuts for st in b.status(s)}
    # status 2 on the looping sliced-ELL form and the structured form (P2's routes) and on the three-rows-per-thread form (P4)
    assert 2 in tc.BATCHES[1].status("scaling=0 max_iter=3625") and tc.BATCHES[3].status("max_iter=450")[:2] == [2, 2]
    twins = 0
    for b in tc.BATCHES:
        kinds = b.build()[1]
        for s in _uncapped(b):
            for k, (st, it) in zip(kinds, b.want[s]):
                assert st == {"base": 1, "twin": 1, "prim": -3, "dual": -4}[k], (b, s, k, st)
                twins += k == "twin"
    assert twins == 2 * (9 + 3)                                                # two per uncapped settings set of P1 and of P2


def _counts(b, s, kind):
    return [it for k, (_, it) in zip(b.build()[1], b.want[s]) if k == kind]


def test_every_setting_changes_a_count():
    """A kernel that ignored eps_prim_inf, eps_dual_inf, scaling, alpha or check_termination would still match the default
    column; it must not match these."""
    p1, p2 = tc.BATCHES[:2]
    for b, names in ((p1, ("eps_inf=1e-2", "eps_inf=1e-6")), (p2, ("eps_inf=1e-2",))):
        for s in names:
            for kind in ("prim", "dual"):
                assert _counts(b, s, kind) != _counts(b, "default", kind), (b, s, kind)
            for kind in ("base", "twin"):                                      # ... and touches nothing else
                assert _counts(b, s, kind) == _counts(b, "default", kind)
    for b in tc.BATCHES:
        if "scaling=0" in b.sets:
            assert all(a != d for a, d in zip(_counts(b, "scaling=0", "base"), _counts(b, "default", "base"))), b
    for s in ("scaling=3", "alpha=1.0", "check_termination=1"):
        assert p1.want[s] != p1.want["default"]
    # each tolerance moves its own certificate and not the other: one tolerance read in the other's place shows in the sets
    # that hold them apart
    for kind, own in (("prim", "eps_prim_inf"), ("dual", "eps_dual_inf")):
        for s in ("eps_prim_inf=1e-2 eps_dual_inf=1e-6", "eps_prim_inf=1e-6 eps_dual_inf=1e-2"):
            same = "eps_inf=1e-2" if tc.SETTINGS[s][own] == 1e-2 else "eps_inf=1e-6"
            other = "eps_inf=1e-6" if same == "eps_inf=1e-2" else "eps_inf=1e-2"
            assert _counts(p1, s, kind) == _counts(p1, same, kind) != _counts(p1, other, kind)
    # the three-rows-per-thread form: the slower dual problem of P4 moves with eps_dual_inf (its first one is certified at the
    # first check whatever the tolerance)
    p4 = tc.BATCHES[3]
    assert p4.want["default"][4] == (-4, 125) and p4.want["eps_inf=1e-2"][4] == (-4, 25)
    # check_termination = 0: one test at the cap; max_iter = 213 ends five problems between two checks, one of them converged
    assert {it for _, it in p1.want["check_termination=0 max_iter=150"]} == {150}
    assert 213 % 25 and p1.want["max_iter=213"].count((-2, 213)) == 4 and p1.want["max_iter=213"].count((1, 213)) == 1


def test_iterates_that_a_cut_stops_are_still_comparable():
    """The GPU file compares x across routes at 1e-10 on every problem that is not certified infeasible -- the dual problems a
    cut stops on their ray included.  The table only holds cuts at which the oracle's own two precisions agree to half of that
    on every such iterate (max_iter = 575 on P2 would give 1.1e-10, 4013 on P1 1e-8)."""
    worst = 0.0
    for b in tc.BATCHES:
        probs, _ = b.build()
        for s in b.sets:
            for p, (st, _) in zip(probs, b.want[s]):
                if st == -2:
                    worst = max(worst, np.abs(o.solve(*p, **tc.SETTINGS[s]).x - o.solve(*p, extended=True, **tc.SETTINGS[s]).x).max())
    assert 0.0 < worst < 0.5e-10, worst
    # ... and the cuts past 300 iterations leave no dual problem running
    for b in tc.BATCHES:
        for s in b.sets:
            if tc.SETTINGS[s].get("max_iter", 0) > 300:
                assert all(st in (-4, 4) for k, st in zip(b.build()[1], b.status(s)) if k == "dual"), (b, s)


def test_settings_sets_of_every_pattern():
    p1, p2, p3, p4, e0, e1 = tc.BATCHES
    assert len(p1.sets) == 14 and set(p1.sets) | set(p2.sets) | set(p4.sets) == set(tc.SETTINGS)
    assert p2.sets == ["default", "eps_inf=1e-2", "scaling=0", "max_iter=150", "max_iter=300", "max_iter=27000", "scaling=0 max_iter=3625"]
    assert p3.sets == tc.FEW and p4.sets == tc.FEW + ["max_iter=450"] and e0.sets == ["default"] and e1.sets == ["default"]
    assert p1.wv_kept is not None and {p1.build()[1][k] for k in p1.wv_kept} >= {"prim", "dual"}


@pytest.mark.parametrize("batch", tc.BATCHES, ids=repr)
def test_mask_of_every_route(switches, batch):
    P, _, A = batch.build()[0][0][:3]
    for route, (sw, masks) in tc.ROUTES.items():
        with switches.context() as mp:
            for k, v in sw.items():
                mp.setenv(k, v)
            mask = plans(P, A)[0]
        if route in batch.routes:
            assert mask == masks[batch.pattern], (route, mask)
        elif (batch.pattern, route) in tc.NOT_A_ROUTE:
            assert mask == tc.NOT_A_ROUTE[(batch.pattern, route)], (route, mask)
    assert set(batch.routes) == {r for r, (_, masks) in tc.ROUTES.items() if batch.pattern in masks}
    assert tc.HOME[batch.pattern] in batch.routes


@pytest.mark.parametrize("batch", tc.BATCHES, ids=repr)
def test_instantiation_of_the_sliced_ell_and_register_offset_kernels(switches, batch):
    """The mask says 4 for the capped, the looping and the three-rows-per-thread form of qp_admm_fast_kernel alike: the plan
    says which one runs.  Every accepted (TR, TC) names a case of fast_launch / reg_launch."""
    P, _, A = batch.build()[0][0][:3]
    key = batch.name if batch.pattern == "P4" else batch.pattern
    _, fast, reg, rl = plans(P, A, with_rl=True)
    assert fast == tc.FAST_PLAN[key] and fast[5] <= 160 * 1024, fast
    assert fast[1:5] in tc.FAST_INSTANTIATIONS
    assert fast[4] == (3 if len(batch.build()[0][0][3]) > 1024 else 2)
    if key in tc.REG_PLAN:
        assert reg == tc.REG_PLAN[key] and reg[1:6] in tc.REG_INSTANTIATIONS, reg
        assert reg[6] + 44032 <= 160 * 1024                                   # (static LDS of qp_admm_reg_kernel on top)
    else:
        assert reg[0] == 0, reg
    if key in tc.RL_PLAN:
        assert rl == tc.RL_PLAN[key] and rl[4] + 40 * 1024 <= 160 * 1024, rl
    else:
        assert rl[0] == 0, rl


def test_rows_per_thread_rule_and_accepted_tiles_over_a_sweep(switches):
    """penalty_qp shapes across the tiles of both kernels: whatever the planners accept is an instantiation, and the rows-per-
    thread rule turns at m = 1024 -> 1025 (fast_plan_build refuses m > 1536)."""
    seen_fast, seen_reg = set(), set()
    for T, d, r in ((6, 3, 4), (16, 2, 1), (11, 3, 1), (13, 5, 1), (16, 8, 1), (18, 8, 1), (20, 8, 1), (20, 7, 10), (26, 6, 1), (60, 1, 7), (64, 1, 7)):
        P, _, A, l, _ = tc.penalty_qp(np.random.default_rng(0), T, d, r)
        _, fast, reg = plans(P, A)
        if fast[0]:
            assert fast[1:5] in tc.FAST_INSTANTIATIONS and fast[4] == (3 if len(l) > 1024 else 2), (T, d, r, fast)
            seen_fast.add(fast[1:3])
        if reg[0]:
            assert reg[1:6] in tc.REG_INSTANTIATIONS, (T, d, r, reg)
            seen_reg.add(reg[1:3])
    assert seen_fast == set(tc.TILES) and seen_reg >= {(1, 2), (5, 9)}, (seen_fast, seen_reg)
