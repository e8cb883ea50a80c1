"""The tiers a live handle runs are the ones the host-only chooser names (qp_choose_tiers, csrc/qp_tier_choice.cpp): sco_debug_qp_tiers
of a handle = sco_debug_plan_tiers of its pattern, under every route of tests/test_qp_launch_plan.py.  Handles are created
and closed; only the last case solves."""
import ctypes as C

import numpy as np
import pytest

from sco_py_amd import _lib
from test_qp_launch_plan import ROUTES, dense_row_pattern, penalty_pattern, plan_tiers, set_route
from test_qp_plan import _patterns, penalty_qp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name, batch", [("3x6", 4), ("dense rows", 3)])
def test_a_handle_runs_the_tiers_the_chooser_names(gpu, monkeypatch, name, batch, route):
    pattern = penalty_pattern(6, 3, 4) if name == "3x6" else dense_row_pattern()
    set_route(monkeypatch, route)
    want = plan_tiers(pattern)
    lib = _lib.load()
    lib.sco_debug_qp_tiers.restype = C.c_int; lib.sco_debug_qp_tiers.argtypes = [C.c_void_p]
    qp = _lib.BatchedQP(batch, *pattern)
    try:
        assert lib.sco_debug_qp_tiers(qp._h) == want
    finally:
        qp.close()


def test_adaptive_rho_on_the_dense_global_memory_form_is_refused(gpu, monkeypatch):
    set_route(monkeypatch, "FORCE_BIG+NO_BT")
    rng = np.random.default_rng(6)
    probs = [penalty_qp(rng, 6, 3, 4) for _ in range(4)]
    Pp, Pi, _, Ap, Ai, _ = _patterns(probs[0][0], probs[0][2])
    vals = [_patterns(P, A) for P, q, A, l, u in probs]
    qp = _lib.BatchedQP(4, len(probs[0][1]), len(probs[0][3]), Pp, Pi, Ap, Ai)
    try:
        qp.load(np.array([v[2] for v in vals]), np.array([p[1] for p in probs]), np.array([v[5] for v in vals]),
                np.array([p[3] for p in probs]), np.array([p[4] for p in probs]))
        with pytest.raises(_lib.ScoHipError) as e:
            qp.solve(_lib.default_qp_settings(adaptive_rho=1))
        assert e.value.code == -5
        assert "adaptive_rho: the dense form of the global-memory tier cannot park a solve" in str(e.value)
    finally:
        qp.close()
