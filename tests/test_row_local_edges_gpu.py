"""The row-local ADMM kernel (csrc/sco_admm_rl.hip) at the edges of its thread and tile plan: every batch of tests/rl_cases.py
with the wavefront tier off (SCO_QP_NO_WV=1) and row multiplicities on the hinge rows, on the tier the case names
(sco_debug_qp_tiers of a live handle), all problems against the oracle ADMM (status, iteration count, x, y, residuals:
test_qp_gpu._check), then again without the row-local kernel (SCO_QP_NO_RL=1) and with one lane per core column
(SCO_QP_RL_SPLIT=0: no helper lanes): same statuses and iteration counts, |dx| < 1e-10.  tests/test_row_local_edges.py pins
the plan -- the instantiation -- of each pattern under the same switches, and the oracle's verdict on each batch."""
import numpy as np
import pytest

import rl_cases as rc
from sco_py_amd import _lib
from test_qp_gpu import _check, _stack, _tiers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_row_local_kernel_at_the_edge(gpu, monkeypatch, case):
    for name in ("SCO_QP_NO_RL", "SCO_QP_RL_SPLIT", "SCO_QP_RL_ALIGNED", "SCO_QP_RL_CLOSED", "SCO_QP_RL_LAY8", "SCO_QP_FACTOR_CHOLESKY"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SCO_QP_NO_WV", "1")
    probs, w = case.build()
    n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
    assert _tiers(n, m, Pp, Pi, Ap, Ai) == case.mask
    settings = _lib.default_qp_settings(**case.okw) if case.okw else None
    tol = dict(resid_tol=1e-7) if case.okw.get("adaptive_rho") else {}     # (as test_adaptive_rho_matches_the_oracle_rule)
    _, x, st, it = _check(probs, w=w, settings=settings, **tol, **case.okw)
    assert list(st) == case.status(len(probs)), st
    ok = np.isin(st, (1, 2, -2))                        # (the iterate of a certified-infeasible problem is a ray, not an answer)
    for switch, value, mask in (("SCO_QP_NO_RL", "1", None), ("SCO_QP_RL_SPLIT", "0", case.unsplit_mask)):
        with monkeypatch.context() as mp:
            mp.setenv(switch, value)
            got = _tiers(n, m, Pp, Pi, Ap, Ai)
            assert (not got & 1) if mask is None else got == mask, (switch, got)
            _, x2, st2, it2 = _check(probs, w=w, settings=settings, check=[], **case.okw)
        assert np.array_equal(st, st2) and np.array_equal(it, it2), (switch, st, st2, it, it2)
        assert np.abs(x[ok] - x2[ok]).max(initial=0.0) < 1e-10, (switch, np.abs(x[ok] - x2[ok]).max())
