"""Every ADMM kernel on every branch of the OSQP termination test: each batch of tests/term_cases.py under each of its settings
sets on each of its routes (row-local, wavefront, register-offset, sliced-ELL in its capped, looping and three-rows-per-thread
forms, generic, dense global memory, structured), with sco_debug_qp_tiers of a live handle as the proof of the route.
  - every problem against the oracle ADMM with the same settings: status, iteration count, x, y, residuals
    (test_qp_gpu._check; the oracle is solved once per batch and settings set and remembered);
  - the statuses against the literals of the table;
  - against the pattern's own route (term_cases.HOME): statuses and counts equal, |dx| < 1e-10 on the problems that are not
    certified infeasible;
  - on the wavefront route, the tier's iteration counter: the wavefront kernel itself ran -- and certified -- the problems
    its value test keeps.
tests/test_termination_tiers.py pins the table, the masks and the instantiations without a GPU."""
import numpy as np
import pytest

import term_cases as tc
from oracle import osqp_ref as o
from sco_py_amd import _lib
from test_qp_gpu import TOL, _check, _stack, _tiers
from test_wavefront_edges_gpu import wv_counted  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

_ORACLE = {}      # (problem, settings) -> the oracle's result
_HOME = {}        # (batch, settings set) -> (x, status, iterations) on the pattern's own route


@pytest.fixture(autouse=True)
def oracle_once(monkeypatch):
    """test_qp_gpu._check asks the oracle per call; the same problem under the same settings gets the same answer."""
    real = o.solve

    def solve(P, q, A, l, u, w=None, **okw):
        assert w is None
        key = (hash(tuple(np.ascontiguousarray(a).tobytes() for a in (P, q, A, l, u))), tuple(sorted(okw.items())))
        if key not in _ORACLE:
            _ORACLE[key] = real(P, q, A, l, u, **okw)
        return _ORACLE[key]

    monkeypatch.setattr(o, "solve", solve)


def _run(monkeypatch, batch, route, name, check):
    """The batch on `route` under settings set `name`: (x, status, iterations), compared with the oracle where check is None."""
    probs, _ = batch.build()
    okw = tc.SETTINGS[name]
    with monkeypatch.context() as mp:
        for k in tc.SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in tc.ROUTES[route][0].items():
            mp.setenv(k, v)
        n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
        assert _tiers(n, m, Pp, Pi, Ap, Ai) == tc.ROUTES[route][1][batch.pattern], (route, "the handle is not on this route")
        tol = dict(resid_tol=TOL) if batch.resid_parity else {}
        _, x, st, it = _check(probs, settings=_lib.default_qp_settings(**okw) if okw else None, check=check, **tol, **okw)
    return x, st, it


@pytest.mark.parametrize("batch,route,name", tc.RUNS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_termination_on_every_kernel(gpu, request, monkeypatch, batch, route, name):
    counted = request.getfixturevalue("wv_counted") if route == "wavefront" else None
    x, st, it = _run(monkeypatch, batch, route, name, None)
    assert [(int(s), int(i)) for s, i in zip(st, it)] == batch.want[name], (st, it)
    if route == "wavefront":
        assert len(counted) == 1
        assert counted[0] == int(it[batch.wv_kept].sum()), ("iterations run by the wavefront kernel", counted[0], it)
    home = tc.HOME[batch.pattern]
    if route == home:
        _HOME[(batch.name, name)] = (x, st, it)
        return
    if (batch.name, name) not in _HOME:
        _HOME[(batch.name, name)] = _run(monkeypatch, batch, home, name, [])
    x_h, st_h, it_h = _HOME[(batch.name, name)]
    assert np.array_equal(st, st_h) and np.array_equal(it, it_h), (st, st_h, it, it_h)
    ok = np.isin(st, (1, 2, -2))                        # (the iterate of a certified-infeasible problem is a ray, not an answer)
    print("|dx| per problem against", home, ["%.1e" % v for v in np.abs(x - x_h).max(axis=1)], "|x|", ["%.1e" % v for v in np.abs(x).max(axis=1)])
    assert np.abs(x[ok] - x_h[ok]).max(initial=0.0) < 1e-10, np.abs(x[ok] - x_h[ok]).max()
