"""The wavefront ADMM kernel (csrc/sco_admm_wv.hip) at the edges of its lane and block layout: every batch of
tests/wv_cases.py on the tier against the oracle ADMM (status, iteration count, x, y, residuals: test_qp_gpu._check) and
against the row-local kernel (same statuses and counts, |dx| < 1e-10), with the tier's own iteration counter as the proof
that the wavefront kernel did the work.  tests/test_wavefront_edges.py holds the plan of each pattern and the oracle's
verdict on each batch."""
import ctypes as C

import numpy as np
import pytest

import wv_cases as wc
from sco_py_amd import _lib
from test_qp_gpu import _check, _stack, _tiers

pytestmark = pytest.mark.gpu


def _wv_iters(qp):
    lib = _lib.load()
    lib.sco_debug_qp_wv_iters.restype = C.c_int
    lib.sco_debug_qp_wv_iters.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    out = C.c_ulonglong(0)
    assert lib.sco_debug_qp_wv_iters(qp._h, C.byref(out)) == 0
    return int(out.value)


@pytest.fixture
def wv_counted(monkeypatch):
    """Every BatchedQP.solve appends the iterations the wavefront kernel ran during it (nothing in a plain QP solve resets
    the counter: the difference around the solve is this solve's)."""
    log = []
    real = _lib.BatchedQP.solve

    def solve(self, settings=None):
        before = _wv_iters(self)
        out = real(self, settings)
        log.append(_wv_iters(self) - before)
        return out

    monkeypatch.setattr(_lib.BatchedQP, "solve", solve)
    return log


@pytest.mark.parametrize("case", wc.CASES, ids=repr)
def test_wavefront_kernel_at_the_edge(gpu, monkeypatch, wv_counted, case):
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    probs, w, check, tier = case.build()
    n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
    assert _tiers(n, m, Pp, Pi, Ap, Ai) & 32, "pattern did not land on the wavefront tier"
    settings = _lib.default_qp_settings(**case.okw) if case.okw else None
    _, x_wv, st_wv, it_wv = _check(probs, w=w, settings=settings, check=check, **case.okw)
    assert len(wv_counted) == 1
    assert wv_counted[0] == int(it_wv[tier].sum()), ("iterations run by the wavefront kernel", wv_counted[0], it_wv)
    if case.status == "max_iter":
        assert np.all(st_wv == -2) and np.all(it_wv == case.okw["max_iter"])
    elif not isinstance(case.status, (list, tuple)):
        assert np.all(st_wv[check] == case.status), st_wv
    monkeypatch.setenv("SCO_QP_NO_WV", "1")
    assert not _tiers(n, m, Pp, Pi, Ap, Ai) & 32
    _, x_rl, st_rl, it_rl = _check(probs, w=w, settings=settings, check=[], **case.okw)
    assert wv_counted[1] == 0
    assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
    ok = np.isin(st_wv, (1, 2, -2))                     # (the iterate of a certified-infeasible problem is a ray, not an answer)
    assert np.abs(x_wv[ok] - x_rl[ok]).max(initial=0.0) < 1e-10, np.abs(x_wv[ok] - x_rl[ok]).max()


@pytest.mark.parametrize("shape,seed", wc.REPEAT, ids=["%dx%dx%d" % s for s, _ in wc.REPEAT])
def test_wavefront_kernel_is_run_to_run_deterministic(gpu, monkeypatch, shape, seed):
    """One wavefront per problem, every sum in a fixed lane order: two solves of a batch give identical bits in x, y and the
    iteration counts (<7,4,3,10,3> at 7 x 20 and the run-time lanes-per-block kernel at 7 x 14)."""
    from test_qp_plan import penalty_qp
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    rng = np.random.default_rng(seed)
    probs = [penalty_qp(rng, *shape) for _ in range(6)]
    w = wc.hinge_weights(rng, probs)
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    outs = []
    for _ in range(2):
        qp = _lib.BatchedQP(6, n, m, Pp, Pi, Ap, Ai)
        try:
            qp.load(Pval, q, Aval, l, u, w)
            outs.append(qp.solve())
            assert _wv_iters(qp) == int(outs[-1][3].sum())
        finally:
            qp.close()
    (x0, y0, s0, i0, _), (x1, y1, s1, i1, _) = outs
    assert np.all(s0 == 1)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)
    _check(probs[:2], w=w[:2])                       # and they are the oracle's answers


@pytest.mark.parametrize("T", wc.ARM_HORIZONS, ids=["7x%d LPB=0 kernel" % T for T in wc.ARM_HORIZONS])
def test_arm_family_on_the_LPB0_kernel_through_the_device_loop(gpu, monkeypatch, T):
    """The default arm family with 13, 14 and 16 timesteps: every round of the SQP loop forced onto the wavefront tier, which
    runs these horizons on the instantiation with run-time lanes per block.  Decisions, QP statuses, iteration counts and
    trajectories of the flat oracle, time slices of 300."""
    from oracle import arm_family as af
    from sco_py_amd import batch as sb
    from test_sqp_gpu import _compare
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    lib = _lib.load()
    lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
    nb = 6
    a, probs = af.make_batch(nb, T=T)
    with sb.TrajOptBatch(nb, a["d"], a["T"], a["K"], a["O"]) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"])
        tb.solve(_lib.default_sqp_params(admm_slice=300))
        res = tb.fetch(); res.trace = tb.trace(); res.timing = tb.last_timing()
        rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    assert rounds > 0
    _compare(res, probs, range(0, nb, 2))
