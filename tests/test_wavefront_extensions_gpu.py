"""The opt-in extensions on the wavefront ADMM tier (csrc/sco_admm_wv.hip): warm start (sco_qp_settings.warm_start,
sco_sqp_params.warm_start_qps) and adaptive rho (sco_qp_settings.adaptive_rho, the ADAPT instantiation of the kernel).

Every test sends small batches to the tier (SCO_WV_MIN_PER_CU=0) and reads the tier's own iteration counter, or the SQP
loop's count of wavefront rounds, as the proof that the wavefront kernel did the work.  Adaptive rho is checked against the
CPU oracle with the same rule (test_qp_gpu._check: status, iteration count, rho updates, rho estimate, x, y, residuals);
the oracle has no warm start, there the referee is the row-local kernel (SCO_QP_NO_WV=1).  The batches are the four of
tests/wv_ext_cases.py, one per kind of instantiation; tests/test_wavefront_extensions.py holds the oracle's side."""
import ctypes as C

import numpy as np
import pytest

import wv_cases as wc
import wv_ext_cases as wx
from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib, batch as sb
from test_qp_gpu import _check, _stack, _tiers
from test_wavefront_edges_gpu import _wv_iters, wv_counted      # noqa: F401  (wv_counted: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def on_tier(monkeypatch):
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    return monkeypatch


def _adaptive(probs, w, counted, tier=None, check=None, **kw):
    """One adaptive-rho solve of the batch against the oracle; the wavefront counter must hold exactly the iterations of the
    problems in `tier` (default: all)."""
    n, m, Pp, Pi, Ap, Ai, *_ = _stack(probs)
    assert _tiers(n, m, Pp, Pi, Ap, Ai) & 32, "pattern did not land on the wavefront tier"
    k0 = len(counted)
    _, x, st, it = _check(probs, w=w, settings=_lib.default_qp_settings(adaptive_rho=1, **kw), adaptive_rho=1, expand_dups=0,
                          resid_tol=1e-7, check=check, **kw)
    assert len(counted) == k0 + 1
    took = it if tier is None else it[list(tier)]
    assert counted[k0] == int(took.sum()), ("iterations run by the wavefront kernel", counted[k0], it)
    return x, st, it


# ---- 1. adaptive rho against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", wx.BATCHES, ids=wx.IDS)
def test_adaptive_rho_on_the_wavefront_tier_matches_the_oracle(gpu, on_tier, wv_counted, shape, seed):
    probs, w = wx.build(shape, seed)
    ref = wx.oracle_adaptive(shape, seed)
    assert np.all(ref[:, 0] == 1) and (ref[:, 2] >= 1).any(), ref        # some problem parks, refactors and resumes
    _, st, it = _adaptive(probs, w, wv_counted)
    assert np.array_equal(st, ref[:, 0]) and np.array_equal(it, ref[:, 1])


@pytest.mark.parametrize("kw", [dict(adaptive_rho_interval=50), dict(adaptive_rho_interval=250, adaptive_rho_tolerance=2.0)],
                         ids=["interval 50", "interval 250, tolerance 2"])
def test_adaptive_rho_interval_and_tolerance_on_the_wavefront_tier(gpu, on_tier, wv_counted, kw):
    probs, w = wx.build(*wx.BATCHES[3])
    _adaptive(probs, w, wv_counted, **kw)


# ---- 2. warm start against the row-local kernel ------------------------------------------------------------------------
def _warm_sequence(probs, w, counted):
    """The sequence of test_qp_gpu.test_warm_start_is_opt_in_and_converges_to_the_same_answer: cold, warm, a perturbed q cold,
    the perturbed q warm from the old QP's solution.  Returns the four (x, status, iterations) and the wavefront counts."""
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    q2 = q + 0.05 * np.random.default_rng(11).standard_normal(q.shape)
    warm = _lib.default_qp_settings(warm_start=1)
    k0 = len(counted)
    qp = _lib.BatchedQP(len(probs), n, m, Pp, Pi, Ap, Ai)
    try:
        qp.load(Pval, q, Aval, l, u, w)
        outs = [qp.solve(), qp.solve(warm)]
        qp.load(Pval, q2, Aval, l, u, w)
        outs.append(qp.solve())
        qp.load(Pval, q, Aval, l, u, w); qp.solve()                      # previous solution = the old QP's
        qp.load(Pval, q2, Aval, l, u, w)
        outs.append(qp.solve(warm))
    finally:
        qp.close()
    cnt = counted[k0:]
    return [(o[0], o[2], o[3]) for o in outs], [cnt[0], cnt[1], cnt[2], cnt[4]]


@pytest.mark.parametrize("shape,seed", wx.BATCHES, ids=wx.IDS)
def test_warm_start_on_the_wavefront_tier_agrees_with_the_row_local_kernel(gpu, on_tier, wv_counted, shape, seed):
    probs, w = wx.build(shape, seed)
    wv, cnt = _warm_sequence(probs, w, wv_counted)
    for (x, st, it), c in zip(wv, cnt):
        assert c == int(it.sum()), ("iterations run by the wavefront kernel", c, it)      # the warm solves included
    (x0, st0, it0), (xw, stw, itw), (xc, stc, itc), (xw2, stw2, itw2) = wv
    assert np.all(st0 == 1) and np.all(stw == 1) and np.all(itw <= it0) and itw.sum() < 0.5 * it0.sum(), (it0, itw)
    assert np.abs(xw - x0).max() < 1e-5
    assert np.array_equal(stc, stw2) and np.abs(xw2 - xc).max() < 1e-4
    assert itw2.sum() < itc.sum(), (itc, itw2)
    on_tier.setenv("SCO_QP_NO_WV", "1")
    rl, cnt = _warm_sequence(probs, w, wv_counted)
    assert cnt == [0, 0, 0, 0]
    for (x_wv, st_wv, it_wv), (x_rl, st_rl, it_rl) in zip(wv, rl):
        assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl), (st_wv, st_rl, it_wv, it_rl)
        assert np.abs(x_wv - x_rl).max() < 1e-10, np.abs(x_wv - x_rl).max()


# ---- 3. park and resume ------------------------------------------------------------------------------------------------
def test_adaptive_rho_parks_and_resumes_like_the_row_local_kernel(gpu, on_tier, wv_counted):
    """The QP layer's adaptive loop parks a solve at every rho change: the wavefront kernel parks, the factorisation runs
    again on the new rho and the kernel resumes, for as many launches as the batch has rho changes.  Statuses, iteration
    counts and rho updates of a run on the row-local ADAPT kernel, which resumes from the same parked layout."""
    probs, w = wx.build(*wx.BATCHES[2])
    ref = wx.oracle_adaptive(*wx.BATCHES[2])
    assert (ref[:, 2] >= 1).any()
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    runs = []
    for no_wv in ("0", "1"):
        on_tier.setenv("SCO_QP_NO_WV", no_wv)
        qp = _lib.BatchedQP(len(probs), n, m, Pp, Pi, Ap, Ai)
        try:
            qp.load(Pval, q, Aval, l, u, w)
            x, y, st, it, _ = qp.solve(_lib.default_qp_settings(adaptive_rho=1))
            rho, nupd = qp.adaptive_info()
        finally:
            qp.close()
        runs.append((x, st, it, rho, nupd))
    (x_wv, st_wv, it_wv, rho_wv, n_wv), (x_rl, st_rl, it_rl, rho_rl, n_rl) = runs
    assert wv_counted == [int(it_wv.sum()), 0]
    assert np.array_equal(n_wv, ref[:, 2]) and n_wv.max() >= 1
    assert np.array_equal(st_wv, st_rl) and np.array_equal(it_wv, it_rl) and np.array_equal(n_wv, n_rl)
    assert np.all(np.abs(rho_wv - rho_rl) < 1e-4 * rho_rl) and np.abs(x_wv - x_rl).max() < 1e-10


def _sqp(arrays, params, qp_settings=None):
    with sb.TrajOptBatch(arrays["B"], arrays["d"], arrays["T"], arrays["K"], arrays["O"]) as tb:
        tb.load(arrays["x0"], arrays["start"], arrays["goal"], arrays["link_len"], arrays["point_link"], arrays["point_frac"],
                arrays["obstacles"])
        tb.solve(params, qp_settings)
        res = tb.fetch(); res.trace = tb.trace(); res.timing = tb.last_timing()
        lib = _lib.load()
        lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
        res.wv_rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    return res


WARM = dict(warm_start_qps=1, compound_penalty=0, duplicate_rows=0, max_sqp_iters=12)


def test_warm_started_qps_park_at_slice_ends_and_resume(gpu, on_tier):
    """Time slices of 300 iterations against unsliced launches, every round on the wavefront tier: a warm-started QP that
    needs more than one slice parks and resumes, and nothing but the schedule changes."""
    arrays, _ = af.make_batch(6, T=12)
    whole = _sqp(arrays, _lib.default_sqp_params(admm_slice=-1, **WARM))
    cut = _sqp(arrays, _lib.default_sqp_params(admm_slice=300, **WARM))
    for res in (whole, cut):
        assert res.wv_rounds > 0 and res.timing["other_launches"] == 0, res.timing
    assert max(tr[:, 7].max() for tr in cut.trace) > 300                # some QP did park
    assert cut.timing["wv_launches"] > whole.timing["wv_launches"]
    for b in range(6):
        assert np.array_equal(cut.trace[b][:, [0, 6, 7]], whole.trace[b][:, [0, 6, 7]]), b
    assert np.array_equal(cut.success, whole.success) and np.array_equal(cut.admm_iters, whole.admm_iters)
    assert np.abs(cut.x - whole.x).max() < 1e-10


# ---- 4. through the device loop ----------------------------------------------------------------------------------------
def _adaptive_loop(kw):
    arrays, probs = af.make_batch(6, **kw)
    res = _sqp(arrays, _lib.default_sqp_params(admm_slice=300), _lib.default_qp_settings(adaptive_rho=1))
    assert res.wv_rounds > 0 and res.timing["wv_iters"] > 0 and res.timing["other_launches"] == 0, res.timing
    return res, probs


def test_adaptive_rho_in_the_device_loop_on_the_wavefront_tier(gpu, on_tier):
    """The 3-DOF x 6 part of test_sqp_gpu.test_adaptive_rho_in_the_device_loop with every round on the wavefront tier and time
    slices of 300, every second problem: against the flat oracle with the same rho rule the decisions, the QP statuses, the
    trajectories, and the iteration counts of the projection and the first penalty QP.  A later, ill-conditioned QP that
    runs towards max_iter sits so close to a rho threshold that the oracle's KKT route and the device's reduced system part
    ways there (that test's docstring) -- and so do the two device kernels, whose sums differ in their last bits.  Measured
    here: fifth QP of problem 4, 8250 iterations in the oracle and 5975 on this tier; fourth QP of problem 1, 89000 on this
    tier and 27950 on the row-local kernel, same decision and status."""
    res, probs = _adaptive_loop(dict(d=3, T=6, K=2, O=2))
    for b in range(0, 6, 2):
        ref = sr.penalty_sqp(sr.trajopt_flat(probs[b]), qp_settings=dict(adaptive_rho=1))
        tr, rt = res.trace[b], ref.trace[:64]
        print("problem", b, "device", tr[:, [0, 6, 7]].tolist(), "oracle", rt[:, [0, 6, 7]].tolist())
        assert tr.shape == rt.shape and np.array_equal(tr[:, 0], rt[:, 0]), b          # same decisions
        assert np.array_equal(tr[:, 6], rt[:, 6]) and np.array_equal(tr[:2, 7], rt[:2, 7]), b
        assert bool(res.success[b]) == ref.success
        assert np.abs(res.x[b] - ref.x).max() < 1e-4, (b, np.abs(res.x[b] - ref.x).max())
        assert abs(res.max_violation[b] - ref.max_violation) < 1e-5


def test_adaptive_rho_in_the_device_loop_on_the_wavefront_tier_7dof(gpu, on_tier):
    """The 7-DOF part of that test at 12 timesteps (<8,2,2,8>): the well-conditioned part, i.e. the projection and the first
    penalty QP, decision, status and iteration count, and the merits to 1e-6.  Beyond it the oracle and the device differ
    as they do at 7-DOF x 20 on every tier: measured here, the fourth QP of problem 0 ends with status 2 in the oracle and
    1 on the device."""
    res, probs = _adaptive_loop(dict(T=12))
    for b in range(0, 6, 2):
        ref = sr.penalty_sqp(sr.trajopt_flat(probs[b]), qp_settings=dict(adaptive_rho=1))
        print("problem", b, "device", res.trace[b][:, [0, 6, 7]].tolist(), "oracle", ref.trace[:, [0, 6, 7]].tolist())
        assert np.array_equal(res.trace[b][:2, [0, 6, 7]], ref.trace[:2, [0, 6, 7]]), b
        assert np.abs(res.trace[b][:2, 1:4] - ref.trace[:2, 1:4]).max() < 1e-6 * (1 + np.abs(ref.trace[:2, 1:4]).max())


@pytest.mark.parametrize("kw", [dict(d=3, T=6, K=2, O=2), dict(T=12)], ids=["3-DOF x 6", "7-DOF x 12"])
def test_warm_started_qps_in_the_device_loop_on_the_wavefront_tier(gpu, on_tier, kw):
    """The properties of test_sqp_gpu.test_warm_started_qps_in_the_device_loop with every round on the wavefront tier, and the
    row-local kernel as the referee: same success flags, trajectories within the QP tolerance (1e-4)."""
    arrays, _ = af.make_batch(6, **kw)
    B, T, d = arrays["B"], arrays["T"], arrays["d"]
    cold = _sqp(arrays, _lib.default_sqp_params(compound_penalty=0, duplicate_rows=0, max_sqp_iters=12))
    w1 = _sqp(arrays, _lib.default_sqp_params(**WARM))
    w2 = _sqp(arrays, _lib.default_sqp_params(**WARM))
    assert w1.wv_rounds > 0 and w1.timing["wv_iters"] > 0, w1.timing
    assert np.array_equal(w1.x, w2.x) and np.array_equal(w1.admm_iters, w2.admm_iters)
    print("ADMM iterations cold", cold.admm_iters.sum(), "warm", w1.admm_iters.sum())
    assert w1.admm_iters.sum() < 0.8 * cold.admm_iters.sum()
    assert (cold.success & w1.success).sum() >= 0.8 * cold.success.sum()
    assert np.all(w1.max_violation[w1.success] <= 1e-4)
    x = w1.x.reshape(B, T, d)
    assert np.abs(x[:, 0, :] - arrays["start"]).max() < 1e-4 and np.abs(x[:, -1, :] - arrays["goal"]).max() < 1e-4
    on_tier.setenv("SCO_QP_NO_WV", "1")
    rl = _sqp(arrays, _lib.default_sqp_params(**WARM))
    assert rl.wv_rounds == 0
    assert np.array_equal(w1.success, rl.success)
    assert np.abs(w1.x - rl.x).max() < 1e-4, np.abs(w1.x - rl.x).max()


# ---- 5. one problem fails the value test -------------------------------------------------------------------------------
def test_adaptive_rho_leaves_odd_value_structure_to_the_row_local_adapt_kernel(gpu, on_tier, wv_counted):
    """The mixed batch of tests/wv_cases.py with adaptive rho: the problems that fail the value test run on the row-local
    ADAPT kernel behind the wavefront one, launch after launch, and each kernel clears the rho flags of its own problems
    only.  Every result is the oracle's; the wavefront counter holds the ordinary problems' iterations alone."""
    case = next(c for c in wc.CASES if c.seed == 7001)
    probs, w, check, tier = case.build()
    assert 0 < len(tier) < len(probs)
    _adaptive(probs, w, wv_counted, tier=tier, check=check)
