"""The block sweeps of the wavefront ADMM kernel after the idle issue slots were taken out (csrc/sco_admm_wv.hip: wv_slots,
wv_matvec, wv_meet, the hand-overs of sweep_res): the accumulators of a DPP chain are initialised inside the chain's
statement, and the lane swaps take operands that need no select behind them.  No f64
operation changed its form, its operands or its order, so nothing may change in any result.

The referee is the row-local kernel (SCO_QP_NO_WV=1), which applies the dense inverse and shares nothing with the sweeps:
equal statuses and ADMM iteration counts, the tier's own counter equal to the iterations it reports (the wavefront kernel did
the work), |dx| <= 1e-9, and two runs on the tier give identical bits.  QP layer, four problems per case, max_iter 600,
check_termination 25; on the CPU oracle the problems of these seeds need 175 ... 1325 iterations, so most cases end some
problems through the converged branch of the test and some at max_iter (asserted for "7x20").

Cases, by what they reach (wv_slots: 1 = initialisations inside, 4 = hand-overs):
  7x20          <7,4,3,10,3,0,0>, both items, the G-resident sweep on an even NSTEP: the flagship instantiation.
  7x17          the same kernel with two dummy blocks at the start of either chain: G = 0 and a zero accumulator there, the
                products of zeros must still store +0 (the row-local kernel never sees those blocks: any other bit would show
                as a different iterate).
  8x9 dense     <8,2,2,8,0,0,0>: the eight-term chain, dense blocks of order 8.
  7x14          <7,4,3,10,0,0,0>: run-time lanes per block.
  3x7, 4x21     <8,1,1,4,0,0,0> (two waves per SIMD) and <8,2,2,10,0,0,0> with full chains.
  link 20x7     <7,4,3,10,0,1,2>, a link plan (LNK = 2, asserted on the host plan: two link slots per variable slot): the
                initialisations only (wv_slots = 1).
  7x20 adaptive <7,4,3,10,3,3,0> (EXT = 3): the 7-wide adaptive-rho kernel is the one instantiation on the LDS-fed sweep
                (wv_gres_fits; every NSTEP that is built is even, so no horizon reaches that sweep through an odd NSTEP).
  3x7 adaptive  <8,1,1,4,0,3,0>: adaptive rho on the G-resident sweep.
  7x20 warm     <7,4,3,10,3,1,0>: a warm-started solve of a perturbed q; this instantiation takes the hand-overs only (wv_slots = 4)."""
import numpy as np
import pytest

import wv_cases as wc
import wv_link_cases as lc
from sco_py_amd import _lib
from test_qp_gpu import _stack, _tiers
from test_qp_plan import penalty_qp
from test_wavefront_edges import wv_plan
from test_wavefront_edges_gpu import _wv_iters
from test_wavefront_link import link_plan

pytestmark = pytest.mark.gpu

NB = 4
MAX_ITER, CHECK = 600, 25
TOL = 1e-9


def _hw(make, seed, *args):
    def build():
        rng = np.random.default_rng(seed)
        probs = [make(rng, *args) for _ in range(NB)]
        return probs, wc.hinge_weights(rng, probs)
    return build


# name, build, <BS, NS, NV, NSTEP> and lanes per block (None: a plan with link slots), settings, warm
CASES = [
    ("7x20", _hw(penalty_qp, 9100, 20, 7, 10), ((7, 4, 3, 10), 3), {}, False),
    ("7x17 dummy blocks", _hw(penalty_qp, 9101, 17, 7, 10), ((7, 4, 3, 10), 3), {}, False),
    ("8x9 dense", _hw(wc.dense_p_blocks, 9102, 9, 8, 8), ((8, 2, 2, 8), 5), {}, False),
    ("7x14 run-time lanes per block", _hw(penalty_qp, 9103, 14, 7, 10), ((7, 4, 3, 10), 4), {}, False),
    ("3x7", _hw(penalty_qp, 9104, 7, 3, 4), ((8, 1, 1, 4), 8), {}, False),
    ("4x21 full chains", _hw(penalty_qp, 9105, 21, 4, 4), ((8, 2, 2, 10), 2), {}, False),
    ("link 20x7", lambda: lc.batch(lc.one_sided, (20, 7, 10), 0.15, B=NB), None, {}, False),
    ("7x20 adaptive", _hw(penalty_qp, 9106, 20, 7, 10), ((7, 4, 3, 10), 3), dict(adaptive_rho=1), False),
    ("3x7 adaptive", _hw(penalty_qp, 9107, 7, 3, 4), ((8, 1, 1, 4), 8), dict(adaptive_rho=1), False),
    ("7x20 warm", _hw(penalty_qp, 9108, 20, 7, 10), ((7, 4, 3, 10), 3), {}, True),
]


def _solve(stacked, w, settings, warm):
    """(x, y, status, iterations) of the batch and the iterations the wavefront kernel ran for that solve."""
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = stacked
    qp = _lib.BatchedQP(Pval.shape[0], n, m, Pp, Pi, Ap, Ai)
    try:
        qp.load(Pval, q, Aval, l, u, w)
        if warm:                                        # the previous solution of the handle, then a perturbed q from it
            qp.solve(_lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK, **settings))
            seen = _wv_iters(qp)
            q2 = q + 0.05 * np.random.default_rng(11).standard_normal(q.shape)
            qp.load(Pval, q2, Aval, l, u, w)
            x, y, st, it, _ = qp.solve(_lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK, warm_start=1, **settings))
            return x, y, st, it, _wv_iters(qp) - seen
        x, y, st, it, _ = qp.solve(_lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK, **settings))
        return x, y, st, it, _wv_iters(qp)
    finally:
        qp.close()


@pytest.mark.parametrize("name,build,plan,settings,warm", CASES, ids=[c[0] for c in CASES])
def test_sweeps_on_the_tier_against_the_row_local_kernel(gpu, monkeypatch, name, build, plan, settings, warm):
    probs, w = build()
    stacked = _stack(probs)
    n, m, Pp, Pi, Ap, Ai = stacked[:6]
    if plan:
        info = wv_plan(probs[0][0], probs[0][2])
        assert info[0] == 1 and tuple(info[4:8]) == plan[0] and info[3] == plan[1], info      # fits, <BS, NS, NV, NSTEP>, lanes per block
    else:
        info = link_plan(probs[0][0], probs[0][2])
        assert tuple(info[:8]) == lc.PLAN[(20, 7, 10)] and info[10] > 0 and info[11] == 2, info      # link rows on two slots: LNK = 2
        assert wv_plan(probs[0][0], probs[0][2])[0] == 0, "the link-free plan takes this pattern: not an LNK = 2 launch"
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    outs = []
    for no_wv in (None, None, "1"):
        if no_wv:
            monkeypatch.setenv("SCO_QP_NO_WV", no_wv)
        else:
            monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
        assert bool(_tiers(n, m, Pp, Pi, Ap, Ai) & 32) == (no_wv is None)
        outs.append(_solve(stacked, w, settings, warm))
        x, y, st, it, on_tier = outs[-1]
        assert on_tier == (int(it.sum()) if no_wv is None else 0), (on_tier, it)      # the tier ran every iteration, or none
    (x0, y0, s0, i0, _), (x1, y1, s1, i1, _), (xr, yr, sr_, ir, _) = outs
    print("statuses", s0, "iterations", i0)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)
    assert np.array_equal(s0, sr_) and np.array_equal(i0, ir), (s0, sr_, i0, ir)
    # the row-local kernel alone converges or stops at max_iter (there: -2, or 2 when the ten times wider test passes)
    assert np.all((sr_ == 1) | ((ir == MAX_ITER) & np.isin(sr_, (2, -2)))), (sr_, ir)
    if name == "7x20":
        assert ((sr_ == 1) & (ir < MAX_ITER)).any() and (ir == MAX_ITER).any(), (sr_, ir)      # both ends of the loop
    err = float(np.abs(x0 - xr).max())
    print("max |dx| = %.3e" % err)
    assert err <= TOL, err
