"""The G-resident sweep of the wavefront ADMM kernel (csrc/sco_admm_wv.hip: GRES, wv_gres_slot): a chain runs on two DPP
rows, handed over in the middle of every pass, every lane with its rows of G in registers.

Batches of 8 problems of the arm family go through the device SQP loop with every round on the wavefront tier
(SCO_WV_MIN_PER_CU=0); the referee is the same batch with the tier switched off (SCO_QP_NO_WV=1: the row-local kernel, which
applies the dense inverse and shares nothing with the sweeps).  Every decision, QP status, QP count and ADMM iteration count
is equal, |dx| <= 1e-9, and two runs on the tier give identical bits.

Horizons (7-DOF, 10 hinge rows per timestep unless noted; the plan of each is wv_plan_build's, tests/test_wavefront_edges.py):
3, 9, 10 run on <8,2,2,8> (3: one real block per chain, the chains' first halves hold only dummy blocks; 10: the chains
are as long as a half); 17, 18, 20 on <7,4,3,10,3> (17: its shortest chains, 20: the headline shape).  7-DOF x 21 does not
fit the tier at all (two lanes per block: four variable slots, wv_plan_build refuses): the case stays, as the proof that the
horizon past the tier's last still takes the row-local kernel, and 4-DOF x 21 with 4 hinge rows per timestep runs the longest
chains a 10-step kernel serves (<8,2,2,10,0>, ten real blocks on either side of the middle block);
6-DOF x 20 with 6 hinge rows per timestep on <8,2,2,10,0>; 7-DOF with 4 hinge rows per timestep at 3 and 8 timesteps on
<8,1,1,4> (3: an all-dummy first half, 8: every slot of chain A real).  The 8-wide blocks are the dense-P pattern of order 8
of tests/wv_cases.py, at the QP layer.  One case runs on time slices of 100 iterations: every QP parks and resumes, and the
resident G is read again by every launch."""
import ctypes as C

import numpy as np
import pytest

import wv_cases as wc
from oracle import arm_family as af
from sco_py_amd import _lib, batch as sb
from test_qp_gpu import _stack, _tiers
from test_wavefront_edges_gpu import _wv_iters

pytestmark = pytest.mark.gpu

NB = 8
LIGHT = dict(K=2, O=2)                 # 4 hinge rows per timestep: one row slot per lane at 8 lanes per block
CASES = [
    ("7x3", dict(T=3), None), ("7x9", dict(T=9), None), ("7x10", dict(T=10), None), ("7x17", dict(T=17), None),
    ("7x18", dict(T=18), None), ("7x20", dict(T=20), None), ("7x21 (not on the tier)", dict(T=21), None),
    ("4x21: full chains of the 10-step kernel", dict(T=21, d=4, **LIGHT), None),
    ("6x20 on the LPB=0 kernel", dict(T=20, d=6, K=3, O=2), None),
    ("7x3 on the 4-step kernel", dict(T=3, **LIGHT), None), ("7x8 on the 4-step kernel", dict(T=8, **LIGHT), None),
    ("7x20 in slices of 100: park and resume", dict(T=20), 100),
]


def _loop(a, admm_slice):
    lib = _lib.load()
    lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
    with sb.TrajOptBatch(NB, a["d"], a["T"], a["K"], a["O"]) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"])
        tb.solve(_lib.default_sqp_params(admm_slice=admm_slice) if admm_slice else None)
        res = tb.fetch(); res.trace = tb.trace()
        rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    return res, rounds


def _same_run(r0, r1, bits):
    for b in range(NB):
        t0, t1 = r0.trace[b], r1.trace[b]
        assert t0.shape == t1.shape, (b, t0.shape, t1.shape)
        assert np.array_equal(t0[:, 0], t1[:, 0]), (b, t0[:, 0], t1[:, 0])                  # decisions
        assert np.array_equal(t0[:, 6:8], t1[:, 6:8]), (b, t0[:, 6:8], t1[:, 6:8])          # QP status, ADMM iterations
        if bits:
            assert np.array_equal(t0, t1), b
    for name in ("success", "sqp_iters", "qp_solves", "admm_iters"):
        assert np.array_equal(getattr(r0, name), getattr(r1, name)), (name, getattr(r0, name), getattr(r1, name))
    err = float(np.abs(r0.x - r1.x).max())
    print("max |dx| = %.3e" % err)
    if bits:
        assert np.array_equal(r0.x, r1.x), err
    assert err <= 1e-9, err


@pytest.mark.parametrize("name,kw,admm_slice", CASES, ids=[c[0] for c in CASES])
def test_device_loop_on_the_resident_sweep_against_the_row_local_kernel(gpu, monkeypatch, name, kw, admm_slice):
    a, _ = af.make_batch(NB, **kw)
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    wv0, rounds = _loop(a, admm_slice)
    assert (rounds > 0) == ("not on the tier" not in name), ("rounds on the wavefront tier", rounds)
    wv1, _ = _loop(a, admm_slice)
    monkeypatch.setenv("SCO_QP_NO_WV", "1")
    rl, rounds_rl = _loop(a, admm_slice)
    assert rounds_rl == 0
    if admm_slice:                                      # QPs longer than a slice: they parked and resumed
        assert max(int(t[:, 7].max()) for t in wv0.trace) > admm_slice
    _same_run(wv0, wv1, bits=True)
    _same_run(wv0, rl, bits=False)


def test_blocks_of_order_8_on_the_resident_sweep(gpu, monkeypatch):
    case = [c for c in wc.CASES if "order 8" in c.name][0]
    probs, w, _, _ = case.build()
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    outs = []
    for no_wv in (None, None, "1"):
        if no_wv:
            monkeypatch.setenv("SCO_QP_NO_WV", no_wv)
        else:
            monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
        assert bool(_tiers(n, m, Pp, Pi, Ap, Ai) & 32) == (no_wv is None)
        qp = _lib.BatchedQP(len(probs), n, m, Pp, Pi, Ap, Ai)
        try:
            qp.load(Pval, q, Aval, l, u, w)
            outs.append(qp.solve())
            assert _wv_iters(qp) == (int(outs[-1][3].sum()) if no_wv is None else 0)
        finally:
            qp.close()
    (x0, y0, s0, i0, _), (x1, y1, s1, i1, _), (xr, yr, sr_, ir, _) = outs
    assert np.all(s0 == 1)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)
    assert np.array_equal(s0, sr_) and np.array_equal(i0, ir), (s0, sr_, i0, ir)
    assert np.abs(x0 - xr).max() <= 1e-9, np.abs(x0 - xr).max()
