"""The tail of the wavefront ADMM kernel's row phase (csrc/sco_admm_wv.hip: wv_rows_early): the instantiations with three
compile-time lanes per block read the extra rows' shares and the partial column sums in one batch behind the phase's first
WV_SYNC and in front of the core-variable loop; link plans, stacked plans and run-time lanes per block keep the order of
before.  The sums keep their operands and their order, so nothing may change in any result.

The referee is the row-local kernel (SCO_QP_NO_WV=1), which shares nothing with the row phase: equal decisions, statuses, QP
counts and ADMM iteration counts, |dx| <= 1e-9, and two runs on the tier give identical bits.

a. The device SQP loop, 8 problems of the arm family, max_iter 2000, check_termination 25, time slices of 60 and of 6250
   iterations (60: every QP parks and resumes many times, x / z / y go out and the right-hand side is rebuilt by the row
   phase's MODE 0; 6250: no QP parks).  7-DOF at 17, 19 and 20 timesteps runs on <7,4,3,10,3>, the new order (17 and 19: odd
   horizons, padded chains, the middle block at an odd position; the start pins put an extra row on seven lanes of 64); 4 and 5
   timesteps run on <8,1,1,4,0> with run-time lanes per block, short chains with dummy blocks; velocity limits are a link plan
   and joint limits a stacked plan (both <8,...,0,.,2>).
b. The QP layer, patterns of tests/wv_cases.py, wv_link_cases.py and wv_stack_cases.py, 8 problems each: pins on the first
   and the last timestep at 20 x 7 (extra rows on 14 lanes), a timestep without hinge rows at 18 x 7 and a variable without
   its box row at 19 x 7, all on <7,4,3,10,3>; two variables per block (21 x 2: lanes whose variable slots are all empty);
   dense blocks of order 8; 7-DOF x 14 on run-time lanes per block; one link plan and one stacked plan."""
import ctypes as C

import numpy as np
import pytest

import wv_cases as wc
import wv_link_cases as lc
import wv_stack_cases as sc
from oracle import arm_family as af
from sco_py_amd import _lib, batch as sb
from test_qp_gpu import _stack, _tiers
from test_qp_plan import penalty_qp
from test_wavefront_edges import wv_plan
from test_wavefront_edges_gpu import _wv_iters

pytestmark = pytest.mark.gpu

NB = 8
MAX_ITER, CHECK = 2000, 25
TOL = 1e-9                                  # the bound of tests/test_wavefront_gres_gpu.py
LIGHT = dict(K=2, O=2)

LOOP_CASES = [
    ("7x17 slices of 60", dict(T=17), 60), ("7x19 slices of 6250", dict(T=19), 6250), ("7x20 slices of 60", dict(T=20), 60),
    ("7x20 slices of 6250", dict(T=20), 6250),
    ("7x4 slices of 60", dict(T=4, **LIGHT), 60), ("7x5 slices of 6250", dict(T=5, **LIGHT), 6250),
    ("link plan 3x6 slices of 60", dict(d=3, T=6, vel_limit=0.6, **LIGHT), 60),
    ("stacked plan 3x6 slices of 60", dict(d=3, T=6, joint_limit=0.3, **LIGHT), 60),
]


def _loop(a, admm_slice):
    lib = _lib.load()
    lib.sco_debug_sqp_wv_rounds.restype = C.c_int; lib.sco_debug_sqp_wv_rounds.argtypes = [C.c_void_p]
    with sb.TrajOptBatch(NB, a["d"], a["T"], a["K"], a["O"], vel_limits=a.get("vmax") is not None,
                         joint_limits=a.get("jlo") is not None) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"],
                vmax=a.get("vmax"), jlo=a.get("jlo"), jhi=a.get("jhi"))
        tb.solve(_lib.default_sqp_params(admm_slice=admm_slice), _lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK))
        res = tb.fetch(); res.trace = tb.trace(); res.timing = tb.last_timing()      # (timing: sco_sqp_last_tiers)
        res.wv_rounds = lib.sco_debug_sqp_wv_rounds(tb._h)
    return res


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
    assert err <= TOL, err


@pytest.mark.parametrize("name,kw,admm_slice", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_device_loop_on_the_tier_against_the_row_local_kernel(gpu, monkeypatch, name, kw, admm_slice):
    a, _ = af.make_batch(NB, **kw)
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    monkeypatch.delenv("SCO_QP_NO_WV", raising=False)
    wv0 = _loop(a, admm_slice)
    assert wv0.wv_rounds > 0 and wv0.timing["wv_launches"] > 0 and wv0.timing["wv_iters"] > 0, wv0.timing
    wv1 = _loop(a, admm_slice)
    monkeypatch.setenv("SCO_QP_NO_WV", "1")
    rl = _loop(a, admm_slice)
    assert rl.wv_rounds == 0 and rl.timing["wv_iters"] == 0, rl.timing
    longest = max(int(t[:, 7].max()) for t in wv0.trace)
    if admm_slice == 60:                                # QPs longer than a slice: they parked and resumed
        assert longest > admm_slice, longest
    assert longest <= MAX_ITER, longest
    _same_run(wv0, wv1, bits=True)
    _same_run(wv0, rl, bits=False)


def _hw(make, *args):
    def build():
        rng = np.random.default_rng(8800 + args[0])
        probs = [make(rng, *args) for _ in range(NB)]
        return probs, wc.hinge_weights(rng, probs)
    return build


QP_CASES = [
    ("pins on the first and last timestep 20x7", _hw(wc.goal_pins, 20, 7, 10), (7, 4, 3, 10), 3),
    ("timestep 9 of 18 without hinge rows", _hw(wc.empty_timestep, 18, 7, 10, 9), (7, 4, 3, 10), 3),
    ("variable 70 of 19x7 without its box row", _hw(wc.no_box_row, 19, 7, 10, 70), (7, 4, 3, 10), 3),
    ("two variables per block 21x2", _hw(penalty_qp, 21, 2, 3), (8, 2, 2, 10), 2),
    ("dense blocks of order 8, 9x8", _hw(wc.dense_p_blocks, 9, 8, 8), (8, 2, 2, 8), 5),
    ("run-time lanes per block 14x7", _hw(penalty_qp, 14, 7, 10), (7, 4, 3, 10), 4),
    ("link plan 20x7", lambda: lc.batch(lc.one_sided, (20, 7, 10), 0.15, B=NB), None, 3),
    ("stacked plan 20x7", lambda: sc.batch((20, 7, 10), B=NB), None, 3),
]


@pytest.mark.parametrize("name,build,inst,lpb", QP_CASES, ids=[c[0] for c in QP_CASES])
def test_patterns_on_the_tier_against_the_row_local_kernel(gpu, monkeypatch, name, build, inst, lpb):
    probs, w = build()
    n, m, Pp, Pi, Ap, Ai, Pval, q, Aval, l, u = _stack(probs)
    if inst:                                            # (the plan of a pattern with link slots: tests/test_wavefront_link.py, _stack.py)
        info = wv_plan(probs[0][0], probs[0][2])
        assert info[0] == 1 and tuple(info[4:8]) == inst and info[3] == lpb, info   # fits, <BS, NS, NV, NSTEP>, lanes per block
    monkeypatch.setenv("SCO_WV_MIN_PER_CU", "0")
    settings = _lib.default_qp_settings(max_iter=MAX_ITER, check_termination=CHECK)
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
            outs.append(qp.solve(settings))
            assert _wv_iters(qp) == (int(outs[-1][3].sum()) if no_wv is None else 0)      # the tier ran every iteration, or none
        finally:
            qp.close()
    (x0, y0, s0, i0, _), (x1, y1, s1, i1, _), (xr, yr, sr_, ir, _) = outs
    print("statuses", s0, "iterations", i0)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and np.array_equal(i0, i1) and np.array_equal(s0, s1)
    assert np.array_equal(s0, sr_) and np.array_equal(i0, ir), (s0, sr_, i0, ir)
    ok = np.isin(s0, (1, 2, -2))                        # (the iterate of a certified-infeasible problem is a ray, not an answer)
    assert ok.any(), s0
    err = float(np.abs(x0[ok] - xr[ok]).max())
    print("max |dx| = %.3e" % err)
    assert err <= TOL, err
