"""Mixed ADMM rounds of the device SQP loop (csrc/sco_sqp.hip, csrc/sco_qp.hip): in a wavefront round with fewer live problems
than the chip holds, the problems with most in front of them run on the row-local kernel on the CUs the wavefront launch
leaves free.  Only the kernel that runs a given slice moves, so against the plain schedule (SCO_SQP_MIX=0) and the all-row-local
loop (SCO_QP_NO_WV=1) the bar is the one of test_wavefront_rounds_then_row_local_tail_agree_with_the_row_local_loop: equal
admm_iters, success, qp_solves and trace columns 0, 4, 5, 6, 7, |dx| < 1e-9 -- and the oracle on every 160th problem."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib, batch as sb
from test_sqp_gpu import _compare

pytestmark = pytest.mark.gpu

SMALL = dict(d=3, T=6, K=2, O=2)
QUIRKS_OFF = dict(compound_penalty=0, duplicate_rows=0, max_sqp_iters=20)
MIX_VARS = ("SCO_SQP_MIX", "SCO_QP_NO_WV", "SCO_SQP_MIX_PICK", "SCO_SQP_MIX_SLICES", "SCO_SQP_MIX_SLACK", "SCO_WV_MIN_PER_CU",
            "SCO_SQP_GROUPS", "SCO_SQP_SELECT", "SCO_SQP_SLICE", "SCO_SQP_XCDS")


@contextlib.contextmanager
def _env(**kw):
    """The scheduling variables are read by every solve: all unset but the given ones, the caller's put back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in MIX_VARS}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k in MIX_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@functools.lru_cache(maxsize=None)
def _batch(nb, family):
    return af.make_batch(nb, **dict(family))


@functools.lru_cache(maxsize=None)
def _solve(nb, family, params, env):
    """One solve of the batch; shared by the tests (nothing changes a result afterwards).  Returns the result with the mixed
    rounds and summed side windows of the solve."""
    arrays, _ = _batch(nb, family)
    lib = _lib.load()
    with _env(**dict(env)):
        with sb.TrajOptBatch(nb, arrays["d"], arrays["T"], arrays["K"], arrays["O"]) as tb:
            tb.load(arrays["x0"], arrays["start"], arrays["goal"], arrays["link_len"], arrays["point_link"],
                    arrays["point_frac"], arrays["obstacles"])
            tb.solve(_lib.default_sqp_params(**dict(params)))
            r = tb.fetch(); r.trace = tb.trace()
            out = (C.c_int * 2)()
            assert lib.sco_debug_sqp_mixed(tb._h, out) == 0
            r.mixed = (int(out[0]), int(out[1]))
    return r


def _same(a, b):
    assert np.array_equal(a.admm_iters, b.admm_iters) and np.array_equal(a.success, b.success) and np.array_equal(a.qp_solves, b.qp_solves)
    assert all(np.array_equal(x[:, [0, 4, 5, 6, 7]], y[:, [0, 4, 5, 6, 7]]) for x, y in zip(a.trace, b.trace))
    assert np.abs(a.x - b.x).max() < 1e-9, np.abs(a.x - b.x).max()


def _key(d):
    return tuple(sorted(d.items()))


def _case(nb, family, params, env, oracle_params=None):
    fam, par = _key(family), _key(params)
    mixed = _solve(nb, fam, par, _key(env))
    plain = _solve(nb, fam, par, _key(dict(SCO_SQP_MIX="0")))
    row_local = _solve(nb, fam, par, _key(dict(SCO_QP_NO_WV="1")))
    print("mixed rounds %d, side windows summed %d" % mixed.mixed)
    assert mixed.mixed[0] > 0 and mixed.mixed[1] > 0, mixed.mixed
    assert plain.mixed == (0, 0) and row_local.mixed == (0, 0)
    _same(mixed, plain)
    _same(mixed, row_local)
    _compare(mixed, _batch(nb, fam)[1], range(0, nb, 160), oracle_params)
    return mixed


def test_mixed_rounds_small_family(gpu):
    """(a) 1280 problems of 3 x 6, slices of 400."""
    _case(1280, SMALL, dict(admm_slice=400), {})


def test_mixed_rounds_quirks_off_many_qp_starts(gpu):
    """(b) the same batch in intended mode with slices of 175: many QPs start on either side of a mixed round."""
    _case(1280, SMALL, dict(admm_slice=175, **QUIRKS_OFF), {},
          sr.SolverParams(compound_penalty=False, duplicate_rows=False, max_qp_solves=20))


@pytest.mark.parametrize("env", [dict(SCO_SQP_MIX_PICK="tail"), dict(SCO_SQP_MIX_SLICES="1"), dict(SCO_SQP_MIX_SLICES="3")],
                         ids=["side window from the tail in odd rounds", "1 side slice", "3 side slices"])
def test_mixed_rounds_side_window_variants(gpu, env):
    """(c) problems change sides inside one QP in both directions (tail pick); the side launch runs 1 or 3 slices."""
    _case(1280, SMALL, dict(admm_slice=400), env)


def test_mixed_rounds_default_family(gpu):
    """(d) 1040 problems of the default 7 x 20 family, default slice."""
    _case(1040, {}, {}, {})


def test_mixed_rounds_are_deterministic(gpu):
    """(e) two solves with the same settings: bit-identical x, iteration counts and traces (k depends only on live counts that
    are read back in order)."""
    fam, par = _key(SMALL), _key(dict(admm_slice=400))
    a = _solve(1280, fam, par, ())
    b = _solve.__wrapped__(1280, fam, par, ())
    assert a is not b and a.mixed == b.mixed and a.mixed[0] > 0
    assert np.array_equal(a.x, b.x) and np.array_equal(a.admm_iters, b.admm_iters)
    assert all(np.array_equal(x, y) for x, y in zip(a.trace, b.trace))
