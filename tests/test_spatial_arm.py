"""The spatial serial-arm family (SCO_FAM_ARM_SPATIAL) without a GPU: its NumPy definition, the planar reduction, the layout
rules, the object-API recogniser and the flat oracle against runs of the reference's own modules."""
import ctypes as C
import os

import numpy as np
import pytest

import conftest as ct
import spatial_build as sbd
import spatial_cases as sc
from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib
from sco_py_amd import workloads as wl
from sco_py_amd.sco_osqp import compile as cp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG = -1
VEL, JL, EE, OBJ_PROGRAM, ACC, OBJ_BLOCK, OBJ_WIDE = 16, 32, 64, 128, 256, 512, 1024
ARM, SPATIAL = 1, 7


def test_analytic_jacobian_agrees_with_numeric_differences():
    """20 random configurations of the 7-joint arm.  Bound: the ladder's smallest step is 1/512, so rounding of |g| <= 2
    enters a difference quotient with 2.2e-16 * 2 * 256 = 1.1e-13 and Richardson's weights at most double it; the truncation
    term of the four-level ladder, (1/64)^8, is below that.  1e-11 leaves two orders above both and is six below a wrong
    entry (the entries are O(0.1 .. 1))."""
    pr = af.make_problem(3, **sc.MID)
    geo = sbd.geometry(pr)
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(20):
        th = rng.uniform(-np.pi, np.pi, size=pr["d"])
        J = wl.spatial_dist_jac(th, *geo)
        N = sr.fd_jacobian(lambda v: wl.spatial_dist(v, *geo), th)
        assert J.shape == N.shape == (pr["K"] * pr["O"], pr["d"])
        worst = max(worst, float(np.abs(J - N).max()))
        for k, lk in enumerate(pr["point_link"]):                 # exactly 0 behind the point's link, on both paths
            assert not np.any(J[k * pr["O"]:(k + 1) * pr["O"], lk + 1:]) and not np.any(N[k * pr["O"]:(k + 1) * pr["O"], lk + 1:])
    print("worst |J - numdiff| = %.2e" % worst)
    assert worst < 1e-11


def test_longdouble_kinematics_round_to_the_float64_rows():
    pr = af.make_problem(1, **sc.MID)
    geo = sbd.geometry(pr)
    th = pr["x0"][:pr["d"]]
    a, b = wl.spatial_dist(th, *geo), wl.spatial_dist(th, *geo, dtype=np.longdouble)
    assert a.dtype == b.dtype == np.float64 and np.abs(a - b).max() < 16 * np.spacing(1.0)


@pytest.mark.parametrize("i", range(4))
def test_planar_reduction(i):
    """All axes (0, 0, 1), offsets along x, spheres in the plane: the spatial rows are the planar arm's.  4 ulp of 1.0: the
    link points lie within the unit disc, so positions and distances round in units of at most ulp(1) = 2.2e-16."""
    pr = af.make_problem(i, d=3, T=6, K=2, O=2)
    sp = sbd.planar_as_spatial(pr)
    geo = sbd.geometry(sp)
    worst = 0.0
    for t in range(pr["T"]):
        th = pr["x0"][t * 3:(t + 1) * 3]
        worst = max(worst, float(np.abs(wl.spatial_dist(th, *geo) -
                                        wl.arm_dist(th, pr["link_len"], pr["point_link"], pr["point_frac"], pr["obstacles"])).max()))
    print("worst value difference %.2e" % worst)
    assert worst <= 4 * np.spacing(1.0)
    a = sr.penalty_sqp(sr.trajopt_flat(pr))
    b = sr.penalty_sqp(sbd.flat_problem(sp))
    print("|dx| = %.2e" % float(np.abs(a.x - b.x).max()))
    assert np.array_equal(a.trace[:, 0], b.trace[:, 0]) and np.array_equal(a.trace[:, 6:8], b.trace[:, 6:8])
    assert a.success == b.success and np.abs(a.x - b.x).max() < 1e-9


# ---------------------------------------------------------------------------
# layout and descriptor rules (host code, through sco_debug_sqp_layout)
# ---------------------------------------------------------------------------
def _layout(family, dof, horizon, K, O, span=0, n_eq_rows=0, rows=None):
    lib = _lib.load()
    desc = _lib.TrajoptDesc(1, dof, horizon, K, O, family, 0, 2, span, n_eq_rows)
    n_rows, rp, ci, eq = 0, None, None, None
    if rows is not None:
        rp, ci, eq = (np.ascontiguousarray(a, dtype=np.int32) for a in rows)
        n_rows = len(eq)
    dims = np.zeros(22, dtype=np.int32); sizes = np.zeros(15, dtype=np.int32)
    args = (C.byref(desc), n_rows, _lib.iptr(rp), _lib.iptr(ci), _lib.iptr(eq), _lib.iptr(dims), _lib.iptr(sizes))
    rc = lib.sco_debug_sqp_layout(*args, None, None)
    if rc:
        return rc, None
    ints = np.full(int(sizes[:13].sum()), -7, dtype=np.int32); vals = np.full(int(sizes[13:].sum()), np.nan)
    assert lib.sco_debug_sqp_layout(*args, _lib.iptr(ints), _lib.dptr(vals)) == 0
    return 0, (dims, sizes, ints, vals)


@pytest.mark.parametrize("shape", [(3, 6, 2, 2), (7, 20, 5, 2)])
@pytest.mark.parametrize("flags", [0, VEL | JL])
def test_layout_is_the_planar_arms(shape, flags):
    rc1, a = _layout(ARM | flags, *shape)
    rc7, b = _layout(SPATIAL | flags, *shape)
    assert rc1 == 0 and rc7 == 0
    assert a[0][19] == 0 and b[0][19] == 4                        # RowFamily: ROWS_ARM, ROWS_SPATIAL
    assert np.array_equal(np.delete(a[0], 19), np.delete(b[0], 19))
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_descriptor_rules():
    ok = lambda *a, **k: _layout(*a, **k)[0]
    assert ok(SPATIAL, 16, 4, 1, 1) == 0 and ok(SPATIAL, 17, 4, 1, 1) == ERR_ARG          # dof <= 16
    assert ok(SPATIAL, 3, 6, 9, 7) == 0                                                      # any n_points, n_obstacles >= 1
    assert ok(SPATIAL, 3, 6, 0, 2) == ERR_ARG and ok(SPATIAL, 3, 6, 2, 0) == ERR_ARG
    assert ok(SPATIAL | ACC, 3, 6, 2, 2) == 0 and ok(SPATIAL | VEL | JL | ACC, 3, 6, 2, 2) == 0
    rows = ([0, 2, 3], [0, 17, 4], [1, 0])                                                   # general affine rows
    rc, lay = _layout(SPATIAL, 3, 6, 2, 2, rows=rows)
    assert rc == 0 and lay[0][8] == 2 and lay[0][9] == 3
    for bad in (EE, OBJ_PROGRAM, OBJ_BLOCK, OBJ_PROGRAM | OBJ_BLOCK, OBJ_WIDE, OBJ_WIDE | OBJ_PROGRAM, OBJ_WIDE | OBJ_BLOCK):
        assert ok(SPATIAL | bad, 3, 6, 2, 2) == ERR_ARG, bad
    assert ok(SPATIAL, 3, 6, 2, 2, span=2) == ERR_ARG
    assert ok(SPATIAL, 3, 6, 2, 2, n_eq_rows=1) == ERR_ARG
    assert ok(SPATIAL, 3, 6, 2, 2, span=1) == 0
    for fam in (0, 6, 15):                                                                   # still no such families
        assert ok(fam, 3, 6, 2, 2) == ERR_ARG


def test_binding_and_constants():
    from sco_py_amd import batch as sb
    assert sb.SCO_FAM_ARM_SPATIAL == 7 and "sco_sqp_load_spatial" in _lib.ABI
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "sco_hip.h")) as fh:
        assert "#define SCO_FAM_ARM_SPATIAL 7" in fh.read()


# ---------------------------------------------------------------------------
# the object API's recogniser
# ---------------------------------------------------------------------------
def test_compile_prob_recognises_the_family():
    pr = af.make_problem(0, **sc.SMALL)
    prob, _, _, _ = sbd.build_prob(ct.mirror_mods(), pr, device_exprs=True)
    c = cp.compile_prob(prob)
    assert c is not None, cp.last_reason()
    assert c.pr["spatial"] and (c.pr["d"], c.pr["T"], c.pr["K"], c.pr["O"]) == (3, 6, 2, 2)
    for k in wl.SPATIAL_KEYS + ("x0", "start", "goal", "point_link"):
        assert np.array_equal(c.pr[k], pr[k]), k
    other, _, _, _ = sbd.build_prob(ct.mirror_mods(), af.make_problem(5, **sc.SMALL), device_exprs=True)
    assert cp.compile_prob(other).key == c.key                     # structure, not numbers
    assert cp.compile_prob(sbd.build_prob(ct.mirror_mods(), pr, device_exprs=True, analytic_jac=True)[0]).key != c.key
    lim = cp.compile_prob(sbd.build_prob(ct.mirror_mods(), af.make_problem(0, vel_limit=0.45, joint_limit=0.15, groups="split", **sc.SMALL),
                                         device_exprs=True)[0])
    assert lim is not None and lim.key != c.key and lim.pr["vmax"] == 0.45 and lim.pr["groups"][0] == ["head"]
    a = cp._stack([c, cp.compile_prob(other)])
    assert a["spatial"] and a["spheres"].shape == (2, 2, 4) and a["joint_axis"].shape == (2, 3, 3)


def test_compile_prob_refuses_what_the_device_template_lacks():
    pr = af.make_problem(0, **sc.SMALL)
    prob, _, _, _ = sbd.build_prob(ct.mirror_mods(), pr, device_exprs=True)
    e = prob._nonlin_cnt_exprs[2].expr.expr
    e.spheres = e.spheres + 0.01                                    # geometry of its own on one timestep
    assert cp.compile_prob(prob) is None and "per-timestep geometry" in cp.last_reason()
    prob, _, _, _ = sbd.build_prob(ct.mirror_mods(), pr, device_exprs=True)
    for be in prob._nonlin_cnt_exprs:                               # an arm of four joints on a state of three numbers
        be.expr.expr.joint_off = np.zeros((4, 3)); be.expr.expr.joint_axis = np.tile([0.0, 0.0, 1.0], (4, 1))
    assert cp.compile_prob(prob) is None and "joint count" in cp.last_reason()
    prob, _, _, _ = sbd.build_prob(ct.mirror_mods(), pr)            # plain Expr bodies keep the host loop
    assert cp.compile_prob(prob) is None


# ---------------------------------------------------------------------------
# the oracle against the reference's own modules
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.GOLDEN, ids=lambda c: c[0])
def test_flat_oracle_reproduces_reference_runs(case):
    """tests/golden/trajopt_spatial.npz (make_golden_spatial.py): every QP the reference assembled, statuses, iteration
    counts and the answer -- finite differences, analytic Jacobian, and four joints with velocity limits."""
    prefix, kw, i, analytic = case
    g = np.load(os.path.join(GOLD, "trajopt_spatial.npz"))
    out = sr.penalty_sqp(sbd.flat_problem(af.make_problem(i, **kw), analytic_jac=analytic), record_qps=True)
    gq = ct.load_golden_qps(g, prefix, sparse=True)
    assert len(gq) == len(out.qps) >= 3
    for k, (a, b) in enumerate(zip(gq, out.qps)):
        P, q, A, l, u = ct.expand_weighted_qp(b)
        ct.assert_qp_close(a, P, q, A, l, u, (prefix, k), tol=1e-9)
        assert a["status"] == b["status"] and a["iters"] == b["iters"], (prefix, k)
        assert np.abs(a["x"] - b["x"]).max() < 1e-9, (prefix, k)
    assert out.success == bool(g[prefix + "success"])
    assert np.abs(out.x - g[prefix + "x"]).max() < 1e-9
    assert abs(out.max_violation - float(g[prefix + "max_violation"])) < 1e-9


def test_mirror_api_reproduces_a_reference_run(oracle_qp_backend):
    prefix, kw, i, analytic = sc.GOLDEN[0]
    g = np.load(os.path.join(GOLD, "trajopt_spatial.npz"))
    mods = ct.mirror_mods()
    prob, traj, _, _ = sbd.build_prob(mods, af.make_problem(i, **kw), analytic_jac=analytic)
    ok = mods.Solver().solve(prob, method="penalty_sqp")
    gold = ct.load_golden_qps(g, prefix, sparse=True)
    assert [a["iters"] for a in gold] == [r["iters"] for r in oracle_qp_backend]
    assert ok == bool(g[prefix + "success"]) and np.abs(traj.get_value().ravel() - g[prefix + "x"]).max() < 1e-9


def test_generator_leaves_the_other_workloads_alone_and_batches_carry_the_geometry():
    before = af.make_problem(2, d=3, T=6, K=2, O=2)
    af.make_problem(2, **sc.SMALL)
    after = af.make_problem(2, d=3, T=6, K=2, O=2)
    assert all(np.array_equal(before[k], after[k]) for k in ("x0", "start", "goal", "obstacles"))
    arrays, probs = af.make_batch(3, first=4, **sc.SMALL)
    assert arrays["spatial"] and arrays["spheres"].shape == (3, 2, 4) and arrays["point_rad"].shape == (3, 2)
    assert np.array_equal(arrays["joint_axis"][1], probs[1]["joint_axis"]) and np.array_equal(probs[1]["x0"], af.make_problem(5, **sc.SMALL)["x0"])
    assert np.abs(np.sqrt(np.sum(arrays["joint_axis"] ** 2, axis=2)) - 1.0).max() < 1e-12
    with pytest.raises(ValueError):
        af.make_problem(0, reach=True, **sc.SMALL)
