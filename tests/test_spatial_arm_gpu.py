"""The spatial serial-arm family (SCO_FAM_ARM_SPATIAL) on the device: the resident penalty-SQP loop against the flat oracle
(tests/spatial_build.py), against runs of the reference's own modules, against the planar family on the reduction
problem, through the object API, on the wavefront tier, and the call-order and argument rules of sco_sqp_load_spatial."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import conftest as ct
import spatial_build as sbd
import spatial_cases as sc
from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib, batch as sb
from sco_py_amd import devexpr as dx
from sco_py_amd.sco_osqp import batching

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-6          # abs, BASELINE.json north_star


def _compare_one(res, b, ref):
    """The assertions of tests/test_sqp_gpu.py:_compare for problem b of a device result against one oracle run."""
    tr = res.trace[b]
    rt = ref.trace[:64]                       # the device keeps the first 64 decisions of a problem
    assert tr.shape == rt.shape, (b, tr.shape, ref.trace.shape)
    assert np.array_equal(tr[:, 0], rt[:, 0]), (b, tr[:, 0], rt[:, 0])                     # same decisions
    assert np.array_equal(tr[:, 6:8], rt[:, 6:8]), (b, tr[:, 6:8], rt[:, 6:8])             # QP status + iterations
    assert np.abs(tr[:, 1:4] - rt[:, 1:4]).max() < 1e-7 * (1 + np.abs(rt[:, 1:4]).max()), b
    assert np.array_equal(tr[:, 4:6], rt[:, 4:6]), b                                       # trust, penalty
    assert np.abs(res.x[b] - ref.x).max() < TOL, (b, np.abs(res.x[b] - ref.x).max())
    assert bool(res.success[b]) == ref.success
    assert (res.sqp_iters[b], res.qp_solves[b], res.admm_iters[b]) == (ref.sqp_iters, ref.qp_solves, ref.admm_iters)
    assert abs(res.max_violation[b] - ref.max_violation) < 1e-7


def _device_params(params):
    return _lib.default_sqp_params(**{k: int(v) for k, v in params.items()})


@functools.lru_cache(maxsize=None)
def _config_run(name):
    """One device batch per configuration: its screened seeds, in the order of spatial_cases.SEEDS."""
    kw, params, analytic = sc.CONFIGS[name]
    probs = [af.make_problem(i, **kw) for i in sc.SEEDS[name]]
    return sb.solve_batch(sbd.stack(probs), params=_device_params(params), analytic_jac=analytic), probs


@pytest.mark.parametrize("name,k", [(n, k) for n in sc.CONFIGS for k in range(len(sc.SEEDS[n]))],
                         ids=lambda v: str(v))
def test_device_loop_matches_the_oracle(gpu, name, k):
    """(3,6,2,2) and (7,12,5,2), parity and intended mode; on the small shape also analytic Jacobians, velocity limits, and
    joint limits with disjoint constraint groups."""
    assert len(sc.SEEDS[name]) >= 6                                   # at most 2 of the first 8 seeds dropped
    kw, params, analytic = sc.CONFIGS[name]
    res, probs = _config_run(name)
    ref = sr.penalty_sqp(sbd.flat_problem(probs[k], analytic_jac=analytic), sr.SolverParams(**params))
    _compare_one(res, k, ref)
    if kw.get("groups"):
        assert sorted(res.nonconverged_groups[k]) == sorted(ref.nonconverged_groups), (k, res.nonconverged_groups[k])


def test_make_batch_arrays_are_what_the_builder_stacks(gpu):
    arrays, probs = af.make_batch(3, **sc.SMALL)
    mine = sbd.stack(probs)
    a, b = sb.solve_batch(arrays), sb.solve_batch(mine)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.admm_iters, b.admm_iters)


def test_reference_golden_runs_through_the_device(gpu):
    g = np.load(os.path.join(GOLD, "trajopt_spatial.npz"))
    for prefix, kw, i, analytic in sc.GOLDEN:
        res = sb.solve_batch(sbd.stack([af.make_problem(i, **kw)]), analytic_jac=analytic)
        gq = ct.load_golden_qps(g, prefix, sparse=True)
        assert np.abs(res.x[0] - g[prefix + "x"]).max() < TOL, prefix
        assert bool(res.success[0]) == bool(g[prefix + "success"]), prefix
        assert [int(v) for v in res.trace[0][:, 6]] == [q["status"] for q in gq], prefix
        assert [int(v) for v in res.trace[0][:, 7]] == [q["iters"] for q in gq], prefix


def test_planar_reduction_on_the_device(gpu):
    """The planar problems on a family-7 handle (all axes z, spheres in the plane) against the same problems on a family-1
    handle."""
    arrays, probs = af.make_batch(4, d=3, T=6, K=2, O=2)
    planar = sb.solve_batch(arrays)
    spatial = sb.solve_batch(sbd.stack([sbd.planar_as_spatial(p) for p in probs]))
    for b in range(4):
        a, s = planar.trace[b], spatial.trace[b]
        assert a.shape == s.shape and np.array_equal(a[:, 0], s[:, 0]) and np.array_equal(a[:, 6:8], s[:, 6:8]), b
        assert np.abs(planar.x[b] - spatial.x[b]).max() < TOL, b
        assert bool(planar.success[b]) == bool(spatial.success[b])


def _device_exprs(prob):
    out = [be.expr.expr for be in prob._nonlin_cnt_exprs]
    assert out and all(isinstance(e, dx.SpatialArmSpheresExpr) for e in out)
    return out


def test_object_api_runs_the_resident_loop(gpu):
    """Solver().solve(prob) and solve_many on Probs built from SpatialArmSpheresExpr: the resident loop, no Python
    evaluation, and the bits of solve_batch."""
    mods = ct.mirror_mods()
    recs = [af.make_problem(i, **sc.SMALL) for i in range(3)]
    batch = sb.solve_batch(sbd.stack(recs))
    for i, pr in enumerate(recs):
        prob, traj, step_vars, _ = sbd.build_prob(mods, pr, device_exprs=True)
        solver = mods.Solver()
        ok = solver.solve(prob, method="penalty_sqp")
        assert solver.last_path == "device" and solver.last_device["rounds"] > 0
        assert sum(e.host_evals for e in _device_exprs(prob)) == 0
        assert ok == bool(batch.success[i]) and np.array_equal(traj.get_value().ravel(), batch.x[i])
        assert np.array_equal(solver.last_device["traces"][0], batch.trace[i])
        assert np.array_equal(step_vars[2].get_value().ravel(), batch.x[i][6:9])
    built = [sbd.build_prob(mods, pr, device_exprs=True) for pr in recs]
    oks, stats = batching.solve_many([b[0] for b in built])
    assert stats["device_problems"] == 3 and stats["device_batches"] == 1 and stats["last_device"]["rounds"] > 0
    for i, (prob, traj, _, _) in enumerate(built):
        assert oks[i] == bool(batch.success[i]) and np.array_equal(traj.get_value().ravel(), batch.x[i])
        assert sum(e.host_evals for e in _device_exprs(prob)) == 0


def test_full_batch_inherits_the_wavefront_tier(gpu):
    """1024 problems of (7,20,5,2): the QP pattern is the planar arm's, so the rounds run on the wavefront tier; every 128th
    problem against the oracle."""
    B = 1024
    arrays, probs = af.make_batch(B, d=7, T=20, K=5, O=2, spatial=True)
    res = sb.solve_batch(arrays)
    assert res.timing["wv_launches"] > 0 and res.timing["wv_iters"] > 0
    assert np.all(np.isfinite(res.x)) and np.all(res.qp_solves >= 2)
    for b in range(0, B, 128):
        _compare_one(res, b, sr.penalty_sqp(sbd.flat_problem(probs[b])))


def test_call_order_and_argument_rules(gpu):
    lib = _lib.load()
    arrays, _ = af.make_batch(2, **sc.SMALL)
    geo = lambda a: [_lib.dptr(np.ascontiguousarray(a[k])) for k in ("joint_off", "joint_axis", "point_pos", "point_rad", "spheres")]
    base = (arrays["x0"], arrays["start"], arrays["goal"], arrays["link_len"], arrays["point_link"], arrays["point_frac"], arrays["obstacles"])
    with sb.TrajOptBatch(2, 3, 6, 2, 2, spatial=True) as tb:
        assert lib.sco_sqp_load_spatial(tb._h, *geo(arrays)) == -4                        # before sco_sqp_load
        _lib.check(lib.sco_sqp_load(tb._h, *[_lib.iptr(a) if a.dtype == np.int32 else _lib.dptr(a) for a in base]))
        with pytest.raises(_lib.ScoHipError) as e:
            tb.solve()                                                                    # solve before sco_sqp_load_spatial
        assert e.value.code == -4 and "sco_sqp_load_spatial" in str(e.value)
        for key, idx, val in (("joint_axis", (1, 2, 0), 0.9), ("point_rad", (0, 1), -0.01), ("spheres", (1, 0, 3), -1e-3),
                              ("spheres", (0, 1, 1), np.nan), ("joint_off", (1, 0, 2), np.inf), ("point_pos", (0, 0, 0), np.nan)):
            bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in arrays.items()}
            bad[key][idx] = val
            assert lib.sco_sqp_load_spatial(tb._h, *geo(bad)) == -1, key
        ptrs = geo(arrays)
        for k in range(5):
            assert lib.sco_sqp_load_spatial(tb._h, *[None if j == k else p for j, p in enumerate(ptrs)]) == -1
        with pytest.raises(_lib.ScoHipError) as e:
            tb.solve()                                                                    # a refused load loads nothing
        assert e.value.code == -4
        with pytest.raises(ValueError):
            tb.load(*base)                                                                # the Python layer asks for the geometry
        # a second load followed by a solve matches a fresh handle
        other, _ = af.make_batch(2, first=5, **sc.SMALL)
        tb.load(*[other[k] for k in ("x0", "start", "goal", "link_len", "point_link", "point_frac", "obstacles")],
                **{k: other[k] for k in ("joint_off", "joint_axis", "point_pos", "point_rad", "spheres")})
        tb.solve(); first = tb.fetch()
        tb.load(*base, **{k: arrays[k] for k in ("joint_off", "joint_axis", "point_pos", "point_rad", "spheres")})
        tb.solve(); again = tb.fetch()
    fresh = sb.solve_batch(arrays)
    assert np.array_equal(again.x, fresh.x) and np.array_equal(again.admm_iters, fresh.admm_iters)
    assert np.array_equal(first.x, sb.solve_batch(other).x) and not np.array_equal(first.x, again.x)
    with sb.TrajOptBatch(2, 3, 6, 2, 2) as planar:                                         # a handle of another family
        assert lib.sco_sqp_load_spatial(planar._h, *geo(arrays)) == -1
    for kw in (dict(reach=True), dict(ee_cost=True), dict(point=True)):
        with pytest.raises(ValueError):
            sb.TrajOptBatch(2, 3, 6, 2, 2, spatial=True, **kw)
    desc = _lib.TrajoptDesc(2, 3, 6, 2, 2, 7 | 64, 0, 2, 0, 0)                             # family 7 with the end-effector term
    h = C.c_void_p()
    assert lib.sco_sqp_create(0, C.byref(desc), C.byref(h)) == -1
