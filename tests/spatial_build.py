"""Build problems of the spatial-arm family (SCO_FAM_ARM_SPATIAL) for the flat oracle and through the sco_py object API.

Test infrastructure next to tests/trajopt_build.py, which knows the other families: the objective and the linear rows are
the same, the non-linear blocks are one LEqExpr per timestep on ``workloads.spatial_dist``.  Shared by
tests/golden/make_golden_spatial.py (which passes the REFERENCE's modules) and the parity tests."""
import numpy as np

from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import workloads as wl


def geometry(pr):
    return tuple(pr[k] for k in ("joint_off", "joint_axis", "point_link", "point_pos", "point_rad", "spheres"))


def flat_problem(pr, analytic_jac=False, dtype=np.float64):
    """FlatProblem of one ``workloads.make_problem(i, spatial=True, ...)`` instance: objective, linear rows and projection
    weights from sco_ref.trajopt_flat, then one "leq" Block per timestep on the spatial rows.  ``dtype``: the arithmetic of
    the forward kinematics (the rows come back as float64 either way)."""
    flat = sr.trajopt_flat(pr)
    d, T, R = pr["d"], pr["T"], pr["K"] * pr["O"]
    geo = geometry(pr)
    f = lambda th: wl.spatial_dist(th, *geo, dtype=dtype)
    jac = (lambda th: wl.spatial_dist_jac(th, *geo, dtype=dtype)) if analytic_jac else None
    flat.blocks = [sr.Block("leq", f, np.arange(t * d, (t + 1) * d), np.zeros(R), jac=jac,
                            groups=pr["groups"][t] if pr.get("groups") is not None else None) for t in range(T)]
    return flat


def planar_as_spatial(pr):
    """The planar-arm problem ``pr`` written as a spatial one: every axis (0, 0, 1), joint i at the end of link i - 1, link
    points on the x axis of their frame, radius 0, spheres in the plane z = 0."""
    d, K, O = pr["d"], pr["K"], pr["O"]
    off = np.zeros((d, 3)); off[1:, 0] = pr["link_len"][:-1]
    axis = np.zeros((d, 3)); axis[:, 2] = 1.0
    pos = np.zeros((K, 3)); pos[:, 0] = pr["point_frac"] * pr["link_len"][pr["point_link"]]
    sph = np.zeros((O, 4)); sph[:, :2] = pr["obstacles"][:, :2]; sph[:, 3] = pr["obstacles"][:, 2]
    out = dict(pr)
    out.update(spatial=True, joint_off=off, joint_axis=axis, point_pos=pos, point_rad=np.zeros(K), spheres=sph)
    return out


def stack(probs):
    """Batch arrays (layout of workloads.make_batch) of spatial problem dictionaries that need not come from the generator."""
    p0 = probs[0]
    a = dict(d=p0["d"], T=p0["T"], K=p0["K"], O=p0["O"], B=len(probs), spatial=True,
             point_link=np.asarray(p0["point_link"], dtype=np.int32), point_frac=np.asarray(p0["point_frac"], dtype=np.float64))
    for k in ("x0", "start", "goal", "link_len") + wl.SPATIAL_KEYS:
        a[k] = np.stack([np.asarray(p[k], dtype=np.float64) for p in probs])
    a["obstacles"] = np.zeros((len(probs), p0["O"], 3))
    if p0.get("vmax") is not None:
        a["vmax"] = np.array([p["vmax"] for p in probs])
    if p0.get("jlo") is not None:
        a["jlo"] = np.stack([p["jlo"] for p in probs]); a["jhi"] = np.stack([p["jhi"] for p in probs])
    if p0.get("groups") is not None:
        a["groups"] = p0["groups"]
    return a


def build_prob(mods, pr, analytic_jac=False, device_exprs=False):
    """The object-API ``Prob`` of a spatial problem, built as tests/trajopt_build.py builds the planar one: a trajectory
    Variable with the smoothing objective, the pins, velocity and joint limits, and one Variable per timestep with one
    LEqExpr.  mods: the reference's modules or the mirror's; device_exprs (mirror only): the bodies are
    ``devexpr.SpatialArmSpheresExpr``."""
    d, T = pr["d"], pr["T"]
    n_x = d * T
    prob = mods.Prob()
    atoms = np.empty((n_x, 1), dtype=object)
    for t in range(T):
        for j in range(d):
            v = mods.OSQPVar("q%03d_%02d" % (t, j))
            prob.add_osqp_var(v)
            atoms[t * d + j, 0] = v
    traj = mods.Variable(atoms, pr["x0"].reshape(n_x, 1).copy())
    prob.add_var(traj)
    Q = af.smooth_Q(d, T, pr.get("obj_w"), pr.get("acc_w"))
    prob.add_obj_expr(mods.BoundExpr(mods.QuadExpr(Q, np.zeros((1, n_x)), np.zeros((1, 1))), traj))
    pins = np.zeros((2 * d, n_x))
    for j in range(d):
        pins[j, j] = 1.0
        pins[d + j, (T - 1) * d + j] = 1.0
    rhs = np.concatenate([pr["start"], pr["goal"]]).reshape(-1, 1)
    prob.add_cnt_expr(mods.BoundExpr(mods.EqExpr(mods.AffExpr(pins, np.zeros((2 * d, 1))), rhs), traj))
    if pr.get("vmax") is not None:
        V = af.velocity_rows(d, T)
        prob.add_cnt_expr(mods.BoundExpr(mods.LEqExpr(mods.AffExpr(V, np.zeros((V.shape[0], 1))),
                                                      np.full((V.shape[0], 1), pr["vmax"])), traj))
    if pr.get("jlo") is not None:
        eye = np.eye(n_x)
        prob.add_cnt_expr(mods.BoundExpr(mods.LEqExpr(mods.AffExpr(eye, np.zeros((n_x, 1))),
                                                      np.tile(pr["jhi"], T).reshape(-1, 1)), traj))
        prob.add_cnt_expr(mods.BoundExpr(mods.LEqExpr(mods.AffExpr(-eye, np.zeros((n_x, 1))),
                                                      -np.tile(pr["jlo"], T).reshape(-1, 1)), traj))
    geo = geometry(pr)
    R = pr["K"] * pr["O"]
    step_vars = []
    for t in range(T):
        sv = mods.Variable(atoms[t * d:(t + 1) * d, :], pr["x0"][t * d:(t + 1) * d].reshape(d, 1).copy())
        step_vars.append(sv)
        if device_exprs:
            from sco_py_amd import devexpr as dx
            e = dx.SpatialArmSpheresExpr(*geo, analytic=analytic_jac)
        else:
            f = lambda x: wl.spatial_dist(x.ravel(), *geo).reshape(-1, 1)
            e = mods.Expr(f, lambda x: wl.spatial_dist_jac(x.ravel(), *geo)) if analytic_jac else mods.Expr(f)
        gids = pr["groups"][t] if pr.get("groups") is not None else None
        prob.add_cnt_expr(mods.BoundExpr(mods.LEqExpr(e, np.zeros((R, 1))), sv), gids)
    return prob, traj, step_vars, atoms
