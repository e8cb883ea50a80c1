"""Problem layout of the SQP layer (csrc/sqp_layout.cpp, through sco_debug_sqp_layout / sco_debug_sqp_check_program): host
arithmetic only.  The layout against the flat oracle's linear rows and blocks, the descriptor rules, the program check."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import arm_family as af
from oracle import sco_ref as sr
from sco_py_amd import _lib
from sco_py_amd.rowexpr import X, compile_rows

ERR_ARG = -1
VEL, JL, EE, OBJ_PROGRAM, ACC, OBJ_BLOCK, OBJ_WIDE = 16, 32, 64, 128, 256, 512, 1024
ARM, REACH, POINT, QUADRATIC, PROGRAM = 1, 2, 3, 4, 5
DIMS = ["NE", "S", "ds", "NBt", "Req", "m_pin", "m_vel", "m_jl", "m_gen", "nnz_gen", "R", "n_x", "n_slack", "n", "m_lin", "m_nl",
        "m", "NB", "RM", "point", "cost", "acc"]
INTS = ["Pp0", "Pi0", "Ap0", "Ai0", "Pp1", "Pi1", "Ap1", "Ai1", "jpos", "epos", "ppos", "gpos0", "gpos1"]


def _desc(batch=1, dof=2, horizon=3, n_points=1, n_obstacles=2, family=ARM, span=0, n_eq_rows=0):
    return _lib.TrajoptDesc(batch, dof, horizon, n_points, n_obstacles, family, 0, 2, span, n_eq_rows)


def _last_error():
    return (_lib.load().sco_last_error() or b"").decode()


def _layout(desc, rows=None):
    """(return code, layout): the sizes from a first call without output arrays, then everything."""
    lib = _lib.load()
    n_rows, rp, ci, eq = 0, None, None, None
    if rows is not None:
        rp, ci, eq = (None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in rows[:3])
        n_rows = rows[3] if len(rows) > 3 else len(eq)
    dims = np.zeros(22, dtype=np.int32); sizes = np.zeros(15, dtype=np.int32)
    args = (C.byref(desc), n_rows, _lib.iptr(rp), _lib.iptr(ci), _lib.iptr(eq), _lib.iptr(dims), _lib.iptr(sizes))
    rc = lib.sco_debug_sqp_layout(*args, None, None)
    if rc:
        return rc, None
    ints = np.full(int(sizes[:13].sum()), -7, dtype=np.int32); vals = np.full(int(sizes[13:].sum()), np.nan)
    sizes2 = np.zeros(15, dtype=np.int32)
    assert lib.sco_debug_sqp_layout(*args[:6], _lib.iptr(sizes2), _lib.iptr(ints), _lib.dptr(vals)) == 0
    assert np.array_equal(sizes, sizes2)
    L = SimpleNamespace(**{k: int(v) for k, v in zip(DIMS, dims)})
    for name, part in zip(INTS, np.split(ints, np.cumsum(sizes[:13])[:-1])):
        setattr(L, name, part)
    L.a0c, L.a1c = np.split(vals, [int(sizes[13])])
    return 0, L


# ---------------------------------------------------------------------------
# 1. the layout against the oracle
# ---------------------------------------------------------------------------
def _program_problem(d, T, prog, circles=0, acc=False):
    pr = af.make_problem(0, program=True, d=d, T=T)
    pr["row_program"] = prog; pr["row_params"] = np.zeros(max(prog.n_params, 1))
    pr["O"] = prog.n_rows + circles; pr["obstacles"] = np.zeros((pr["O"], 3))
    if circles:
        pr["circle_rows"] = circles
    if acc:
        pr["acc_w"] = np.ones(d)
    return pr


def _with_general_rows(pr):
    d, T = pr["d"], pr["T"]
    A = np.zeros((2, d * T))
    A[0, [0, d * T - 1]] = 1.0               # an equality spanning the first and the last timestep
    A[1, [1, d, d + 1]] = 1.0                # an inequality on two neighbouring timesteps
    pr["lin_gen"] = dict(A=A, rhs=np.zeros(2), is_eq=np.array([1, 0], dtype=np.int32))
    return pr


CASES = {
    "plain": lambda: af.make_problem(0, d=2, T=3, K=2, O=2),
    "reach": lambda: af.make_problem(0, d=2, T=3, K=2, O=2, reach=True),
    "vel": lambda: af.make_problem(0, d=2, T=3, K=2, O=2, vel_limit=0.5),
    "joint-limits": lambda: af.make_problem(0, d=2, T=3, K=2, O=2, joint_limit=0.3),
    "reach+vel+jl": lambda: af.make_problem(0, d=2, T=3, K=2, O=2, reach=True, vel_limit=0.5, joint_limit=0.3),
    "acc T=3": lambda: af.make_problem(0, d=2, T=3, K=2, O=2, acc_weights=True),
    "acc T=4": lambda: af.make_problem(0, d=2, T=4, K=2, O=2, acc_weights=True),
    "ee-cost": lambda: af.make_problem(0, d=2, T=3, K=1, O=2, ee_cost_weight=1.0),
    "general rows": lambda: _with_general_rows(af.make_problem(0, d=2, T=3, K=2, O=2, vel_limit=0.5)),
    "point": lambda: af.make_problem(0, point=True, d=2, T=3, O=2),
    "quadratic, 1 eq": lambda: af.make_problem(0, quadratic=True, d=2, T=3, O=2, n_eq=1),
    "program span 2": lambda: _program_problem(2, 3, compile_rows([X(0) - X(2), X(1) * X(3)], span=2)),
    "program span 4, 1 eq": lambda: _program_problem(2, 5, compile_rows([X(0) - X(7)], eq_rows=[X(1) - X(6)], span=4)),
    "objective per timestep": lambda: _program_problem(3, 3, compile_rows([X(0) - X(2)], objective=X(0) * X(1) + X(2))),
    "objective per block": lambda: _program_problem(2, 3, compile_rows([X(0) - X(3)], block_objective=X(0) * X(3), span=2, dof=2)),
    "objective per block, acc T=4": lambda: _program_problem(2, 4, compile_rows([X(0) - X(3)], block_objective=X(0) * X(3), span=2, dof=2), acc=True),
    "objective per block span 3, acc": lambda: _program_problem(2, 5, compile_rows([X(0) - X(5)], block_objective=X(0) * X(5), span=3, dof=2), acc=True),
    "circle rows": lambda: _program_problem(2, 3, compile_rows([X(0) - X(1)]), circles=1),
}


def _desc_of(pr):
    prog = pr.get("row_program")
    fam = PROGRAM if prog is not None else QUADRATIC if pr.get("quad_Q") is not None else POINT if pr.get("point") else \
        REACH if pr.get("reach") else ARM
    fam |= (VEL if pr.get("vmax") is not None else 0) | (JL if pr.get("jlo") is not None else 0)
    fam |= (EE if pr.get("cost_weight") is not None else 0) | (ACC if pr.get("acc_w") is not None else 0)
    if prog is not None:
        fam |= (OBJ_PROGRAM if prog.objective else 0) | (OBJ_BLOCK if prog.block_objective else 0) | (OBJ_WIDE if prog.wide else 0)
    n_eq = prog.n_eq if prog is not None else int(pr.get("quad_n_eq") or 0)
    return _desc(1, pr["d"], pr["T"], pr["K"], pr["O"], fam, prog.span if prog is not None else 0, n_eq)


def _flat(pr):
    """The oracle's flat problem; the terms of a block objective as tests/blockobj_build.py:flat appends them."""
    fp = sr.trajopt_flat(pr)
    prog, d = pr.get("row_program"), pr["d"]
    if prog is not None and prog.block_objective:
        for t in range(pr["T"] - prog.span + 1):
            fp.obj_blocks.append(sr.ObjBlock(prog.block_objective_fn(af.step_params(pr, t)), np.arange(t * d, (t + prog.span) * d)))
    return fp


def _dense(Ap, Ai, vals, shape):
    return sp.csc_matrix((vals, Ai, Ap), shape=shape).toarray()


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    pr = CASES[request.param]()
    gen = pr.get("lin_gen")
    rows = None
    if gen is not None:
        G = sp.csr_matrix(gen["A"])
        rows = (G.indptr, G.indices, gen["is_eq"])
    rc, L = _layout(_desc_of(pr), rows)
    assert rc == 0, _last_error()
    return SimpleNamespace(name=request.param, pr=pr, fp=_flat(pr), L=L, rows=rows)


def test_dimensions_have_their_closed_form(case):
    pr, L, fp = case.pr, case.L, case.fp
    d, T, K, O = pr["d"], pr["T"], pr["K"], pr["O"]
    prog = pr.get("row_program")
    reach, vel, jl = bool(pr.get("reach")), pr.get("vmax") is not None, pr.get("jlo") is not None
    S = prog.span if prog is not None else 1
    Req = prog.n_eq if prog is not None else int(pr.get("quad_n_eq") or 0)
    m_gen = 0 if case.rows is None else len(case.rows[2])
    cost = 3 if prog is not None and prog.block_objective else 2 if prog is not None and prog.objective else \
        1 if pr.get("cost_weight") is not None else 0
    NBt, NE, R, n_x = T - S + 1, 2 if reach else 0, K * O, d * T
    want = dict(NE=NE, S=S, ds=S * d, NBt=NBt, Req=Req, m_pin=d if reach else 2 * d, m_vel=2 * d * (T - 1) if vel else 0,
                m_jl=2 * d * T if jl else 0, m_gen=m_gen, nnz_gen=0 if case.rows is None else len(case.rows[1]), R=R, n_x=n_x,
                n_slack=NBt * (R + Req) + 2 * NE, NB=NBt + (1 if reach else 0), RM=max(R, NE) + (1 if cost else 0),
                point=3 if prog is not None else 2 if pr.get("quad_Q") is not None else 1 if pr.get("point") else 0, cost=cost,
                acc=1 if pr.get("acc_w") is not None else 0)
    want["n"] = n_x + want["n_slack"]
    want["m_lin"] = want["m_pin"] + want["m_vel"] + want["m_jl"] + m_gen
    want["m_nl"] = NBt * R + NE
    want["m"] = want["m_lin"] + want["m_nl"] + want["n"]
    assert {k: getattr(L, k) for k in DIMS} == want
    # and the oracle's own counts: linear rows, rows of all blocks, one slack per hinge row and two per equality row
    assert L.m_lin == fp.lin_A.shape[0] and L.m_nl == sum(b.r for b in fp.blocks)
    assert L.n_slack == sum(b.r * (2 if b.kind == "eq" else 1) for b in fp.blocks)
    assert [len(getattr(L, k)) for k in INTS] == [n_x + 1, n_x, n_x + 1, len(L.a0c), L.n + 1, L.Pp1[-1], L.n + 1, len(L.a1c),
                                                  n_x, d, n_x, L.nnz_gen, L.nnz_gen]


def _lin_constants(case):
    """The oracle's linear rows with the general rows' entries at zero (their values are per problem)."""
    lin = case.fp.lin_A.toarray()
    if case.L.m_gen:
        lin[case.L.m_lin - case.L.m_gen:] = 0.0
    return lin


def test_projection_qp_is_the_linear_rows_over_the_identity(case):
    L = case.L
    assert np.array_equal(L.Pp0, np.arange(L.n_x + 1)) and np.array_equal(L.Pi0, np.arange(L.n_x))
    A0 = _dense(L.Ap0, L.Ai0, L.a0c, (L.m_lin + L.n_x, L.n_x))
    assert np.array_equal(A0, np.vstack([_lin_constants(case), np.eye(L.n_x)]))


def test_penalty_qp_linear_rows_and_jacobian_slots(case):
    L, fp, d = case.L, case.fp, case.pr["d"]
    A1 = _dense(L.Ap1, L.Ai1, L.a1c, (L.m, L.n))
    assert np.array_equal(A1[:L.m_lin, :L.n_x], _lin_constants(case)) and not A1[:L.m_lin, L.n_x:].any()
    row0 = np.concatenate([[0], np.cumsum([b.r for b in fp.blocks])])
    for col in range(L.n_x):
        # the rows of exactly those blocks that hold the column, in block order, then the bound row
        want = [L.m_lin + r for k, b in enumerate(fp.blocks) if col in b.idx for r in range(row0[k], row0[k + 1])]
        lo, hi = L.jpos[col], L.Ap1[col + 1] - 1
        assert L.Ap1[col] <= lo and list(L.Ai1[lo:hi]) == want, (col, list(L.Ai1[lo:hi]), want)
        assert not L.a1c[lo:hi].any()                                  # convexify writes the Jacobian there
        assert L.Ai1[hi] == L.m_lin + L.m_nl + col and L.a1c[hi] == 1.0
        assert np.all(L.Ai1[L.Ap1[col]:lo] < L.m_lin)                  # only linear rows in front
    if case.pr.get("reach"):
        for j in range(d):
            col = L.n_x - d + j
            assert L.Ap1[col] <= L.epos[j] and L.epos[j] + 2 < L.Ap1[col + 1]
            assert list(L.Ai1[L.epos[j]:L.epos[j] + 2]) == [L.m_lin + L.NBt * L.R, L.m_lin + L.NBt * L.R + 1]
    else:
        assert not L.epos.any()


def test_slack_columns(case):
    L, fp = case.L, case.fp
    want, row = [], 0
    for b in fp.blocks:                 # a hinge row has one slack (-1), an equality row p (-1) and n (+1)
        for _ in range(b.r):
            want += [(row, -1.0), (row, 1.0)] if b.kind == "eq" else [(row, -1.0)]
            row += 1
    assert len(want) == L.n_slack
    for k, (r, sgn) in enumerate(want):
        col = L.n_x + k
        lo, hi = L.Ap1[col], L.Ap1[col + 1]
        assert list(L.Ai1[lo:hi]) == [L.m_lin + r, L.m_lin + L.m_nl + col] and list(L.a1c[lo:hi]) == [sgn, 1.0]


def test_objective_pattern_and_ppos(case):
    pr, L, fp = case.pr, case.L, case.fp
    d, T = pr["d"], pr["T"]
    want = np.triu(af.smooth_Q(d, T, None, np.ones(d) if L.acc else None) != 0.0)
    for ob in fp.obj_blocks:            # a term per timestep: its diagonal block; a term per block: the band
        want[np.ix_(ob.idx, ob.idx)] |= np.triu(np.ones((len(ob.idx),) * 2, dtype=bool))
    P = sp.csc_matrix((np.ones(len(L.Pi1)), L.Pi1, L.Pp1), shape=(L.n, L.n)).toarray() != 0.0
    assert np.array_equal(P[:L.n_x, :L.n_x], want) and not P[:, L.n_x:].any() and len(L.Pi1) == want.sum()
    for c in range(L.n_x):
        t, j = divmod(c, d)
        if L.cost == 3:                 # entry (r, c) of the band at ppos[c] + r
            for r in range(max(0, t - L.S + 1) * d, c + 1):
                assert L.Pp1[c] <= L.ppos[c] + r < L.Pp1[c + 1] and L.Pi1[L.ppos[c] + r] == r
        else:                           # entry (t d + i, c) of the timestep's diagonal block at ppos[c] + i
            for i in range(j + 1) if L.cost else [j]:
                assert L.Pp1[c] <= L.ppos[c] + i < L.Pp1[c + 1] and L.Pi1[L.ppos[c] + i] == t * d + i


def test_columns_are_sorted_and_general_rows_are_found(case):
    L = case.L
    for ptr, idx in ((L.Pp0, L.Pi0), (L.Ap0, L.Ai0), (L.Pp1, L.Pi1), (L.Ap1, L.Ai1)):
        assert ptr[0] == 0 and ptr[-1] == len(idx)
        for c in range(len(ptr) - 1):
            assert np.all(np.diff(idx[ptr[c]:ptr[c + 1]]) > 0), (case.name, c)
    if case.rows is not None:
        rp, ci, _ = case.rows
        for r in range(L.m_gen):
            for k in range(rp[r], rp[r + 1]):
                for gpos, Ap, Ai in ((L.gpos0, L.Ap0, L.Ai0), (L.gpos1, L.Ap1, L.Ai1)):
                    assert Ap[ci[k]] <= gpos[k] < Ap[ci[k] + 1] and Ai[gpos[k]] == L.m_pin + L.m_vel + L.m_jl + r


# ---------------------------------------------------------------------------
# 2. descriptor rules: per clause of the condition in sco_sqp_create_rows as it stood before the split, the nearest
# accepted descriptor and the refused one
# ---------------------------------------------------------------------------
P1 = dict(family=PROGRAM, n_points=1)
DESCRIPTORS = [
    ("batch", dict(batch=1), dict(batch=0)),
    ("dof", dict(dof=1), dict(dof=0)),
    ("horizon >= 2", dict(horizon=2), dict(horizon=1)),
    ("n_points", dict(n_points=1), dict(n_points=0)),
    ("n_obstacles", dict(n_obstacles=1), dict(n_obstacles=0)),
    ("horizon <= 256", dict(horizon=256), dict(horizon=257)),
    ("unknown flag", dict(family=ARM | VEL | JL | EE | ACC), dict(family=ARM | 2048)),
    ("unknown flag, high", dict(family=ARM), dict(family=ARM | (1 << 30))),
    ("family 0", dict(family=ARM), dict(family=0)),
    ("family 6", dict(**P1), dict(family=6, n_points=1)),
    ("family 15", dict(family=REACH), dict(family=15)),
    ("ee cost width", dict(family=ARM | EE, dof=16), dict(family=ARM | EE, dof=17)),
    ("acc cost horizon", dict(family=ARM | ACC, horizon=3), dict(family=ARM | ACC, horizon=2)),
    ("point: one point", dict(family=POINT, n_points=1), dict(family=POINT, n_points=2)),
    ("point: dof >= 2", dict(family=POINT, n_points=1, dof=2), dict(family=POINT, n_points=1, dof=1)),
    ("point: no ee cost", dict(family=POINT | VEL, n_points=1), dict(family=POINT | EE, n_points=1)),
    ("quadratic: one point", dict(family=QUADRATIC, n_points=1), dict(family=QUADRATIC, n_points=2)),
    ("quadratic: no ee cost", dict(family=QUADRATIC | JL, n_points=1), dict(family=QUADRATIC | EE, n_points=1)),
    ("quadratic: dof", dict(family=QUADRATIC, n_points=1, dof=16), dict(family=QUADRATIC, n_points=1, dof=17)),
    ("program: one point", dict(**P1), dict(family=PROGRAM, n_points=2)),
    ("program: no ee cost", dict(family=PROGRAM | ACC, n_points=1), dict(family=PROGRAM | EE, n_points=1)),
    ("span >= 0", dict(span=0), dict(span=-1)),
    ("span <= 4", dict(span=4, horizon=7, **P1), dict(span=5, horizon=7, **P1)),
    ("span needs the program family", dict(span=1, family=QUADRATIC, n_points=1), dict(span=2, family=QUADRATIC, n_points=1)),
    ("span on the arm", dict(span=1), dict(span=2)),
    ("n_eq_rows >= 0", dict(n_eq_rows=0, **P1), dict(n_eq_rows=-1, **P1)),
    ("n_eq_rows <= n_obstacles", dict(n_eq_rows=2, n_obstacles=2, **P1), dict(n_eq_rows=3, n_obstacles=2, **P1)),
    ("n_eq_rows needs a state family", dict(n_eq_rows=1, family=QUADRATIC, n_points=1), dict(n_eq_rows=1, family=POINT, n_points=1)),
    ("n_eq_rows on the arm", dict(n_eq_rows=0), dict(n_eq_rows=1)),
    ("span * dof <= 32", dict(span=4, dof=8, horizon=5, **P1), dict(span=3, dof=11, horizon=5, **P1)),
    ("span * dof <= 32, span 1", dict(span=1, dof=32, **P1), dict(span=1, dof=33, **P1)),
    ("span < horizon", dict(span=2, horizon=3, **P1), dict(span=3, horizon=3, **P1)),
    ("span < horizon, span 4", dict(span=4, horizon=5, **P1), dict(span=4, horizon=4, **P1)),
    ("objective program: family", dict(family=PROGRAM | OBJ_PROGRAM, n_points=1), dict(family=QUADRATIC | OBJ_PROGRAM, n_points=1)),
    ("objective program: on the arm", dict(family=ARM), dict(family=ARM | OBJ_PROGRAM)),
    ("objective program: span 1", dict(family=PROGRAM | OBJ_PROGRAM, n_points=1, span=1), dict(family=PROGRAM | OBJ_PROGRAM, n_points=1, span=2)),
    ("objective program: dof", dict(family=PROGRAM | OBJ_PROGRAM, n_points=1, dof=16), dict(family=PROGRAM | OBJ_PROGRAM, n_points=1, dof=17)),
    ("block objective: family", dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2), dict(family=ARM | OBJ_BLOCK, n_points=1)),
    ("block objective: span >= 2", dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2), dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=1)),
    ("block objective: state", dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2, dof=8), dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2, dof=9)),
    ("block objective: state, span 4", dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=4, dof=4, horizon=5),
     dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=4, dof=5, horizon=5)),
    ("block objective: not both", dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2), dict(family=PROGRAM | OBJ_BLOCK | OBJ_PROGRAM, n_points=1, span=2)),
    ("block objective: no ee cost", dict(family=PROGRAM | OBJ_BLOCK | ACC, n_points=1, span=2), dict(family=PROGRAM | OBJ_BLOCK | EE, n_points=1, span=2)),
    ("wide: no objective flag", dict(family=PROGRAM | OBJ_WIDE | OBJ_PROGRAM, n_points=1), dict(family=PROGRAM | OBJ_WIDE, n_points=1)),
    ("wide: both objective flags", dict(family=PROGRAM | OBJ_WIDE | OBJ_BLOCK, n_points=1, span=2),
     dict(family=PROGRAM | OBJ_WIDE | OBJ_BLOCK | OBJ_PROGRAM, n_points=1, span=2)),
    ("wide: family", dict(family=ARM | EE), dict(family=ARM | EE | OBJ_WIDE)),
    ("wide: quadratic rows", dict(family=QUADRATIC, n_points=1), dict(family=QUADRATIC | OBJ_WIDE, n_points=1)),
    ("wide objective program: dof", dict(family=PROGRAM | OBJ_WIDE | OBJ_PROGRAM, n_points=1, dof=32), dict(family=PROGRAM | OBJ_PROGRAM, n_points=1, dof=32)),
    ("wide block objective: state", dict(family=PROGRAM | OBJ_WIDE | OBJ_BLOCK, n_points=1, span=2, dof=16),
     dict(family=PROGRAM | OBJ_BLOCK, n_points=1, span=2, dof=16)),
    ("wide block objective: beyond 32", dict(family=PROGRAM | OBJ_WIDE | OBJ_BLOCK, n_points=1, span=4, dof=8, horizon=5),
     dict(family=PROGRAM | OBJ_WIDE | OBJ_BLOCK, n_points=1, span=3, dof=11, horizon=5)),
]


@pytest.mark.parametrize("name,good,bad", DESCRIPTORS, ids=[c[0] for c in DESCRIPTORS])
def test_descriptor_rules(name, good, bad):
    rc, L = _layout(_desc(**good))
    assert rc == 0 and L.n_x == good.get("dof", 2) * good.get("horizon", 3), _last_error()
    assert _layout(_desc(**bad)) == (ERR_ARG, None)
    assert _last_error() == "sco_sqp_create: bad descriptor"


GOOD_ROWS = ([0, 2, 3], [0, 5, 2], [1, 0])          # dof 2, horizon 3: columns 0 .. 5
BAD_ROWS = [
    ("row_ptr[0] != 0", ([1, 2, 3], [0, 5, 2], [1, 0]), "sco_sqp_create_rows: bad row pattern"),
    ("empty row", ([0, 2, 2], [0, 5, 2], [1, 0]), "sco_sqp_create_rows: bad row pattern (empty row or row_ptr not increasing)"),
    ("row_ptr falls", ([0, 3, 2], [0, 2, 5], [1, 0]), "sco_sqp_create_rows: bad row pattern (empty row or row_ptr not increasing)"),
    ("column repeats", ([0, 2, 3], [5, 5, 2], [1, 0]), "sco_sqp_create_rows: column indices must lie in [0, dof * horizon) and increase inside a row"),
    ("column falls", ([0, 2, 3], [5, 0, 2], [1, 0]), "sco_sqp_create_rows: column indices must lie in [0, dof * horizon) and increase inside a row"),
    ("column too large", ([0, 2, 3], [0, 6, 2], [1, 0]), "sco_sqp_create_rows: column indices must lie in [0, dof * horizon) and increase inside a row"),
    ("column negative", ([0, 2, 3], [-1, 5, 2], [1, 0]), "sco_sqp_create_rows: column indices must lie in [0, dof * horizon) and increase inside a row"),
    ("n_rows 65537", ([0], [0], [0], 65537), "sco_sqp_create_rows: bad row pattern"),
    ("n_rows negative", ([0], [0], [0], -1), "sco_sqp_create_rows: bad row pattern"),
    ("no column array", ([0, 2, 3], None, [1, 0], 2), "sco_sqp_create_rows: bad row pattern"),
]


def test_general_row_patterns():
    rc, L = _layout(_desc(), GOOD_ROWS)
    assert rc == 0 and (L.m_gen, L.nnz_gen) == (2, 3), _last_error()
    n = 65536                            # the most rows there may be, one entry each
    rc, L = _layout(_desc(), (np.arange(n + 1), np.arange(n) % 6, np.zeros(n)))
    assert rc == 0 and L.m_gen == n and L.m_lin == 4 + n
    for name, rows, text in BAD_ROWS:
        assert _layout(_desc(), rows) == (ERR_ARG, None), name
        assert _last_error() == text, name


# ---------------------------------------------------------------------------
# 3. the program check
# ---------------------------------------------------------------------------
END, OX, OP, OC, ADD, SUB, MUL, DIV, NEG, SIN, COS, SQRT, EXP, SQUARE = range(14)
STACK = 16
LAYOUT, TAIL, MALFORMED, LEFT = ("sco_sqp_load_program: bad program layout", "sco_sqp_load_program: a row's program must end with SCO_OP_END",
                                 "sco_sqp_load_program: malformed program (operand index, stack depth or opcode)",
                                 "sco_sqp_load_program: a row's program must leave exactly one value")


def _check(rows, family=PROGRAM, span=1, dof=2, O=None, circles=0, n_consts=2, n_params=2, row_ptr=None, n_words=None):
    """rows: one list of (op, arg) per program, SCO_OP_END included."""
    words = np.array([w for r in rows for w in r], dtype=np.int32).reshape(-1, 2)
    if row_ptr is None:
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    n_rows = len(rows) - (1 if family & (OBJ_PROGRAM | OBJ_BLOCK) else 0)
    desc = _desc(dof=dof, horizon=5, n_points=1, n_obstacles=(n_rows + circles) if O is None else O, family=family, span=span)
    rc = _lib.load().sco_debug_sqp_check_program(C.byref(desc), circles, len(words) if n_words is None else n_words,
                                                 _lib.iptr(np.ascontiguousarray(words.ravel())),
                                                 _lib.iptr(np.ascontiguousarray(row_ptr, dtype=np.int32)), n_consts, n_params)
    return rc, (_last_error() if rc else "")


def _deep(n):
    """n pushes, then n - 1 additions: needs a stack of n."""
    return [(OX, 0)] * n + [(ADD, 0)] * (n - 1) + [(END, 0)]


ROW = [(OX, 0), (END, 0)]
PROGRAMS = [
    ("ends with SCO_OP_END", dict(rows=[[(OX, 0), (NEG, 0), (END, 0)]]), dict(rows=[[(OX, 0), (NEG, 0)]]), TAIL),
    ("X index, rows", dict(rows=[[(OX, 1), (END, 0)]]), dict(rows=[[(OX, 2), (END, 0)]]), MALFORMED),
    ("X index negative", dict(rows=[[(OX, 0), (END, 0)]]), dict(rows=[[(OX, -1), (END, 0)]]), MALFORMED),
    ("X index, rows of a block of two timesteps", dict(rows=[[(OX, 3), (END, 0)]], span=2), dict(rows=[[(OX, 4), (END, 0)]], span=2), MALFORMED),
    ("X index, objective per block", dict(rows=[ROW, [(OX, 3), (END, 0)]], span=2, family=PROGRAM | OBJ_BLOCK),
     dict(rows=[ROW, [(OX, 4), (END, 0)]], span=2, family=PROGRAM | OBJ_BLOCK), MALFORMED),
    ("X index, objective per timestep", dict(rows=[ROW, [(OX, 1), (END, 0)]], family=PROGRAM | OBJ_PROGRAM),
     dict(rows=[ROW, [(OX, 2), (END, 0)]], family=PROGRAM | OBJ_PROGRAM), MALFORMED),
    ("P index", dict(rows=[[(OP, 1), (END, 0)]]), dict(rows=[[(OP, 2), (END, 0)]]), MALFORMED),
    ("P without parameters", dict(rows=[ROW], n_params=0), dict(rows=[[(OP, 0), (END, 0)]], n_params=0), MALFORMED),
    ("C index", dict(rows=[[(OC, 1), (END, 0)]]), dict(rows=[[(OC, 2), (END, 0)]]), MALFORMED),
    ("binary operation on one value", dict(rows=[[(OX, 0), (OX, 1), (DIV, 0), (END, 0)]]), dict(rows=[[(OX, 0), (DIV, 0), (END, 0)]]), MALFORMED),
    ("unary operation on nothing", dict(rows=[[(OX, 0), (SQUARE, 0), (END, 0)]]), dict(rows=[[(SQUARE, 0), (OX, 0), (END, 0)]]), MALFORMED),
    ("unknown opcode", dict(rows=[[(OX, 0), (SQUARE, 0), (END, 0)]]), dict(rows=[[(OX, 0), (14, 0), (END, 0)]]), MALFORMED),
    ("negative opcode", dict(rows=[ROW]), dict(rows=[[(OX, 0), (-1, 0), (END, 0)]]), MALFORMED),
    ("SCO_OP_END inside", dict(rows=[ROW]), dict(rows=[[(OX, 0), (END, 0), (END, 0)]]), MALFORMED),
    ("stack depth", dict(rows=[_deep(STACK)]), dict(rows=[_deep(STACK + 1)]), MALFORMED),
    ("one value left", dict(rows=[[(OX, 0), (OX, 1), (SUB, 0), (END, 0)]]), dict(rows=[[(OX, 0), (OX, 1), (END, 0)]]), LEFT),
    ("no value left", dict(rows=[ROW]), dict(rows=[[(END, 0)]]), LEFT),
    ("row_ptr[0]", dict(rows=[ROW, ROW]), dict(rows=[ROW, ROW], row_ptr=[1, 2, 4]), LAYOUT),
    ("row_ptr increases", dict(rows=[ROW, ROW]), dict(rows=[ROW, ROW], row_ptr=[0, 2, 2], O=2), LAYOUT),
    ("row_ptr falls", dict(rows=[ROW, ROW]), dict(rows=[ROW, ROW], row_ptr=[0, 4, 2], O=2), LAYOUT),
    ("row_ptr beyond the words", dict(rows=[ROW, ROW]), dict(rows=[ROW, ROW], row_ptr=[0, 2, 5]), LAYOUT),
    ("row_ptr[R] = n_words", dict(rows=[ROW, ROW]), dict(rows=[ROW, ROW, ROW], row_ptr=[0, 2, 4], O=2), LAYOUT),
    ("objective program missing", dict(rows=[ROW, ROW], family=PROGRAM | OBJ_PROGRAM), dict(rows=[ROW, ROW], family=PROGRAM | OBJ_PROGRAM, O=2, row_ptr=[0, 2, 4, 4]), LAYOUT),
    ("circle rows take no program", dict(rows=[ROW], circles=1), dict(rows=[ROW, ROW], circles=1, O=2), LAYOUT),
    ("n_words", dict(rows=[ROW]), dict(rows=[ROW], n_words=0), LAYOUT),
    ("n_consts", dict(rows=[ROW], n_consts=0), dict(rows=[ROW], n_consts=-1), LAYOUT),
    ("n_params", dict(rows=[ROW], n_params=0), dict(rows=[ROW], n_params=-1), LAYOUT),
]


@pytest.mark.parametrize("name,good,bad,text", PROGRAMS, ids=[c[0] for c in PROGRAMS])
def test_program_check(name, good, bad, text):
    assert _check(**good) == (0, "")
    assert _check(**bad) == (ERR_ARG, text)


def test_program_check_needs_the_program_family():
    assert _check([ROW, ROW], family=QUADRATIC) == (ERR_ARG, "sco_sqp_load_program: family has no row programs")
    assert _check([ROW], dof=0) == (ERR_ARG, "sco_sqp_create: bad descriptor")
