"""Cases of the spatial-arm family (SCO_FAM_ARM_SPATIAL).

GOLDEN: the runs of tests/golden/trajopt_spatial.npz, (prefix, make_problem kwargs, problem index, analytic Jacobian),
recorded from the reference's own modules by tests/golden/make_golden_spatial.py.

CONFIGS / SEEDS: the device parity runs of tests/test_spatial_arm_gpu.py.  A seed is used only if the flat oracle takes the
same decisions (kinds, QP statuses, iteration counts) and ends within 1e-9 of the same trajectory whether the forward
kinematics run in float64 or in numpy.longdouble rounded to float64 -- a run that fails this hangs on the last bit of
a row value, which the device's sincos need not share.  scripts/spatial_screen_seeds.py screens the first 8 seeds of
every configuration and prints this table; at most 2 of 8 may be dropped."""
SMALL = dict(d=3, T=6, K=2, O=2, spatial=True)
MID = dict(d=7, T=12, K=5, O=2, spatial=True)
INTENDED = dict(compound_penalty=False, duplicate_rows=False)

GOLDEN = [("s0_", dict(SMALL), 0, False), ("s0a_", dict(SMALL), 0, True), ("sv1_", dict(SMALL, d=4, T=8, vel_limit=0.45), 1, False)]

# name -> (make_problem kwargs, solver parameters (oracle.sco_ref.SolverParams names), analytic Jacobian)
CONFIGS = {
    "small-parity": (dict(SMALL), {}, False),
    "small-intended": (dict(SMALL), INTENDED, False),
    "small-analytic": (dict(SMALL), {}, True),
    "small-vel": (dict(SMALL, vel_limit=0.45), {}, False),
    "small-jl-groups": (dict(SMALL, joint_limit=0.15, groups="split"), {}, False),
    "mid-parity": (dict(MID), {}, False),
    "mid-intended": (dict(MID), INTENDED, False),
}

# as screened: no seed dropped (worst |dx| between the two evaluations 3.5e-13; the intended-mode runs take 3 .. 20 QPs)
SEEDS = {
    "small-parity": [0, 1, 2, 3, 4, 5, 6, 7],
    "small-intended": [0, 1, 2, 3, 4, 5, 6, 7],
    "small-analytic": [0, 1, 2, 3, 4, 5, 6, 7],
    "small-vel": [0, 1, 2, 3, 4, 5, 6, 7],
    "small-jl-groups": [0, 1, 2, 3, 4, 5, 6, 7],
    "mid-parity": [0, 1, 2, 3, 4, 5, 6, 7],
    "mid-intended": [0, 1, 2, 3, 4, 5, 6, 7],
}
