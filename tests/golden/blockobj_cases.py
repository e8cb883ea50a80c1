"""Cases of tests/golden/trajopt_blockobj.npz: objective programs per constraint block (SCO_FAM_FLAG_OBJ_BLOCK).
(prefix, workloads.make_problem kwargs, problem index, analytic_jac) -- make_problem(i, block_obj=<kind>, ...)."""
EF = dict(block_obj="effort", T=8)
S3 = dict(block_obj="smooth3", T=8)
CASES = [("ef0_", dict(EF), 0, False), ("ef2_", dict(EF), 2, False),
         ("efs_", dict(EF, per_step=True), 1, False),                              # parameters per timestep
         ("efv_", dict(EF, vel_limit=0.6, groups="halves"), 0, False),             # velocity limits, constraint groups
         ("efw_", dict(EF, obj_weights=True, acc_weights=True), 3, False),         # weighted smoothing + acceleration term (S = 2)
         ("eja_", dict(EF), 0, True),                                              # the rows' forward-mode Jacobian
         ("ee0_", dict(block_obj="ee-path", d=4, T=6), 0, False),                  # end-effector path length, ds = 8
         ("s30_", dict(S3), 0, False), ("s31_", dict(S3), 3, False),               # span 3: three blocks share an entry
         ("s3a_", dict(S3, acc_weights=True, per_step=True), 1, False)]            # span 3 with the acceleration term in the band
