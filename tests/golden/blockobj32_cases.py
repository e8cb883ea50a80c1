"""Cases of tests/golden/trajopt_blockobj32.npz: objective terms on 17 to 32 numbers (SCO_FAM_FLAG_OBJ_WIDE).
(prefix, workloads.make_problem kwargs, problem index, analytic_jac) -- make_problem(i, block_obj=<kind>, wide=True, ...);
"attract" is the span-1 objective term of a timestep (SCO_FAM_FLAG_OBJ_PROGRAM) at dof 20."""
CASES = [("e12_", dict(block_obj="ee-path", d=12, T=4, wide=True), 0, False),                          # span 2 x dof 12: 24 numbers
         ("e16_", dict(block_obj="ee-path", d=16, T=3, wide=True), 0, False),                          # span 2 x dof 16: 32
         ("s38_", dict(block_obj="smooth3", d=8, T=5, wide=True), 0, False),                           # span 3 x dof 8: 24
         ("s3a_", dict(block_obj="smooth3", d=10, T=5, wide=True, per_step=True, acc_weights=True), 1, False),   # 30, steps, acc
         ("s48_", dict(block_obj="smooth4", d=8, T=5, wide=True), 0, False),                           # span 4 x dof 8: 32
         ("s3v_", dict(block_obj="smooth3", d=8, T=6, wide=True, vel_limit=0.6, groups="halves"), 0, False),     # limits, groups
         ("e12j_", dict(block_obj="ee-path", d=12, T=4, wide=True), 2, True),                          # the rows' analytic Jacobian
         ("a20_", dict(block_obj="attract", d=20, T=5, wide=True), 0, False)]                          # a timestep's term, dof 20
