"""Cases of tests/golden/trajopt_blockobj4.npz: block objective terms at span 4 and on 16-number block states.
(prefix, workloads.make_problem kwargs, problem index, analytic_jac) -- make_problem(i, block_obj=<kind>, ...)."""
S4 = dict(block_obj="smooth4", T=8)
CASES = [("s40_", dict(S4), 0, False),                                                # span 4 at dof 2: four blocks share an entry
         ("s4w_", dict(block_obj="smooth4", d=4, T=5), 0, False),                     # dof 4: 16 numbers, T = span + 1 (two blocks)
         ("s4a_", dict(S4, acc_weights=True, per_step=True), 1, False),               # the acceleration term inside the band
         ("s4v_", dict(S4, vel_limit=0.6, groups="halves"), 0, False),                # velocity limits, constraint groups
         ("s4j_", dict(S4), 2, True),                                                 # the rows' forward-mode Jacobian
         ("e8_", dict(block_obj="ee-path", d=8, T=4), 0, False)]                      # end-effector path length at dof 8, ds = 16
