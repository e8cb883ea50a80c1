// qp_tier_choice.cpp -- which tiers a handle runs, from its pattern and the create-time switches (qp_tier_plans.h).  Plain
// C++, no HIP call; beside qp_tier.cpp, which stays free of the tier planners.
#include "qp_tier_plans.h"

#include <cstdio>

// Step 1 of sco_qp_create: everything that is decided about the handle, from the pattern and the switches alone.  No HIP
// call: sco_debug_plan_tiers runs it on a machine without a GPU.
int qp_choose_tiers(int n, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai, const QpCreateEnv &env,
                    QpTiers &t, std::string *err) {
  t.factor_cholesky = env.factor_cholesky;
  int rc = qp_plan_build(n, m, Pp, Pi, Ap, Ai, env.no_elim ? 0 : 1, t.plan);
  if (rc != 0) { *err = "sco_qp_create: malformed sparsity pattern"; return SCO_ERR_ARG; }
  const QpPlan &pl = t.plan;
  t.lds_setup = setup_lds_doubles(pl) * sizeof(double);
  t.lds_admm = admm_lds_doubles(n, m, pl.nnzA, pl.n_e, pl.n_c, pl.ncpl) * sizeof(double) + (size_t)m * sizeof(int);
  if (t.lds_setup > SCO_LDS_CAP || t.lds_admm > SCO_LDS_CAP || pl.n_c > SCO_BLOCK || env.force_big) {
    // working set beyond a CU's LDS: the global-memory tier (sco_qp_big.hip)
    bool ok_big = pl.n_c <= 1024 && big_plan_build(pl, t.big);
    if (!ok_big && !env.no_elim) {
      // the global-memory kernels keep an eliminated variable and its (at most two) rows in one thread:
      // send variables with more rows to the core and analyse again
      rc = qp_plan_build(n, m, Pp, Pi, Ap, Ai, 2, t.plan);
      if (rc != 0) { *err = "sco_qp_create: malformed sparsity pattern"; return SCO_ERR_ARG; }
      t.big = BigHost();
      ok_big = pl.n_c <= 1024 && big_plan_build(pl, t.big);
    }
    if (!ok_big) {
      char buf[256];
      snprintf(buf, sizeof buf, "sco_qp_create: pattern not supported (setup %zu B, admm %zu B of LDS, core %d)",
               t.lds_setup, t.lds_admm, pl.n_c);
      *err = buf; return SCO_ERR_CAPACITY;
    }
    t.use_big = true;
    t.use_bt = !env.no_bt && bt_plan_build(pl, t.big, t.bt, env.no_mfma);
    return SCO_OK;
  }
  // on-chip: the first ADMM kernel whose plan fits the pattern is the one this handle runs
  int CW = 0, RW = 0, PX = 0;
  if (!env.no_rl && rl_plan_build(pl, t.rl, env)) {
    t.kern = QP_K_RL;
    // wavefront tier (one wavefront per problem, block-tridiagonal core solve): patterns of trajectory penalty QPs; it
    // needs the row-local kernel beside it for problems whose values leave the penalty-QP structure, and the Gauss-Jordan
    // inversion.  The opt-in extensions (warm start, adaptive rho) run on it too; rows that link two neighbouring timesteps
    // (velocity limits) are allowed, without adaptive rho
    t.use_wv = !env.factor_cholesky && !env.no_wv && wv_plan_build(pl, t.wv, true);
  } else if (!env.no_reg && reg_caps_for(pl, &CW, &RW, &PX) && reg_plan_build(pl, CW, RW, PX, t.reg)) {
    t.kern = QP_K_REG;
  } else if (!env.no_fast && fast_plan_build(pl, t.fast)) {
    t.kern = QP_K_FAST;
  }
  return SCO_OK;
}

// Which ADMM tiers a handle RUNS: bit 0 row-local, 1 register-offset, 2 sliced-ELL (at most one of the three: the handle's
// on-chip kernel; none = the generic kernel), 3 global memory, 4 its structured form, 5 wavefront tier beside the row-local
// kernel, 6 the structured form builds its block normal matrices on the matrix cores (MFMA).  (Bits 1 and 2 said "holds the
// plan" while handles still built plans they could never launch.)
int qp_tier_mask(const QpTiers &t) {
  return (t.kern == QP_K_RL ? 1 : 0) | (t.kern == QP_K_REG ? 2 : 0) | (t.kern == QP_K_FAST ? 4 : 0) | (t.use_big ? 8 : 0) |
         (t.use_bt ? 16 : 0) | (t.use_wv ? 32 : 0) | ((t.use_bt && t.bt.use_mfma) ? 64 : 0);
}
