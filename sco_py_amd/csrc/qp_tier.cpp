// qp_tier.cpp -- tier choice and launch planning of the QP layer: see qp_tier.h.
#include "qp_tier.h"

#include <algorithm>
#include <climits>
#include <cstdlib>

QpCreateEnv qp_create_env() {
  auto on = [](const char *name) { const char *v = getenv(name); return v && v[0] == '1'; };
  QpCreateEnv e;
  e.factor_cholesky = on("SCO_QP_FACTOR_CHOLESKY"); e.no_elim = on("SCO_QP_NO_ELIM");
  e.force_big = on("SCO_QP_FORCE_BIG"); e.no_bt = on("SCO_QP_NO_BT");
  e.no_rl = on("SCO_QP_NO_RL"); e.no_wv = on("SCO_QP_NO_WV"); e.no_reg = on("SCO_QP_NO_REG"); e.no_fast = on("SCO_QP_NO_FAST");
  e.no_mfma = on("SCO_QP_NO_MFMA");
  e.rl_closed = on("SCO_QP_RL_ALIGNED") || on("SCO_QP_RL_CLOSED"); e.rl_lay8 = on("SCO_QP_RL_LAY8");
  { const char *v = getenv("SCO_QP_RL_SPLIT"); e.rl_split_off = v && v[0] == '0'; }
  e.debug_plan = getenv("SCO_DEBUG_PLAN") != nullptr;
  { const char *v = getenv("SCO_WV_JW"); e.wv_jw_off = v && v[0] == '0'; }
  { const char *v = getenv("SCO_WV_JSORT"); e.wv_jsort = !(v && v[0] == '0'); }
  return e;
}

// fewest problems of a launch for which the wavefront tier is the faster one (SCO_WV_MIN_PER_CU: problems per CU, default 2.75;
// 3.0 until the SQP loop learnt mixed rounds, which fill the CUs such a round leaves free: on the 1024-problem 7x20 step 2.5 .. 3.0
// give the same schedule and 2.0 and below a slower one, a step that starts with 700 problems is a quarter faster on this tier
// (profiles/mixed_rounds.md) -- but the schedule tests pin a 700-problem batch, 2.73 per CU of 256, to row-local rounds).
// With adaptive rho the default is "never": a launch then goes by the size of the BATCH, not by how many of its problems are
// still alive (no round selection), a solve parks at every rho change and the launches are short and mostly narrow.  Measured
// on `bench.py --beyond` (1024 problems, 4 per CU, 122 launches of ~100 iterations per step): 503 ms of ADMM launches per
// step on this tier against 285 ms on the row-local kernel (profiles/wv_extensions.md).  The variable still applies when set.
// A plan with link rows (velocity limits) goes by the same rule as a link-free one: on the 1024-problem 7x20 step every run on
// this tier was faster than every run on the row-local kernel (profiles/wv_link_rows.md).
// So does a plan with stacked rows (joint limits: single rows in link slots): 3560 .. 3581 SCO it/s on this tier against
// 2288 .. 2298 on the row-local kernel, three alternating pairs (profiles/wv_stacked_rows.md).
int sco_wv_min_live(int cus, bool adaptive) {
  const char *e = getenv("SCO_WV_MIN_PER_CU");
  if (!e && adaptive) return INT_MAX;
  const double live = (e ? atof(e) : 2.75) * (cus > 0 ? cus : 256);
  return live >= (double)INT_MAX ? INT_MAX : (int)live;
}

int sco_qp_adaptive_interval(const sco_qp_settings *st) {
  if (st->adaptive_rho_interval > 0) {
    // park points sit on termination checks
    if (st->check_termination > 0)
      return std::max(1, (st->adaptive_rho_interval + st->check_termination / 2) / st->check_termination) * st->check_termination;
    return st->adaptive_rho_interval;
  }
  return st->check_termination > 0 ? 4 * st->check_termination : 100;
}

const char *qp_launch_err_text(int err) {
  switch (err) {
    case QP_ERR_WINDOW: return "sco_qp_launch_sliced: launch window not supported by this handle's tier";
    case QP_ERR_ADAPT_DENSE: return "adaptive_rho: the dense form of the global-memory tier cannot park a solve";
    case QP_ERR_ADAPT_SETTINGS: return "adaptive_rho needs adaptive_rho_tolerance > 1 and check_termination > 0";
    case QP_ERR_MIXED: return "sco_qp_launch_sliced: mixed round not supported by this handle or its side window is malformed";
  }
  return "";
}

bool qp_supports_windows(const QpLaunchIn &in) {
  if (in.adaptive_rho) return false;
  if (in.use_big) return in.use_bt;                        // structured global-memory tier
  return in.kern == QP_K_RL && !in.factor_cholesky;
}

static QpLaunchPlan plan_error(QpLaunchPlan p, int rc, int err) { p.rc = rc; p.err = err; return p; }

QpLaunchPlan qp_launch_plan(const QpLaunchIn &in) {
  QpLaunchPlan p;
  const bool adaptive = in.adaptive_rho != 0;
  if (in.window && (!qp_supports_windows(in) || in.b0 < 0 || in.nb <= 0 || in.b0 + in.nb > in.batch))
    return plan_error(p, SCO_ERR_STATE, QP_ERR_WINDOW);
  if (adaptive) {
    if (in.use_big && !in.use_bt) return plan_error(p, SCO_ERR_CAPACITY, QP_ERR_ADAPT_DENSE);
    if (!(in.adaptive_rho_tolerance > 1.0) || in.check_termination <= 0) return plan_error(p, SCO_ERR_ARG, QP_ERR_ADAPT_SETTINGS);
  }
  // every on-chip kernel and the structured global-memory form park and resume a solve; the dense form runs one launch
  // per solve
  const bool can_park = in.use_big ? in.use_bt : true;
  if (!can_park || in.check_termination <= 0 || (in.slice <= 0 && !adaptive)) {
    p.slice = 0;
  } else {
    // slices end on a termination check; adaptive rho without time slicing parks only when rho changes
    const int want = in.slice <= 0 ? in.max_iter : in.slice;
    p.slice = std::max(1, (want + in.check_termination - 1) / in.check_termination) * in.check_termination;
  }
  p.nwg = in.window ? in.nb : in.batch;
  if (adaptive) {
    sco_qp_settings st{};
    st.adaptive_rho_interval = in.adaptive_rho_interval; st.check_termination = in.check_termination;
    p.ad_interval = sco_qp_adaptive_interval(&st);
  }
  // The wavefront tier puts four problems on a CU at ~3.1 us per iteration each where the row-local kernel runs one at
  // ~0.95 us: it is the faster way through a launch only with more than ~3 problems per CU to run (profiles/r04_wv.txt).
  // The SQP loop says per round which one it wants (the window's tier, from its live count: 1 row-local, 2 wavefront,
  // 3 mixed); a launch without a wish goes by its size.
  p.mixed = in.window && in.tier == 3;
  if (p.mixed) {
    const bool at_end = in.side_b0 == in.b0 || in.side_b0 + in.side_nb == in.b0 + in.nb;
    if (!in.use_wv || in.kern != QP_K_RL || adaptive || p.slice <= 0 || !in.has_list || in.side_nb <= 0 || in.side_nb >= in.nb ||
        !at_end || in.side_slices <= 0 || !in.side_ready)
      return plan_error(p, SCO_ERR_STATE, QP_ERR_MIXED);
  }
  // (link rows have no adaptive-rho instantiation on that tier: such launches stay on the row-local kernel)
  p.wv_now = in.use_wv && !(adaptive && in.wv_links) && (in.window && in.tier ? in.tier >= 2 : p.nwg >= in.wv_min);
  p.rho_init = adaptive && in.mask != QP_MASK_NONE;
  p.route = in.use_big ? (in.use_bt ? QP_ROUTE_BIG_BT : QP_ROUTE_BIG_DENSE) : QP_ROUTE_ONCHIP;
  if (p.route != QP_ROUTE_ONCHIP) { p.wv_now = false; return p; }
  p.need = p.wv_now ? (p.mixed ? QP_NEED_SIDE : QP_NEED_NONE) : (in.use_wv ? QP_NEED_WINDOW : QP_NEED_NONE);
  p.cholesky = in.factor_cholesky;
  // tiles of 4 x 4 in the lower triangle of the core, SCO_FACTOR_BLOCK threads: 1 per thread up to order 176, 2 up to 252
  const int nb4 = (in.n_c + 3) / 4, ntiles = nb4 * (nb4 + 1) / 2;
  p.sweep_nt = ntiles <= SCO_FACTOR_BLOCK ? 1 : ntiles <= 2 * SCO_FACTOR_BLOCK ? 2 : 3;
  switch (in.kern) {
    case QP_K_RL: p.admm = p.mixed ? QP_ADMM_MIXED : p.wv_now ? QP_ADMM_WV_RL : QP_ADMM_RL; break;
    case QP_K_REG: p.admm = QP_ADMM_REG; break;
    case QP_K_FAST: p.admm = QP_ADMM_FAST; break;
    default: p.admm = QP_ADMM_GENERIC;
  }
  return p;
}

// ---- debug entry point (include/sco_hip.h): the launch planner on plain numbers
extern "C" int sco_debug_qp_launch_plan(const int *in, const double *tol, int *out) {
  if (!in || !tol || !out) return -1;
  QpLaunchIn li;
  li.kern = in[0]; li.use_big = in[1] != 0; li.use_bt = in[2] != 0; li.use_wv = in[3] != 0; li.wv_links = in[3] == 2; li.factor_cholesky = in[4] != 0;
  li.batch = in[5]; li.n_c = in[6]; li.cus = in[7];
  li.adaptive_rho = in[8]; li.adaptive_rho_interval = in[9]; li.check_termination = in[10]; li.max_iter = in[11];
  li.adaptive_rho_tolerance = *tol;
  li.slice = in[12]; li.mask = in[13];
  const int wv_min_live = sco_wv_min_live(li.cus, li.adaptive_rho != 0);
  li.wv_min = in[14] >= 0 ? in[14] : wv_min_live;
  li.window = in[15] != 0; li.b0 = in[16]; li.nb = in[17]; li.tier = in[18]; li.has_list = in[19] != 0;
  li.side_b0 = in[20]; li.side_nb = in[21]; li.side_slices = in[22]; li.side_ready = in[23] != 0;
  const QpLaunchPlan p = qp_launch_plan(li);
  sco_qp_settings st{};
  st.adaptive_rho_interval = li.adaptive_rho_interval; st.check_termination = li.check_termination;
  const int o[15] = {p.rc, p.err, p.slice, p.nwg, p.rho_init, p.route, p.wv_now, p.mixed, p.need, p.cholesky, p.sweep_nt, p.admm,
                     p.ad_interval, wv_min_live, sco_qp_adaptive_interval(&st)};
  std::copy(o, o + 15, out);
  return 0;
}
