// qp_tier.h -- tier choice and launch planning of the QP layer (sco_qp.hip): host arithmetic only, no device types.
//
// What a launch on a handle does -- which checks it fails, the slice, the tier, which problems get the dense inverse,
// the factor kernel, the sequence of ADMM launches -- is decided here from plain numbers, so that it can be read, and
// tested, without a GPU (tests/test_qp_launch_plan.py, through sco_debug_qp_launch_plan).  sco_qp_launch_sliced issues
// what the plan says and decides nothing again.
//
// What sco_qp_create decides from the environment is read here and nowhere else (qp_create_env): the tier choice and
// every tier planner take a QpCreateEnv and call getenv nowhere.  Three launch-time variables are read elsewhere, on
// purpose, at every launch: SCO_WV_MIN_PER_CU below (sco_wv_min_live), SCO_QP_BT_TRIPLE in big_launch (sco_qp_big.hip) and
// SCO_WV_ABLATE in wv_fill_args (sco_admm_wv.hip; only a -DWV_ABLATE build acts on it).
#pragma once
#include "../../include/sco_hip.h"

#define SCO_FACTOR_BLOCK 1024   // threads of the factor kernels (qp_sweep_kernel, qp_factor_kernel)

// The create-time switches, read once per sco_qp_create (qp_create_env).  Each is on only when the variable's first
// character is '1', but for the last four.
struct QpCreateEnv {
  bool factor_cholesky = false;  // SCO_QP_FACTOR_CHOLESKY: W by Cholesky + triangular inverse (cross-check)
  bool no_elim = false;          // SCO_QP_NO_ELIM: no variable is eliminated (dense core of order n)
  bool force_big = false;        // SCO_QP_FORCE_BIG: the global-memory tier whatever the working set
  bool no_bt = false;            // SCO_QP_NO_BT: not its structured form
  bool no_rl = false, no_wv = false, no_reg = false, no_fast = false;   // SCO_QP_NO_RL / _WV / _REG / _FAST
  // what the tier planners read
  bool no_mfma = false;          // SCO_QP_NO_MFMA: structured global-memory form without the matrix cores (bt_plan_build)
  bool rl_closed = false;        // SCO_QP_RL_ALIGNED or SCO_QP_RL_CLOSED: the aligned closed assignment (rl_plan_build)
  bool rl_lay8 = false;          // SCO_QP_RL_LAY8: 8 column groups of the W tile with the open assignment
  bool rl_split_off = false;     // SCO_QP_RL_SPLIT: on only at '0' -- a column's pairs all on the owner lane
  bool debug_plan = false;       // SCO_DEBUG_PLAN: on when set -- the closed assignment prints its components to stderr
  bool wv_jsort = true;          // SCO_WV_JSORT: off only at '0' -- with a width hint, a block's hinge rows are dealt to the slots widest first (wv_plan_build)
  bool wv_jw_off = false;        // SCO_WV_JW: on only at '0' -- the wavefront tier ignores Jacobian width hints (wv_plan_widths)
};
QpCreateEnv qp_create_env();

// fewest live problems for which a round runs on the wavefront tier (SCO_WV_MIN_PER_CU, read at every call)
int sco_wv_min_live(int cus, bool adaptive = false);
int sco_qp_adaptive_interval(const sco_qp_settings *st);

// the ADMM kernel of an on-chip handle: the first of these whose plan fits the pattern (one per handle)
enum QpKernel { QP_K_RL = 0, QP_K_REG = 1, QP_K_FAST = 2, QP_K_GENERIC = 3 };
enum QpMaskKind { QP_MASK_ARRAY = 0, QP_MASK_ALL = 1, QP_MASK_NONE = 2 };     // the setup mask of a launch

struct QpLaunchIn {
  // the handle
  int kern = QP_K_GENERIC;
  bool use_big = false, use_bt = false;      // global-memory tier / its structured form
  bool use_wv = false;                       // wavefront tier beside the row-local kernel
  bool wv_links = false;                     // ... and its plan holds link or stacked rows (no adaptive-rho instantiation)
  bool factor_cholesky = false;
  int batch = 0, n_c = 0;
  int cus = 0;                               // (wv_min comes from it; the planner itself does not read it)
  // the settings
  int adaptive_rho = 0, adaptive_rho_interval = 0, check_termination = 0, max_iter = 0;
  double adaptive_rho_tolerance = 0.0;
  // the call
  int slice = 0;                             // requested
  int mask = QP_MASK_ARRAY;
  int wv_min = 0;                            // sco_wv_min_live
  bool window = false;                       // a QpGroup is given; the rest describes it
  int b0 = 0, nb = 0, tier = 0;
  bool has_list = false;
  int side_b0 = 0, side_nb = 0, side_slices = 0;
  bool side_ready = false;                   // the side stream and its three events are all there
};

enum QpLaunchErr { QP_ERR_NONE = 0, QP_ERR_WINDOW, QP_ERR_ADAPT_DENSE, QP_ERR_ADAPT_SETTINGS, QP_ERR_MIXED };
const char *qp_launch_err_text(int err);
enum QpRoute { QP_ROUTE_BIG_DENSE = 0, QP_ROUTE_BIG_BT = 1, QP_ROUTE_ONCHIP = 2 };
// problems that get the dense inverse besides those of the setup mask (wv_launch_need): none, the active ones of the
// window whose QP the wavefront tier factored, or those of a mixed round's side window, after the wavefront factorisation
enum QpNeed { QP_NEED_NONE = 0, QP_NEED_WINDOW = 1, QP_NEED_SIDE = 2 };
enum QpAdmmSeq { QP_ADMM_GENERIC = 0, QP_ADMM_FAST, QP_ADMM_REG, QP_ADMM_RL, QP_ADMM_WV_RL, QP_ADMM_MIXED };

struct QpLaunchPlan {
  int rc = SCO_OK, err = QP_ERR_NONE;
  int slice = -1;            // rounded slice, what *sliced gets; -1: a check failed before it was known
  int nwg = 0;               // workgroups of the per-problem kernels
  int ad_interval = 0;       // adaptive rho: iterations between two rho estimates (0: fixed rho)
  bool rho_init = false;     // qp_rho_init_kernel runs
  int route = QP_ROUTE_ONCHIP;
  // on-chip route only
  bool wv_now = false, mixed = false;
  int need = QP_NEED_NONE;
  bool cholesky = false;     // qp_factor_kernel, else qp_sweep_kernel<sweep_nt>
  int sweep_nt = 1;
  int admm = QP_ADMM_GENERIC;
};
// The checks run in this order, and the first that fails names the error: window, adaptive rho, mixed round.
QpLaunchPlan qp_launch_plan(const QpLaunchIn &in);
// launch windows and index lists exist for the paths the bench workloads take: row-local kernel with the Gauss-Jordan
// inversion, and the structured global-memory tier; fixed rho
bool qp_supports_windows(const QpLaunchIn &in);
