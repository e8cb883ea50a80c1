// qp_polish_plan.h -- launch planning of the polish step (sco_qp_polish.hip): host arithmetic only, no device types.
//
// Polish solves, per problem, one dense regularised KKT system of order N = n + k (k = active rows) by an unpivoted
// LDL'.  The dense image of a problem is ld x ld doubles (ld = N rounded up to the 16-wide tile of the factor kernel), and
// the batch is cut into chunks so that the images of one chunk stay under a byte budget.  What the call allocates and
// launches is decided here from plain numbers, so that it can be read, and tested, without a GPU (tests/test_qp_polish.py,
// through sco_debug_polish_plan; scripts/sanitize/polish_plan_sweep.cpp).
#pragma once
#include "../../include/sco_hip.h"

#define SCO_POLISH_TILE 16            // panel width of the factor kernel = edge of an MFMA tile
#define SCO_POLISH_MAX_ORDER 1104     // largest reduced order: holds n + m = 1094 of the 7-DOF x 20 penalty QP (69 tiles)
#define SCO_POLISH_WS_BYTES (1ll << 30)   // default budget of the dense workspace

enum QpPolishErr { QP_POLISH_ERR_NONE = 0, QP_POLISH_ERR_ARG, QP_POLISH_ERR_ORDER, QP_POLISH_ERR_BUDGET };
const char *qp_polish_err_text(int err);

struct QpPolishPlan {
  int rc = SCO_OK, err = QP_POLISH_ERR_NONE;
  int ld = 0;          // leading dimension of a problem's image: n + max_k rounded up to SCO_POLISH_TILE
  int per_chunk = 0;   // problems whose images share the workspace
  int chunks = 0;      // launches of the assemble / factor / solve kernels
  int lds_bytes = 0;   // dynamic LDS of the factor kernel: the 16-column panel (column-major, ld rows), the pivot column's
                       // 16 unscaled entries and the panel's 16 pivots
  long long ws_bytes = 0;   // workspace the call allocates: per_chunk * ld * ld doubles
};

// max_k: most active rows of a problem of the batch (0 .. m); budget: bytes the workspace may take (<= 0: the default,
// or SCO_QP_POLISH_WS_MB megabytes when the environment sets it).  Refusals: a bad argument (SCO_ERR_ARG), n + max_k beyond
// SCO_POLISH_MAX_ORDER, or a budget that does not hold one problem (both SCO_ERR_CAPACITY).
QpPolishPlan qp_polish_plan(int n, int m, int batch, int max_k, long long budget);
// the trailing update of the factor kernel runs on v_mfma_f64_16x16x4 unless SCO_QP_POLISH_NO_MFMA=1 is in the environment
// (read at every call) or the library was built with -DSCO_QP_POLISH_NO_MFMA: then the vector-ALU form of the same tiles
bool qp_polish_use_mfma();
// what sco_qp_polish checks before its first launch: the order the pattern can reach, n + m
bool qp_polish_order_fits(int n, int m);
