// qp_polish_plan.cpp -- see qp_polish_plan.h.  Host only: compiled into libsco_hip.so and, on its own, into the sanitizer
// driver scripts/sanitize/polish_plan_sweep.cpp.
#include "qp_polish_plan.h"

#include <cstdlib>

const char *qp_polish_err_text(int err) {
  switch (err) {
    case QP_POLISH_ERR_ARG: return "sco_qp_polish: bad sizes";
    case QP_POLISH_ERR_ORDER: return "sco_qp_polish: the reduced KKT system is larger than SCO_POLISH_MAX_ORDER (1104)";
    case QP_POLISH_ERR_BUDGET: return "sco_qp_polish: the workspace budget does not hold the dense image of one problem";
  }
  return "";
}

bool qp_polish_order_fits(int n, int m) { return (long long)n + (long long)m <= SCO_POLISH_MAX_ORDER; }

bool qp_polish_use_mfma() {
#ifdef SCO_QP_POLISH_NO_MFMA
  return false;
#else
  const char *e = getenv("SCO_QP_POLISH_NO_MFMA");
  return !(e && e[0] == '1');
#endif
}

static long long polish_budget(long long budget) {
  if (budget > 0) return budget;
  if (const char *e = getenv("SCO_QP_POLISH_WS_MB")) {
    char *end = nullptr;
    const long long mb = strtoll(e, &end, 10);
    if (end != e && mb > 0 && mb <= (1ll << 20)) return mb << 20;
  }
  return SCO_POLISH_WS_BYTES;
}

QpPolishPlan qp_polish_plan(int n, int m, int batch, int max_k, long long budget) {
  QpPolishPlan p;
  if (n <= 0 || m < 0 || batch <= 0 || max_k < 0 || max_k > m) { p.rc = SCO_ERR_ARG; p.err = QP_POLISH_ERR_ARG; return p; }
  const long long N = (long long)n + max_k;
  if (N > SCO_POLISH_MAX_ORDER) { p.rc = SCO_ERR_CAPACITY; p.err = QP_POLISH_ERR_ORDER; return p; }
  const long long ld = (N + SCO_POLISH_TILE - 1) / SCO_POLISH_TILE * SCO_POLISH_TILE;
  const long long image = ld * ld * (long long)sizeof(double);
  long long per = polish_budget(budget) / image;
  if (per < 1) { p.rc = SCO_ERR_CAPACITY; p.err = QP_POLISH_ERR_BUDGET; return p; }
  if (per > batch) per = batch;
  p.ld = (int)ld;
  p.per_chunk = (int)per;
  p.chunks = (int)((batch + per - 1) / per);
  p.lds_bytes = (int)((SCO_POLISH_TILE * ld + 2 * SCO_POLISH_TILE) * (long long)sizeof(double));
  p.ws_bytes = per * image;
  return p;
}
