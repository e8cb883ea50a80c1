// Stand-alone sweep of the polish planner (csrc/qp_polish_plan.cpp) for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       scripts/sanitize/polish_plan_sweep.cpp sco_py_amd/csrc/qp_polish_plan.cpp -o polish_plan_sweep && ./polish_plan_sweep
// n 1 .. 1200 x m in {0, 1, n / 2, n, 2 n} x every k that matters (0, 1, the tile edges, m) x batches 1, 7, 1024, 2^30 x budgets
// from 1 byte to 2^62 (and <= 0, the default and the environment's).  Every accepted plan must hold the order in ld, cover the
// batch with its chunks, stay inside the budget and inside the LDS of a CU; every refusal must have a text.
#include <cstdio>
#include <cstdlib>

#include "../../sco_py_amd/csrc/qp_polish_plan.h"

static int check(int n, int m, int batch, int k, long long budget, long long eff_budget, long long *acc, long long *ref) {
  const QpPolishPlan p = qp_polish_plan(n, m, batch, k, budget);
  if (p.rc != SCO_OK) {
    (*ref)++;
    if (!qp_polish_err_text(p.err)[0] || (p.rc != SCO_ERR_CAPACITY && p.rc != SCO_ERR_ARG)) { printf("refusal without a text or code\n"); return 1; }
    if (p.ld || p.per_chunk || p.chunks || p.ws_bytes) { printf("refused plan with sizes\n"); return 1; }
    // a refusal must have a reason
    const bool bad_arg = n <= 0 || m < 0 || batch <= 0 || k < 0 || k > m;
    const long long N = (long long)n + k, ld = (N + 15) / 16 * 16;
    if (!bad_arg && N <= SCO_POLISH_MAX_ORDER && ld * ld * 8 <= eff_budget) { printf("refused without a reason: n %d k %d\n", n, k); return 1; }
    return 0;
  }
  (*acc)++;
  const long long N = (long long)n + k;
  if (p.ld % SCO_POLISH_TILE || p.ld < N || p.ld >= N + SCO_POLISH_TILE || p.ld > SCO_POLISH_MAX_ORDER || p.per_chunk < 1 || p.per_chunk > batch ||
      (long long)p.chunks * p.per_chunk < batch || (long long)(p.chunks - 1) * p.per_chunk >= batch ||
      p.ws_bytes != (long long)p.per_chunk * p.ld * p.ld * 8 || p.ws_bytes > eff_budget || p.lds_bytes != (16 * p.ld + 32) * 8 ||
      p.lds_bytes > 160 * 1024) {
    printf("bad plan: n %d m %d batch %d k %d budget %lld -> ld %d per %d chunks %d ws %lld lds %d\n", n, m, batch, k, budget, p.ld,
           p.per_chunk, p.chunks, p.ws_bytes, p.lds_bytes);
    return 1;
  }
  return 0;
}

int main() {
  unsetenv("SCO_QP_POLISH_WS_MB");
  const int batches[] = {1, 7, 1024, 1 << 30};
  const long long budgets[] = {1, 2047, 2048, 1 << 20, SCO_POLISH_WS_BYTES, 1ll << 62, 0, -5};
  long long acc = 0, ref = 0;
  for (int n = -1; n <= 1200; n++) {
    const int ms[] = {-1, 0, 1, n / 2, n, 2 * n};
    for (int m : ms) {
      const int ks[] = {-1, 0, 1, 15 - n % 16, 16 - n % 16, 17 - n % 16, m / 2, m - 1, m, m + 1, SCO_POLISH_MAX_ORDER - n, SCO_POLISH_MAX_ORDER - n + 1};
      for (int k : ks)
        for (int batch : batches)
          for (long long budget : budgets)
            if (check(n, m, batch, k, budget, budget > 0 ? budget : SCO_POLISH_WS_BYTES, &acc, &ref)) return 1;
    }
  }
  if (check(5, 5, 0, 0, 0, SCO_POLISH_WS_BYTES, &acc, &ref)) return 1;
  // the environment readers
  setenv("SCO_QP_POLISH_WS_MB", "3", 1);
  QpPolishPlan p = qp_polish_plan(340, 554, 64, 221, 0);                  // 576^2 doubles = 2.53 MiB: one problem per chunk
  if (p.rc != SCO_OK || p.ld != 576 || p.per_chunk != 1 || p.chunks != 64) return 1;
  setenv("SCO_QP_POLISH_WS_MB", "-3", 1);
  p = qp_polish_plan(340, 554, 64, 221, 0);
  if (p.rc != SCO_OK || p.per_chunk != 64) return 1;
  setenv("SCO_QP_POLISH_WS_MB", "99999999999999999999", 1);
  p = qp_polish_plan(340, 554, 64, 221, 0);
  if (p.rc != SCO_OK || p.per_chunk != 64) return 1;
  unsetenv("SCO_QP_POLISH_WS_MB");
  if (!qp_polish_order_fits(340, 754) || qp_polish_order_fits(340, 765) || qp_polish_order_fits(2147483647, 2147483647)) return 1;
#ifndef SCO_QP_POLISH_NO_MFMA
  setenv("SCO_QP_POLISH_NO_MFMA", "1", 1);
  if (qp_polish_use_mfma()) return 1;
  setenv("SCO_QP_POLISH_NO_MFMA", "0", 1);
  if (!qp_polish_use_mfma()) return 1;
#endif
  printf("%lld plans accepted, %lld refused: every accepted plan holds its order and its batch inside the budget\n", acc, ref);
  return 0;
}
