// Stand-alone sweep of the QP launch planner (csrc/qp_tier.cpp) for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       scripts/sanitize/qp_tier_sweep.cpp sco_py_amd/csrc/qp_tier.cpp -o qp_tier_sweep && ./qp_tier_sweep
// Every handle kind x fixed / adaptive rho x no window / windows of every tier / mixed windows, well-formed and malformed
// x slices 0, 1, 130 x batches 1 .. 1300.  Every accepted plan must have 1 <= nwg <= batch.
#include <cstdio>
#include <cstdlib>

#include "../../sco_py_amd/csrc/qp_tier.h"

struct Handle { int kern; bool big, bt, wv, chol; int n_c; };

int main() {
  const Handle handles[] = {
      {QP_K_RL, false, false, true, false, 140},  {QP_K_RL, false, false, false, false, 18},  {QP_K_RL, false, false, false, true, 177},
      {QP_K_REG, false, false, false, false, 30}, {QP_K_FAST, false, false, false, false, 253}, {QP_K_GENERIC, false, false, false, false, 0},
      {QP_K_GENERIC, true, false, false, false, 600}, {QP_K_GENERIC, true, true, false, false, 600}};
  // windows as fractions of the batch (b0, nb in 1/8 of it; 9 = one past the end), tier, side window (offset into the
  // window and length in 1/8 of nb; -1: in the middle), list, side stream and events
  struct Win { int on, b0, nb, tier, side_off, side_nb, list, ready; };
  const Win wins[] = {{0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 8, 0, 0, 0, 1, 0}, {1, 2, 4, 1, 0, 0, 1, 0}, {1, 0, 8, 2, 0, 0, 0, 0},
                      {1, 4, 5, 0, 0, 0, 1, 0}, {1, -1, 4, 1, 0, 0, 1, 0}, {1, 0, 0, 2, 0, 0, 1, 0},
                      {1, 0, 8, 3, 0, 2, 1, 1}, {1, 1, 6, 3, 6, 2, 1, 1}, {1, 0, 8, 3, -1, 2, 1, 1}, {1, 0, 8, 3, 0, 8, 1, 1},
                      {1, 0, 8, 3, 0, 0, 1, 1}, {1, 0, 8, 3, 0, 2, 0, 1}, {1, 0, 8, 3, 0, 2, 1, 0}};
  const int slices[] = {0, 1, 130};
  long long plans = 0, accepted = 0, codes[6] = {0, 0, 0, 0, 0, 0};
  for (const Handle &h : handles)
    for (int adaptive = 0; adaptive < 2; adaptive++)
      for (const Win &w : wins)
        for (int slice : slices)
          for (int batch = 1; batch <= 1300; batch++) {
            QpLaunchIn in;
            in.kern = h.kern; in.use_big = h.big; in.use_bt = h.bt; in.use_wv = h.wv; in.factor_cholesky = h.chol;
            in.batch = batch; in.n_c = h.n_c; in.cus = 256;
            in.adaptive_rho = adaptive; in.adaptive_rho_interval = batch % 3 ? 0 : 60; in.adaptive_rho_tolerance = batch % 7 ? 5.0 : 1.0;
            in.check_termination = batch % 11 ? 25 : 0; in.max_iter = 100000;
            in.slice = slice; in.mask = batch % 3; in.wv_min = adaptive ? 2147483647 : 704;
            in.window = w.on != 0; in.b0 = w.b0 * batch / 8; in.nb = w.nb * batch / 8; in.tier = w.tier; in.has_list = w.list != 0;
            in.side_nb = w.side_nb * in.nb / 8;
            in.side_b0 = in.b0 + (w.side_off < 0 ? in.nb / 3 + 1 : w.side_off * in.nb / 8);
            in.side_slices = 2; in.side_ready = w.ready != 0;
            const QpLaunchPlan p = qp_launch_plan(in);
            plans++; codes[-p.rc]++;
            if (p.rc != SCO_OK) {
              if (!qp_launch_err_text(p.err)[0]) { printf("error without a text\n"); return 1; }
              continue;
            }
            accepted++;
            if (p.nwg < 1 || p.nwg > batch || p.slice < 0 || (p.slice > 0 && p.slice % in.check_termination) || p.sweep_nt < 1 || p.sweep_nt > 3 ||
                (p.mixed && (in.side_b0 < in.b0 || in.side_b0 + in.side_nb > in.b0 + in.nb))) {
              printf("bad plan: batch %d nwg %d slice %d\n", batch, p.nwg, p.slice);
              return 1;
            }
          }
  printf("%lld plans, %lld accepted (rc 0: %lld, -1: %lld, -4: %lld, -5: %lld): every accepted plan has 1 <= nwg <= batch\n", plans, accepted,
         codes[0], codes[1], codes[4], codes[5]);
  // the environment readers
  setenv("SCO_WV_MIN_PER_CU", "1e9", 1);
  if (sco_wv_min_live(256, false) != 2147483647) return 1;
  unsetenv("SCO_WV_MIN_PER_CU");
  if (sco_wv_min_live(0, false) != 704 || sco_wv_min_live(256, true) != 2147483647) return 1;
  setenv("SCO_QP_NO_RL", "1", 1); setenv("SCO_QP_NO_WV", "0", 1);
  const QpCreateEnv e = qp_create_env();
  if (!e.no_rl || e.no_wv || e.no_reg) return 1;
  return 0;
}
