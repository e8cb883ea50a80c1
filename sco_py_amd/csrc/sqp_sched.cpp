// sqp_sched.cpp -- scheduling policy of the SQP round loop: see sqp_sched.h.
#include "sqp_sched.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

SqpSchedEnv sqp_sched_env() {
  SqpSchedEnv e;
  auto env_int = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
  e.slice = std::max(0, env_int("SCO_SQP_SLICE", 0));
  e.groups = env_int("SCO_SQP_GROUPS", 1);
  { const char *v = getenv("SCO_SQP_SELECT"); e.select = !(v && v[0] == '0'); }
  e.mix = env_int("SCO_SQP_MIX", SQP_MIX_DEFAULT);
  e.mix_slack = env_int("SCO_SQP_MIX_SLACK", 1);
  e.mix_slices = env_int("SCO_SQP_MIX_SLICES", 2);
  { const char *v = getenv("SCO_SQP_MIX_PICK"); e.mix_tail = v && !strcmp(v, "tail"); }
  e.xcds = std::max(0, env_int("SCO_SQP_XCDS", 0));
  { const char *v = getenv("SCO_SQP_TRACE_ROUNDS"); e.trace = !v ? 0 : (atoi(v) >= 2 ? 2 : 1); }
  return e;
}

SqpSchedule sqp_schedule_plan(const SqpSchedIn &in) {
  SqpSchedule sc;
  sc.cus = in.cus; sc.wv_min = in.wv_min; sc.handle_wv = in.handle_wv; sc.trace = in.env.trace;
  const int batch = in.batch, cus = in.cus;
  // time slicing (scheduling only): every launch advances each active QP by at most `slice` ADMM iterations; a
  // problem whose QP ended goes through post / pre / setup and joins the next launch with its next QP
  // default slice: 6250 iterations (7-DOF x 20: 964 ms per 1024-batch step against 1106 unsliced); with adaptive rho
  // the QPs are short and every rho change costs its problem a relaunch, so the slice is shorter (scripts/gpu_adaptive_slice_sweep.py)
  int slice = in.admm_slice < 0 ? 0 : (in.admm_slice > 0 ? in.admm_slice : (in.adaptive_rho ? 2000 : 6250));
  if (in.admm_slice == 0) {
    if (in.env.slice > 0) slice = in.env.slice;      // tuning aid: the default slice
    // with at most one problem per CU there is nobody to hand a CU to: slicing would only add relaunches
    if (cus > 0 && batch <= cus) slice = 0;
  }
  sc.slice = slice;
  long long slices_per_qp = slice > 0 ? (in.max_iter + slice - 1) / slice : 1;
  if (in.adaptive_rho) slices_per_qp += in.max_iter / in.adaptive_interval + 1;    // a launch per rho change at most
  // (a round with selection runs at least half of the active problems, hence the factor 2)
  sc.round_cap = 2 * ((long long)in.max_qp_solves + 8) * slices_per_qp;
  // ---- scheduling of the rounds (results never depend on it).  A lock-step round costs ceil(active / CUs) passes of
  // workgroups, so once problems start to finish the last pass of every round is partly empty
  // (profiles/r02_launches.txt: 737 ms per step against 630 ms of work).  Default: ROUND SELECTION -- with more active
  // problems than CUs a round runs a whole number of passes, the problems with most in front of them first
  // (sqp_select_kernel), and SQP_DEPTH rounds are enqueued ahead so the device never waits for the host.
  // Opt-in on top (SCO_SQP_GROUPS = 2..4): the batch is cut into contiguous STREAM GROUPS that run their rounds
  // independently on streams of their own -- each with its own selection since r03 -- so that one group's launch fills the
  // CUs the end of another's leaves free.  (Measured on the 1024-problem 7x20 step: DESIGN.md 3.3.)
  if (slice > 0 && in.supports_groups && cus > 0 && batch >= 2 * cus)
    sc.G = std::max(1, std::min(std::min(in.env.groups, SQP_MAX_GROUPS), batch / cus));
  sc.select = slice > 0 && cus > 0 && batch > cus && in.supports_groups && in.env.select;
  // Tier of a round (handles whose penalty QP has the wavefront tier; warm-started QPs as in parity mode, adaptive rho has
  // no round selection and reaches the tier through wv_plain, sqp_round_plan): with at least wv_min live
  // problems the round runs on the wavefront tier -- every live problem at once, four per CU -- below that on the row-local
  // kernel, one problem per CU in whole passes.  The first is the higher THROUGHPUT while the batch is alive (1024 / 3.1 us
  // against 256 / 0.95 us per iteration), the second the lower LATENCY for the tail of a step; a problem's QP changes kernel
  // at a slice boundary (the parked state is common).  Both kernels agree to rounding (1e-14), not bit for bit: for batches
  // that ever have wv_min live problems the last bits of a result depend on the schedule (SCO_WV_MIN_PER_CU=1e9: never).
  sc.has_wv = sc.select && in.handle_wv;
  // MIXED rounds (SCO_SQP_MIX, one stream group, fixed rho): a wavefront round with fewer live problems than the chip holds
  // leaves CUs empty.  The k problems with most in front of them -- the head of the round's list, which sqp_select_kernel then
  // sorts -- run on the row-local kernel on those CUs instead, mix_slices slices in the time of one wavefront slice, beside the
  // wavefront launch over the rest of the list (sco_qp_launch_sliced, tier 3; k: qp_mix_split).  Per problem the sequence of QPs
  // and every decision is unchanged; which kernel runs a given slice moves, as at wv_min.  SCO_SQP_MIX_PICK=tail (test hook)
  // takes the side window from the end of the list in odd rounds, so that problems change sides in both directions.
  sc.mix_on = sc.has_wv && sc.G == 1 && !in.adaptive_rho && in.env.mix != 0;
  sc.mix_slack = std::max(0, in.env.mix_slack); sc.mix_slices = std::max(1, in.env.mix_slices);
  sc.xcds = sc.mix_on ? (in.env.xcds > 0 ? in.env.xcds : in.xcds) : 1;
  sc.mix_tail = in.env.mix_tail;
  // Rounds kept enqueued ahead of the host: SQP_DEPTH where a round's read-back would otherwise leave the device idle
  // (selection, stream groups, time slices); ONE for the plain unsliced loop over a batch that fits the CUs (the B = 1
  // latency case): there a second round in flight would only be a trailing all-inactive launch sequence per solve.
  sc.depth = (!sc.select && sc.G == 1 && slice == 0) ? 1 : SQP_DEPTH;
  for (int g = 0; g < sc.G; g++) {
    sc.grp[g].b0 = (int)((long long)batch * g / sc.G); sc.grp[g].nb = (int)((long long)batch * (g + 1) / sc.G) - sc.grp[g].b0;
    sc.grp[g].live = sc.G == 1 ? in.n_active : sc.grp[g].nb;       // upper bound of the group's live problems
  }
  return sc;
}

SqpRound sqp_round_plan(const SqpSchedule &sc, int group_nb, int live, int round_index) {
  SqpRound r;
  r.wv_round = sc.has_wv && live >= sc.wv_min;
  // (a pass of the chip = one problem per CU, four on the wavefront tier)
  r.pass = r.wv_round ? SQP_WV_PER_CU * sc.cus : sc.cus;
  r.nwg = group_nb;
  if (sc.select) {
    // compact launch: as many workgroups as the selection can let run -- whole passes, see sqp_select_kernel -- sized from
    // the newest active count the host has
    r.nwg = std::max(1, live <= r.pass ? live : (live / r.pass) * r.pass);
    if (sc.mix_on && r.wv_round && live < SQP_WV_PER_CU * sc.cus && r.nwg <= SQP_SEL_MAX) {
      r.mix_k = qp_mix_split(live, sc.cus, sc.xcds, sc.mix_slack, SQP_WV_PER_CU);
      if (r.mix_k >= r.nwg) r.mix_k = 0;
    }
  }
  if (r.mix_k > 0 && sc.mix_tail && (round_index & 1)) r.side_off = r.nwg - r.mix_k;
  r.tier = r.mix_k > 0 ? 3 : (sc.has_wv ? (r.wv_round ? 2 : 1) : 0);
  r.window = sc.G > 1 || sc.select;
  // without round selection (at most one problem per CU) the launch itself goes by its size (sco_qp_launch_sliced): with
  // SCO_WV_MIN_PER_CU lowered such a round runs on the wavefront tier too, and is counted as one
  const bool wv_plain = !sc.has_wv && sc.handle_wv && r.nwg >= sc.wv_min;
  r.counts_as_wv = r.wv_round || wv_plain;
  return r;
}

int qp_mix_split(int live, int cus, int xcds, int slack, int per_cu) {
  if (live <= 0 || cus <= 0 || xcds <= 0 || per_cu <= 0 || slack < 0 || cus % xcds) return 0;
  if (live > per_cu * (cus - 1)) return 0;
  const int room = cus / xcds;
  auto up = [](int a, int b) { return (a + b - 1) / b; };
  // (the left side is not monotone in k: it steps up every xcds problems and down every per_cu * xcds)
  for (int k = live < cus ? live : cus; k > 0; k--)
    if (up(k, xcds) + slack + up(up(live - k, xcds), per_cu) <= room) return k;
  return 0;
}

void sqp_stage_sweep(const double *begin_ms, const double *end_ms, const int *stage, int n, double ms[5]) {
  struct Edge { double t; int stage, d; };
  std::vector<Edge> edges;
  edges.reserve(2 * (size_t)std::max(n, 0));
  for (int i = 0; i < n; i++)
    if (stage[i] >= 0 && stage[i] < 4 && end_ms[i] > begin_ms[i]) {
      edges.push_back({begin_ms[i], stage[i], 1}); edges.push_back({end_ms[i], stage[i], -1});
    }
  std::sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) { return x.t < y.t; });
  int open_[4] = {0, 0, 0, 0};
  const int prio[4] = {2, 1, 0, 3};
  for (size_t i = 0; i < edges.size(); i++) {
    if (i > 0) {
      const double dt = edges[i].t - edges[i - 1].t;
      for (int k : prio) if (open_[k] > 0) { ms[k] += dt; ms[4] += dt; break; }
    }
    open_[edges[i].stage] += edges[i].d;
  }
}

// ---- debug entry points (include/sco_hip.h): the planners and the sweep on plain numbers
extern "C" int sco_debug_mix_split(int live, int cus, int xcds, int slack, int per_cu) {
  return qp_mix_split(live, cus, xcds, slack, per_cu);
}

extern "C" int sco_debug_sqp_schedule(const int in[12], int plan[20], const int round_in[3], int round_out[8]) {
  if (!in || !plan || (round_in && !round_out)) return -1;
  SqpSchedIn si;
  si.batch = in[0]; si.cus = in[1]; si.admm_slice = in[2]; si.adaptive_rho = in[3]; si.max_iter = in[4];
  si.adaptive_interval = in[5]; si.max_qp_solves = in[6]; si.n_active = in[7]; si.supports_groups = in[8] != 0;
  si.handle_wv = in[9] != 0; si.wv_min = in[10]; si.xcds = in[11];
  if (si.adaptive_rho && si.adaptive_interval <= 0) return -1;
  si.env = sqp_sched_env();
  const SqpSchedule sc = sqp_schedule_plan(si);
  const int head[12] = {sc.slice, sc.G, sc.select, sc.has_wv, sc.mix_on, sc.mix_slack, sc.mix_slices, sc.mix_tail, sc.depth,
                        (int)std::min<long long>(sc.round_cap, INT_MAX), sc.xcds, sc.trace};
  memcpy(plan, head, sizeof head);
  for (int g = 0; g < SQP_MAX_GROUPS; g++) { plan[12 + 2 * g] = sc.grp[g].b0; plan[13 + 2 * g] = sc.grp[g].nb; }
  if (round_in) {
    const SqpRound r = sqp_round_plan(sc, round_in[0], round_in[1], round_in[2]);
    const int out[8] = {r.wv_round, r.pass, r.nwg, r.mix_k, r.side_off, r.tier, r.window, r.counts_as_wv};
    memcpy(round_out, out, sizeof out);
  }
  return 0;
}

extern "C" int sco_debug_stage_sweep(int n, const double *begin_ms, const double *end_ms, const int *stage, double ms[5]) {
  if (n < 0 || !ms || (n > 0 && (!begin_ms || !end_ms || !stage))) return -1;
  for (int k = 0; k < 5; k++) ms[k] = 0.0;
  sqp_stage_sweep(begin_ms, end_ms, stage, n, ms);
  return 0;
}
