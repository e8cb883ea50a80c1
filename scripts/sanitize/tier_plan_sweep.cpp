// Stand-alone sweep of the ADMM tiers' plan builders and the tier choice (csrc/rl_plan.cpp, wv_plan.cpp, big_plan.cpp,
// reg_fast_plan.cpp, qp_tier_choice.cpp) for a sanitizer build on the CPU:
//   cd sco_py_amd/csrc && g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       ../../scripts/sanitize/tier_plan_sweep.cpp qp_plan.cpp sqp_layout.cpp qp_tier.cpp qp_tier_choice.cpp rl_plan.cpp
//       wv_plan.cpp big_plan.cpp reg_fast_plan.cpp -o tier_plan_sweep && ./tier_plan_sweep digests.txt
// Patterns: both QPs of sqp_layout_build over trajectory descriptors (dof 1 .. 8, horizons 2 .. 24 -- past what every
// wavefront instantiation takes --, with and without velocity limits, joint limits and the goal pin, the row families of
// sqp_layout_sweep.cpp), wide descriptors (dof 9 .. 16: block orders 12 and 16 of the structured global-memory form, 12 x 50
// beyond a CU's LDS; 2 x 50 with 10 obstacles: three row slots on a <4,8> tile), trajectory patterns with rows added that
// the wavefront tier refuses for a reason of its own, and random sparse patterns.  Each pattern is analysed at allow_elim
// 0, 1 and 2, every planner runs on every analysis under every combination of the switches it reads (plain struct fields
// of QpCreateEnv), and qp_choose_tiers runs on the pattern under every combination of the planner switches and a walk
// through the tier switches.
// Checks on every accepted plan: every index it hands to its kernel is in range (rows < m, variables < n, value positions
// < nnzA / nnzP, LDS positions inside the plan's own lds_bytes, Sell*::src inside the value array, chunk records
// consistent with nchunks and npart, -1 only where the kernel takes it), its LDS request within the cap its planner promises,
// and a row-local plan names an instantiation its launcher has (layout_rl.h: rl_has_kernel).
// Output: one digest line per pattern and analysis over every field and array of every plan (refused plans included:
// the fields filled so far), one per pattern for the tier choice (return code, mask, error text) -- written to the file
// named on the command line; the counts per planner and per WvWhy code on stdout.  Fails unless every planner accepts and
// refuses at least once, the structured form is built at block orders 4, 8, 12 and 16, and every WvWhy code appears.
// SCO_DEBUG_PLAN stays off: it changes no plan, it prints.
//
// With -DSWEEP_PARENT the same patterns and digests come from a tree in which the planners still sit in the kernel files
// behind sco_internal.h and read the environment themselves (the switches then go through setenv, the tier choice through
// sco_debug_plan_build / sco_debug_plan_tiers / sco_last_error); the checks need the layout headers and are left out.
// profiles/tier_plan_split.md has the comparison.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifdef SWEEP_PARENT
#include "sco_internal.h"
#include "sqp_layout.h"
#else
#include "../../sco_py_amd/csrc/layout_big.h"
#include "../../sco_py_amd/csrc/layout_fast.h"
#include "../../sco_py_amd/csrc/layout_reg.h"
#include "../../sco_py_amd/csrc/layout_rl.h"
#include "../../sco_py_amd/csrc/layout_wv.h"
#include "../../sco_py_amd/csrc/qp_tier_plans.h"
#include "../../sco_py_amd/csrc/sqp_layout.h"
#endif

struct Pat { std::string label; int n = 0, m = 0; std::vector<int> Pp, Pi, Ap, Ai; };

// the switches of a handle as the sweep varies them
struct Sw {
  bool force_big = false, no_bt = false, no_rl = false, no_wv = false, no_reg = false, no_fast = false, no_elim = false, cholesky = false;
  bool no_mfma = false, rl_closed = false, rl_lay8 = false, rl_split_off = false;
};
static Sw planner_sw(int bits) { Sw s; s.no_mfma = bits & 1; s.rl_closed = bits & 2; s.rl_lay8 = bits & 4; s.rl_split_off = bits & 8; return s; }

#ifdef SWEEP_PARENT
extern "C" int sco_debug_plan_build(int n, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai, int allow_elim, int *sizes);
extern "C" int sco_debug_plan_tiers(int *mask);
static void put(const char *name, bool on, const char *val = "1") { if (on) setenv(name, val, 1); else unsetenv(name); }
static void apply(const Sw &s) {
  put("SCO_QP_FORCE_BIG", s.force_big); put("SCO_QP_NO_BT", s.no_bt); put("SCO_QP_NO_RL", s.no_rl); put("SCO_QP_NO_WV", s.no_wv);
  put("SCO_QP_NO_REG", s.no_reg); put("SCO_QP_NO_FAST", s.no_fast); put("SCO_QP_NO_ELIM", s.no_elim); put("SCO_QP_FACTOR_CHOLESKY", s.cholesky);
  put("SCO_QP_NO_MFMA", s.no_mfma); put("SCO_QP_RL_ALIGNED", s.rl_closed); put("SCO_QP_RL_LAY8", s.rl_lay8); put("SCO_QP_RL_SPLIT", s.rl_split_off, "0");
  unsetenv("SCO_QP_RL_CLOSED"); unsetenv("SCO_DEBUG_PLAN");
}
static bool run_rl(const QpPlan &pl, RlHost &rh, const Sw &s) { apply(s); return rl_plan_build(pl, rh); }
static bool run_bt(const QpPlan &pl, const BigHost &bh, BtHost &th, const Sw &s) { apply(s); return bt_plan_build(pl, bh, th); }
static int run_tiers(const Pat &p, const Sw &s, int *mask, std::string *err) {
  apply(s);
  int sizes[16];
  if (sco_debug_plan_build(p.n, p.m, p.Pp.data(), p.Pi.data(), p.Ap.data(), p.Ai.data(), 1, sizes) != SCO_OK) return -99;
  const int rc = sco_debug_plan_tiers(mask);
  if (rc != SCO_OK) *err = sco_last_error();
  return rc;
}
#else
static QpCreateEnv env_of(const Sw &s) {
  QpCreateEnv e;
  e.force_big = s.force_big; e.no_bt = s.no_bt; e.no_rl = s.no_rl; e.no_wv = s.no_wv; e.no_reg = s.no_reg; e.no_fast = s.no_fast;
  e.no_elim = s.no_elim; e.factor_cholesky = s.cholesky;
  e.no_mfma = s.no_mfma; e.rl_closed = s.rl_closed; e.rl_lay8 = s.rl_lay8; e.rl_split_off = s.rl_split_off;
  return e;
}
static bool run_rl(const QpPlan &pl, RlHost &rh, const Sw &s) { return rl_plan_build(pl, rh, env_of(s)); }
static bool run_bt(const QpPlan &pl, const BigHost &bh, BtHost &th, const Sw &s) { return bt_plan_build(pl, bh, th, s.no_mfma); }
static int run_tiers(const Pat &p, const Sw &s, int *mask, std::string *err) {
  QpTiers t;
  const int rc = qp_choose_tiers(p.n, p.m, p.Pp.data(), p.Pi.data(), p.Ap.data(), p.Ai.data(), env_of(s), t, err);
  if (rc == SCO_OK) *mask = qp_tier_mask(t);
  return rc;
}
#endif

// ---- digests: FNV-1a over every field and array
struct Dg {
  uint64_t h = 1469598103934665603ull;
  void i(long long v) { for (int k = 0; k < 8; k++) { h ^= (uint64_t)(v >> (8 * k)) & 255; h *= 1099511628211ull; } }
  template <class T> void v(const std::vector<T> &x) { i((long long)x.size()); for (const T &e : x) i((long long)e); }
  void s(const std::string &x) { i((long long)x.size()); for (char c : x) i(c); }
  void sell(const SellHost &x) { i(x.nitems); i(x.total); v(x.base); v(x.width); v(x.src); v(x.idx); }
};
static void dg_fast(Dg &d, bool ok, const FastHost &f) {
  d.i(ok); d.sell(f.Ac); d.sell(f.Ar); d.sell(f.Ca); d.sell(f.Ce); d.i(f.TR); d.i(f.TC); d.i(f.capped); d.i((long long)f.lds_doubles); d.i((long long)f.lds_bytes);
}
static void dg_reg(Dg &d, bool ok, const RegHost &r) {
  d.i(ok); d.i(r.TR); d.i(r.TC); d.i(r.CW); d.i(r.RW); d.i(r.PX); d.sell(r.Ac); d.sell(r.Ar); d.sell(r.Ca); d.sell(r.Ce); d.i((long long)r.lds_bytes); d.v(r.role); d.v(r.off);
}
static void dg_rl(Dg &d, bool ok, const RlHost &r) {
  d.i(ok); d.i(r.TR); d.i(r.TC); d.i(r.CW); d.i(r.pcw); d.i(r.zpos); d.i(r.merged); d.i(r.aligned); d.i(r.split); d.i(r.lay8); d.i(r.NS);
  d.sell(r.Ac); for (int q = 0; q < 3; q++) d.sell(r.Ar[q]);
  d.i((long long)r.lds_bytes); d.v(r.off); d.v(r.role); d.v(r.pc_ptr); d.v(r.pc_pos); d.v(r.pc_core);
}
static void dg_wv(Dg &d, bool ok, const WvHost &w) {
  d.i(ok); d.i(w.bs); d.i(w.nb); d.i(w.mid); d.i(w.lpb); d.i(w.n_extra); d.i(w.BS); d.i(w.NS); d.i(w.NV); d.i(w.NSTEP); d.i(w.cst_slots);
  d.i((long long)w.g_doubles); d.i((long long)w.lds_doubles); d.i((long long)w.lds_bytes); d.v(w.tab);
  d.i(w.n_link); d.i(w.NL); d.i(w.per_cu); d.i(w.why); d.i(w.n_stack);
}
static void dg_big(Dg &d, bool ok, const BigHost &b) {
  d.i(ok); d.v(b.row_elim); d.v(b.row_epos); d.v(b.er_ptr); d.v(b.er_row); d.v(b.free_rows); d.v(b.pc_ptr); d.v(b.pc_pos); d.v(b.pc_core); d.i((long long)b.ws_doubles);
}
static void dg_bt(Dg &d, bool ok, const BtHost &t) {
  d.i(ok); d.i(t.bs); d.i(t.nb); d.i(t.nchunks); d.i(t.npart); d.i(t.use_part); d.v(t.cent);
  d.i((long long)t.blk_doubles); d.i((long long)t.ws_doubles); d.i((long long)t.lds_bytes); d.v(t.ch_desc); d.v(t.it);
  d.i(t.use_mfma); d.i(t.mf_why); d.v(t.mf_id); d.v(t.mf_h0); d.v(t.mf_h1);
}

// ---- checks (the tree with the layout headers only)
#ifndef SWEEP_PARENT
#define CK(cond) do { if (!(cond)) return #cond; } while (0)
static bool in(int v, int lo, int hi) { return v >= lo && v < hi; }        // lo <= v < hi
// a sliced-ELL image: nitems items, sources in [-1, nsrc), gathered indices < nidx (pairs: rl's images have no idx)
static const char *ck_sell(const SellHost &s, int nitems, int nsrc, int nidx, bool paired) {
  const int ns = (nitems + 63) / 64;
  CK(s.nitems == nitems && (int)s.base.size() == ns + 1 && (int)s.width.size() >= ns && s.base[0] == 0 && s.total == s.base[ns]);
  for (int k = 0; k < ns; k++) CK(s.base[k + 1] == s.base[k] + 64 * s.width[k] && s.width[k] >= 0);
  CK((int)s.src.size() >= s.total && (paired || (int)s.idx.size() >= s.total));
  for (int x : s.src) CK(in(x, -1, nsrc));
  if (!paired) for (int k = 0; k < s.total; k++) CK(s.src[k] < 0 ? s.idx[k] == 0 : (int)s.idx[k] < nidx);
  return nullptr;
}
static const char *ck_sell4(const QpPlan &pl, const SellHost &Ac, const SellHost &Ar, const SellHost &Ca, const SellHost &Ce) {
  if (const char *e = ck_sell(Ac, pl.n, pl.nnzA, pl.m, false)) return e;
  if (const char *e = ck_sell(Ar, pl.m, pl.nnzA, pl.n, false)) return e;
  if (const char *e = ck_sell(Ca, pl.n_c, pl.ncpl, pl.n_e, false)) return e;
  return ck_sell(Ce, pl.n_e, pl.ncpl, pl.n_c, false);
}
static const char *ck_fast(const QpPlan &pl, const FastHost &f) {
  if (const char *e = ck_sell4(pl, f.Ac, f.Ar, f.Ca, f.Ce)) return e;
  CK(f.lds_bytes <= (size_t)SCO_LDS_CAP && f.lds_doubles * 8 <= f.lds_bytes && f.TR >= 1 && f.TR <= 5 && GI * f.TR >= pl.n_c && GJ * f.TC >= pl.n_c);
  return nullptr;
}
static const char *ck_reg(const QpPlan &pl, const RegHost &r) {
  if (const char *e = ck_sell4(pl, r.Ac, r.Ar, r.Ca, r.Ce)) return e;
  CK(r.lds_bytes + REG_STATIC_LDS <= (size_t)SCO_LDS_CAP && r.TR >= 1 && r.TR <= 5 && RGI * r.TR >= pl.n_c && RGJ * r.TC >= pl.n_c);
  const int slots = r.CW + 2 * r.RW + r.PX, lds_el = (int)(r.lds_bytes / 8);
  CK((int)r.off.size() == slots * RT && (int)r.role.size() == 8 * RT);
  CK(pl.n < CAP_N && pl.m < CAP_M && pl.n_c < CAP_NC && pl.n_e < CAP_N);      // the spare zero element of every gathered vector
  for (int t = 0; t < RT; t++) {
    CK(in(r.role[t], -1, pl.n_c) && in(r.role[RT + t], -1, pl.n) && in(r.role[2 * RT + t], -1, pl.n_e));
    CK((r.role[t] >= 0) == (r.role[RT + t] >= 0) && !(r.role[t] >= 0 && r.role[2 * RT + t] >= 0));
    for (int k = 3; k <= 6; k++) CK(in(r.role[k * RT + t], 0, lds_el));
    for (int k = 0; k < r.CW; k++) CK(r.off[k * RT + t] % 8 == 0 && r.off[k * RT + t] / 8 <= pl.m);
    for (int k = 0; k < 2 * r.RW; k++) CK(r.off[(r.CW + k) * RT + t] % 8 == 0 && r.off[(r.CW + k) * RT + t] / 8 <= pl.n);
    for (int k = 0; k < r.PX; k++) CK(r.off[(r.CW + 2 * r.RW + k) * RT + t] % 8 == 0 && r.off[(r.CW + 2 * r.RW + k) * RT + t] / 8 <= std::max(pl.n_c, pl.n_e));
  }
  return nullptr;
}
static const char *ck_pc(const QpPlan &pl, const std::vector<int> &ptr, const std::vector<int> &pos, const std::vector<int> &core) {
  CK((int)ptr.size() == pl.n_c + 1 && ptr[0] == 0 && ptr[pl.n_c] == (int)pos.size() && pos.size() == core.size());
  for (int c = 0; c < pl.n_c; c++) CK(ptr[c + 1] >= ptr[c]);
  for (size_t k = 0; k < pos.size(); k++) CK(in(pos[k], 0, pl.nnzP) && in(core[k], 0, pl.n_c));
  return nullptr;
}
static const char *ck_rl(const QpPlan &pl, const RlHost &r) {
  CK(r.lds_bytes + 40 * 1024 <= (size_t)SCO_LDS_CAP && r.NS >= 2 && r.NS <= LNS_MAX);
  CK(r.CW == LCW || r.CW == LCW_MAX || (r.NS == 3 && r.CW == LCW_MAX3));
  CK(rl_has_kernel(r.TR, r.TC, r.CW, r.NS, r.aligned ? 2 : r.lay8 ? 1 : 0));      // rl_launch has this instantiation
  const int CP = r.CW / 2, RP = (r.CW > LCW ? LRW_MAX : LRW) / 2, slots = CP + r.NS * RP + 1, lds_el = (int)(r.lds_bytes / 8);
  CK((int)r.off.size() == slots * LT && (int)r.role.size() == RL_ROLES * LT);
  // (the images have one item per thread, or, in the compact form of the closed assignments, one per thread with entries)
  if (const char *e = ck_sell(r.Ac, r.Ac.nitems, pl.nnzA, 0, true)) return e;
  CK(r.Ac.nitems >= 1 && r.Ac.nitems <= LT);
  int images = r.Ac.total;
  for (int q = 0; q < r.NS; q++) {
    if (const char *e = ck_sell(r.Ar[q], r.Ar[q].nitems, pl.nnzA, 0, true)) return e;
    CK(r.Ar[q].nitems >= 1 && r.Ar[q].nitems <= LT);
    images += r.Ar[q].total;
  }
  CK(r.zpos >= 0 && r.zpos + 1 < LCAP_M - 1 && r.pcw >= 0);
  auto R = [&](int row, int t) { return r.role[(size_t)row * LT + t]; };
  for (int t = 0; t < LT; t++) {
    CK(in(R(0, t), -1, pl.n_c) && in(R(1, t), -1, pl.n) && in(R(2, t), -1, pl.n_e) && in(R(3, t), -1, pl.n));
    CK(in(R(11, t), -1, pl.nnzP) && in(R(12, t), -1, pl.nnzP));
    // image bases: a thread without entries reads the 64 x 16 zeros behind the images; the reads of its trip count stay inside
    CK(in(R(8, t), 0, images + 128) && R(8, t) + 128 * std::max(0, R(13, t) / 2 - 1) + 1 < lds_el && in(R(13, t), 0, LCW_MAX3 + 1));
    for (int q = 0; q < r.NS; q++) {
      const int i = R(ROLE_ROW(q), t);
      CK(in(i, -1, pl.m) && in(R(ROLE_RBASE(q), t), 0, images + 128) && in(R(ROLE_RWID(q), t), 0, LRW_MAX + 1));
      CK(R(ROLE_RBASE(q), t) + 128 * std::max(0, R(ROLE_RWID(q), t) / 2 - 1) + 1 < lds_el);
      CK(i < 0 ? R(ROLE_POS(q), t) == -1 && R(ROLE_EPOS(q), t) == -1 : in(R(ROLE_POS(q), t), 0, LCAP_M - 1) && in(R(ROLE_EPOS(q), t), -1, pl.nnzA));
    }
    for (int rr = 0; rr < AL_TR; rr++) CK(in(R(ROLE_WROW(rr), t), -1, pl.n_c));
    CK(in(R(ROLE_XOUT, t), -1, pl.n_c));
    for (int k = 0; k < CP; k++) CK(r.off[(size_t)k * LT + t] % 8 == 0 && r.off[(size_t)k * LT + t] / 8 + 1 < LCAP_M);
    for (int k = 0; k < r.NS * RP + 1; k++) CK(r.off[(size_t)(CP + k) * LT + t] % 8 == 0 && r.off[(size_t)(CP + k) * LT + t] / 8 + 1 < LCAP_NC);
  }
  return ck_pc(pl, r.pc_ptr, r.pc_pos, r.pc_core);
}
static const char *ck_wv(const QpPlan &pl, const WvHost &w) {
  CK(w.why == WV_OK && w.lds_bytes <= 40 * 1024 && w.lds_bytes == w.lds_doubles * 8 && w.per_cu == SCO_WV_PER_CU);
  CK(w.bs >= 1 && w.bs <= w.BS && w.nb * w.bs == pl.n_c && w.mid == w.nb / 2 && w.mid <= w.NSTEP && w.nb - 1 - w.mid <= w.NSTEP);
  CK(w.NS <= WV_MAXNS && w.NV <= WV_MAXNV && w.lpb >= 1 && w.lpb <= 8 && w.lpb * w.NV >= w.bs && (w.NL == 0 || w.NL == WV_NL));
  CK((w.NL > 0) == (w.n_link + w.n_stack > 0) && w.n_extra <= WV_T);
  const int npos = 2 * w.NSTEP + 2;
  const WvTab T = wv_tab_layout(w.NS, w.NV, w.NL);
  CK((int)w.tab.size() == T.total * 64 && w.cst_slots == wv_cst_slots(w.NS, w.NV, w.NV * w.NL));
  CK(w.g_doubles == (size_t)npos * 64 + 2 * (size_t)npos * 8 + 8 && w.g_doubles < w.lds_doubles);
  auto A = [&](int off, int l) { return w.tab[(size_t)off * 64 + l]; };
  for (int l = 0; l < 64; l++) {
    CK(in(A(T.pos, l), 0, npos));                                    // every lane sits on a block position: never -1
    for (int q = 0; q < w.NS; q++) {
      const int h = A(T.hrow + q, l);
      CK(in(h, -1, pl.m));
      if (h < 0) continue;                                            // an empty hinge slot: the kernel reads nothing else of it
      CK(in(A(T.hbrow + q, l), 0, pl.m) && in(A(T.hevar + q, l), 0, pl.n) && in(A(T.heidx + q, l), 0, pl.n_e));
      CK(in(A(T.hepos + q, l), 0, pl.nnzA) && in(A(T.hbpos + q, l), 0, pl.nnzA));
      for (int k = 0; k < 8; k++) CK(in(A(T.hjpos + q * 8 + k, l), -1, pl.nnzA));
    }
    for (int v = 0; v < w.NV; v++) {
      CK(in(A(T.vpk + v, l), 0, 8 * npos) && in(A(T.vpkm + v, l), 0, 8 * npos) && in(A(T.vpkp + v, l), 0, 8 * npos));   // never -1
      CK(in(A(T.vvar + v, l), -1, pl.n) && in(A(T.vrow + v, l), -1, pl.m) && in(A(T.vpm + v, l), -1, pl.nnzP) && in(A(T.vpp + v, l), -1, pl.nnzP));
      CK(A(T.vrow + v, l) < 0 ? A(T.vpos + v, l) == -1 : in(A(T.vpos + v, l), 0, pl.nnzA));
      for (int k = 0; k < 8; k++) CK(in(A(T.vpd + v * 8 + k, l), -1, pl.nnzP));
      for (int s = 0; s < w.NL; s++) {
        const int i = v * w.NL + s, row = A(T.lrow + i, l);
        CK(in(row, -1, pl.m) && (row < 0 ? A(T.lplo + i, l) == -1 && A(T.lphi + i, l) == -1 : in(A(T.lplo + i, l), 0, pl.nnzA) && in(A(T.lphi + i, l), -1, pl.nnzA)));
      }
    }
    CK(in(A(T.xpk, l), 0, 8 * npos) && in(A(T.xrow, l), -1, pl.m) && (A(T.xrow, l) < 0 ? A(T.xpos, l) == -1 : in(A(T.xpos, l), 0, pl.nnzA)));
  }
  return nullptr;
}
static const char *ck_big(const QpPlan &pl, const BigHost &b) {
  CK((int)b.row_elim.size() == pl.m && (int)b.row_epos.size() == pl.m && (int)b.er_ptr.size() == pl.n_e + 1 && b.er_ptr[pl.n_e] == (int)b.er_row.size());
  for (int i = 0; i < pl.m; i++) CK(in(b.row_elim[i], -1, pl.n_e) && (b.row_elim[i] < 0 ? b.row_epos[i] == -1 : in(b.row_epos[i], 0, pl.nnzA)));
  for (int e = 0; e < pl.n_e; e++) CK(in(b.er_ptr[e + 1] - b.er_ptr[e], 0, 3));
  for (int i : b.er_row) CK(in(i, 0, pl.m));
  for (int i : b.free_rows) CK(in(i, 0, pl.m));
  return ck_pc(pl, b.pc_ptr, b.pc_pos, b.pc_core);
}
static const char *ck_bt(const QpPlan &pl, const BtHost &t) {
  CK((t.bs == 4 || t.bs == 8 || t.bs == 12 || t.bs == 16) && t.bs <= BT_MAXBS && t.nb * t.bs >= pl.n_c && (t.nb - 1) * t.bs < pl.n_c);
  CK(t.lds_bytes + 1024 <= (size_t)SCO_LDS_CAP && t.blk_doubles == 2 * (size_t)t.nb * t.bs * t.bs);
  CK((int)t.ch_desc.size() == t.nchunks * CH_STRIDE && (int)t.it.size() == t.nchunks * 64 * 8 && (int)t.cent.size() == 4 * t.nb * t.bs);
  CK(t.use_part ? t.npart > 0 : t.npart == 0);
  for (int v : t.cent) CK(v == -1 || (v >= 0 && v < t.npart) || (v <= -2 && -(v + 2) < pl.nnzA));
  for (int ch = 0; ch < t.nchunks; ch++) {
    const int *d = &t.ch_desc[(size_t)ch * CH_STRIDE], na = d[1];
    CK(in(d[0], 0, 3) && in(na, 1, 65));
    if (d[0] == 0) {
      CK(in(d[2], 1, 17) && d[3] >= 0 && d[3] + na <= pl.m && d[4] >= 0 && d[4] + d[2] <= pl.n_c);
      CK(d[5] >= 0 && d[6] >= 0 && d[5] + (d[2] - 1) * d[6] + na - 1 < pl.nnzA && d[7] >= 0 && d[7] + na <= pl.n_e && d[8] >= 0 && d[8] + na <= pl.n);
      CK(d[9] < 0 ? d[9] == -1 && d[12] == -1 : d[9] + na <= pl.m && in(d[12], 0, pl.nnzA) && in(d[12] + (na - 1) * d[13], 0, pl.nnzA));
      CK(in(d[10], 0, pl.nnzA) && in(d[10] + (na - 1) * d[11], 0, pl.nnzA) && (!t.use_part || (d[14] >= 0 && d[14] + d[2] <= t.npart)));
    }
    for (int l = 0; l < 64; l++) {
      const int *r = &t.it[((size_t)ch * 64 + l) * 8];
      if (l >= na) { for (int k = 0; k < 8; k++) CK(r[k] == -1); continue; }
      CK(in(r[0], -1, pl.n_e) && in(r[1], -1, pl.n) && in(r[2], -1, pl.m) && in(r[3], -1, pl.m) && in(r[4], -1, pl.nnzA) && in(r[5], -1, pl.nnzA));
      CK(in(r[6], -1, pl.n_c) && in(r[7], -1, pl.nnzA) && (r[0] >= 0) == (r[1] >= 0) && (r[0] >= 0 || r[2] >= 0));
    }
  }
  if (t.use_mfma) {
    CK(t.mf_why == 0 && t.bs >= 12 && (int)t.mf_id.size() == t.nb * 256 && (int)t.mf_h0.size() == pl.nS && (int)t.mf_h1.size() == pl.nS);
    for (int v : t.mf_id) CK(in(v, -1, pl.nS));
    for (int id = 0; id < pl.nS; id++) CK(t.mf_h0[id] >= 0 && t.mf_h0[id] <= t.mf_h1[id] && t.mf_h1[id] <= (int)pl.sa_row.size());
  } else CK(t.mf_why != 0 && t.mf_id.empty());
  return nullptr;
}
#else
static const char *ck_fast(const QpPlan &, const FastHost &) { return nullptr; }
static const char *ck_reg(const QpPlan &, const RegHost &) { return nullptr; }
static const char *ck_rl(const QpPlan &, const RlHost &) { return nullptr; }
static const char *ck_wv(const QpPlan &, const WvHost &) { return nullptr; }
static const char *ck_big(const QpPlan &, const BigHost &) { return nullptr; }
static const char *ck_bt(const QpPlan &, const BtHost &) { return nullptr; }
#endif

// ---- patterns
static Pat from_qp(const std::string &label, const SqpQpPattern &q, int n, int m) {
  Pat p; p.label = label; p.n = n; p.m = m; p.Pp = q.Pp; p.Pi = q.Pi; p.Ap = q.Ap; p.Ai = q.Ai;
  return p;
}
// rows appended behind the last one: rows[r] = the (ascending) variables of new row m + r
static Pat with_rows(const Pat &p, const std::string &tag, const std::vector<std::vector<int>> &rows) {
  Pat o = p; o.label += tag; o.Ap.assign(1, 0); o.Ai.clear();
  for (int j = 0; j < p.n; j++) {
    o.Ai.insert(o.Ai.end(), p.Ai.begin() + p.Ap[j], p.Ai.begin() + p.Ap[j + 1]);
    for (size_t r = 0; r < rows.size(); r++) if (std::find(rows[r].begin(), rows[r].end(), j) != rows[r].end()) o.Ai.push_back(p.m + (int)r);
    o.Ap.push_back((int)o.Ai.size());
  }
  o.m = p.m + (int)rows.size();
  return o;
}

struct Count { long long acc = 0, ref = 0; void add(bool ok) { (ok ? acc : ref)++; } };
static Count n_fast, n_reg, n_rl, n_wv, n_big, n_bt;
static long long n_why[11], n_tier_rc[8], n_bs[17], n_patterns, n_plans;
static FILE *out;

static int fail(const Pat &p, int ae, const char *who, const char *what) {
  printf("BAD PLAN: %s allow_elim %d %s: %s\n", p.label.c_str(), ae, who, what);
  return 1;
}

static int sweep(const Pat &p) {
  n_patterns++;
  for (int ae = 0; ae <= 2; ae++) {
    QpPlan pl;
    Dg d;
    const int rc = qp_plan_build(p.n, p.m, p.Pp.data(), p.Pi.data(), p.Ap.data(), p.Ai.data(), ae, pl);
    d.i(rc);
    if (rc != 0) { fprintf(out, "%s ae%d malformed %016llx\n", p.label.c_str(), ae, (unsigned long long)d.h); continue; }
    d.i(pl.n_e); d.i(pl.n_c); d.i(pl.nS);
    std::string flags;
    {
      FastHost f; const bool ok = fast_plan_build(pl, f);
      dg_fast(d, ok, f); n_fast.add(ok); n_plans++; flags += ok ? 'F' : 'f';
      if (ok) if (const char *e = ck_fast(pl, f)) return fail(p, ae, "fast", e);
    }
    {
      RegHost r; int CW = 0, RW = 0, PX = 0;
      const bool caps = reg_caps_for(pl, &CW, &RW, &PX) != 0, ok = caps && reg_plan_build(pl, CW, RW, PX, r);
      d.i(caps); d.i(CW); d.i(RW); d.i(PX); dg_reg(d, ok, r); n_reg.add(ok); n_plans++; flags += ok ? 'G' : 'g';
      if (ok) if (const char *e = ck_reg(pl, r)) return fail(p, ae, "reg", e);
    }
    for (int bits = 0; bits < 16; bits += 2) {                       // closed, lay8, split off
      RlHost r; const bool ok = run_rl(pl, r, planner_sw(bits));
      dg_rl(d, ok, r); n_rl.add(ok); n_plans++; if (!bits) flags += ok ? 'R' : 'r';
      if (ok) if (const char *e = ck_rl(pl, r)) return fail(p, ae, "rl", e);
    }
    for (int links = 0; links < 2; links++) {
      WvHost w; const bool ok = wv_plan_build(pl, w, links != 0);
      dg_wv(d, ok, w); n_wv.add(ok); n_plans++; flags += ok ? 'W' : 'w';
      if (w.why < 0 || w.why > 10 || ok != (w.why == WV_OK)) return fail(p, ae, "wv", "why out of range or not WV_OK on an accepted plan");
      n_why[w.why]++;
      if (ok) if (const char *e = ck_wv(pl, w)) return fail(p, ae, "wv", e);
    }
    {
      BigHost b; const bool ok = big_plan_build(pl, b);
      dg_big(d, ok, b); n_big.add(ok); n_plans++; flags += ok ? 'B' : 'b';
      if (ok) if (const char *e = ck_big(pl, b)) return fail(p, ae, "big", e);
      if (ok && pl.n_c <= 1024)
        for (int nm = 0; nm < 2; nm++) {
          BtHost t; const bool okt = run_bt(pl, b, t, planner_sw(nm));
          dg_bt(d, okt, t); n_bt.add(okt); n_plans++; if (!nm) flags += okt ? 'T' : 't';
          if (okt) { n_bs[t.bs]++; if (const char *e = ck_bt(pl, t)) return fail(p, ae, "bt", e); }
        }
    }
    fprintf(out, "%s ae%d n_e %d n_c %d %s %016llx\n", p.label.c_str(), ae, pl.n_e, pl.n_c, flags.c_str(), (unsigned long long)d.h);
  }
  // the tier choice: every combination of the planner switches, then a walk through the tier switches
  Dg d;
  std::string masks;
  std::vector<Sw> sws;
  for (int bits = 0; bits < 16; bits++) sws.push_back(planner_sw(bits));
  { Sw s; s.force_big = true; sws.push_back(s); s.no_mfma = true; sws.push_back(s); s.no_bt = true; sws.push_back(s); }
  { Sw s; s.no_wv = true; sws.push_back(s); s.no_rl = true; sws.push_back(s); s.no_reg = true; sws.push_back(s); s.no_fast = true; sws.push_back(s); }
  { Sw s; s.no_elim = true; sws.push_back(s); s.force_big = true; sws.push_back(s); }
  { Sw s; s.cholesky = true; sws.push_back(s); }
  for (const Sw &s : sws) {
    int mask = -1; std::string err;
    const int rc = run_tiers(p, s, &mask, &err);
    d.i(rc); d.i(mask); d.s(err);
    if (rc > 0 || rc < -7 || (rc != SCO_OK && err.empty())) { printf("tier choice: rc %d without a text on %s\n", rc, p.label.c_str()); return 1; }
    n_tier_rc[-rc]++;
    char buf[16]; snprintf(buf, sizeof buf, " %d", rc == SCO_OK ? mask : rc); masks += buf;
  }
  fprintf(out, "%s tiers%s %016llx\n", p.label.c_str(), masks.c_str(), (unsigned long long)d.h);
  return 0;
}

// The Jacobian width hint on the penalty QP of a descriptor (sqp_row_widths -> wv_plan_widths): for link points on the
// given links, the widths stay inside [0, bs], the profile covers them or is the generic one, the switch forces the generic
// one, a hint of any kind leaves every other field and table of the plan alone, and hints with entries out of range (0,
// negative, beyond bs) promise nothing.
static long long n_hint, n_profiled;
#ifndef SWEEP_PARENT
static int sweep_hint(const sco_trajopt_desc &desc, const SqpLayout &L, const Pat &q1, const std::vector<int> &links) {
  QpPlan pl;
  if (qp_plan_build(q1.n, q1.m, q1.Pp.data(), q1.Pi.data(), q1.Ap.data(), q1.Ai.data(), 1, pl) != 0) return 0;
  WvHost w;
  if (!wv_plan_build(pl, w, true)) return 0;
  Dg d0; dg_wv(d0, true, w);
  std::vector<int> rw;
  const bool hint = sqp_row_widths(L.point, L.S, desc.dof, desc.n_obstacles, L.R, L.NBt, L.m_lin, L.m, links.data(), rw);
  if ((int)rw.size() != L.m) return fail(q1, 1, "hint", "row_width is not m long");
  const bool arm = L.point == ROWS_ARM || L.point == ROWS_SPATIAL;
  if (hint != arm) return fail(q1, 1, "hint", "hint for a family without the guarantee, or none for one with it");
  for (int variant = 0; variant < 4; variant++) {
    std::vector<int> h = rw;
    if (variant == 2) for (size_t i = 0; i < h.size(); i += 3) h[i] = -5;               // promises withdrawn row by row
    if (variant == 3) for (size_t i = 0; i < h.size(); i += 2) h[i] = 1000;             // widths beyond the block
    wv_plan_widths(w, hint ? h.data() : nullptr, variant == 1);
    n_hint++;
    for (int q = 0; q < WV_MAXNS; q++) if (w.jw[q] < 0 || w.jw[q] > w.bs || (q >= w.NS && w.jw[q])) return fail(q1, 1, "hint", "width out of range");
    if (w.jw_profile) {
      n_profiled++;
      if (variant == 1 || !hint) return fail(q1, 1, "hint", "a profile with the switch off or without a hint");
      if (!(w.BS == 7 && w.NS == 4 && w.NSTEP == 10 && w.lpb == 3 && !w.NL)) return fail(q1, 1, "hint", "a profile on a plan without profiled kernels");
      for (int q = 0; q < 4; q++) if (wv_jw(w.jw_profile, q, w.BS) < w.jw[q] || wv_jw(w.jw_profile, q, w.BS) > w.BS) return fail(q1, 1, "hint", "profile does not cover the widths");
    }
    Dg d1; dg_wv(d1, true, w);
    if (d1.h != d0.h) return fail(q1, 1, "hint", "the hint moved the plan");
    // the same hint as sort_width: the rows dealt by width -- same shape and LDS request, every index in range, the same rows
    WvHost ws;
    if (!wv_plan_build(pl, ws, true, hint ? h.data() : nullptr)) return fail(q1, 1, "hint", "sort_width refused an accepted pattern");
    if (const char *e = ck_wv(pl, ws)) return fail(q1, 1, "hint sorted", e);
    if (ws.tab.size() != w.tab.size() || ws.lds_bytes != w.lds_bytes || ws.BS != w.BS || ws.NS != w.NS || ws.NV != w.NV || ws.NSTEP != w.NSTEP || ws.lpb != w.lpb)
      return fail(q1, 1, "hint", "sort_width changed the shape of the plan");
    const WvTab T = wv_tab_layout(w.NS, w.NV, w.NL);
    std::vector<int> ra, rb;
    for (int q = 0; q < w.NS; q++) for (int l = 0; l < 64; l++) { ra.push_back(w.tab[(size_t)(T.hrow + q) * 64 + l]); rb.push_back(ws.tab[(size_t)(T.hrow + q) * 64 + l]); }
    std::sort(ra.begin(), ra.end()); std::sort(rb.begin(), rb.end());
    if (ra != rb) return fail(q1, 1, "hint", "sort_width lost or doubled a hinge row");
    wv_plan_widths(ws, hint ? h.data() : nullptr, false);
    for (int q = 1; q < ws.NS; q++) if (ws.jw[q] > ws.jw[q - 1]) return fail(q1, 1, "hint", "sorted widths do not fall from slot to slot");
  }
  return 0;
}
#endif

static const char *only_tag;      // argv[2]: sweep only the descriptors of this tag (a quick partial run; no coverage verdict)
static int sweep_desc(const sco_trajopt_desc &desc, const char *tag) {
  if (only_tag && strcmp(only_tag, tag)) return 0;
  const char *err = nullptr;
  if (sqp_check_desc(&desc, 0, nullptr, nullptr, nullptr, &err) != SCO_OK) return 0;
  const SqpLayout L = sqp_layout_build(desc, 0, nullptr, nullptr, nullptr);
  char label[128];
  snprintf(label, sizeof label, "%s:fam%d:d%d:T%d:o%d:s%d:e%d", tag, desc.family, desc.dof, desc.horizon, desc.n_obstacles, desc.span, desc.n_eq_rows);
  if (sweep(from_qp(std::string(label) + ":qp0", L.qp0, L.n_x, L.m_lin + L.n_x))) return 1;
  const Pat q1 = from_qp(std::string(label) + ":qp1", L.qp1, L.n, L.m);
  if (sweep(q1)) return 1;
#ifndef SWEEP_PARENT
  {
    // link points spread over the links, all on the first, all on the last, and in descending order
    const int K = desc.n_points, d = desc.dof;
    std::vector<int> spread(K), first(K, 0), last(K, d - 1), down(K);
    for (int k = 0; k < K; k++) { spread[k] = std::min(d - 1, ((k + 1) * d - 1) / K); down[k] = std::max(0, d - 1 - k); }
    for (const auto &links : {spread, first, last, down}) if (sweep_hint(desc, L, q1, links)) return 1;
  }
#endif
  // rows the wavefront tier refuses for a reason of its own, added to the penalty QP of the plain descriptors
  if ((desc.family & ~15) == 0 && desc.dof >= 2 && desc.dof <= 3 && desc.horizon >= 4 && desc.horizon <= 5) {
    const int d = desc.dof;
    if (sweep(with_rows(q1, ":link3", {{0, d}, {0, d}, {0, d}}))) return 1;                // a third link row on one pair
    if (sweep(with_rows(q1, ":same", {{0, 1}}))) return 1;                                 // two core variables of one block
    if (sweep(with_rows(q1, ":far", {{0, 2 * d}}))) return 1;                              // blocks that are not neighbours
    if (sweep(with_rows(q1, ":index", {{0, d + 1}}))) return 1;                            // different in-block indices
    if (sweep(with_rows(q1, ":three", {{0, d, 2 * d}}))) return 1;                         // three core variables
    if (sweep(with_rows(q1, ":stack", {{d}, {d}, {d}, {d}}))) return 1;                    // single rows beyond the free link slots
  }
  return 0;
}

int main(int argc, char **argv) {
  out = argc > 1 ? fopen(argv[1], "w") : stdout;
  if (!out) { printf("cannot write %s\n", argv[1]); return 1; }
  only_tag = argc > 2 ? argv[2] : nullptr;
  // ---- trajectory descriptors
  const int horizons[] = {2, 3, 5, 9, 10, 17, 18, 21, 22, 24};
  const int fams[] = {SCO_FAM_ARM_CIRCLES, SCO_FAM_ARM_REACH, SCO_FAM_POINT_CIRCLES, SCO_FAM_STATE_QUADRATIC, SCO_FAM_STATE_PROGRAM};
  for (int fam : fams)
    for (int fl = 0; fl < 4; fl++)
      for (int dof = 1; dof <= 8; dof++)
        for (int T : horizons)
          for (int var = 0; var < (fam >= SCO_FAM_STATE_QUADRATIC ? 3 : 1); var++) {
            // var 1: the last row of a block an equality; var 2 (programs): blocks of two timesteps
            const int family = fam | (fl & 1 ? SCO_FAM_FLAG_VEL_LIMITS : 0) | (fl & 2 ? SCO_FAM_FLAG_JOINT_LIMITS : 0);
            if (var == 2 && fam != SCO_FAM_STATE_PROGRAM) continue;
            const sco_trajopt_desc desc = {3, dof, T, fam <= SCO_FAM_ARM_REACH ? 2 : 1, 2, family, 0, 0, var == 2 ? 2 : 0, var == 1 ? 1 : 0};
            if (sweep_desc(desc, "traj")) return 1;
          }
  // ---- descriptors with a Jacobian width hint that reaches a profiled kernel: 7 joints, 17 .. 20 timesteps, 5 link points,
  // two obstacles, planar and spatial (the other descriptors of the sweep take the hint too, and stay generic)
  for (int fam : {SCO_FAM_ARM_CIRCLES, SCO_FAM_ARM_REACH, SCO_FAM_ARM_SPATIAL})
    for (int T = 16; T <= 21; T++) {
      const sco_trajopt_desc desc = {3, 7, T, 5, 2, fam, 0, 0, 0, 0};
      if (sweep_desc(desc, "hint")) return 1;
    }
  // ---- wide descriptors: block orders 12 and 16 of the structured form; 12 x 50 is beyond a CU's LDS without force_big
  // ... and a long narrow one (2 x 50, 10 obstacles): 500 slacks beside a core of 100 leave too few threads for the free rows
  // in two row slots, on a W tile that has no three-slot kernel (rl_plan_build refuses; the tier choice goes on)
  {
    const int wide[][3] = {{9, 4, 2}, {12, 6, 2}, {12, 50, 8}, {13, 5, 3}, {16, 4, 2}, {16, 12, 6}, {2, 50, 10}};
    for (const auto &w : wide)
      for (int fl = 0; fl < 4; fl += 3) {
        const sco_trajopt_desc desc = {3, w[0], w[1], 1, w[2], SCO_FAM_POINT_CIRCLES | (fl ? SCO_FAM_FLAG_VEL_LIMITS | SCO_FAM_FLAG_JOINT_LIMITS : 0), 0, 0, 0, 0};
        if (sweep_desc(desc, "wide")) return 1;
      }
  }
  // ---- random sparse patterns: a diagonal of P on some variables, a few off-diagonal entries, rows of 1 .. 4 entries;
  // every eighth one banded (the structured form takes those), every 500th larger than the on-chip planners' caps
  unsigned long long rng = 88172645463325252ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (unsigned)(rng >> 11); };
  for (int it = 0; it < (only_tag ? 0 : 3000); it++) {
    const bool large = it % 500 == 499, banded = it % 8 == 0;
    Pat p;
    p.n = large ? 520 + next() % 600 : 2 + next() % 60; p.m = large ? 1100 + next() % 2200 : next() % 120;
    char label[64]; snprintf(label, sizeof label, "rand%d:n%d:m%d", it, p.n, p.m); p.label = label;
    const int pd = next() % 3, poff = next() % 3;
    std::vector<std::vector<int>> pcol(p.n), acol(p.n);
    for (int j = 0; j < p.n; j++) {
      if (pd == 0 || (pd == 1 && next() % 2)) pcol[j].push_back(j);
      if (poff && j > 0 && next() % (poff == 1 ? 6 : 2) == 0) pcol[j].push_back(banded ? std::max(0, j - 1 - (int)(next() % 3)) : (int)(next() % j));
    }
    for (int i = 0; i < p.m; i++) {
      const int k = 1 + next() % 4, j0 = next() % p.n;
      for (int e = 0; e < k; e++) acol[banded ? std::min(p.n - 1, j0 + e) : (int)(next() % p.n)].push_back(i);
    }
    p.Pp.assign(1, 0); p.Ap.assign(1, 0);
    for (int j = 0; j < p.n; j++) {
      for (std::vector<int> *c : {&pcol[j], &acol[j]}) { std::sort(c->begin(), c->end()); c->erase(std::unique(c->begin(), c->end()), c->end()); }
      p.Pi.insert(p.Pi.end(), pcol[j].begin(), pcol[j].end()); p.Pp.push_back((int)p.Pi.size());
      p.Ai.insert(p.Ai.end(), acol[j].begin(), acol[j].end()); p.Ap.push_back((int)p.Ai.size());
    }
    if (sweep(p)) return 1;
  }
  if (out != stdout) fclose(out);

  printf("%lld patterns, %lld plans\n", n_patterns, n_plans);
  const struct { const char *name; const Count *c; } planners[] = {{"fast_plan_build", &n_fast}, {"reg_plan_build", &n_reg}, {"rl_plan_build", &n_rl},
                                                                   {"wv_plan_build", &n_wv}, {"big_plan_build", &n_big}, {"bt_plan_build", &n_bt}};
  bool covered = true;
  for (const auto &pc : planners) {
    printf("%-16s accepted %8lld  refused %8lld\n", pc.name, pc.c->acc, pc.c->ref);
    covered = covered && pc.c->acc > 0 && pc.c->ref > 0;
  }
  printf("bt_plan_build block orders: 4: %lld  8: %lld  12: %lld  16: %lld\n", n_bs[4], n_bs[8], n_bs[12], n_bs[16]);
  covered = covered && n_bs[4] && n_bs[8] && n_bs[12] && n_bs[16];
  const char *why_name[11] = {"WV_OK", "WV_WHY_OTHER", "WV_WHY_LINKS_OFF", "WV_WHY_THIRD_LINK", "WV_WHY_SAME_BLOCK", "WV_WHY_FAR_BLOCKS",
                              "WV_WHY_INDEX", "WV_WHY_THREE_CORE", "WV_WHY_LDS", "WV_WHY_SHAPE", "WV_WHY_STACKED"};
  for (int w = 0; w <= 10; w++) {
    printf("  %-18s %8lld\n", why_name[w], n_why[w]);
    if (!n_why[w]) covered = false;
  }
  printf("qp_choose_tiers: SCO_OK %lld  SCO_ERR_ARG %lld  SCO_ERR_CAPACITY %lld\n", n_tier_rc[0], n_tier_rc[-SCO_ERR_ARG], n_tier_rc[-SCO_ERR_CAPACITY]);
  printf("width hints: %lld applied, %lld with a profile\n", n_hint, n_profiled);
#ifndef SWEEP_PARENT
  if (!n_hint || !n_profiled) covered = false;
#endif
  if (only_tag) { printf("partial sweep (%s): every accepted plan of it keeps its indices in range\n", only_tag); return 0; }
  if (!covered) { printf("COVERAGE: a planner, a block order or a WvWhy code did not appear\n"); return 1; }
  printf("every accepted plan keeps its indices in range and its LDS request within its planner's cap\n");
  return 0;
}
