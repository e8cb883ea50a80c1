// qp_debug.cpp -- the host-only debug entry points of the QP layer (include/sco_hip.h, sco_debug_*): views of the symbolic
// analysis, the tier plans and the tier choice for the CPU test-suite.  Plain C++, no HIP call.  Every entry point reads the
// environment afresh (qp_create_env), so a test that sets a variable and then asks for a plan sees it.
#include "qp_tier_plans.h"
#include "layout_fast.h"
#include "layout_wv.h"

#include <algorithm>
#include <cstring>

// --------------------------------------------------------------------------
// Host-only debug view of the symbolic analysis (no HIP call): lets the CPU
// test-suite check the plans against a NumPy emulation of the kernels.
// sizes[16]: n_e, n_c, ncpl, nS, len(cp_row), len(sa_row), len(ss_k1), nnzFull
// --------------------------------------------------------------------------
static QpPlan g_dbg_plan;
extern "C" int sco_debug_plan_build(int n, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                                    int allow_elim, int *sizes) {
  int rc = qp_plan_build(n, m, Pp, Pi, Ap, Ai, allow_elim, g_dbg_plan);
  if (rc) return SCO_ERR_ARG;
  const QpPlan &p = g_dbg_plan;
  sizes[0] = p.n_e; sizes[1] = p.n_c; sizes[2] = p.ncpl; sizes[3] = p.nS;
  sizes[4] = (int)p.cp_row.size(); sizes[5] = (int)p.sa_row.size(); sizes[6] = (int)p.ss_k1.size();
  sizes[7] = (int)p.Fi.size();
  return SCO_OK;
}
// Host-only: would the pattern last given to sco_debug_plan_build land on the row-local tier, and with what shape?
// info[0] fits, [1] CW (value slots per column = 2 x operand pairs), [2] TR, [3] TC, [4] dynamic LDS bytes, [5] closed plan,
// [6] 1 = aligned closed plan (one barrier per iteration), 2 = 8 column groups of the W tile with the open assignment,
// [7] row slots per thread
extern "C" int sco_debug_rl_plan(int *info) {
  RlHost rh;
  const bool ok = rl_plan_build(g_dbg_plan, rh, qp_create_env());
  info[0] = ok ? 1 : 0; info[1] = rh.CW; info[2] = rh.TR; info[3] = rh.TC; info[4] = (int)rh.lds_bytes; info[5] = rh.merged ? 1 : 0; info[6] = rh.aligned ? 1 : rh.lay8 ? 2 : 0; info[7] = rh.NS;
  return SCO_OK;
}
// Host-only: the sliced-ELL plan of that pattern (whether or not an earlier tier of the choice takes it) and the
// instantiation fast_launch would pick.  info[0] fits, [1] TR, [2] TC, [3] capped dots (<12, 8, 12, 8>; 0: the looping form),
// [4] rows per thread, [5] LDS bytes
extern "C" int sco_debug_fast_plan(int *info) {
  FastHost fh;
  const bool ok = fast_plan_build(g_dbg_plan, fh);
  const int nq = fast_rows_per_thread(g_dbg_plan.m);
  info[0] = ok ? 1 : 0; info[1] = fh.TR; info[2] = fh.TC; info[3] = (fh.capped && nq == 2) ? 1 : 0; info[4] = nq; info[5] = (int)fh.lds_bytes;
  return SCO_OK;
}
// Host-only: the register-offset plan of that pattern.  info[0] fits (the caps and the per-thread programs), [1] TR, [2] TC,
// [3] CW, [4] RW, [5] PX, [6] dynamic LDS bytes (the kernel's static LDS comes on top: reg_static_lds)
extern "C" int sco_debug_reg_plan(int *info) {
  RegHost rh;
  int CW = 0, RW = 0, PX = 0;
  const bool ok = reg_caps_for(g_dbg_plan, &CW, &RW, &PX) && reg_plan_build(g_dbg_plan, CW, RW, PX, rh);
  info[0] = ok ? 1 : 0; info[1] = rh.TR; info[2] = rh.TC; info[3] = rh.CW; info[4] = rh.RW; info[5] = rh.PX; info[6] = (int)rh.lds_bytes;
  return SCO_OK;
}
// Host-only: would that pattern land on the wavefront tier with the link-free plan?  info[0] fits, [1] block order,
// [2] blocks, [3] lanes per block, [4] instantiation BS, [5] NS, [6] NV, [7] NSTEP, [8] LDS bytes, [9] second single rows
static bool dbg_wv_plan(bool allow_links, int *info, WvHost &wh) {
  const bool ok = wv_plan_build(g_dbg_plan, wh, allow_links);
  info[0] = ok ? 1 : 0; info[1] = wh.bs; info[2] = wh.nb; info[3] = wh.lpb; info[4] = wh.BS; info[5] = wh.NS; info[6] = wh.NV;
  info[7] = wh.NSTEP; info[8] = (int)wh.lds_bytes; info[9] = wh.n_extra;
  return ok;
}
extern "C" int sco_debug_wv_plan(int *info) {
  WvHost wh;
  dbg_wv_plan(false, info, wh);
  return SCO_OK;
}
// ... and with the plan a handle builds, link rows allowed: the ten fields above, then [10] link rows, [11] link slots per
// variable slot (0: no link rows), [12] problems per CU, [13] why the plan was refused (WvWhy: 0 accepted, 1 other,
// 2 link rows not allowed, 3 a third link row on one pair, 4 two core variables of one block without a slack, 5 blocks that
// are not neighbours, 6 different in-block indices, 7 three or more core variables, 8 LDS, 9 no instantiation for the shape)
extern "C" int sco_debug_wv_link_plan(int *info) {
  WvHost wh;
  dbg_wv_plan(true, info, wh);
  info[10] = wh.n_link; info[11] = wh.NL; info[12] = wh.per_cu; info[13] = wh.why;
  return SCO_OK;
}
// ... the same fourteen fields (why: also 10 = single rows of a variable beyond its free link slots or beyond the extra-row
// lanes), then [14] stacked rows: single rows held in a variable slot's link slots with an empty partner
extern "C" int sco_debug_wv_stack_plan(int *info) {
  WvHost wh;
  dbg_wv_plan(true, info, wh);
  info[10] = wh.n_link; info[11] = wh.NL; info[12] = wh.per_cu; info[13] = wh.why; info[14] = wh.n_stack;
  return SCO_OK;
}
// Host-only: the plan of a handle (link rows allowed) with the Jacobian width hint row_width[m] (null: none), under SCO_WV_JW
// as it stands.  info[0] fits, [1 .. 4] widths of the hinge slots, [5] the width profile of the launch (packed, 0 = generic),
// [6] LDS bytes, [7 .. 10] <BS, NS, NV, NSTEP>, [11] lanes per block
extern "C" int sco_debug_wv_widths(const int *row_width, int info[12]) {
  if (!info) return SCO_ERR_ARG;
  WvHost wh;
  const QpCreateEnv env = qp_create_env();
  const bool ok = wv_plan_build(g_dbg_plan, wh, true, env.wv_jsort && !env.wv_jw_off ? row_width : nullptr);
  if (ok) wv_plan_widths(wh, row_width, env.wv_jw_off);
  info[0] = ok ? 1 : 0;
  for (int q = 0; q < 4; q++) info[1 + q] = wh.jw[q];
  info[5] = wh.jw_profile; info[6] = (int)wh.lds_bytes; info[7] = wh.BS; info[8] = wh.NS; info[9] = wh.NV; info[10] = wh.NSTEP;
  info[11] = wh.lpb;
  return SCO_OK;
}
// Host-only: the structured global-memory plan of that pattern.  info[0] fits, [1] block order, [2] blocks, [3] block normal
// matrices on the matrix cores, [4] why not (BtHost::mf_why), [5] LDS bytes
extern "C" int sco_debug_bt_plan(int *info) {
  BigHost bh; BtHost th;
  const bool ok = g_dbg_plan.n_c <= 1024 && big_plan_build(g_dbg_plan, bh) && bt_plan_build(g_dbg_plan, bh, th, qp_create_env().no_mfma);
  info[0] = ok ? 1 : 0; info[1] = th.bs; info[2] = th.nb; info[3] = th.use_mfma ? 1 : 0; info[4] = th.mf_why; info[5] = (int)th.lds_bytes;
  return SCO_OK;
}
// Host-only: the mask sco_debug_qp_tiers would give for a handle created now -- under the SCO_QP_* switches as they stand --
// from the pattern last given to sco_debug_plan_build (whatever allow_elim was passed there)
extern "C" int sco_debug_plan_tiers(int *mask) {
  const QpPlan &p = g_dbg_plan;
  if (!mask || p.n <= 0) return SCO_ERR_ARG;
  QpTiers t;
  std::string err;
  if (const int rc = qp_choose_tiers(p.n, p.m, p.Pp.data(), p.Pi.data(), p.Ap.data(), p.Ai.data(), qp_create_env(), t, &err)) {
    sco_set_error(err);
    return rc;
  }
  *mask = qp_tier_mask(t);
  return SCO_OK;
}
extern "C" int sco_debug_plan_get(const char *name, int *out, int cap) {
  const QpPlan &p = g_dbg_plan;
  const std::vector<int> *v = nullptr;
#define F(x) if (!strcmp(name, #x)) v = &p.x;
  F(Rp) F(Rj) F(Rpos) F(Fp) F(Fi) F(Fpos) F(Pdiag) F(elim_var) F(core_var) F(elim_of) F(core_of)
  F(e_ptr) F(pair_core) F(pair_elim) F(cp_ptr) F(cp_row) F(cp_pa) F(cp_pe) F(a_ptr) F(a_pair)
  F(s_a) F(s_b) F(s_ppos) F(sa_ptr) F(sa_row) F(sa_pa) F(sa_pb) F(ss_ptr) F(ss_k1) F(ss_k2) F(ss_e)
#undef F
  if (!v) return SCO_ERR_ARG;
  if ((int)v->size() > cap) return SCO_ERR_CAPACITY;
  std::copy(v->begin(), v->end(), out);
  return (int)v->size();
}
// out[5] = pair, row, slot, vidx, eidx of block position pos in the NSTEP-step kernel (-1s: no sweep lane holds it)
extern "C" int sco_debug_wv_gres_slot(int nstep, int pos, int out[5]) {
  if (!out || nstep <= 0) return SCO_ERR_ARG;
  const WvGresSlot s = wv_gres_slot(nstep, pos);
  out[0] = s.pair; out[1] = s.row; out[2] = s.slot; out[3] = s.vidx; out[4] = s.eidx;
  return SCO_OK;
}
