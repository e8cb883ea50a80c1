// qp_tier_plans.h -- the host plans of the ADMM tiers and the tier choice of a handle: what a planner hands to its
// kernel file's upload and launch code.  No device type and no HIP header: the planners (rl_plan.cpp, wv_plan.cpp,
// big_plan.cpp, reg_fast_plan.cpp), the tier choice (qp_tier.cpp) and the debug views (qp_debug.cpp) are plain C++, built
// and swept by a host compiler alone (scripts/sanitize/tier_plan_sweep.cpp, tests/test_host_only_sources.py).  The device
// side of every tier -- *Dev, arguments, upload, launch -- is sco_internal.h, which includes this header.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/sco_hip.h"
#include "layout_qp.h"      // SCO_LDS_CAP: no planner promises its kernel more LDS than that
#include "qp_plan.h"
#include "qp_tier.h"

void sco_set_error(const std::string &msg);     // (sco_qp.hip: the text behind sco_last_error)

// ---- fast ADMM path (sco_admm_fast.hip) ------------------------------------
// Sliced-ELL image of a sparse operator: slices of 64 items, entry k of item
// (slice s, lane l) at base[s] + 64 k + l; idx = 16-bit index of the gathered
// vector element, src = position of the value in the flat per-problem array.
struct SellHost {
  int nitems = 0, total = 0;
  std::vector<int> base, width, src;
  std::vector<unsigned short> idx;
};
struct FastHost { SellHost Ac, Ar, Ca, Ce; int TR = 1, TC = 2; bool capped = false; size_t lds_doubles = 0, lds_bytes = 0; };
bool fast_plan_build(const QpPlan &pl, FastHost &fh);

// ---- register-resident ADMM path (sco_admm_reg.hip) -------------------------
// Per-thread programs: slot s of thread t at [s * 512 + t]; slots = CW column
// entries, 2 x RW row entries, PX coupling entries.
struct RegHost {
  int TR = 1, TC = 2, CW = 0, RW = 0, PX = 0;
  SellHost Ac, Ar, Ca, Ce;
  size_t lds_bytes = 0;
  std::vector<int> role;
  std::vector<unsigned short> off;
};
int reg_caps_for(const QpPlan &pl, int *CW, int *RW, int *PX);
size_t reg_static_lds();              // static LDS of qp_admm_reg_kernel, bytes (the dynamic part: RegHost::lds_bytes)
bool reg_plan_build(const QpPlan &pl, int CW, int RW, int PX, RegHost &rh);

// ---- row-local ADMM path (sco_admm_rl.hip): the coupling block never materialises
struct RlHost {
  int TR = 1, TC = 2, CW = 12;     // CW: slots for a core variable's column entries (12 or 16)
  int pcw = 0;                     // most P entries in a core variable's column (<= 4: cached in LDS for the termination test)
  int zpos = 0;                    // LDS position of the always-zero pair of the row vectors
  bool merged = false;             // closed thread assignment: phases (Y) and (1) share a wavefront, one barrier less per iteration
  bool aligned = false;            // closed assignment + the W rows of a wavefront's core columns in that wavefront: phases
                                   // (3), (Y), (1) are wavefront-local, ONE barrier per iteration (double-buffered right-hand side)
  bool split = false;              // a core column's entries in two neighbouring lanes (owner + helper), phase (1) on twice the lanes
  bool lay8 = false;               // 8 column groups of the W tile (3 x 18) with the open assignment
  int NS = 2;                      // row slots per thread (3: patterns with more than 1024 rows)
  SellHost Ac, Ar[3];
  size_t lds_bytes = 0;
  std::vector<unsigned short> off;
  std::vector<int> role, pc_ptr, pc_pos, pc_core;
};
size_t rl_reported_static_lds();      // what sco_qp_info adds for qp_admm_rl_kernel's static LDS, bytes (see there: not today's size)
bool rl_plan_build(const QpPlan &pl, RlHost &rh, const QpCreateEnv &env);   // env: rl_closed, rl_lay8, rl_split_off, debug_plan

// ---- wavefront tier (sco_admm_wv.hip): one wavefront per problem, block-tridiagonal core solve, four problems per CU
#define SCO_WV_PER_CU 4       // (wv_launch's LDS request keeps a fifth workgroup off a CU: one wavefront per SIMD)
struct WvHost {
  int bs = 0, nb = 0, mid = 0, lpb = 0, n_extra = 0;    // block order, blocks, middle block, lanes per block, second single rows
  int BS = 8, NS = 1, NV = 1, NSTEP = 4;                 // instantiation: mat-vec width, hinge-row / variable slots per lane, sweep steps
  int cst_slots = 0;
  size_t g_doubles = 0, lds_doubles = 0, lds_bytes = 0;
  std::vector<int> tab;                                  // lane tables (wv_tab_layout)
  // link rows (rows on one in-block index of two neighbouring blocks: velocity limits): how many, link slots per variable
  // slot (0: a link-free plan, the tables and the kernel of such a plan are untouched), problems per CU the LDS leaves room
  // for, and why the plan was refused (WvWhy)
  int n_link = 0, NL = 0, per_cu = SCO_WV_PER_CU, why = 0;
  // stacked rows (single rows of a core variable other than its last one, held in the variable slot's free link slots with an
  // empty partner: joint limits).  NL = WV_NL whenever n_link + n_stack > 0
  int n_stack = 0;
  // Jacobian widths (wv_plan_widths): jw[q] = leading in-block columns of hinge slot q that may hold a non-zero, by the
  // caller's hint (bs without one); jw_profile = the compiled width profile the launch runs (packed, layout_wv.h: it
  // dominates jw slot by slot; 0 = the generic kernel, every slot at the full width)
  int jw[4] = {0, 0, 0, 0}, jw_profile = 0;
  bool jsorted = false;                                  // the rows were dealt by width (wv_plan_build's sort_width)
};
// row_width[m]: for every row the count of leading in-block columns that may be non-zero, <= 0 = no promise (null: none for
// any row).  Only hinge rows are read.  off (SCO_WV_JW=0): the widths are recorded, the generic profile runs.  The lane
// tables, the LDS request and the row assignment stay as wv_plan_build left them.
void wv_plan_widths(WvHost &wh, const int *row_width, bool off);
#define WV_NL 2               // link slots per variable slot: two one-sided rows per joint and transition, or one two-sided row
// why wv_plan_build refused a pattern (sco_debug_wv_link_plan, info[13])
enum WvWhy { WV_OK = 0, WV_WHY_OTHER = 1, WV_WHY_LINKS_OFF = 2, WV_WHY_THIRD_LINK = 3, WV_WHY_SAME_BLOCK = 4, WV_WHY_FAR_BLOCKS = 5,
             WV_WHY_INDEX = 6, WV_WHY_THREE_CORE = 7, WV_WHY_LDS = 8, WV_WHY_SHAPE = 9,
             WV_WHY_STACKED = 10 };   // single rows of a variable beyond its free link slots, or beyond the extra-row lanes
// sort_width[m] (may be null): a block's hinge rows are dealt to lanes and slots in descending order of their width
// (wv_plan_widths' reading of an entry; rows of equal width keep their order) instead of row order: slot 0 gets the widest
// rows.  A block's partial column sums then add in another order: results move at rounding level (SCO_WV_JSORT=0 keeps the row order).
bool wv_plan_build(const QpPlan &pl, WvHost &wh, bool allow_links, const int *sort_width = nullptr);

// ---- big tier (sco_qp_big.hip): everything in HBM/L2, 1024 threads per problem
struct BigHost {
  std::vector<int> row_elim, row_epos, er_ptr, er_row, free_rows, pc_ptr, pc_pos, pc_core;
  size_t ws_doubles = 0;
};
bool big_plan_build(const QpPlan &pl, BigHost &bh);
// structured variant of the big tier: block-tridiagonal core solve (factors in LDS) and
// dense row blocks addressed without index arrays
struct BtHost {
  int bs = 0, nb = 0, nchunks = 0, npart = 0;
  bool use_part = false;          // dense chunks reduce A' t in the wavefront (no product round trip)
  std::vector<int> cent;          // [n_c padded][4] column contributions: >= 0 partial index, <= -2 product position, -1 none
  size_t blk_doubles = 0, ws_doubles = 0, lds_bytes = 0;
  std::vector<int> ch_desc, it;     // it: 8 ints per chunk slot (e, j, r0, r1, ep0, ep1, core idx, core pos)
  // r04 (N1): block normal matrices on the matrix cores.  For blocks of order >= 12 whose hinge rows are dense, the sum over
  // those rows inside every diagonal-block entry of S is formed by v_mfma_f64_16x16x4 (one wavefront per block) between the
  // terms that come before them in the entry's list and the ones after: mf_id [nb][256] entry id of tile position (i, j),
  // i >= j (-1: none); mf_h0 / mf_h1 [nS] the run of hinge-row terms inside the entry's A' R A list (h0 = h1: none)
  bool use_mfma = false;
  int mf_why = 0;                 // 0 used, 1 switched off, 2 block order outside 12 .. 16, 3 hinge terms not one run, 4 rows differ between entries, 5 hole in a block, 6 no hinge rows
  std::vector<int> mf_id, mf_h0, mf_h1;
};
bool bt_plan_build(const QpPlan &pl, const BigHost &bh, BtHost &th, bool no_mfma);

// Everything sco_qp_create decides about a handle before it allocates (qp_choose_tiers, qp_tier.cpp: host code, no HIP
// call).  Of the tier plans only those the handle can launch are built: the global-memory tier (and its structured form),
// or the ONE on-chip kernel that runs -- the first of row-local, register-offset, sliced-ELL whose plan fits, else the
// generic kernel -- and the wavefront tier beside the row-local kernel.
struct QpTiers {
  QpPlan plan;                         // (after the second analysis, where the global-memory tier asked for one)
  size_t lds_setup = 0, lds_admm = 0;  // dynamic LDS of qp_setup_kernel (with the packed S) and qp_admm_kernel
  bool factor_cholesky = false;        // SCO_QP_FACTOR_CHOLESKY=1: W by Cholesky + triangular inverse (cross-check)
  bool use_big = false, use_bt = false;
  int kern = QP_K_GENERIC;             // QpKernel: the on-chip ADMM kernel of this handle (!use_big)
  bool use_wv = false;
  BigHost big;
  BtHost bt;
  RlHost rl;
  WvHost wv;
  RegHost reg;
  FastHost fast;
};
// SCO_OK, or an SCO_ERR_* with *err set to the text for sco_set_error
int qp_choose_tiers(int n, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai, const QpCreateEnv &env, QpTiers &t,
                    std::string *err);
int qp_tier_mask(const QpTiers &t);    // the bits of sco_debug_qp_tiers
