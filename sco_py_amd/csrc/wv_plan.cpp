// wv_plan.cpp -- host plan of the wavefront tier (kernels: sco_admm_wv.hip): which patterns the tier takes, the lane
// tables its kernels follow, its LDS request.  Plain C++, no HIP call; the layout both sides agree on is layout_wv.h.
#include "qp_tier_plans.h"
#include "layout_wv.h"

#include <algorithm>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------------------------
// host plan
// ---------------------------------------------------------------------------------------------------------------------
// Why a pattern without a block structure has none, for the refusal's reason only: the block order is read off P (the
// smoothing objective couples c with c + bs) and the rows without a slack are judged by it.
static int wv_why_no_blocks(const QpPlan &pl) {
  int bs = 0;
  for (int c = 0; c < pl.n; c++)
    for (int t = pl.Pp[c]; t < pl.Pp[c + 1]; t++) {
      const int r = pl.Pi[t];
      if (r != c && pl.core_of[r] >= 0 && pl.core_of[c] >= 0) bs = std::max(bs, std::abs(pl.core_of[c] - pl.core_of[r]));
    }
  if (bs <= 0 || pl.n_c % bs) return WV_WHY_OTHER;
  int why = WV_WHY_OTHER;
  for (int i = 0; i < pl.m; i++) {
    int nc = 0, c0 = -1, c1 = -1; bool slack = false;
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int j = pl.Rj[s];
      if (pl.elim_of[j] >= 0) { slack = true; continue; }
      const int c = pl.core_of[j];
      if (!nc) c0 = c1 = c; else { c0 = std::min(c0, c); c1 = std::max(c1, c); }
      nc++;
    }
    if (slack || nc < 2) continue;
    if (nc >= 3) return WV_WHY_THREE_CORE;
    if (c1 / bs == c0 / bs) why = WV_WHY_SAME_BLOCK;
    else if (c1 % bs != c0 % bs) why = WV_WHY_INDEX;
    else if (c1 / bs > c0 / bs + 1) why = WV_WHY_FAR_BLOCKS;
  }
  return why;
}

bool wv_plan_build(const QpPlan &pl, WvHost &wh, bool allow_links, const int *sort_width) {
  wh = WvHost();
  wh.why = WV_WHY_OTHER;
  const int n_c = pl.n_c, n_e = pl.n_e, m = pl.m;
  if (n_e <= 0 || n_c <= 0) return false;
  // ---- block structure of S: within a block, or between neighbouring blocks at equal in-block index
  int hb = 0;
  for (int id = 0; id < pl.nS; id++) hb = std::max(hb, pl.s_a[id] - pl.s_b[id]);
  auto valid = [&](int bs) {
    if (bs <= 0 || bs > 8 || n_c % bs) return false;
    for (int id = 0; id < pl.nS; id++) {
      const int a = pl.s_a[id], b = pl.s_b[id], ta = a / bs, tb = b / bs;
      if (!(ta == tb || (ta == tb + 1 && a % bs == b % bs))) return false;
    }
    return true;
  };
  int bs = 0;
  if (valid(hb)) bs = hb; else if (valid(n_c)) bs = n_c; else { wh.why = wv_why_no_blocks(pl); return false; }
  const int nb = n_c / bs;
  for (int e = 0; e < n_e; e++) if (pl.Pdiag[pl.elim_var[e]] >= 0) return false;      // no P entry on an eliminated variable
  // ---- rows
  std::vector<int> h_of(n_e, -1), b_of(n_e, -1), hblk(n_e, -1);
  std::vector<std::vector<int>> single(n_c), link(n_c);       // link[c]: the rows on c and c + bs, in row order
  for (int i = 0; i < m; i++) {
    int ne = 0, nc = 0, e = -1, blk = -1, c0 = -1, c1 = -1; bool one_blk = true;
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int j = pl.Rj[s];
      if (pl.elim_of[j] >= 0) { ne++; e = pl.elim_of[j]; }
      else {
        const int c = pl.core_of[j], t = c / bs;
        if (nc && t != blk) one_blk = false;
        if (!nc) c0 = c1 = c; else { c0 = std::min(c0, c); c1 = std::max(c1, c); }
        blk = t; nc++;
      }
    }
    if (ne == 1 && nc >= 1 && one_blk) { if (h_of[e] >= 0) return false; h_of[e] = i; hblk[e] = blk; }
    else if (ne == 1 && nc == 0) { if (b_of[e] >= 0) return false; b_of[e] = i; }
    else if (ne == 0 && nc == 1) single[pl.core_of[pl.Rj[pl.Rp[i]]]].push_back(i);
    else if (ne == 0 && nc == 2) {
      // a link row: no slack, one in-block index of two neighbouring blocks; it belongs to the variable of the earlier block
      if (one_blk) { wh.why = WV_WHY_SAME_BLOCK; return false; }
      if (c1 % bs != c0 % bs) { wh.why = WV_WHY_INDEX; return false; }
      if (c1 != c0 + bs) { wh.why = WV_WHY_FAR_BLOCKS; return false; }
      if (!allow_links) { wh.why = WV_WHY_LINKS_OFF; return false; }
      if ((int)link[c0].size() >= WV_NL) { wh.why = WV_WHY_THIRD_LINK; return false; }
      link[c0].push_back(i); wh.n_link++;
    }
    else { if (ne == 0 && nc >= 3) wh.why = WV_WHY_THREE_CORE; return false; }
  }
  wh.NL = wh.n_link > 0 ? WV_NL : 0;
  for (int e = 0; e < n_e; e++)
    if (h_of[e] < 0 || b_of[e] < 0 || pl.Ap[pl.elim_var[e] + 1] - pl.Ap[pl.elim_var[e]] != 2) return false;
  // ---- single rows.  The variable's own slot takes its LAST single row (the box row: below); xrow[c] is the row it gives to
  // an extra-row lane, stack[c] the rows it holds in its free link slots
  int n_extra = 0; bool plain = true;
  std::vector<int> xrow(n_c, -1);
  std::vector<std::vector<int>> stack(n_c);
  for (int c = 0; c < n_c; c++) { if (single[c].size() > 2) plain = false; if (single[c].size() == 2) n_extra++; }
  if (plain && n_extra <= WV_T) {
    // at most two single rows per variable and a lane for every second one: the first row of a pair on an extra-row lane
    for (int c = 0; c < n_c; c++) if (single[c].size() == 2) xrow[c] = single[c][0];
  } else {
    // STACKED rows: the rows in front of the last one go into the variable's free link slots, filled from the back, in row
    // order.  One row may be left over: the variable's first (the place of a pin in the reference's row order), which takes
    // an extra-row lane.  A variable with two single rows keeps its first one on a lane while lanes last (handed out in
    // column order, behind the left-over rows), then stacks it.  (A pin that ends up in a slot -- three single rows with both
    // slots free -- fails the value test, rho_eq: such problems run on the row-local kernel.)
    if (!allow_links) return false;
    int n_left = 0;
    for (int c = 0; c < n_c; c++) {
      const int k = (int)single[c].size(), free_slots = WV_NL - (int)link[c].size();
      if (k < 3) continue;
      if (k - 1 > free_slots + 1) { wh.why = WV_WHY_STACKED; return false; }
      const int ns = std::min(free_slots, k - 1);
      stack[c].assign(single[c].end() - 1 - ns, single[c].end() - 1);
      if (k - 1 > ns) { xrow[c] = single[c][0]; n_left++; }
    }
    if (n_left > WV_T) { wh.why = WV_WHY_STACKED; return false; }
    n_extra = n_left;
    for (int c = 0; c < n_c; c++) {
      if (single[c].size() != 2) continue;
      if (n_extra < WV_T) { xrow[c] = single[c][0]; n_extra++; }
      else if ((int)link[c].size() < WV_NL) stack[c].push_back(single[c][0]);
      else { wh.why = WV_WHY_STACKED; return false; }
    }
    for (int c = 0; c < n_c; c++) wh.n_stack += (int)stack[c].size();
  }
  wh.NL = wh.n_link + wh.n_stack > 0 ? WV_NL : 0;
  // ---- lanes
  int lpb = 0;
  for (int L = 8; L >= 1; L--) if (nb <= 4 * (16 / L)) { lpb = L; break; }
  if (!lpb) return false;
  const int bpr = 16 / lpb;
  std::vector<std::vector<int>> hin(nb);
  for (int e = 0; e < n_e; e++) hin[hblk[e]].push_back(e);          // elimination order = row order inside a block
  if (sort_width) {
    auto width = [&](int e) { const int w = sort_width[h_of[e]]; return (w > 0 && w < bs) ? w : bs; };
    for (auto &v : hin) std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return width(a) > width(b); });
    wh.jsorted = true;
  }
  int maxh = 0;
  for (auto &v : hin) maxh = std::max(maxh, (int)v.size());
  const int NS = std::max(1, (maxh + lpb - 1) / lpb), NV = (bs + lpb - 1) / lpb;
  const int mid = nb / 2;
  // instantiations <BS, NS, NV, NSTEP>, the smallest that holds the shape first (row slots and padded block steps of a larger one
  // are executed all the same): <8, 1, 1, 4>, <8, 2, 2, 8>, <8, 2, 2, 10>, and <7, 4, 3, 10> for the 7-DOF x 20 shapes.  A shape that
  // would need more (e.g. 4-DOF x 24: 3 row slots, 12 steps) stays on the row-local tier: an instantiation with 4 x 4 slots and 16
  // steps (r04, dropped) held 496 VGPRs and 42 KB of LDS -- three problems per CU at half the row-local kernel's rate
  // (profiles/r04_tier_choice.txt).
  if (NS <= 1 && NV <= 1 && mid <= 4) { wh.BS = 8; wh.NS = 1; wh.NV = 1; wh.NSTEP = 4; }
  else if (NS <= 2 && NV <= 2 && mid <= 8) { wh.BS = 8; wh.NS = 2; wh.NV = 2; wh.NSTEP = 8; }
  else if (NS <= 2 && NV <= 2 && mid <= 10) { wh.BS = 8; wh.NS = 2; wh.NV = 2; wh.NSTEP = 10; }
  else if (bs == 7 && NS <= 4 && NV <= 3 && mid <= 10) { wh.BS = 7; wh.NS = 4; wh.NV = 3; wh.NSTEP = 10; }
  else { wh.why = WV_WHY_SHAPE; return false; }
  wh.bs = bs; wh.nb = nb; wh.mid = mid; wh.lpb = lpb; wh.n_extra = n_extra;
  const int NSTEP = wh.NSTEP, lenB = nb - 1 - mid, npos = 2 * NSTEP + 2, dummy = npos - 1;
  auto pos_of = [&](int t) { return t < mid ? NSTEP - mid + t : t == mid ? NSTEP : 2 * NSTEP + 1 - lenB + (nb - 1 - t); };
  auto apos = [&](int row, int var) {            // position of A(row, var) in the CSC value array
    for (int s = pl.Rp[row]; s < pl.Rp[row + 1]; s++) if (pl.Rj[s] == var) return pl.Rpos[s];
    return -1;
  };
  auto ppos = [&](int va, int vb) {              // position of P(va, vb) in the upper-triangular CSC array
    const int r = std::min(va, vb), c = std::max(va, vb);
    for (int t = pl.Pp[c]; t < pl.Pp[c + 1]; t++) if (pl.Pi[t] == r) return t;
    return -1;
  };
  const WvTab T = wv_tab_layout(wh.NS, wh.NV, wh.NL);
  wh.tab.assign((size_t)T.total * 64, -1);
  auto at = [&](int off, int lane) -> int & { return wh.tab[(size_t)off * 64 + lane]; };
  for (int l = 0; l < 64; l++) {
    at(T.pos, l) = dummy;                                           // idle lanes sit on the all-zero dummy block
    for (int v = 0; v < wh.NV; v++) { at(T.vpk + v, l) = wv_vidx(npos, dummy, v & 7); at(T.vpkm + v, l) = wv_vidx(npos, dummy, 0); at(T.vpkp + v, l) = wv_vidx(npos, dummy, 0); }
    at(T.xpk, l) = wv_vidx(npos, dummy, 0);
  }
  int xl = 0;
  for (int t = 0; t < nb; t++) {
    const int base = 16 * (t / bpr) + lpb * (t % bpr), p = pos_of(t);
    for (int sub = 0; sub < lpb; sub++) at(T.pos, base + sub) = p;
    for (int r = 0; r < (int)hin[t].size(); r++) {
      const int e = hin[t][r], l = base + r % lpb, q = r / lpb, ve = pl.elim_var[e];
      at(T.hrow + q, l) = h_of[e]; at(T.hbrow + q, l) = b_of[e]; at(T.hevar + q, l) = ve; at(T.heidx + q, l) = e;
      at(T.hepos + q, l) = apos(h_of[e], ve); at(T.hbpos + q, l) = apos(b_of[e], ve);
      for (int k = 0; k < bs; k++) at(T.hjpos + q * 8 + k, l) = apos(h_of[e], pl.core_var[t * bs + k]);
    }
    for (int k = 0; k < bs; k++) {
      const int l = base + k % lpb, v = k / lpb, c = t * bs + k, var = pl.core_var[c];
      at(T.vvar + v, l) = var; at(T.vpk + v, l) = wv_vidx(npos, p, k);
      at(T.vpkm + v, l) = t > 0 ? wv_vidx(npos, pos_of(t - 1), k) : wv_vidx(npos, dummy, 0);
      at(T.vpkp + v, l) = t + 1 < nb ? wv_vidx(npos, pos_of(t + 1), k) : wv_vidx(npos, dummy, 0);
      // the variable's own slot takes its LAST single row: the reference appends the bound / trust-region rows behind all
      // constraint rows (osqp_utils.py:185-189), so that is the box row, which sits on the base rho; an earlier one (a pin:
      // equality, rho_eq) goes to the general extra-row lanes
      if (!single[c].empty()) { at(T.vrow + v, l) = single[c].back(); at(T.vpos + v, l) = apos(single[c].back(), var); }
      for (int k2 = 0; k2 < bs; k2++) at(T.vpd + v * 8 + k2, l) = ppos(var, pl.core_var[t * bs + k2]);
      at(T.vpm + v, l) = t > 0 ? ppos(var, pl.core_var[(t - 1) * bs + k]) : -1;
      at(T.vpp + v, l) = t + 1 < nb ? ppos(var, pl.core_var[(t + 1) * bs + k]) : -1;
      if (xrow[c] >= 0) { at(T.xrow, xl) = xrow[c]; at(T.xpos, xl) = apos(xrow[c], var); at(T.xpk, xl) = wv_vidx(npos, p, k); xl++; }
      const int nlk = (int)link[c].size();
      for (int s = 0; s < nlk; s++) {                               // (link[c] is empty in the last block: c + bs does not exist)
        const int i = v * wh.NL + s, row = link[c][s];
        at(T.lrow + i, l) = row; at(T.lplo + i, l) = apos(row, var); at(T.lphi + i, l) = apos(row, pl.core_var[c + bs]);
      }
      // stacked rows behind them: no partner entry (lphi stays -1, the kernel takes it as coefficient 0), also in the last
      // block, where the partner's place is the dummy block
      for (int s = 0; s < (int)stack[c].size(); s++) {
        const int i = v * wh.NL + nlk + s, row = stack[c][s];
        at(T.lrow + i, l) = row; at(T.lplo + i, l) = apos(row, var); at(T.lphi + i, l) = -1;
      }
    }
  }
  // LDS of the ADMM kernel (doubles): G, ef, en, em | r, x~, x, extra | Jacobian rows (unless they live in registers) | partials
  const bool jreg = wv_jreg(wh.NS, wh.BS);
  wh.g_doubles = (size_t)npos * 64 + 2 * (size_t)npos * 8 + 8;
  // (+ the constants of the termination test, lane-minor: 3 NS + 5 NV + 1 slots of 64 doubles)
  wh.lds_doubles = wh.g_doubles + 4 * (size_t)npos * 8 + (jreg ? 0 : (size_t)wh.NS * 512) + (size_t)npos * lpb * 8 + (size_t)wv_ck_slots(wh.NS, wh.NV) * 64;
  wh.cst_slots = wv_cst_slots(wh.NS, wh.NV, 0);
  if (wh.NL) {
    // link rows: one more block vector (the partner's share of the right-hand side); where the instantiation keeps the
    // slots' four constants in lane-private LDS, they take the place of the constants of the termination test
    const int nl = wh.NV * wh.NL;
    wh.lds_doubles += (size_t)npos * 8;
    if (!wv_link_regs(wh.BS)) wh.lds_doubles = wh.lds_doubles - (size_t)wv_ck_slots(wh.NS, wh.NV) * 64 + (size_t)nl * 4 * 64;
    wh.cst_slots = wv_cst_slots(wh.NS, wh.NV, nl);
  }
  wh.lds_bytes = wh.lds_doubles * sizeof(double);
  // the tier pays only with FOUR problems per CU (one wavefront per SIMD): 40 KB each at most
  wh.per_cu = SCO_WV_PER_CU;
  const bool fits = wh.lds_bytes <= 40 * 1024;
  wh.why = fits ? WV_OK : WV_WHY_LDS;
  wv_plan_widths(wh, nullptr, false);       // no hint: every slot at the full width, the generic kernel
  return fits;
}

// Jacobian widths of the hinge slots from the caller's hint, and the compiled profile that covers them (layout_wv.h).
// Nothing else of the plan changes: the rows stay on their lanes and slots, so a block's partial column sums add in the
// order they did.
void wv_plan_widths(WvHost &wh, const int *row_width, bool off) {
  const WvTab T = wv_tab_layout(wh.NS, wh.NV, wh.NL);
  wh.jw_profile = 0;
  for (int q = 0; q < WV_MAXNS; q++) wh.jw[q] = 0;
  if (wh.tab.size() < (size_t)T.total * 64) return;                 // (a refused pattern: no tables)
  for (int q = 0; q < wh.NS && q < WV_MAXNS; q++)
    for (int l = 0; l < 64; l++) {
      const int h = wh.tab[(size_t)(T.hrow + q) * 64 + l];
      if (h < 0) continue;
      const int w = row_width ? row_width[h] : 0;
      // (no promise, w <= 0, and a width of the whole block or beyond it both mean every column: bs)
      wh.jw[q] = std::max(wh.jw[q], (w > 0 && w < wh.bs) ? w : wh.bs);
    }
  if (off || !row_width) return;
  // profiles exist for <7,4,3,10,3> without link rows (wv_launch); of those that cover the widths, the one with the fewest
  // columns; none: the generic kernel
  if (!(wh.BS == 7 && wh.NS == 4 && wh.NSTEP == 10 && wh.lpb == 3 && !wh.NL) || !wv_jreg(wh.NS, wh.BS)) return;
  int best = 0, best_cols = 4 * wh.BS;
#define X(a, b, c, d) \
  if (wh.jw[0] <= (a) && wh.jw[1] <= (b) && wh.jw[2] <= (c) && wh.jw[3] <= (d) && (a) + (b) + (c) + (d) < best_cols) { \
    best = WV_JW_PACK(a, b, c, d); best_cols = (a) + (b) + (c) + (d); \
  }
  WV_JW_PROFILES(X)
#undef X
  wh.jw_profile = best;
}
