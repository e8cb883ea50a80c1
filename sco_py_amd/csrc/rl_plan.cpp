// rl_plan.cpp -- host plan of the row-local tier (kernel: sco_admm_rl.hip): thread assignment, per-thread programs,
// paired sliced-ELL images, LDS request.  Plain C++, no HIP call; the role rows and slot widths both sides agree on are
// layout_rl.h.  The opt-in assignments come in through QpCreateEnv (qp_tier.h): nothing here reads the environment.
#include "qp_tier_plans.h"
#include "layout_rl.h"

#include <algorithm>
#include <cstdio>
#include <map>

// Paired sliced-ELL: slices of 64 items (one wavefront); entries 2h and 2h+1 of lane l
// sit next to each other at base[s] + (64 h + l) * 2, so one ds_read_b128 per lane
// (contiguous 1 KiB per wave instruction, conflict-free) fetches two values.
static void build_sell2(int nitems, const std::vector<int> &ptr, const std::vector<int> &src, SellHost &out) {
  out.nitems = nitems;
  const int ns = (nitems + 63) / 64;
  out.base.assign(ns + 1, 0); out.width.assign(std::max(ns, 1), 0);
  for (int s = 0; s < ns; s++) {
    int w = 0;
    for (int it = s * 64; it < std::min(nitems, s * 64 + 64); it++) w = std::max(w, ptr[it + 1] - ptr[it]);
    w = (w + 1) & ~1;
    out.width[s] = w; out.base[s + 1] = out.base[s] + 64 * w;
  }
  out.total = out.base[ns];
  out.idx.clear(); out.src.assign(std::max(out.total, 1), -1);
  for (int it = 0; it < nitems; it++) {
    const int s = it / 64, l = it % 64;
    for (int k = 0; k < ptr[it + 1] - ptr[it]; k++)
      out.src[out.base[s] + (64 * (k / 2) + l) * 2 + (k & 1)] = src[ptr[it] + k];
  }
}

// --------------------------------------------------------------------------
// host: thread assignment and per-thread programs
// --------------------------------------------------------------------------
// Thread assignment in which every core column sits in the SAME wavefront as all of its rows ("closed"): the
// connected components of the row / core-column graph (rows of one eliminated variable tied together) are packed
// whole into wavefronts.  Then the column sums A_C' t' of phase (1) only read t' values written by their own
// wavefront, phase (1) follows phase (Y) without a workgroup barrier, and all eight wavefronts share the column
// work (in a trajectory QP a component is a timestep).  False if a component needs more than 64 threads or the
// components do not pack: the caller keeps the barrier then.
// cols_cap > 0 (aligned form): a wavefront also owns the W rows of its core columns, at most cols_cap of them; the core
// columns of wavefront w, in tile-row order, come back in wave_cols[w].
static bool rl_assign_closed(const QpPlan &pl, const std::vector<int> &row_elim, const std::vector<std::vector<int>> &erows,
                             std::vector<int> &slot_row, std::vector<int> &thr_core, std::vector<int> &thr_elim, const bool debug_print,
                             const int cols_cap = 0, std::vector<std::vector<int>> *wave_cols = nullptr) {
  const int m = pl.m, nc = pl.n_c, ne = pl.n_e;
  std::vector<int> uf(m + nc + ne);
  for (size_t i = 0; i < uf.size(); i++) uf[i] = (int)i;
  auto find = [&](int a) { while (uf[a] != a) { uf[a] = uf[uf[a]]; a = uf[a]; } return a; };
  auto unite = [&](int a, int b) { a = find(a); b = find(b); if (a != b) uf[a] = b; };
  for (int i = 0; i < m; i++)
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int c = pl.core_of[pl.Rj[s]];
      if (c >= 0) unite(i, m + c);
    }
  for (int e = 0; e < ne; e++) for (int i : erows[e]) unite(m + nc + e, i);
  struct Comp { std::vector<int> cols, elims, free_rows; int need = 0; };
  std::vector<Comp> comps;
  std::vector<int> comp_of(uf.size(), -1);
  auto comp = [&](int node) -> Comp & {
    const int r = find(node);
    if (comp_of[r] < 0) { comp_of[r] = (int)comps.size(); comps.emplace_back(); }
    return comps[comp_of[r]];
  };
  for (int c = 0; c < nc; c++) comp(m + c).cols.push_back(c);
  for (int e = 0; e < ne; e++) comp(m + nc + e).elims.push_back(e);
  for (int i = 0; i < m; i++) if (row_elim[i] < 0) comp(i).free_rows.push_back(i);
  for (Comp &k : comps) {
    int spare = 0;
    for (int e : k.elims) spare += 2 - (int)erows[e].size();
    const int extra = std::max(0, (int)k.free_rows.size() - spare);
    k.need = std::max((int)k.elims.size() + (extra + 1) / 2, (int)k.cols.size());
    if (debug_print) fprintf(stderr, "comp: cols %zu elims %zu free %zu need %d\n", k.cols.size(), k.elims.size(), k.free_rows.size(), k.need);
    if (k.need > 64) return false;
    if (k.need == 0) k.need = 1;
  }
  std::vector<int> order(comps.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return comps[a].need > comps[b].need; });
  int load[LWV] = {0}, ncols[LWV] = {0};
  std::vector<std::vector<int>> bin(LWV);
  for (int k : order) {
    int best = -1;
    for (int w = 0; w < LWV; w++)
      if (load[w] + comps[k].need <= 64 && (cols_cap <= 0 || ncols[w] + (int)comps[k].cols.size() <= cols_cap) &&
          (best < 0 || load[w] < load[best])) best = w;
    if (best < 0) return false;
    load[best] += comps[k].need; ncols[best] += (int)comps[k].cols.size(); bin[best].push_back(k);
  }
  if (wave_cols) {
    wave_cols->assign(LWV, std::vector<int>());
    for (int w = 0; w < LWV; w++)
      for (int k : bin[w]) for (int c : comps[k].cols) (*wave_cols)[w].push_back(c);
  }
  slot_row.assign(2 * LT, -1); thr_core.assign(LT, -1); thr_elim.assign(LT, -1);
  for (int w = 0; w < LWV; w++) {
    int base = 64 * w;
    for (int k : bin[w]) {
      const Comp &K = comps[k];
      int t = base;
      for (int e : K.elims) {
        thr_elim[t] = e;
        for (size_t q = 0; q < erows[e].size(); q++) slot_row[q * LT + t] = erows[e][q];
        t++;
      }
      for (size_t j = 0; j < K.cols.size(); j++) thr_core[base + (int)j] = K.cols[j];
      // rows without an eliminated variable: the threads behind the eliminated ones first (slot 0, then 1), then
      // the slots the eliminated variables left empty
      std::vector<int> slots;
      for (int q = 0; q < 2; q++) for (int u = t; u < base + K.need; u++) slots.push_back(q * LT + u);
      for (int q = 0; q < 2; q++) for (int u = base; u < t; u++) if (slot_row[q * LT + u] < 0) slots.push_back(q * LT + u);
      if (slots.size() < K.free_rows.size()) return false;
      for (size_t j = 0; j < K.free_rows.size(); j++) slot_row[slots[j]] = K.free_rows[j];
      base += K.need;
    }
  }
  return true;
}

static bool rl_plan_build_ns(const QpPlan &pl, RlHost &rh, const QpCreateEnv &env, const int ns_min, const bool allow_aligned = false) {
  if (pl.n_c + 4 > LCAP_NC || pl.m >= LNS_MAX * LT || pl.n_e > LT || pl.n_c > LT || pl.nnzA >= 65536 || pl.n > 2 * LT) return false;
  const int m = pl.m;
  // rows of every eliminated variable; every row's eliminated variable
  std::vector<int> row_elim(m, -1), row_epos(m, -1);
  std::vector<std::vector<int>> erows(pl.n_e);
  for (int i = 0; i < m; i++)
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int e = pl.elim_of[pl.Rj[s]];
      if (e >= 0) {
        if (row_elim[i] >= 0) return false;          // two eliminated variables in one row
        row_elim[i] = e; row_epos[i] = pl.Rpos[s]; erows[e].push_back(i);
      }
    }
  for (int e = 0; e < pl.n_e; e++) if (erows[e].size() > 2) return false;
  // ---- thread assignment: slot (q, t) -> row, thread -> core / eliminated variable
  std::vector<int> slot_row, thr_core, thr_elim;
  // The closed assignment is measured slower on the trajectory QPs (every wavefront then runs the widest row AND
  // column code, 957 against 871 ms per bench step), so it is opt-in: SCO_QP_RL_CLOSED=1.
  rh.NS = 2;
  // The ALIGNED closed assignment (r03; opt-in with SCO_QP_RL_ALIGNED=1, measured slower, see below): the wavefront
  // that holds a connected component's rows and columns also holds the W rows of those columns, so the mat-vec totals a
  // row needs are produced by its own wavefront: (3) -> (Y) -> (1) run without a workgroup barrier, ONE barrier per
  // iteration is left (before (3): the whole right-hand side), and the two wavefronts of a SIMD drift apart: the
  // latency-bound phases of one overlap the multiply-adds of the other.  For cores of 129 .. 144 variables (the tile
  // of that layout is 3 x 18 with 8 column groups); a pattern whose components do not pack keeps the open assignment.
  // Measured (profiles/r03_ab.txt): 1.057 against 0.932 us per iteration.  Every wavefront then runs every kind of work
  // at a third of its lanes (21 columns, ~45 row threads per wavefront): 176 instead of ~140 VALU and 39 instead of ~20
  // LDS instructions per wavefront and iteration, and an iteration costs what its instructions cost, not what its
  // barriers cost.
  const bool want_closed = env.rl_closed;     // SCO_QP_RL_ALIGNED or SCO_QP_RL_CLOSED (r02) = the aligned form now
  std::vector<std::vector<int>> wave_cols;
  rh.aligned = allow_aligned && ns_min == 2 && want_closed && pl.n_c > 128 && pl.n_c <= 8 * AL_TC &&
               rl_assign_closed(pl, row_elim, erows, slot_row, thr_core, thr_elim, env.debug_plan, AL_ROWS, &wave_cols);
  // The 8-column-group W layout with the OPEN assignment (r03): the W phase costs 3 swap folds + one quad step per
  // wavefront instead of 5 + 4 (a lane-swap instruction costs ~12 cycles, a multiply-add 4.5: scripts/microbench/inst_cost.hip),
  // six wavefronts carry W rows instead of eight.  Measured neutral without and slower with the termination test
  // (0.929 / 1.048 against 0.932 / 1.009 us per iteration, profiles/r03_ab.txt): 54 instead of 45 multiply-adds and 9
  // instead of 5 reads of the right-hand side eat what the reduction saves.  Opt-in: SCO_QP_RL_LAY8=1.
  rh.lay8 = !rh.aligned && ns_min == 2 && env.rl_lay8 && pl.n_c > 128 && pl.n_c <= 8 * AL_TC;
  rh.merged = rh.aligned;
  // every open plan puts a core column on a lane pair (2 n_c <= 312 lanes: n_c <= LCAP_NC - 4); SCO_QP_RL_SPLIT=0 keeps
  // all of a column's pairs on the owner and leaves the helper lane empty (the r02 distribution of the work)
  const bool split_pairs = !env.rl_split_off;
  rh.split = !rh.merged;
  if (!rh.merged) {
    // two row slots per thread; a pattern with more rows than that (velocity + joint limits at 7-DOF x 20: 1100) takes
    // the three-slot instantiation.  The rows of an eliminated variable (<= 2) always sit in slots 0 and 1 of its thread.
    for (int ns = ns_min; ns <= LNS_MAX; ns++) {
      rh.NS = ns;
      slot_row.assign((size_t)ns * LT, -1); thr_core.assign(LT, -1); thr_elim.assign(LT, -1);
      for (int e = 0; e < pl.n_e; e++) {               // eliminated variable e -> thread e
        thr_elim[e] = e;
        for (size_t q = 0; q < erows[e].size(); q++) slot_row[q * LT + e] = erows[e][q];
      }
      // far from the eliminated-variable threads.  Split form (r03): the entries of a core column go to TWO neighbouring
      // lanes (owner = even lane, helper = odd lane: half of the operand pairs each), their partial sums meet in one
      // quad_perm step -- phase (1) reads half as many operands per lane and runs on twice as many wavefronts
      for (int c = 0; c < pl.n_c; c++) thr_core[rh.split ? LT - 2 - 2 * c : LT - 1 - c] = c;
      int cur = 0;
      std::vector<int> order;                        // free slots: threads without an eliminated variable first
      for (int q = 0; q < ns; q++) for (int t = pl.n_e; t < LT; t++) order.push_back(q * LT + t);
      for (int q = 0; q < ns; q++) for (int t = 0; t < pl.n_e; t++) order.push_back(q * LT + t);
      bool ok = true;
      for (int i = 0; i < m && ok; i++) {
        if (row_elim[i] >= 0) continue;
        while (cur < (int)order.size() && slot_row[order[cur]] >= 0) cur++;
        if (cur >= (int)order.size()) ok = false;
        else slot_row[order[cur]] = i;
      }
      if (ok) break;
      if (ns == LNS_MAX) return false;
    }
  }
  if (rh.NS != 2) rh.lay8 = false;
  // ---- LDS positions of the row vectors (t', and w y / dy of the termination test).  A gather-dot reads its
  // operands two at a time (one ds_read_b128 per aligned PAIR of positions), so rows that one column reads together
  // should sit next to each other: rows with several core entries grouped by their set of columns (the rows of one
  // constraint block; a velocity limit and its negated copy), then the rows with a single core entry grouped by that column
  // (trust-region row, pin, joint limit of the same variable), every group on an even position.  Rows without a
  // core entry are never gathered and get no position.
  std::vector<int> pos(m, -1);
  int npos = 0;
  {
    std::vector<int> ncore(m, 0), onecol(m, -1);
    for (int i = 0; i < m; i++)
      for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
        const int c = pl.core_of[pl.Rj[s]];
        if (c >= 0) { ncore[i]++; onecol[i] = c; }
      }
    {
      // rows with several core entries: rows with the SAME set of core columns next to each other (the rows of a
      // constraint block already are; a velocity limit and its negated copy are d (T - 1) rows apart), groups in order
      // of first appearance, every group on an even position
      std::map<std::vector<int>, int> group_of;
      std::vector<std::vector<int>> groups;
      for (int i = 0; i < m; i++) {
        if (ncore[i] < 2) continue;
        std::vector<int> sig;
        for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) { const int c = pl.core_of[pl.Rj[s]]; if (c >= 0) sig.push_back(c); }
        std::sort(sig.begin(), sig.end());
        auto it = group_of.find(sig);
        if (it == group_of.end()) { group_of[sig] = (int)groups.size(); groups.emplace_back(1, i); }
        else groups[it->second].push_back(i);
      }
      for (const auto &g : groups) {
        npos = (npos + 1) & ~1;
        for (int i : g) pos[i] = npos++;
      }
    }
    std::vector<std::vector<int>> singles(pl.n_c);
    for (int i = 0; i < m; i++) if (ncore[i] == 1) singles[onecol[i]].push_back(i);
    for (int c = 0; c < pl.n_c; c++) {
      if (singles[c].empty()) continue;
      npos = (npos + 1) & ~1;
      for (int i : singles[c]) pos[i] = npos++;
    }
    npos = (npos + 1) & ~1;                            // the always-zero pair sits at npos, npos + 1
    rh.zpos = npos;
    npos += 2;
    for (int i = 0; i < m; i++) if (ncore[i] == 0) pos[i] = npos++;    // written, never gathered (no predicate in the loop)
    if (npos > LCAP_M - 1) return false;                 // position LCAP_M - 1 takes the stores of empty row slots
  }
  const int zcore = (pl.n_c + 1) & ~1;                 // always-zero pair of the core vectors
  if (zcore + 2 > LCAP_NC) return false;
  // pair lists: item -> [(pair index, source of the even element, source of the odd element)], -1 = structural zero
  struct Pair { int p, s0, s1; };
  auto make_pairs = [](std::vector<std::pair<int, int>> ent) {       // (position, source) -> pairs by position / 2
    std::sort(ent.begin(), ent.end());
    std::vector<Pair> out;
    for (auto &e : ent) {
      if (out.empty() || out.back().p != e.first / 2) out.push_back({e.first / 2, -1, -1});
      ((e.first & 1) ? out.back().s1 : out.back().s0) = e.second;
    }
    return out;
  };
  const int NSv = rh.NS;
  std::vector<std::vector<Pair>> colp(LT), rowp[LNS_MAX];
  for (int q = 0; q < NSv; q++) rowp[q].resize(LT);
  size_t maxc = 0, maxr = 0;
  for (int t = 0; t < LT; t++) {
    const int c = thr_core[t];
    if (c >= 0) {
      const int j = pl.core_var[c];
      std::vector<std::pair<int, int>> ent;
      for (int p = pl.Ap[j]; p < pl.Ap[j + 1]; p++) ent.push_back({pos[pl.Ai[p]], p});
      colp[t] = make_pairs(ent);
      if (rh.split && split_pairs) {                     // the second half of the pairs: the helper lane t + 1
        const size_t keep = (colp[t].size() + 1) / 2;
        colp[t + 1].assign(colp[t].begin() + keep, colp[t].end());
        colp[t].resize(keep);
      }
      maxc = std::max(maxc, colp[t].size());
    }
    for (int q = 0; q < NSv; q++) {
      const int i = slot_row[q * LT + t];
      if (i < 0) continue;
      std::vector<std::pair<int, int>> ent;
      for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
        const int c2 = pl.core_of[pl.Rj[s]];
        if (c2 >= 0) ent.push_back({c2, pl.Rpos[s]});
      }
      rowp[q][t] = make_pairs(ent);
      if (rowp[q][t].size() > LRW_MAX / 2) return false;
      maxr = std::max(maxr, rowp[q][t].size());
    }
  }
  if (maxc > (NSv > 2 ? LCW_MAX3 : LCW_MAX) / 2) return false;
  if (maxc > LCW / 2 || maxr > LRW / 2) rh.CW = LCW_MAX;      // the wide instantiation: 8 pairs per column, 5 per row
  // three row slots: 10 pairs per column thread, 5 per row -- unless the split plan leaves every column thread <= 6 pairs and
  // every row <= 4 (velocity + joint limits at 7-DOF x 20: 5 + 5 pairs): then the narrow offsets do, with far fewer registers
  if (NSv > 2) rh.CW = (maxc <= LCW / 2 && maxr <= LRW / 2) ? LCW : LCW_MAX3;
  // ---- sliced-ELL images in thread order: two value slots per pair
  // Open assignment: item = thread.  Closed assignments spread every kind of work over all wavefronts (a wavefront holds
  // ~21 of the 140 columns), so an image with one item per THREAD would be 8 full slices per operator and overflow LDS:
  // there the items are the threads that have entries, in thread order (`ipos[t]`: image position of thread t's first
  // value, -1 = none: such a thread reads the zero block behind the images), and a wavefront's trip count is the
  // widest of its own threads (`iwid`).  Its active lanes still read consecutive 16-byte pieces: conflict-free.
  const bool compact = rh.merged;
  auto image = [&](const std::vector<std::vector<Pair>> &items, SellHost &out, std::vector<int> &ipos, std::vector<int> &iwid) {
    std::vector<int> ptr(1, 0), src, item_of(LT, -1);
    int nit = 0;
    for (int t = 0; t < LT; t++) {
      if (compact && items[t].empty()) continue;
      for (const Pair &pr : items[t]) { src.push_back(pr.s0); src.push_back(pr.s1); }
      ptr.push_back((int)src.size());
      item_of[t] = nit++;
    }
    if (nit == 0) { ptr.push_back(0); nit = 1; }
    build_sell2(nit, ptr, src, out);
    ipos.assign(LT, -1); iwid.assign(LT, 0);
    for (int t = 0; t < LT; t++) {
      if (item_of[t] >= 0) ipos[t] = out.base[item_of[t] / 64] + 2 * (item_of[t] % 64);
      if (!compact) iwid[t] = out.width[t / 64];
    }
    if (compact)
      for (int w = 0; w < LWV; w++) {
        int mx = 0;
        for (int t = 64 * w; t < 64 * w + 64; t++) mx = std::max(mx, 2 * (int)items[t].size());
        for (int t = 64 * w; t < 64 * w + 64; t++) iwid[t] = mx;
      }
  };
  std::vector<int> cpos, cwid, rpos[LNS_MAX], rwid[LNS_MAX];
  image(colp, rh.Ac, cpos, cwid);
  size_t rtot = 0;
  for (int q = 0; q < NSv; q++) { image(rowp[q], rh.Ar[q], rpos[q], rwid[q]); rtot += rh.Ar[q].total; }
  const int zblock = rh.Ac.total + (int)rtot;          // 64 x 16 zeros behind the images (kernel prologue)
  rh.lds_bytes = 8 * ((size_t)rh.Ac.total + rtot + 64 * 16 + (2 * NSv + 5) * LT) + 12 * 4 * LCAP_NC;   // + check constants
  // ---- per-thread tables: packed pair offsets (bytes) and roles
  const int CPv = rh.CW / 2;
  const int RPv = (rh.CW > LCW ? LRW_MAX : LRW) / 2;          // pairs per row slot
  const int slots = CPv + NSv * RPv + 1;                         // + 1: the last register of a slot is packed from two table rows
  rh.off.assign((size_t)slots * LT, 0);
  rh.role.assign((size_t)RL_ROLES * LT, -1);
  for (int t = 0; t < LT; t++) {
    for (int k = 0; k < CPv; k++) rh.off[(size_t)k * LT + t] = (unsigned short)(8 * rh.zpos);               // zero pair of t'
    for (int k = 0; k < NSv * RPv + 1; k++) rh.off[(size_t)(CPv + k) * LT + t] = (unsigned short)(8 * zcore);   // zero pair of x_C
    // role table: 0 core idx, 1 core var, 2 elim idx, 3 elim var, 4/5 row of slot 0/1,
    //             6/7 CSC position of the row's eliminated coefficient, 8 col base, 9/10 row bases,
    //             11/12 position of P_jj for the core / eliminated variable, 13-15 trip counts,
    //             16/17 LDS position of the row of slot 0/1
    rh.role[(size_t)8 * LT + t] = cpos[t] >= 0 ? cpos[t] : zblock + 2 * (t % 64);
    for (int q = 0, acc = rh.Ac.total; q < NSv; acc += rh.Ar[q].total, q++) {
      rh.role[(size_t)ROLE_RBASE(q) * LT + t] = rpos[q][t] >= 0 ? acc + rpos[q][t] : zblock + 2 * (t % 64);
      rh.role[(size_t)ROLE_RWID(q) * LT + t] = rwid[q][t];
    }
    rh.role[(size_t)13 * LT + t] = cwid[t];                  // wave-uniform trip counts (value slots = 2 x pairs)
    const int c = thr_core[t];
    if (c >= 0) {
      const int j = pl.core_var[c];
      rh.role[t] = c; rh.role[(size_t)LT + t] = j; rh.role[(size_t)11 * LT + t] = pl.Pdiag[j];
    }
    for (size_t k = 0; k < colp[t].size(); k++) rh.off[k * LT + t] = (unsigned short)(16 * colp[t][k].p);   // owner or helper
    const int e = thr_elim[t];
    if (e >= 0) {
      rh.role[(size_t)2 * LT + t] = e; rh.role[(size_t)3 * LT + t] = pl.elim_var[e];
      rh.role[(size_t)12 * LT + t] = pl.Pdiag[pl.elim_var[e]];
    }
    if (rh.aligned || rh.lay8) {
      const int wv = t / 64, lane = t % 64, g = (lane >> 1) & 7, h = (lane >> 4) & 3;
      for (int rr = 0; rr < AL_TR; rr++) {
        const int lr = g * AL_TR + rr;
        // open assignment: wavefront w carries the W rows 24 w .. 24 w + 23 (six wavefronts at 140 core variables)
        rh.role[(size_t)ROLE_WROW(rr) * LT + t] = rh.aligned ? (lr < (int)wave_cols[wv].size() ? wave_cols[wv][lr] : -1)
                                                             : (wv * AL_ROWS + lr < pl.n_c ? wv * AL_ROWS + lr : -1);
      }
      // after the folds (rl_reduce_al) the total of tile row 0 / 1 / 2 sits in the lanes with (bit 5, bit 4) = 00 / 10 / 01
      const int rr_out = h == 0 ? 0 : h == 2 ? 1 : h == 1 ? 2 : -1;
      if ((lane & 1) == 0 && rr_out >= 0) rh.role[(size_t)ROLE_XOUT * LT + t] = rh.role[(size_t)ROLE_WROW(rr_out) * LT + t];
    }
    for (int q = 0; q < NSv; q++) {
      const int i = slot_row[q * LT + t];
      rh.role[(size_t)ROLE_ROW(q) * LT + t] = i;
      if (i < 0) continue;
      rh.role[(size_t)ROLE_POS(q) * LT + t] = pos[i];
      if (row_elim[i] >= 0) {
        if (row_elim[i] != e) return false;
        if (q >= 2) return false;                    // an eliminated variable's rows live in slots 0 and 1
        rh.role[(size_t)ROLE_EPOS(q) * LT + t] = row_epos[i];
      }
      for (size_t k = 0; k < rowp[q][t].size(); k++)
        rh.off[(size_t)(CPv + q * RPv + k) * LT + t] = (unsigned short)(16 * rowp[q][t][k].p);
    }
  }
  // P restricted to the core (for the dual residual): core c -> (position in triu values, core index)
  rh.pc_ptr.assign(pl.n_c + 1, 0);
  for (int c = 0; c < pl.n_c; c++) {
    const int j = pl.core_var[c];
    for (int p = pl.Fp[j]; p < pl.Fp[j + 1]; p++) {
      const int c2 = pl.core_of[pl.Fi[p]];
      if (c2 < 0) return false;                    // an eliminated variable has no off-diagonal P entry
      rh.pc_pos.push_back(pl.Fpos[p]); rh.pc_core.push_back(c2);
    }
    rh.pc_ptr[c + 1] = (int)rh.pc_pos.size();
    rh.pcw = std::max(rh.pcw, rh.pc_ptr[c + 1] - rh.pc_ptr[c]);
  }
  rh.TR = std::max(1, (pl.n_c + LGI - 1) / LGI);
  rh.TC = 2 * rh.TR;
  if (rh.TR == 5 && pl.n_c <= LGJ * 9) rh.TC = 9;
  if (rh.NS != 2) rh.lay8 = false;
  if (rh.aligned || rh.lay8) { rh.TR = AL_TR; rh.TC = AL_TC; }
  // the wide variants and the three-slot ones exist for the 5-row tiles only: a plan rl_launch has no kernel for is refused
  if (!rl_has_kernel(rh.TR, rh.TC, rh.CW, rh.NS, rh.aligned ? 2 : rh.lay8 ? 1 : 0)) return false;
  return rh.lds_bytes + 40 * 1024 <= SCO_LDS_CAP;   // + 37.5 KB of static LDS
}

// Two row slots per thread where the pattern allows it; otherwise (more than 1024 rows, or more than 8 operand pairs in
// a column) the three-slot instantiation with ten pairs per column.
bool rl_plan_build(const QpPlan &pl, RlHost &rh, const QpCreateEnv &env) {
  {
    RlHost al;
    if (rl_plan_build_ns(pl, al, env, 2, true) && al.aligned) { rh = al; return true; }
  }
  {
    RlHost two;
    if (rl_plan_build_ns(pl, two, env, 2)) { rh = two; return true; }
  }
  RlHost three;
  if (!rl_plan_build_ns(pl, three, env, 3)) return false;
  rh = three;
  return true;
}

size_t rl_reported_static_lds() { return RL_REPORTED_STATIC_LDS; }
