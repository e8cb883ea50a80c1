// big_plan.cpp -- host plans of the global-memory tier (kernels: sco_qp_big.hip): the dense form's row and column lists
// (big_plan_build) and the structured form's blocks, row chunks and column contributions (bt_plan_build; the header of
// sco_qp_big.hip's second half describes that form).  Plain C++, no HIP call; layout_big.h holds what both sides agree on.
#include "qp_tier_plans.h"
#include "layout_big.h"

#include <algorithm>

// --------------------------------------------------------------------------
// host plan: dense form
// --------------------------------------------------------------------------
bool big_plan_build(const QpPlan &pl, BigHost &bh) {
  const int m = pl.m;
  bh.row_elim.assign(m, -1); bh.row_epos.assign(m, -1);
  std::vector<std::vector<int>> erows(pl.n_e);
  for (int i = 0; i < m; i++)
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int e = pl.elim_of[pl.Rj[s]];
      if (e >= 0) {
        if (bh.row_elim[i] >= 0) return false;
        bh.row_elim[i] = e; bh.row_epos[i] = pl.Rpos[s]; erows[e].push_back(i);
      }
    }
  bh.er_ptr.assign(pl.n_e + 1, 0);
  for (int e = 0; e < pl.n_e; e++) {
    if (erows[e].size() > 2) return false;
    for (int i : erows[e]) bh.er_row.push_back(i);
    bh.er_ptr[e + 1] = (int)bh.er_row.size();
  }
  for (int i = 0; i < m; i++) if (bh.row_elim[i] < 0) bh.free_rows.push_back(i);
  bh.pc_ptr.assign(pl.n_c + 1, 0);
  for (int c = 0; c < pl.n_c; c++) {
    const int j = pl.core_var[c];
    for (int p = pl.Fp[j]; p < pl.Fp[j + 1]; p++) {
      const int c2 = pl.core_of[pl.Fi[p]];
      if (c2 < 0) return false;
      bh.pc_pos.push_back(pl.Fpos[p]); bh.pc_core.push_back(c2);
    }
    bh.pc_ptr[c + 1] = (int)bh.pc_pos.size();
  }
  bh.ws_doubles = 3 * (size_t)m + pl.n_e + 2 * (size_t)pl.n_c + pl.n + (size_t)pl.n_c * pl.n_c;
  return true;
}

// --------------------------------------------------------------------------
// host plan: structured form.  no_mfma (SCO_QP_NO_MFMA): the block normal matrices stay off the matrix cores
// --------------------------------------------------------------------------
bool bt_plan_build(const QpPlan &pl, const BigHost &bh, BtHost &th, bool no_mfma) {
  int hb = 0;
  for (int id = 0; id < pl.nS; id++) hb = std::max(hb, pl.s_a[id] - pl.s_b[id]);
  if (hb > BT_MAXBS || pl.n_c <= 0) return false;
  th.bs = hb <= 4 ? 4 : hb <= 8 ? 8 : hb <= 12 ? 12 : 16;
  th.nb = (pl.n_c + th.bs - 1) / th.bs;
  const size_t ncp = (size_t)th.nb * th.bs;
  th.blk_doubles = 2 * ncp * th.bs;
  const int m = pl.m;
  // core entries of every row: (core index, CSC position)
  auto row_core = [&](int i, std::vector<int> &cols, std::vector<int> &pos) {
    cols.clear(); pos.clear();
    for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
      const int c = pl.core_of[pl.Rj[s]];
      if (c >= 0) { cols.push_back(c); pos.push_back(pl.Rpos[s]); }
    }
  };
  // one item = an eliminated variable with its (at most two) rows, or a row without one
  struct Item { int e, j, r0, r1, ep0, ep1; bool dense_ok, simple; std::vector<int> cols, pos; };
  std::vector<Item> items;
  std::vector<int> c0, p0, c1, p1;
  for (int e = 0; e < pl.n_e; e++) {
    Item it; it.e = e; it.j = pl.elim_var[e]; it.r0 = it.r1 = it.ep0 = it.ep1 = -1; it.dense_ok = false; it.simple = true;
    const int nr = bh.er_ptr[e + 1] - bh.er_ptr[e];
    if (nr == 0) { items.push_back(it); continue; }
    int ra = bh.er_row[bh.er_ptr[e]], rb = nr > 1 ? bh.er_row[bh.er_ptr[e] + 1] : -1;
    row_core(ra, c0, p0);
    c1.clear(); p1.clear();
    if (rb >= 0) { row_core(rb, c1, p1); if (c1.size() > c0.size()) { std::swap(ra, rb); std::swap(c0, c1); std::swap(p0, p1); } }
    it.r0 = ra; it.r1 = rb; it.ep0 = bh.row_epos[ra]; it.ep1 = rb >= 0 ? bh.row_epos[rb] : -1;
    // dense: the primary row carries every core entry, in consecutive core columns at a constant CSC stride
    it.dense_ok = c1.empty() && !c0.empty() && (int)c0.size() <= 16;
    for (size_t k = 1; it.dense_ok && k < c0.size(); k++)
      it.dense_ok = c0[k] == c0[0] + (int)k && p0[k] - p0[k - 1] == p0[1] - p0[0];
    it.cols = c0; it.pos = p0;
    it.simple = c1.empty() && c0.size() <= 1;
    items.push_back(it);
  }
  th.ch_desc.clear(); th.it.clear(); th.npart = 0;
  auto push_chunk = [&](int kind, const std::vector<Item> &its, size_t first, size_t cnt) {
    std::vector<int> dsc(CH_STRIDE, 0);
    const Item &f = its[first];
    dsc[0] = kind; dsc[1] = (int)cnt;
    if (kind == 0) {
      dsc[2] = (int)f.cols.size(); dsc[3] = f.r0; dsc[4] = f.cols[0]; dsc[5] = f.pos[0];
      dsc[6] = f.pos.size() > 1 ? f.pos[1] - f.pos[0] : 0;
      dsc[7] = f.e; dsc[8] = f.j; dsc[9] = f.r1; dsc[10] = f.ep0; dsc[12] = f.ep1;
      if (cnt > 1) { dsc[11] = its[first + 1].ep0 - f.ep0; dsc[13] = its[first + 1].ep1 - f.ep1; }
      dsc[14] = th.npart; th.npart += (int)f.cols.size();
    }
    th.ch_desc.insert(th.ch_desc.end(), dsc.begin(), dsc.end());
    for (size_t l = 0; l < 64; l++) {
      const bool on = l < cnt;
      const Item *t = on ? &its[first + l] : nullptr;
      const bool one = on && t->cols.size() == 1;
      const int rec[8] = {on ? t->e : -1, on ? t->j : -1, on ? t->r0 : -1, on ? t->r1 : -1, on ? t->ep0 : -1,
                          on ? t->ep1 : -1, one ? t->cols[0] : -1, one ? t->pos[0] : -1};
      th.it.insert(th.it.end(), rec, rec + 8);
    }
  };
  // dense runs: consecutive eliminated variables whose primary rows are consecutive rows with the
  // same core columns, and whose every index is an affine function of the position in the run
  std::vector<Item> generic;
  size_t i0 = 0;
  while (i0 < items.size()) {
    size_t i1 = i0 + 1;
    if (items[i0].dense_ok) {
      while (i1 < items.size() && items[i1].dense_ok) {
        const Item &p = items[i1 - 1], &c = items[i1], &f = items[i0], &g = items[i0 + 1];
        bool ok = c.r0 == p.r0 + 1 && c.j == p.j + 1 && c.cols == f.cols && (c.r1 < 0) == (f.r1 < 0) &&
                  (c.r1 < 0 || c.r1 == p.r1 + 1) && c.ep0 - p.ep0 == g.ep0 - f.ep0 && c.ep1 - p.ep1 == g.ep1 - f.ep1;
        for (size_t k = 0; ok && k < f.pos.size(); k++) ok = c.pos[k] == p.pos[k] + 1;
        if (!ok) break;
        i1++;
      }
    }
    if (items[i0].dense_ok && i1 - i0 >= 16) {
      for (size_t f = i0; f < i1; f += 64) push_chunk(0, items, f, std::min<size_t>(64, i1 - f));
    } else {
      for (size_t f = i0; f < i1; f++) generic.push_back(items[f]);
    }
    i0 = i1;
  }
  for (int i : bh.free_rows) {
    Item it; it.e = it.j = it.r1 = it.ep0 = it.ep1 = -1; it.r0 = i; it.dense_ok = false; it.simple = true;
    row_core(i, it.cols, it.pos);
    if (it.cols.size() > 1) it.simple = false;
    generic.push_back(it);
  }
  // kind 2: items whose rows hold at most one core entry (bound rows, pins) -- direct indices;
  // kind 1: everything else walks the CSR arrays
  std::vector<Item> simple, complex_;
  for (const Item &it : generic) (it.simple ? simple : complex_).push_back(it);
  for (size_t f = 0; f < simple.size(); f += 64) push_chunk(2, simple, f, std::min<size_t>(64, simple.size() - f));
  for (size_t f = 0; f < complex_.size(); f += 64) push_chunk(1, complex_, f, std::min<size_t>(64, complex_.size() - f));
  th.nchunks = (int)(th.ch_desc.size() / CH_STRIDE);
  // contributions to every core column of A' t: partial sums of the dense chunks + products of the other rows
  th.cent.assign(4 * ncp, -1);
  th.use_part = th.npart > 0;
  {
    std::vector<int> fill(ncp, 0);
    auto add = [&](int c, int v) { if (fill[c] < 4) th.cent[4 * c + fill[c]] = v; fill[c]++; };
    for (int ch = 0; ch < th.nchunks; ch++) {
      const int *dsc = &th.ch_desc[(size_t)ch * CH_STRIDE];
      if (dsc[0] == 0) {
        for (int k = 0; k < dsc[2]; k++) add(dsc[4] + k, dsc[14] + k);
      } else {
        for (int l = 0; l < dsc[1]; l++) {
          const int *rec = &th.it[((size_t)ch * 64 + l) * 8];
          for (int q = 2; q <= 3; q++) {
            const int i = rec[q];
            if (i < 0) continue;
            for (int s = pl.Rp[i]; s < pl.Rp[i + 1]; s++) {
              const int c = pl.core_of[pl.Rj[s]];
              if (c >= 0) add(c, -(pl.Rpos[s] + 2));
            }
          }
        }
      }
    }
    for (size_t c = 0; c < ncp; c++) if (fill[c] > 4) th.use_part = false;
  }
  if (!th.use_part) th.npart = 0;
  // factors; r/y, z/x~ (+ 64 zeros), x, q; partial sums; column metadata; chunk descriptors
  th.lds_bytes = 8 * (th.blk_doubles + 4 * ncp + 64 + th.npart) + 4 * (4 * ncp + th.ch_desc.size() + th.nchunks);
  if (th.lds_bytes + 1024 > SCO_LDS_CAP) return false;
  th.ws_doubles = 3 * (size_t)m + pl.n_e + pl.n + pl.nnzA + 64;
  // ---- N1: MFMA formation of the diagonal blocks' J' R J (blocks of order 12 .. 16, dense hinge rows)
  th.use_mfma = false;
  if (no_mfma) { th.mf_why = 1; return true; }
  th.mf_why = 2;
  if (th.bs >= 12 && th.bs <= 16) {
    const int bs = th.bs, nb = th.nb;
    // hinge rows of a block: one eliminated variable, core entries in that block only
    std::vector<int> row_blk(m, -1);
    for (int i = 0; i < m; i++) {
      int ne = 0, blk = -1; bool ok = true;
      for (int s2 = pl.Rp[i]; s2 < pl.Rp[i + 1]; s2++) {
        const int j = pl.Rj[s2];
        if (pl.elim_of[j] >= 0) ne++;
        else { const int t = pl.core_of[j] / bs; if (blk >= 0 && t != blk) ok = false; blk = t; }
      }
      if (ne == 1 && blk >= 0 && ok) row_blk[i] = blk;
    }
    th.mf_id.assign((size_t)nb * 256, -1); th.mf_h0.assign(pl.nS, 0); th.mf_h1.assign(pl.nS, 0);
    bool ok = true; int used = 0;
    std::vector<std::vector<int>> ref_rows(nb);
    for (int id = 0; id < pl.nS && ok; id++) {
      const int sa = pl.s_a[id], sb = pl.s_b[id], t = sa / bs;
      if (sb / bs != t) continue;
      int h0 = -1, h1 = -1;
      std::vector<int> rows;
      for (int q = pl.sa_ptr[id]; q < pl.sa_ptr[id + 1]; q++)
        if (row_blk[pl.sa_row[q]] == t) { if (h0 < 0) h0 = q; else if (q != h1) { ok = false; th.mf_why = 3; } h1 = q + 1; rows.push_back(pl.sa_row[q]); }
      if (h0 < 0) { h0 = h1 = pl.sa_ptr[id]; }
      // every entry of the block sums over the SAME hinge rows in the same order (dense Jacobian block): else no MFMA
      if (sa % bs == 0 && sb % bs == 0) ref_rows[t] = rows;
      th.mf_h0[id] = h0; th.mf_h1[id] = h1;
      th.mf_id[(size_t)t * 256 + (sa % bs) * 16 + (sb % bs)] = id;
    }
    for (int id = 0; id < pl.nS && ok; id++) {
      const int sa = pl.s_a[id], sb = pl.s_b[id], t = sa / bs;
      if (sb / bs != t) continue;
      if (th.mf_h1[id] - th.mf_h0[id] != (int)ref_rows[t].size()) { ok = false; th.mf_why = 4; break; }
      for (int q = th.mf_h0[id]; q < th.mf_h1[id]; q++) if (pl.sa_row[q] != ref_rows[t][q - th.mf_h0[id]]) { ok = false; th.mf_why = 4; break; }
      used += th.mf_h1[id] > th.mf_h0[id];
    }
    // (every lower-triangle position of every full block must be a structural entry: the diagonal always is)
    for (int t = 0; t < nb && ok; t++)
      for (int i = 0; i < bs && ok; i++)
        for (int j = 0; j <= i && ok; j++)
          if ((size_t)t * bs + i < (size_t)pl.n_c && th.mf_id[(size_t)t * 256 + i * 16 + j] < 0 && !ref_rows[t].empty()) { ok = false; th.mf_why = 5; }
    if (ok) th.mf_why = used > 0 ? 0 : 6;
    th.use_mfma = ok && used > 0;
    if (!th.use_mfma) { th.mf_id.clear(); th.mf_h0.clear(); th.mf_h1.clear(); }
  }
  return true;
}
