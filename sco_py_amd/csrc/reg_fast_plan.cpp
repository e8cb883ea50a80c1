// reg_fast_plan.cpp -- host plans of the two on-chip tiers that keep the four sparse operators of an iteration as
// sliced-ELL images in LDS: the sliced-ELL kernel (sco_admm_fast.hip, fast_plan_build) and the register-offset kernel
// (sco_admm_reg.hip, reg_caps_for + reg_plan_build).  Plain C++, no HIP call; layout_fast.h and layout_reg.h hold what
// planner and kernel agree on.
#include "qp_tier_plans.h"
#include "layout_fast.h"
#include "layout_reg.h"

#include <algorithm>

// --------------------------------------------------------------------------
// host: sliced-ELL construction
// --------------------------------------------------------------------------
static void build_sell(int nitems, const std::vector<int> &ptr, const std::vector<int> &idx,
                       const std::vector<int> &src, SellHost &out) {
  out.nitems = nitems;
  const int ns = (nitems + 63) / 64;
  out.base.assign(ns + 1, 0); out.width.assign(std::max(ns, 1), 0);
  for (int s = 0; s < ns; s++) {
    int w = 0;
    for (int it = s * 64; it < std::min(nitems, s * 64 + 64); it++) w = std::max(w, ptr[it + 1] - ptr[it]);
    out.width[s] = w; out.base[s + 1] = out.base[s] + 64 * w;
  }
  out.total = out.base[ns];
  out.idx.assign(std::max(out.total, 1), 0); out.src.assign(std::max(out.total, 1), -1);
  for (int it = 0; it < nitems; it++) {
    const int s = it / 64, l = it % 64;
    for (int k = 0; k < ptr[it + 1] - ptr[it]; k++) {
      const int p = out.base[s] + 64 * k + l;
      out.idx[p] = (unsigned short)idx[ptr[it] + k];
      out.src[p] = src[ptr[it] + k];
    }
  }
}

bool fast_plan_build(const QpPlan &pl, FastHost &fh) {
  if (pl.n > FT || pl.m > 3 * FT || pl.nnzA >= 65536 || pl.n_c > 32 * 5) return false;
  std::vector<int> ident(std::max(pl.nnzA, pl.ncpl) + 1);
  for (size_t i = 0; i < ident.size(); i++) ident[i] = (int)i;
  build_sell(pl.n, pl.Ap, pl.Ai, ident, fh.Ac);                       // A by column: idx = row, src = CSC position
  build_sell(pl.m, pl.Rp, pl.Rj, pl.Rpos, fh.Ar);                      // A by row:    idx = column
  {
    std::vector<int> eidx(pl.ncpl), srck(pl.ncpl);
    for (int t = 0; t < pl.ncpl; t++) { eidx[t] = pl.pair_elim[pl.a_pair[t]]; srck[t] = pl.a_pair[t]; }
    build_sell(pl.n_c, pl.a_ptr, eidx, srck, fh.Ca);                   // K_CE by core: idx = eliminated index
  }
  build_sell(pl.n_e, pl.e_ptr, pl.pair_core, ident, fh.Ce);            // K_CE by eliminated: idx = core index
  fh.TR = std::max(1, (pl.n_c + GI - 1) / GI);
  fh.TC = 2 * fh.TR;
  if (fh.TR == 5 && pl.n_c <= GJ * 9) fh.TC = 9;        // 140-order core: 5 x 9 tile
  auto maxw = [](const SellHost &h) { int w = 0; for (int x : h.width) w = std::max(w, x); return w; };
  fh.capped = maxw(fh.Ac) <= 12 && maxw(fh.Ar) <= 8 && maxw(fh.Ca) <= 12 && maxw(fh.Ce) <= 8;
  const int ps = GI * fh.TR + 1;
  const size_t scratch = std::max<size_t>((size_t)GJ * ps, 2 * (size_t)pl.n + 2 * (size_t)pl.m);
  fh.lds_doubles = (size_t)fh.Ac.total + fh.Ar.total + fh.Ca.total + fh.Ce.total +   // values
                   pl.n + pl.m + pl.n_e + (size_t)GJ * fh.TC + (size_t)GI * fh.TR +  // xt, t, ge, r, xc
                   scratch + FW * 8;
  fh.lds_bytes = fh.lds_doubles * 8 + 2 * ((size_t)fh.Ac.total + fh.Ar.total + fh.Ca.total + fh.Ce.total + 8 + 64 * 12);
  return fh.lds_bytes <= SCO_LDS_CAP;
}

size_t reg_static_lds() { return REG_STATIC_LDS; }

// --------------------------------------------------------------------------
// host: per-thread programs
// --------------------------------------------------------------------------
bool reg_plan_build(const QpPlan &pl, int CW, int RW, int PX, RegHost &rh) {
  // one spare element per gathered vector serves as the always-zero target of padded slots
  if (pl.n >= CAP_N || pl.m >= CAP_M || pl.n_c >= CAP_NC || pl.n_e >= CAP_N || pl.nnzA >= 65536) return false;
  rh.CW = CW; rh.RW = RW; rh.PX = PX;
  {
    std::vector<int> ident(std::max(pl.nnzA, pl.ncpl) + 1);
    for (size_t i = 0; i < ident.size(); i++) ident[i] = (int)i;
    build_sell(pl.n, pl.Ap, pl.Ai, ident, rh.Ac);
    build_sell(pl.m, pl.Rp, pl.Rj, pl.Rpos, rh.Ar);
    std::vector<int> eidx(pl.ncpl), srck(pl.ncpl);
    for (int t = 0; t < pl.ncpl; t++) { eidx[t] = pl.pair_elim[pl.a_pair[t]]; srck[t] = pl.a_pair[t]; }
    build_sell(pl.n_c, pl.a_ptr, eidx, srck, rh.Ca);
    build_sell(pl.n_e, pl.e_ptr, pl.pair_core, ident, rh.Ce);
    // room for the unrolled reads that run past the last slice
    rh.lds_bytes = 8 * ((size_t)rh.Ac.total + rh.Ar.total + rh.Ca.total + rh.Ce.total + 64 * 16);
    if (rh.lds_bytes + REG_STATIC_LDS > SCO_LDS_CAP) return false;
  }
  rh.TR = std::max(1, (pl.n_c + RGI - 1) / RGI);
  rh.TC = 2 * rh.TR;
  if (rh.TR == 5 && pl.n_c <= RGJ * 9) rh.TC = 9;
  const int slots = CW + 2 * RW + PX;
  rh.off.assign((size_t)slots * RT, 0);
  rh.role.assign((size_t)8 * RT, -1);     // [0] core owned, [1] core variable, [2] elim index,
                                          // [3] col base, [4] row0 base, [5] row1 base, [6] pair base (LDS element index)
  // padded slots gather the spare zero element of their vector
  for (int t = 0; t < RT; t++) {
    for (int k = 0; k < CW; k++) rh.off[(size_t)k * RT + t] = (unsigned short)(8 * pl.m);
    for (int k = 0; k < 2 * RW; k++) rh.off[(size_t)(CW + k) * RT + t] = (unsigned short)(8 * pl.n);
    for (int k = 0; k < PX; k++) rh.off[(size_t)(CW + 2 * RW + k) * RT + t] = (unsigned short)(8 * pl.n_c);
    rh.role[(size_t)3 * RT + t] = 0; rh.role[(size_t)4 * RT + t] = 0; rh.role[(size_t)5 * RT + t] = 0;
    rh.role[(size_t)6 * RT + t] = 0;
  }
  // columns: thread j
  for (int j = 0; j < pl.n; j++) {
    const int w = pl.Ap[j + 1] - pl.Ap[j];
    if (w > CW) return false;
    for (int k = 0; k < w; k++)
      rh.off[(size_t)k * RT + j] = (unsigned short)(8 * pl.Ai[pl.Ap[j] + k]);      // byte offset into t / w*y
    rh.role[(size_t)3 * RT + j] = rh.Ac.base[j / 64] + (j % 64);
  }
  // rows: thread i % RT, slot i / RT
  for (int i = 0; i < pl.m; i++) {
    const int w = pl.Rp[i + 1] - pl.Rp[i];
    if (w > RW) return false;
    const int t = i % RT, q = i / RT;
    for (int k = 0; k < w; k++)
      rh.off[(size_t)(CW + q * RW + k) * RT + t] = (unsigned short)(8 * pl.Rj[pl.Rp[i] + k]);   // into x~ / x
    rh.role[(size_t)(4 + q) * RT + t] = rh.Ar.base[i / 64] + (i % 64);
  }
  // eliminated variables: owner = the thread of their column
  std::vector<char> elim_owner(RT, 0);
  for (int e = 0; e < pl.n_e; e++) {
    const int t = pl.elim_var[e];
    const int w = pl.e_ptr[e + 1] - pl.e_ptr[e];
    if (w > PX) return false;
    elim_owner[t] = 1;
    rh.role[(size_t)2 * RT + t] = e;
    for (int k = 0; k < w; k++)
      rh.off[(size_t)(CW + 2 * RW + k) * RT + t] = (unsigned short)(8 * pl.pair_core[pl.e_ptr[e] + k]);   // into x_C
    rh.role[(size_t)6 * RT + t] = rh.Ac.total + rh.Ar.total + rh.Ca.total + rh.Ce.base[e / 64] + (e % 64);
  }
  // core variables: prefer threads without a column, never an eliminated-variable owner
  {
    std::vector<int> cand;
    for (int t = RT - 1; t >= pl.n; t--) cand.push_back(t);
    for (int t = 0; t < pl.n; t++) if (!elim_owner[t]) cand.push_back(t);
    if ((int)cand.size() < pl.n_c) return false;
    for (int c = 0; c < pl.n_c; c++) {
      const int t = cand[c];
      const int w = pl.a_ptr[c + 1] - pl.a_ptr[c];
      if (w > PX) return false;
      rh.role[t] = c;
      rh.role[(size_t)RT + t] = pl.core_var[c];
      for (int k = 0; k < PX; k++)       // padded slots of a core owner gather the zero element of g_E
        rh.off[(size_t)(CW + 2 * RW + k) * RT + t] = (unsigned short)(8 * pl.n_e);
      for (int k = 0; k < w; k++) {
        const int pair = pl.a_pair[pl.a_ptr[c] + k];
        rh.off[(size_t)(CW + 2 * RW + k) * RT + t] = (unsigned short)(8 * pl.pair_elim[pair]);   // into g_E
      }
      rh.role[(size_t)6 * RT + t] = rh.Ac.total + rh.Ar.total + rh.Ca.base[c / 64] + (c % 64);
    }
  }
  return true;
}

// cap sets instantiated: A = (12, 8, 10) [7-DOF x 20 penalty QP], B = (12, 8, 12) generic small
int reg_caps_for(const QpPlan &pl, int *CW, int *RW, int *PX) {
  int cw = 0, rw = 0, px = 0;
  for (int j = 0; j < pl.n; j++) cw = std::max(cw, pl.Ap[j + 1] - pl.Ap[j]);
  for (int i = 0; i < pl.m; i++) rw = std::max(rw, pl.Rp[i + 1] - pl.Rp[i]);
  for (int c = 0; c < pl.n_c; c++) px = std::max(px, pl.a_ptr[c + 1] - pl.a_ptr[c]);
  for (int e = 0; e < pl.n_e; e++) px = std::max(px, pl.e_ptr[e + 1] - pl.e_ptr[e]);
  if (cw > 12 || rw > 8 || px > 12) return 0;
  *CW = 12; *RW = 8; *PX = px <= 10 ? 10 : 12;
  return 1;
}
