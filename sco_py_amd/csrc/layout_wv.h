// layout_wv.h -- what wv_plan_build (wv_plan.cpp) and the kernels of the wavefront tier (sco_admm_wv.hip) must agree on:
// lane tables, block positions, LDS and constant slots.  Every rule stands here once; no HIP header.
#pragma once
#include "layout_qp.h"

#define WV_T 64
#define WV_MAXNS 4
#define WV_MAXNV 4
// The only -D switch of the tier that changes the layout (0: the Jacobian rows of every instantiation in LDS), hence here,
// where the planner sees it too; the timing switches that leave the layout alone stay in sco_admm_wv.hip.
#ifndef WV_JREG
#define WV_JREG 1
#endif
// The lane's Jacobian rows in REGISTERS where the instantiation has room (NS x BS <= 28 doubles: every instantiation built
// today), else lane-private in LDS, NS x 512 doubles of the plan's request (qp_admm_wv_kernel says why).
SCO_HD constexpr bool wv_jreg(int NS, int BS) { return WV_JREG && NS * BS <= 28; }

// Jacobian WIDTHS of the hinge slots (wv_plan_widths; qp_admm_wv_kernel's JW).  A caller of the QP layer may promise that a
// hinge row holds non-zeros only in its first w in-block columns (the serial-arm families: sqp_rows.h); slot q of the
// kernel then needs jw[q] = the largest w over the rows the plan dealt to it, and every pass over the slot's Jacobian row
// stops there.  A width profile is the four jw packed four bits each, slot 0 lowest; 0 = the generic kernel, every slot at
// the full width BS.  The compiled profiles of the 7-wide NS = 4 kernels with three lanes per block, <7,4,3,10,3>: the
// planner picks from this list, wv_launch (sco_admm_wv.hip) instantiates it and says how to add one.
#define WV_JW_PACK(a, b, c, d) ((a) | ((b) << 4) | ((c) << 8) | ((d) << 12))
#define WV_JW_PROFILES(X) \
  X(3, 5, 7, 7)      /* 7 joints, 5 link points on links 1, 2, 4, 5, 6, two obstacles: the 7 x 20 arm workloads */ \
  X(7, 6, 3, 2)      /* the same rows dealt to the slots by width (wv_plan_build's sort_width; SCO_WV_JSORT=0: row order, the line above) */
SCO_HD constexpr int wv_jw(int JW, int q, int BS) { return JW ? (JW >> (4 * q)) & 15 : BS; }

SCO_HD inline size_t wv_tri(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }   // packed lower, j <= i

// LDS layouts chosen against bank conflicts (r04 PMC: 42 % of the LDS cycles of the first version were conflicts, the LDS
// pipe of a CU with four of these wavefronts was busy 68 % of the time).  A 64-byte row per lane at a 64-byte lane stride
// puts lanes i and i + 4 on the same banks for every 16-byte piece; instead the four pieces of a vector are stored
// PIECE-MAJOR, 16 bytes per block (or per lane slot) inside a piece:
//   block vectors (r, x~, x, extra)  index(pos, k) = (k >> 1) * 2 NPOS + 2 pos + (k & 1)
//   partial column sums              index(j, slot) = j * 2 NSLOT + 2 slot              (slot = pos * lpb + part)
//   rows of G, block pos             index(row i, col c) = 64 pos + 16 ((c >> 1) + shift & 3) + 2 i + (c & 1), shift = 1 for
//                                    the blocks of chain B (both chains read their piece j in the same instruction)
SCO_HD inline int wv_vidx(int npos, int pos, int k) { return (k >> 1) * 2 * npos + 2 * pos + (k & 1); }
SCO_HD inline int wv_gidx(int nstep, int pos, int i, int c) { return 64 * pos + 16 * (((c >> 1) + (pos > nstep ? 1 : 0)) & 3) + 2 * i + (c & 1); }

// The G-resident sweep (WV_GRES, qp_admm_wv_kernel) runs a chain on TWO DPP rows: with HS = (NSTEP + 1) / 2, rows 0 and 1
// (pair 0) take the first HS positions of chains A and B, rows 2 and 3 (pair 1) the rest and the middle block, every lane
// with its rows of G in registers: slot s of a lane is the s-th position of its half, the middle block sits in slot HS of
// pair 1 (both of its rows compute it, row 2 stores it).  Block position -> (row pair, row of the pair = chain, register
// slot, index of component 0 of its r / x~ inside a block vector, index of its couplings inside ef / en).
struct WvGresSlot { int pair, row, slot, vidx, eidx; };
SCO_HD inline WvGresSlot wv_gres_slot(int nstep, int pos) {
  const int hs = (nstep + 1) / 2, npos = 2 * nstep + 2;
  WvGresSlot s = {-1, -1, -1, -1, -1};
  if (pos < 0 || pos > 2 * nstep) return s;                       // (2 nstep + 1: the dummy block of idle lanes, no sweep lane)
  if (pos == nstep) { s.pair = 1; s.row = 0; s.slot = hs; }
  else {
    const int chain = pos > nstep ? 1 : 0, st = pos - (chain ? nstep + 1 : 0);
    s.pair = st >= hs ? 1 : 0; s.row = chain; s.slot = st - (s.pair ? hs : 0);
  }
  s.vidx = wv_vidx(npos, pos, 0); s.eidx = pos * 8;
  return s;
}
// int tables, [..][64] lane-minor; offsets in units of 64 ints
struct WvTab {
  int pos, hrow, hbrow, hevar, heidx, hepos, hbpos, hjpos, vvar, vrow, vpos, vpk, vpkm, vpkp, vpd, vpm, vpp, xrow, xpos, xpk, total;
  int lrow, lplo, lphi;           // link slots, NV x NL each, behind everything else (NL = 0: none, `total` as without them)
};
// link slot s of variable slot v (the variable is the row's end in block t, its partner the same in-block index of block
// t + 1): lrow the row, lplo / lphi the CSC positions of A(row, own) and A(row, partner); the partner's place in a block
// vector is the slot's vpkp
SCO_HD inline WvTab wv_tab_layout(int NS, int NV, int NL = 0) {
  WvTab t; int o = 0;
  t.pos = o; o += 1;
  t.hrow = o; o += NS; t.hbrow = o; o += NS; t.hevar = o; o += NS; t.heidx = o; o += NS; t.hepos = o; o += NS; t.hbpos = o; o += NS;
  t.hjpos = o; o += NS * 8;
  t.vvar = o; o += NV; t.vrow = o; o += NV; t.vpos = o; o += NV; t.vpk = o; o += NV; t.vpkm = o; o += NV; t.vpkp = o; o += NV;
  t.vpd = o; o += NV * 8; t.vpm = o; o += NV; t.vpp = o; o += NV;
  t.xrow = o; o += 1; t.xpos = o; o += 1; t.xpk = o; o += 1;
  t.lrow = o; o += NV * NL; t.lplo = o; o += NV * NL; t.lphi = o; o += NV * NL;
  t.total = o;
  return t;
}
// constants of the termination test, [slot][64] per problem: hinge slot q: 1/E_h, 1/E_b, 1/D_e; variable slot v: 1/D_c,
// 1/E_0, P(c, c-), P(c, c+), P(c, c), then P(c, block)[8] (read only by problems whose P has entries off these three
// diagonals: pflag); extra row: 1/E_x.  The scalings themselves (E, D) are formed from the reciprocals when the
// certificates' norms need them: the fetch of these constants is what a checked iteration costs most
// (every wavefront of the chip asks for them at the same time).
SCO_HD inline int wv_cst_h(int q) { return 3 * q; }
SCO_HD inline int wv_cst_v(int NS, int v) { return 3 * NS + 13 * v; }
SCO_HD inline int wv_cst_x(int NS, int NV) { return 3 * NS + 13 * NV; }
// link slot i = v NL + s: 1/E of its row (plans with link rows only)
SCO_HD inline int wv_cst_l(int NS, int NV, int i) { return 3 * NS + 13 * NV + 1 + i; }
// how many of these slots a problem has (WvHost::cst_slots), nl = NV NL link slots included
SCO_HD constexpr int wv_cst_slots(int NS, int NV, int nl) { return 3 * NS + 13 * NV + 1 + nl; }
// The copy of them the kernel keeps in LDS, lane-minor, without the P(c, block)[8]: 3 per hinge slot, 5 per variable slot,
// the extra row's -- wv_ck_slots of 64 doubles in the plan's LDS request
SCO_HD constexpr int wv_ck_h(int q) { return 3 * q; }
SCO_HD constexpr int wv_ck_v(int NS, int v) { return 3 * NS + 5 * v; }
SCO_HD constexpr int wv_ck_x(int NS, int NV) { return 3 * NS + 5 * NV; }
SCO_HD constexpr int wv_ck_slots(int NS, int NV) { return 3 * NS + 5 * NV + 1; }
// The four constants of a link slot (its two A entries, l, u) live in registers where the instantiation has room for them,
// else lane-private in LDS, by the compiler's resource report (profiles/wv_link_rows.md): the 7-wide instantiations hold
// 256 + ~200 registers without link rows and would spill with 48 more.  In LDS they take the place of the constants of the
// termination test (qp_admm_wv_kernel, CKG), so that the plan stays within 40 KB.
SCO_HD constexpr bool wv_link_regs(int BS) { return BS != 7; }
