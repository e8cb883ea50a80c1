// sco_admm_wv.hip -- "wavefront" tier of the ADMM solve: ONE wavefront per problem, several problems per CU.
//
// Same algorithm as every other tier (OSQP's ADMM behind /root/reference/sco_py/sco_osqp/osqp_utils.py:195-216, reduced
// system K x~ = sigma x - q + A'(R z - y) with the hinge slacks eliminated in closed form, qp_plan.h).  What changes is
// the algebra of the core solve and, with it, how much of the chip one problem needs:
//
//   * the reduced matrix S of a trajectory penalty QP is BLOCK TRIDIAGONAL (one block per timestep, order bs = DOF;
//     the off-diagonal blocks come from the smoothness objective and are diagonal matrices).  The row-local tier
//     (sco_admm_rl.hip) applies the dense inverse W = S^-1 -- 157 KB of registers at 7 x 20, 71 % of its multiply-adds,
//     and the reason one problem fills a CU.  Here S is factored once per QP as a TWISTED block LDL' (blocks
//     eliminated from both ends towards the middle, explicit pivot inverses G_t = Sigma_t^-1: nb x bs x bs numbers,
//     9 KB) and every iteration runs two forward and two backward block sweeps, the two chains side by side in two
//     16-lane DPP rows, a bs x bs mat-vec = bs `v_fmac_f64_dpp row_newbcast` instructions;
//   * all row / variable state of a problem lives in the registers of ONE wavefront (lane = (timestep, part): NS hinge
//     row slots with their slack variable and its bound row, NV core-variable slots with their box row), the Jacobian
//     rows in lane-private LDS; partial column sums and the sweep's vectors go through 10 KB of LDS; no barrier ever
//     waits for another wavefront.  A problem needs <= 40 KB of LDS and one wavefront: 4 problems per CU.
//
// The tier takes patterns with this structure only (wv_plan_build): hinge rows inside one timestep with their slack and its
// bound row, at most two single rows per core variable, and LINK rows -- no slack, the same in-block index of two
// neighbouring timesteps, at most WV_NL per pair (velocity limits; the LNK instantiations of the kernel, fixed rho only).
// More single rows on a variable (joint limits: two one-sided rows next to the trust-box row, and a pin on the first and
// last timestep) are STACKED rows: the rows in front of the last one sit in the variable's free link slots with an empty
// partner (lphi = -1, coefficient 0), at most one left-over first row on an extra-row lane.  A stacked row is a link row in
// everything else: base rho, weight 1, the LNK instantiations, no adaptive rho.  Velocity AND joint limits would need four
// slots per variable: refused (WV_WHY_STACKED), the row-local kernel runs them.
// Per problem it takes only VALUES with the structure of a penalty QP (hinge rows l = -inf with one common weight, slack
// rows [0, inf), everything on the base rho, link rows with weight 1: checked by qp_wv_factor_kernel).  A problem that fails the value test is left to the row-local kernel, which the launcher runs
// right behind this one for exactly those problems -- so the tier never changes what is solved, only where.
//
// Block positions.  The sweeps are unrolled NSTEP times (a template argument); both chains are padded AT THEIR START
// with all-zero dummy blocks to exactly NSTEP blocks, so one instantiation serves every horizon up to 2 NSTEP + 1:
//   positions 0 .. NSTEP-1      chain A = blocks 0 .. mid-1 (the real ones last),
//   position  NSTEP             the middle block mid = nb / 2,
//   positions NSTEP+1 .. 2NSTEP chain B = blocks nb-1 .. mid+1 (the real ones last),
//   position  2NSTEP+1          dummy block of idle lanes.
// A dummy block has G = 0 and zero couplings: it maps zeros to zeros and the stores into it write zeros.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "sco_admm_check.h"
#include "layout_wv.h"      // lane tables, block positions, LDS and constant slots: shared with wv_plan_build (wv_plan.cpp)

// timing switches of diagnostic builds (scripts/build_ablate.py wv:...); none of them changes the layout
#ifndef WV_PD
#define WV_PD 3       // block steps between the LDS reads of a sweep step and its arithmetic
#endif
typedef double d2 __attribute__((ext_vector_type(2)));

// (a VALU write of the broadcast operand needs two wait states before a DPP instruction reads it: the first of a chain
// carries them itself, inline assembly is opaque to the compiler's hazard recogniser.  Plain `asm`, not `asm volatile`:
// a volatile statement is a scheduling barrier, and the loads of the next block step have to move above this one's chain)
#ifndef WV_KEEP
#define WV_KEEP 8        // blocks of G per chain the forward sweep keeps in registers for the backward sweep
#endif
#ifndef WV_VARIANT
#define WV_VARIANT 0          // timing variants (scripts/build_ablate.py wv:WV_VARIANT=1): 1 = plain v_fmac_f64 instead of the DPP broadcasts (results wrong)
#endif
#ifndef WV_GRES
#define WV_GRES 1             // 0 = every instantiation on the LDS-fed sweep (scripts/build_ablate.py wv:WV_GRES=0)
#endif
#ifndef WV_ROWS_EARLY
#define WV_ROWS_EARLY 1       // 0 = the row phase reads its partial sums behind the core-variable loop, as before (scripts/build_ablate.py wv:WV_ROWS_EARLY=0)
#endif
// the sweep's issue slots (profiles/wv_sweep_slots.md; each 0 = the form of before, scripts/build_ablate.py wv:<NAME>=0)
#ifndef WV_MV_INIT
#define WV_MV_INIT 1          // wv_matvec: the accumulators' initialisations inside the chain's statement, as its wait states
#endif
#ifndef WV_HANDOVER
#define WV_HANDOVER 1         // lane-swap hand-overs of the sweeps: the swap's two operands chosen so that no select and no copy follows
#endif
#ifndef WV_JWIDTH
#define WV_JWIDTH 1           // 0 = every launch on the generic kernel whatever width profile the plan holds (scripts/build_ablate.py wv:WV_JWIDTH=0)
#endif
#if WV_VARIANT == 1
#define WV_FMAC_DPP(acc, w, g, k) asm("v_fmac_f64 %0, %1, %2" : "+v"(acc) : "v"(w), "v"(g))
#endif

// (v_rcp_f64, one instruction: these reciprocals only scale the norms of the infeasibility tests)
__device__ __forceinline__ double wv_recip(double x) { return x != 0.0 ? __builtin_amdgcn_rcp(x) : 0.0; }

int wv_upload(const WvHost &wh, int batch, int n, int m, std::vector<void *> &allocs, WvDev &wd) {
  void *p = nullptr;
  SCO_HIP(hipMalloc(&p, wh.tab.size() * sizeof(int))); allocs.push_back(p);
  SCO_HIP(hipMemcpy(p, wh.tab.data(), wh.tab.size() * sizeof(int), hipMemcpyHostToDevice)); wd.tab = (const int *)p;
  SCO_HIP(hipMalloc(&p, (size_t)batch * wh.g_doubles * sizeof(double))); allocs.push_back(p); wd.G = (double *)p;
  SCO_HIP(hipMalloc(&p, (size_t)batch * wh.cst_slots * 64 * sizeof(double))); allocs.push_back(p); wd.cst = (double *)p;
  SCO_HIP(hipMalloc(&p, (size_t)batch * sizeof(double))); allocs.push_back(p); wd.wc = (double *)p;
  SCO_HIP(hipMalloc(&p, (size_t)batch * sizeof(int))); allocs.push_back(p); wd.ok = (int *)p;
  SCO_HIP(hipMemset(p, 0, (size_t)batch * sizeof(int)));
  SCO_HIP(hipMalloc(&p, (size_t)batch * sizeof(int))); allocs.push_back(p); wd.rl_need = (int *)p;
  SCO_HIP(hipMemset(p, 0, (size_t)batch * sizeof(int)));
  SCO_HIP(hipMalloc(&p, sizeof(unsigned long long))); allocs.push_back(p); wd.it_count = (unsigned long long *)p;
  SCO_HIP(hipMemset(p, 0, sizeof(unsigned long long)));
  SCO_HIP(hipMalloc(&p, (size_t)batch * sizeof(int))); allocs.push_back(p); wd.pflag = (int *)p;
  SCO_HIP(hipMemset(p, 0, (size_t)batch * sizeof(int)));
  SCO_HIP(hipMalloc(&p, (size_t)batch * sizeof(int))); allocs.push_back(p); wd.w_ready = (int *)p;
  SCO_HIP(hipMemset(p, 0, (size_t)batch * sizeof(int)));
  SCO_HIP(hipMalloc(&p, (size_t)batch * (size_t)(n + m) * sizeof(double))); allocs.push_back(p); wd.scr = (double *)p;
  return SCO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernel arguments
// ---------------------------------------------------------------------------------------------------------------------
struct WvArgs {
  int n, m, n_e, n_c, nnzA, nnzP, max_iter, check, slice;
  int b0; const int *list;
  int bs, nb, mid, lpb, n_extra, NS, NV, NSTEP, cst_slots, NL; size_t g_doubles;      // (NL fills the padding in front of g_doubles)
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  const int *tab;
  double *G, *cst, *wc, *scr; int *ok, *rl_need, *w_ready, *pflag; unsigned long long *it_count;
  const double *As, *Ps, *qs, *ls, *us, *rhov, *kee_inv, *cscale, *D, *E, *S;
  const int *w, *active, *setup_active;
  const int *Ap, *Ai, *Rp, *Rj, *Rpos, *Fp, *Fi, *Fpos;
  double *x, *y, *resid; int *status, *iters, *prog;
  double *sx, *sz, *sy, *st, *sg;
  int ablate;        // diagnostic (SCO_WV_ABLATE, read by builds with -DWV_ABLATE only): 1 = no sweeps, 2 = no row passes, 16 = no termination test behind the checked iteration, 64 = no infeasibility certificates (timing only, results wrong)
  // the opt-in extensions (behind everything else: the fields above keep their places): warm = start from the handle's previous
  // solution in x / y; ad_interval > 0 = adaptive rho (the ADAPT instantiation): rho is rho_b[b], estimated again every
  // ad_interval iterations; when it must change the solve parks with the new value and smask[b] = rflag[b] = 1
  int warm, ad_interval; double ad_tol; double *rho_b; int *rflag, *smask, *nupd;
  // the width profile of the launch (WvHost::jw_profile, packed: layout_wv.h; 0 = every hinge slot at the full width): read by
  // the factor kernel's value test only, the ADMM kernel has it as a template argument
  int jw;
};

// Wavefront-wide max / sum in registers, every lane ends with the result: wave_reduce_all of sco_lanes.h.
__device__ __forceinline__ double wv_wmax(double v) { return wave_reduce_all<true>(v); }
__device__ __forceinline__ double wv_wsum(double v) { return wave_reduce_all<false>(v); }
// The hand-overs of the sweeps (WV_HANDOVER) pick the a and b of lane_swap so that the swapped registers ARE what the next
// step needs: a copy of both halves in front of each swap, two selects per half behind it and the wait states between were
// 29 issue slots of the 7-wide iteration.
// The two chains meet: a = b = the last forward vector of the lane's chain (even rows chain A, odd rows chain B).  Behind
// the swap a holds chain A's vector on EVERY row (the even rows kept their own, the odd rows got the even rows') and b chain
// B's: the operands of the middle block as they are.  (Before, and still without DIRECT: vother = chain ? a : b, then
// vA = chain ? vother : vlast and vB = chain ? vlast : vother -- four selects per register half that pick, on every row,
// exactly these two registers.)
template <bool DIRECT>
__device__ __forceinline__ void wv_meet(double vlast, int chain, double &vA, double &vB) {
  if (DIRECT) {
    vA = vlast; vB = vlast;
    lane_swap<16>(vA, vB);
  } else {
    lane_u2 lo, hi;
    lane_swap_halves<16>(vlast, vlast, lo, hi);
    // .x: odd rows now hold the even rows' values; .y: even rows now hold the odd rows' values
    const double vother = chain ? __hiloint2double((int)hi.x, (int)lo.x) : __hiloint2double((int)hi.y, (int)lo.y);
    vA = chain ? vother : vlast; vB = chain ? vlast : vother;
  }
}
// the limit of upper_is_infinite / lower_is_infinite and osqp_row_leaves_cone (sco_admm_check.h): keep them one value
#define WV_BIG (SCO_INFTY * SCO_MIN_SCALING)

// ---------------------------------------------------------------------------------------------------------------------
// factor kernel: value test, twisted block factorisation G_t = Sigma_t^-1, constants of the termination test
// ---------------------------------------------------------------------------------------------------------------------
// LNK: link slots per variable slot (0: the kernel of a link-free plan, which holds no code of theirs)
template <int LNK>
__global__ __launch_bounds__(WV_T) void qp_wv_factor_kernel(WvArgs a) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int b = a.list ? a.list[g + a.b0] : g + a.b0;
  if (b < 0) return;
  if (a.setup_active && !a.setup_active[b]) { if (lane == 0) a.rl_need[b] = 0; return; }
  const int n = a.n, m = a.m, bs = a.bs, nb = a.nb, mid = a.mid, NS = a.NS, NV = a.NV, NSTEP = a.NSTEP;
  const WvTab T = wv_tab_layout(NS, NV, LNK);
  const int *tab = a.tab;
  const double *ls = a.ls + (size_t)b * m, *us = a.us + (size_t)b * m, *rho = a.rhov + (size_t)b * m;
  const int *w = a.w + (size_t)b * m;
  const double *D = a.D + (size_t)b * n, *E = a.E + (size_t)b * m, *Ps = a.Ps + (size_t)b * a.nnzP;
  double *cst = a.cst + (size_t)b * a.cst_slots * 64;
  // ---- value structure of a penalty QP (else the row-local kernel takes the problem); the base rho is the problem's own
  // with adaptive rho (the setup kernel has just built d.rho from it)
  const double rho_base = a.rho_b ? a.rho_b[b] : a.rho;
  int bad = 0, wk = 0, offd = 0;      // offd: P has entries inside a block off its diagonal
  for (int q = 0; q < NS; q++) { const int h = tab[(T.hrow + q) * 64 + lane]; if (h >= 0) wk = max(wk, w[h]); }
  wk = (int)wv_wmax((double)wk);
  for (int q = 0; q < NS; q++) {
    const int h = tab[(T.hrow + q) * 64 + lane], br = tab[(T.hbrow + q) * 64 + lane], ev = tab[(T.hevar + q) * 64 + lane];
    double eh = 0.0, eb = 0.0, de = 0.0;
    if (h >= 0) {
      if (!(ls[h] < -WV_BIG) || rho[h] != rho_base || w[h] != wk) bad = 1;
      if (!(us[br] > WV_BIG) || ls[br] != 0.0 || rho[br] != rho_base || w[br] != 1) bad = 1;
      eh = E[h]; eb = E[br]; de = D[ev];
      // a width profile runs only on rows that keep the caller's promise: a non-zero at or beyond the slot's width sends the
      // problem to the row-local kernel like any other failed test (a wrong hint costs speed, never a result)
      if (a.jw)
        for (int k = wv_jw(a.jw, q, bs); k < bs; k++) {
          const int jp = tab[(T.hjpos + q * 8 + k) * 64 + lane];
          if (jp >= 0 && a.As[(size_t)b * a.nnzA + jp] != 0.0) bad = 1;
        }
    }
    double *c = cst + (size_t)wv_cst_h(q) * 64 + lane;
    c[0] = h >= 0 ? 1.0 / eh : 0.0; c[64] = h >= 0 ? 1.0 / eb : 0.0; c[128] = h >= 0 ? 1.0 / de : 0.0;
  }
  for (int v = 0; v < NV; v++) {
    const int var = tab[(T.vvar + v) * 64 + lane], r0 = tab[(T.vrow + v) * 64 + lane];
    double *c = cst + (size_t)wv_cst_v(NS, v) * 64 + lane;
    if (r0 >= 0 && (rho[r0] != rho_base || w[r0] != 1)) bad = 1;
    c[0] = var >= 0 ? 1.0 / D[var] : 0.0;
    c[64] = r0 >= 0 ? 1.0 / E[r0] : 0.0;
    const int pm = tab[(T.vpm + v) * 64 + lane], pp = tab[(T.vpp + v) * 64 + lane];
    c[2 * 64] = pm >= 0 ? Ps[pm] : 0.0; c[3 * 64] = pp >= 0 ? Ps[pp] : 0.0;
    const int kown = (tab[(T.vpk + v) * 64 + lane] / (2 * (2 * NSTEP + 2)) << 1) | (tab[(T.vpk + v) * 64 + lane] & 1);   // in-block index of the variable
    double pdiag = 0.0;
    for (int k = 0; k < 8; k++) {
      const int pd = tab[(T.vpd + v * 8 + k) * 64 + lane];
      const double pv = pd >= 0 ? Ps[pd] : 0.0;
      c[(5 + k) * 64] = pv;
      if (var >= 0 && k == kown) pdiag = pv; else if (var >= 0 && pv != 0.0) offd = 1;
    }
    c[4 * 64] = pdiag;
  }
  {
    const int xr = tab[T.xrow * 64 + lane];
    double *c = cst + (size_t)wv_cst_x(NS, NV) * 64 + lane;
    c[0] = xr >= 0 ? 1.0 / E[xr] : 0.0;
  }
  if constexpr (LNK > 0) {
    // link rows sit on the base rho with weight 1 like the box rows (an equality link row has rho_eq: row-local kernel)
    for (int i = 0; i < NV * LNK; i++) {
      const int lr = tab[(T.lrow + i) * 64 + lane];
      if (lr >= 0 && (rho[lr] != rho_base || w[lr] != 1)) bad = 1;
      cst[(size_t)wv_cst_l(NS, NV, i) * 64 + lane] = lr >= 0 ? 1.0 / E[lr] : 0.0;
    }
  }
  bad = (int)wv_wmax((double)bad); offd = (int)wv_wmax((double)offd);
  if (lane == 0) a.pflag[b] = offd;
  // (a failed value test: the dense inverse is formed right behind this kernel, so W will be ready)
  if (lane == 0) { a.ok[b] = !bad; a.rl_need[b] = bad; a.w_ready[b] = bad; a.wc[b] = (double)wk; }
  if (bad) return;
  // ---- twisted block factorisation.  Lane (i, j) = (lane >> 3, lane & 7) holds entry (i, j) of the current 8 x 8 block
  // (entries beyond bs: identity).
  const double *S = a.S + (size_t)b * a.n_c * a.n_c;
  double *G = a.G + (size_t)b * a.g_doubles;
  const int npos = 2 * NSTEP + 2;
  double *ef = G + (size_t)npos * 64, *en = ef + npos * 8, *em = en + npos * 8;
  for (size_t t = lane; t < a.g_doubles; t += WV_T) G[t] = 0.0;
  __threadfence_block(); __syncthreads();
  const int i = lane >> 3, j = lane & 7;
  auto Sblk = [&](int t) -> double {            // entry (i, j) of diagonal block t
    if (i >= bs || j >= bs) return i == j ? 1.0 : 0.0;
    const int ca = t * bs + max(i, j), cb = t * bs + min(i, j);
    return S[wv_tri(ca, cb)];
  };
  auto Soff = [&](int t, int k) -> double {     // coupling between blocks t and t + 1 at in-block index k
    return (k < bs && t >= 0 && t + 1 < nb) ? S[wv_tri((t + 1) * bs + k, t * bs + k)] : 0.0;
  };
  auto invert = [&](double M) -> double {       // Gauss-Jordan without pivoting (S is positive definite)
    for (int p = 0; p < 8; p++) {
      const double piv = __shfl(M, p * 8 + p), rowp = __shfl(M, p * 8 + j), colp = __shfl(M, i * 8 + p);
      const double inv = 1.0 / piv;
      if (i == p && j == p) M = inv;
      else if (i == p) M = rowp * inv;
      else if (j == p) M = -colp * inv;
      else M = M - colp * rowp * inv;
    }
    return M;
  };
  double Gmid_corr = 0.0;                        // E G E of the two chains' last blocks, subtracted from the middle block
  for (int chain = 0; chain < 2; chain++) {
    const int len = chain ? nb - 1 - mid : mid, p0 = chain ? 2 * NSTEP + 1 - len : NSTEP - len;
    double Gp = 0.0;
    for (int s = 0; s < len; s++) {
      const int t = chain ? nb - 1 - s : s, p = p0 + s;
      const int tl = chain ? t : t - 1;           // link (tl, tl + 1) joins t with its predecessor in the chain
      const double ei = s > 0 ? Soff(tl, i) : 0.0, ej = s > 0 ? Soff(tl, j) : 0.0;
      const double M = Sblk(t) - ei * Gp * ej;
      Gp = invert(M);
      G[wv_gidx(NSTEP, p, i, j)] = Gp;
      const int tn = chain ? t - 1 : t;           // link (tn, tn + 1) joins t with the next block towards the middle
      if (lane < 8) { ef[p * 8 + lane] = s > 0 ? Soff(tl, lane) : 0.0; en[p * 8 + lane] = Soff(tn, lane); }
    }
    if (len > 0) {
      const int tl = chain ? mid : mid - 1;       // link between the chain's last block and the middle block
      Gmid_corr += Soff(tl, i) * Gp * Soff(tl, j);
    }
  }
  {
    const double Gm = invert(Sblk(mid) - Gmid_corr);
    G[wv_gidx(NSTEP, NSTEP, i, j)] = Gm;
    if (lane < 8) { ef[NSTEP * 8 + lane] = Soff(mid - 1, lane); em[lane] = Soff(mid, lane); }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// ADMM kernel
// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double wv_min(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double wv_max(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// a row of G: BS doubles (the eighth of a 7-wide row is not loaded: its register would be free at once and the allocator
// reuses it for the next load, which then has to wait for this one)
template <int BS> struct WvRow { d2 a, b, c; d2 d; };
// p: piece 0 of the lane's row (pieces 0 .. 2 follow at 16-double steps), pd: its piece 3 (wrapped for chain B)
template <int BS>
__device__ __forceinline__ WvRow<BS> wv_row(const double *p, const double *pd) {
  WvRow<BS> r;
  r.a = *(const d2 *)p; r.b = *(const d2 *)(p + 16); r.c = *(const d2 *)(p + 32);
  if (BS > 7) r.d = *(const d2 *)pd; else { r.d.x = pd[0]; r.d.y = 0.0; }
  return r;
}

// The chain's text.  Operands of every statement that uses it: %0, %1 the two accumulators, %2 the broadcast vector w, %3..%9
// the row of G (WV_G7), %10 its eighth entry where BS is 8.
#define WV_DPP_STEP(acc, g, k) "v_fmac_f64_dpp " acc ", %2, " g " row_newbcast:" #k " row_mask:0xf bank_mask:0xf\n\t"
#define WV_DPP_CHAIN7 WV_DPP_STEP("%0", "%3", 0) WV_DPP_STEP("%1", "%4", 1) WV_DPP_STEP("%0", "%5", 2) WV_DPP_STEP("%1", "%6", 3) \
                      WV_DPP_STEP("%0", "%7", 4) WV_DPP_STEP("%1", "%8", 5) WV_DPP_STEP("%0", "%9", 6)
#define WV_G7 "v"(g0.x), "v"(g0.y), "v"(g1.x), "v"(g1.y), "v"(g2.x), "v"(g2.y), "v"(g3.x)

// ZERO: the sum starts from 0 (forward steps, the middle block), else from `init` (backward steps: the forward vector)
// INIT: the initialisations inside the statement (wv_slots bit 0), else in front of it with s_nop 1 as the wait states
template <int BS, bool ZERO, bool INIT>
__device__ __forceinline__ double wv_matvec(double init, double w, const WvRow<BS> &g) {
  const d2 g0 = g.a, g1 = g.b, g2 = g.c, g3 = g.d;
  // two accumulators: a dependent v_fmac_f64_dpp issues every 8.5 cycles, two interleaved chains every 6.5
  // (scripts/microbench/wave_cost.hip).  The WHOLE chain sits in one asm statement behind the wait states its first
  // broadcast needs: as separate statements the scheduler was free to put a VALU write of w directly in front of a later
  // broadcast (seen as wrong results of one build, r04, when only the first pair was tied together), and the hazard
  // recogniser does not look into inline assembly.
  // The two wait states ARE the accumulators' initialisations (WV_MV_INIT): a lone wavefront pays an issue slot for an
  // s_nop as for any instruction, and the two v_mov_b64 the chain needs anyway covered nothing where the compiler put them, in
  // front of the write of w.  Inside the statement, whoever wrote w last, two VALU instructions stand between that write
  // and the first broadcast read.  The accumulators are written before the inputs are read: early-clobber outputs.
#if WV_VARIANT == 1
  double acc = ZERO ? 0.0 : init, acc2 = 0.0;
  WV_FMAC_DPP(acc, w, g0.x, 0); WV_FMAC_DPP(acc2, w, g0.y, 1);
  WV_FMAC_DPP(acc, w, g1.x, 2); WV_FMAC_DPP(acc2, w, g1.y, 3);
  WV_FMAC_DPP(acc, w, g2.x, 4); WV_FMAC_DPP(acc2, w, g2.y, 5); WV_FMAC_DPP(acc, w, g3.x, 6);
  if (BS > 7) WV_FMAC_DPP(acc2, w, g3.y, 7);
#else
  double acc = ZERO ? 0.0 : init, acc2 = 0.0;
  if (!INIT) {
    if (BS > 7) asm("s_nop 1\n\t" WV_DPP_CHAIN7 WV_DPP_STEP("%1", "%10", 7) : "+v"(acc), "+v"(acc2) : "v"(w), WV_G7, "v"(g3.y));
    else asm("s_nop 1\n\t" WV_DPP_CHAIN7 : "+v"(acc), "+v"(acc2) : "v"(w), WV_G7);
  } else if (BS > 7) {
    if (ZERO) asm("v_mov_b64 %1, 0\n\tv_mov_b64 %0, 0\n\t" WV_DPP_CHAIN7 WV_DPP_STEP("%1", "%10", 7) : "=&v"(acc), "=&v"(acc2) : "v"(w), WV_G7, "v"(g3.y));
    else asm("v_mov_b64 %1, 0\n\tv_mov_b64 %0, %11\n\t" WV_DPP_CHAIN7 WV_DPP_STEP("%1", "%10", 7) : "=&v"(acc), "=&v"(acc2) : "v"(w), WV_G7, "v"(g3.y), "v"(init));
  } else {
    if (ZERO) asm("v_mov_b64 %1, 0\n\tv_mov_b64 %0, 0\n\t" WV_DPP_CHAIN7 : "=&v"(acc), "=&v"(acc2) : "v"(w), WV_G7);
    else asm("v_mov_b64 %1, 0\n\tv_mov_b64 %0, %10\n\t" WV_DPP_CHAIN7 : "=&v"(acc), "=&v"(acc2) : "v"(w), WV_G7, "v"(init));
  }
#endif
  return acc + acc2;
}
#undef WV_G7
#undef WV_DPP_CHAIN7
#undef WV_DPP_STEP

// Hand-over of LDS data between lanes of the ONE wavefront of a workgroup: the LDS unit works through a wavefront's
// instructions in issue order, so a read issued after a write sees it; all that is needed is that the compiler keeps the
// program order (a wavefront-scope fence emits no instruction).  __syncthreads() would add s_waitcnt lgkmcnt(0) + s_barrier
// four times per iteration.  (wave_lds_fence of sco_lanes.h is the same hand-over with a release / acquire pair of fences; this
// kernel's code is scheduled around the single fence, so it keeps its own.)
#define WV_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// opaque copy of a pointer: loads through it cannot be hoisted out of the iteration loop (the constants of the termination
// test and the lane tables are read on checked iterations only; hoisted, they would occupy ~170 registers for the whole solve)
template <typename T>
__device__ __forceinline__ const T *wv_opaque(const T *p) { asm volatile("" : "+v"(p)); return p; }

// State and constants of a lane's link slots (qp_admm_wv_kernel, LNK > 0; slot i = v LNK + s): z, y, the clipped delta_y of
// the checked iteration, x~ of the partners during a row pass; the four constants of a slot (its two A entries, l, u) in
// registers (REG) or lane-private in LDS at lkl (pairs: piece 2 i = the two A entries, piece 2 i + 1 = l, u; 16 bytes per
// lane and piece).  The kernel of a link-free plan holds the empty specialisation: nothing of this exists there.
template <int NV, int LNK, bool REG> struct WvLinks {
  static constexpr int N = NV * LNK;
  double alo[REG ? N : 1], ahi[REG ? N : 1], l[REG ? N : 1], u[REG ? N : 1], z[N], y[N], d[N], xp[NV];
  double *lkl;
  // The constants of the link slots of variable slot v -- asked for where they are used, one variable slot at a time: fetched
  // for all slots at the top of a phase they would be 48 live registers on top of the 7-wide instantiations' 460, i.e. scratch.
  __device__ __forceinline__ void consts(int v, double (&la)[LNK], double (&lh)[LNK], double (&ll)[LNK], double (&lu)[LNK]) const {
#pragma unroll
    for (int s = 0; s < LNK; s++) {
      const int i = v * LNK + s;
      if constexpr (REG) { la[s] = alo[i]; lh[s] = ahi[i]; ll[s] = l[i]; lu[s] = u[i]; }
      else {
        const d2 ca = *(const d2 *)(lkl + (2 * i) * 128), cb = *(const d2 *)(lkl + (2 * i + 1) * 128);
        la[s] = ca.x; lh[s] = ca.y; ll[s] = cb.x; lu[s] = cb.y;
      }
    }
  }
};
template <int NV, bool REG> struct WvLinks<NV, 0, REG> {};

// EXT: the opt-in extensions, in instantiations of their own as in sco_admm_rl.hip: the default kernel (EXT = 0, parity mode)
// holds no code of theirs.  Bit 0: the solve may start warm (WvArgs::warm); bit 1 (ADAPT): the adaptive-rho variant.
// ADAPT: the problem's rho is rho_b[b]; at every ad_interval-th iteration, behind the termination test, the kernel forms
// OSQP's estimate (osqp_rho_estimate, sco_admm_check.h) from norms that ride along in that test, and when rho must change it
// parks the solve like a used-up slice.  The setup and factor kernels then run for the problem again (smask) and the next
// launch resumes it: the right-hand side is rebuilt from x, z, y on every resume, so the new rho needs nothing further.
//
// GRES: the G-resident sweep (wv_gres_slot).  G is a constant of the QP; the LDS-fed sweep streams it through LDS every
// iteration, 16 lanes wide, and is bound by that.  Here every sweep lane keeps its rows of G in registers over
// the plain iterations (read again from the LDS image behind every termination test): HS + 1 blocks of registers instead of
// the ring, the kept blocks and the NSTEP intermediate vectors of the LDS-fed form, and no LDS read of G in the iteration
// loop.  The arithmetic of every block step is the LDS-fed sweep's, instruction for instruction, on the same values: the
// results are bit-identical.  An instantiation takes this form where it fits without scratch and without more accumulation
// registers than the LDS-fed form (wv_gres_fits, from the compiler's resource report: profiles/wv_gres.md).
constexpr bool wv_gres_fits(int BS, int NS, int NV, int NSTEP, int LPB, int EXT) {
  // (the 7-wide adaptive-rho instantiations stay on the LDS-fed sweep: <7,4,3,10,0,3> would take 246 accumulation registers
  // against 244, <7,4,3,10,3,3> is at 256 + 256 either way)
  return WV_GRES != 0 && NSTEP % 2 == 0 && !(BS == 7 && (EXT & 2));
}
// The row phase with its partial-sum reads in ONE batch behind the first WV_SYNC, in front of the core-variable loop, which
// needs none of them: the round trip runs under that loop's arithmetic instead of in front of the sums.  The
// batch is NV x (LPB + 1) live doubles across the loop: an instantiation takes this order where it fits without scratch and
// without more accumulation registers than before (profiles/wv_row_handover.md).  Link plans store oLK inside the variable
// loop and run-time lanes per block loop over lpb: both keep the old order.
constexpr bool wv_rows_early(int BS, int NS, int NV, int NSTEP, int LPB, int EXT, int LNK) {
  // (<7,4,3,10,3,3> is at 256 + 256 registers as it is: the adaptive-rho instantiations keep the old order)
  return WV_ROWS_EARLY != 0 && LNK == 0 && LPB > 0 && !(EXT & 2);
}
// The sweep's issue slots (profiles/wv_sweep_slots.md), a mask: 1 = the accumulators' initialisations inside wv_matvec's
// statement, 4 = the hand-overs with chosen swap operands.  The early-clobber accumulators hold a few registers longer: an
// instantiation takes an item where it fits without scratch and without more accumulation registers than before, from the
// compiler's resource report.
constexpr int wv_slots(int BS, int NS, int NV, int NSTEP, int LPB, int EXT, int LNK) {
  int sl = (WV_MV_INIT ? 1 : 0) | (WV_HANDOVER ? 4 : 0);
  // (link and stacked plans: with the hand-overs <8,2,2,10,0,0,2> takes 147 accumulation registers against 144 and both
  // <8,2,2,8,0,.,2> one or two more)
  if (LNK > 0) sl &= 1;
  // (<7,4,3,10,3,1,0>, the 7-wide kernel that may start warm: 206 accumulation registers against 204 with the initialisations
  // inside)
  if (BS == 7 && LPB == 3 && EXT == 1) sl &= 4;
  return sl;
}
//
// LNK: link slots per variable slot (WV_NL; 0 = the kernel of a link-free plan, which holds no code of theirs).  A link row
// has no slack and two core variables, the same in-block index k of blocks t and t + 1 (a velocity limit).  It belongs to the
// lane and variable slot of (t, k): z and y in registers, x~ of both ends from the block vectors, the OSQP update of a box row
// on the base rho.  Its share of the right-hand side for (t, k) joins the slot's own part; the share for (t + 1, k) goes
// through one more block vector in LDS (oLK, next to the extra rows' oEX), stored in front of the phase's first WV_SYNC and
// read behind it by the partner.  Every (t + 1, k) has one writer lane, and the rows of a pair add in slot order.
// A STACKED row (a single row of (t, k) in a link slot: joint limits) is that row without the partner entry: its coefficient
// there is 0, so what it adds to the link vector, to A'y and to A dx at the partner's place is an exact zero -- also in the
// last block, whose partner place is the dummy block.
//
// JW: the width profile (layout_wv.h; 0 = every slot at the full width BS).  Hinge slot q holds, loads and multiplies the
// columns k < wv_jw(JW, q, BS) of its Jacobian row only: the others are exact zeros in every problem that reaches this
// kernel (the factor kernel's value test), and fma(0, x, s) = s for finite x -- but for the sign of a zero sum, -0 + +0 = +0.
// What remains keeps its order and form.
template <int BS, int NS, int NV, int NSTEP, int LPB, int EXT, int LNK, int JW>
__global__ __launch_bounds__(WV_T) void qp_admm_wv_kernel(WvArgs a) {
  constexpr bool ADAPT = (EXT & 2) != 0;
  static_assert(JW == 0 || (wv_jreg(NS, BS) && NS <= 4), "width profiles: Jacobian rows in registers, four slots");
  // column k of hinge slot q takes part (a constant once the slot loops are unrolled; the generic kernel has no such test)
#define WV_COL(q, k) (JW == 0 || (k) < wv_jw(JW, q, BS))
  static_assert(!(LNK > 0 && ADAPT), "adaptive rho on link patterns stays on the row-local kernel (qp_launch_plan)");
  constexpr int NLK = LNK > 0 ? NV * LNK : 1;           // link slots of a lane
  constexpr bool LREG = wv_link_regs(BS);
  constexpr bool GRES = wv_gres_fits(BS, NS, NV, NSTEP, LPB, EXT);
  constexpr bool EARLY = wv_rows_early(BS, NS, NV, NSTEP, LPB, EXT, LNK);
  constexpr int SL = wv_slots(BS, NS, NV, NSTEP, LPB, EXT, LNK);
  constexpr int HS = (NSTEP + 1) / 2, H2 = NSTEP - HS;
  const int g = blockIdx.x, lane = threadIdx.x;
  const int b = a.list ? a.list[g + a.b0] : g + a.b0;
  if (b < 0 || (a.active && !a.active[b])) return;
  if (!a.ok[b]) return;                          // not a penalty-QP value structure: the row-local kernel solves it
  // phases switched off for timing (results wrong): only in a build with -DWV_ABLATE (scripts/build_ablate.py wv:WV_ABLATE),
  // the shipped loop tests nothing
#ifdef WV_ABLATE
  const int ablate = a.ablate;
#else
  constexpr int ablate = 0;
#endif
  const int n = a.n, m = a.m, lpb = LPB > 0 ? LPB : a.lpb;
  constexpr int NPOS = 2 * NSTEP + 2;
  // LDS (doubles), compile-time offsets: the vectors sit at fixed distances from each other
  // The lane's Jacobian rows: constants of the solve, read twice per iteration.  In REGISTERS where the instantiation has
  // room (NS x BS <= 28 doubles: every instantiation built today), else lane-private in LDS: the kernel is bound by the CU's LDS
  // pipe (four wavefronts share it), and these rows were a third of a wavefront's LDS bytes per iteration.
  constexpr bool JREG = wv_jreg(NS, BS);
  constexpr int oG = 0, oEF = oG + NPOS * 64, oEN = oEF + NPOS * 8, oEM = oEN + NPOS * 8, oR = oEM + 8, oXT = oR + NPOS * 8,
                oXC = oXT + NPOS * 8, oEX = oXC + NPOS * 8, oLK = oEX + NPOS * 8, oJ = oLK + (LNK > 0 ? NPOS * 8 : 0),
                oPART = oJ + (JREG ? 0 : NS * 512);
  constexpr int NVEC = LNK > 0 ? 5 : 4;                 // block vectors behind the factor: r, x~, x, extra (, link)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int *tab0 = a.tab;
  constexpr int oPOS = 0, oHROW = 1, oHBROW = oHROW + NS, oHEVAR = oHBROW + NS, oHEIDX = oHEVAR + NS, oHEPOS = oHEIDX + NS,
                oHBPOS = oHEPOS + NS, oHJPOS = oHBPOS + NS, oVVAR = oHJPOS + 8 * NS, oVROW = oVVAR + NV, oVPOS = oVROW + NV,
                oVPK = oVPOS + NV, oVPKM = oVPK + NV, oVPKP = oVPKM + NV, oXROW = oVPKP + NV + 8 * NV + 2 * NV, oXPOS = oXROW + 1,
                oXPK = oXPOS + 1, oLROW = oXPK + 1, oLPLO = oLROW + NV * LNK, oLPHI = oLPLO + NV * LNK;
  const double *As = a.As + (size_t)b * a.nnzA, *qs = a.qs + (size_t)b * n, *lsg = a.ls + (size_t)b * m, *usg = a.us + (size_t)b * m;
  const double *cstg0 = a.cst + (size_t)b * a.cst_slots * 64 + lane;
  double rho_in = a.rho;
  if constexpr (ADAPT) {
    rho_in = a.rho_b[b];
    // (the row-local kernel behind this one skips the problems of this tier, ok[b]: each clears the flags of its own)
    if (lane == 0) { a.rflag[b] = 0; a.smask[b] = 0; }
  }
  const double rho0 = rho_in, rinv0 = 1.0 / rho0, wc = a.wc[b], rw = wc * rho0;
  const double sigma = a.sigma, alpha = a.alpha, oma = 1.0 - alpha;
  const double cscale = a.cscale[b], cinv = 1.0 / cscale;
  const int it0 = a.slice > 0 ? a.prog[b] : 0;
  const bool resume = it0 > 0;
  const double *sxg = a.sx + (size_t)b * n, *szg = a.sz + (size_t)b * m, *syg = a.sy + (size_t)b * m;

  // ---- LDS: factor, zeroed vectors
  {
    const double *Gg = a.G + (size_t)b * a.g_doubles;
    for (int t = lane; t < oR; t += WV_T) lds[t] = Gg[t];
    for (int t = lane; t < NVEC * NPOS * 8; t += WV_T) lds[oR + t] = 0.0;
    for (int t = lane; t < NPOS * lpb * 8; t += WV_T) lds[oPART + t] = 0.0;
  }
  // ---- LDS: the constants of the termination test (scalings of the lane's rows and variables, its P entries), lane-minor.
  // They are constants of the solve; as registers (fetched one iteration ahead of every test) they cost 70 VGPRs for the
  // whole launch -- beyond 256 every use of a register is a v_accvgpr move.
  // (CKG: an instantiation that keeps its link slots' constants in LDS gives them this place -- they are read in every
  // iteration -- and fetches the constants of the test from global memory at every checked iteration, as the dense P
  // constants are: with both in LDS the 7-wide plan takes 51 KB, three problems per CU, and a batch of four per CU runs in
  // two rounds, profiles/wv_link_rows.md)
  constexpr bool CKG = LNK > 0 && !LREG;
  const int oCK = oPART + NPOS * lpb * 8;
  double *const ckl = lds + oCK + lane;
  if constexpr (!CKG) {
#pragma unroll
    for (int q = 0; q < NS; q++)
#pragma unroll
      for (int k = 0; k < 3; k++) ckl[(wv_ck_h(q) + k) * 64] = cstg0[(wv_cst_h(q) + k) * 64];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
      for (int k = 0; k < 5; k++) ckl[(wv_ck_v(NS, v) + k) * 64] = cstg0[(wv_cst_v(NS, v) + k) * 64];
    ckl[wv_ck_x(NS, NV) * 64] = cstg0[wv_cst_x(NS, NV) * 64];
  }
#define CKH(q, k) (CKG ? wv_opaque(cstg0)[(wv_cst_h(q) + (k)) * 64] : ckl[(wv_ck_h(q) + (k)) * 64])
#define CKV(v, k) (CKG ? wv_opaque(cstg0)[(wv_cst_v(NS, v) + (k)) * 64] : ckl[(wv_ck_v(NS, v) + (k)) * 64])
#define CKX (CKG ? wv_opaque(cstg0)[wv_cst_x(NS, NV) * 64] : ckl[wv_ck_x(NS, NV) * 64])
  // (1/E of a link slot's row comes from global memory at the checked iteration in every instantiation, as the dense P
  // constants do)
#define CKL(i) wv_opaque(cstg0)[wv_cst_l(NS, NV, i) * 64]
  // ---- lane roles (row layout): pointers into the vectors of the lane's block
  const int pos_r = tab0[oPOS * 64 + lane];
  double *const xt_p = lds + oXT + pos_r * 2;                                   // x~ of the block, piece 0 (xc: + (oXC - oXT))
  const int nslot2 = NPOS * lpb * 2;                                            // doubles of one piece of the partial sums
  double *const part_p = lds + oPART + (pos_r * lpb + (lane & 15) % lpb) * 2;   // the lane's partial column sums, piece 0
  double *const jl_p = lds + oJ + lane * 2;                                     // Jacobian rows, lane-private
  // hinge slots: constants and state
  bool h_on[NS];
  double h_ae[NS], h_ab[NS], h_u[NS], h_q[NS], h_kinv[NS], h_z[NS], h_y[NS], h_zb[NS], h_yb[NS], h_xe[NS], h_ge[NS];
  double hJ[JREG ? NS : 1][8];
#pragma unroll
  for (int q = 0; q < NS; q++) {
    const int h = tab0[(oHROW + q) * 64 + lane], br = tab0[(oHBROW + q) * 64 + lane], ev = tab0[(oHEVAR + q) * 64 + lane];
    const bool on = h >= 0;
    h_on[q] = on;
    h_ae[q] = on ? As[tab0[(oHEPOS + q) * 64 + lane]] : 0.0;
    h_ab[q] = on ? As[tab0[(oHBPOS + q) * 64 + lane]] : 0.0;
    h_u[q] = on ? usg[h] : 0.0;
    h_q[q] = on ? qs[ev] : 0.0;
    h_kinv[q] = on ? a.kee_inv[(size_t)b * a.n_e + tab0[(oHEIDX + q) * 64 + lane]] : 0.0;
    h_z[q] = on && resume ? szg[h] : 0.0; h_y[q] = on && resume ? syg[h] : 0.0;
    h_zb[q] = on && resume ? szg[br] : 0.0; h_yb[q] = on && resume ? syg[br] : 0.0;
    h_xe[q] = on && resume ? sxg[ev] : 0.0; h_ge[q] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int j0 = on ? tab0[(oHJPOS + q * 8 + 2 * k) * 64 + lane] : -1, j1 = on ? tab0[(oHJPOS + q * 8 + 2 * k + 1) * 64 + lane] : -1;
      d2 v; v.x = j0 >= 0 && WV_COL(q, 2 * k) ? As[j0] : 0.0; v.y = j1 >= 0 && WV_COL(q, 2 * k + 1) ? As[j1] : 0.0;
      if (JREG) { hJ[q][2 * k] = v.x; hJ[q][2 * k + 1] = v.y; }
      else *(d2 *)(jl_p + (q * 4 + k) * 128) = v;
    }
  }
  // core-variable slots
  double *v_p[NV];                       // address of x~ of the variable (r, x, extra: fixed distances)
  const double *v_pp[NV];                // its component in the first partial-sum slot of its block
  bool v_on[NV], v_r0on[NV];
  int v_pkm[NV], v_pkp[NV];               // positions of the variable's neighbours in time inside a block vector (P entries)
  double v_x[NV], v_q[NV], v_a[NV], v_l[NV], v_u[NV], v_z[NV], v_y[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const int var = tab0[(oVVAR + v) * 64 + lane], r0 = tab0[(oVROW + v) * 64 + lane];
    const int vix = tab0[(oVPK + v) * 64 + lane], vk = ((vix / (2 * NPOS)) << 1) | (vix & 1), vpos = (vix % (2 * NPOS)) >> 1;
    v_on[v] = var >= 0; v_p[v] = lds + oXT + vix;
    v_pp[v] = lds + oPART + (vk >> 1) * nslot2 + vpos * lpb * 2 + (vk & 1);
    v_q[v] = var >= 0 ? qs[var] : 0.0; v_x[v] = var >= 0 && resume ? sxg[var] : 0.0;
    v_a[v] = r0 >= 0 ? As[tab0[(oVPOS + v) * 64 + lane]] : 0.0;
    v_l[v] = r0 >= 0 ? lsg[r0] : 0.0; v_u[v] = r0 >= 0 ? usg[r0] : 0.0;
    v_z[v] = r0 >= 0 && resume ? szg[r0] : 0.0; v_y[v] = r0 >= 0 && resume ? syg[r0] : 0.0;
    v_r0on[v] = r0 >= 0; v_pkm[v] = tab0[(oVPKM + v) * 64 + lane]; v_pkp[v] = tab0[(oVPKP + v) * 64 + lane];
  }
  // extra single rows (a second row on a core variable: pins), one per lane
  const int x_row = tab0[oXROW * 64 + lane];
  double *const x_p = lds + oXT + tab0[oXPK * 64 + lane];
  const double x_a = x_row >= 0 ? As[tab0[oXPOS * 64 + lane]] : 0.0, x_l = x_row >= 0 ? lsg[x_row] : 0.0, x_u = x_row >= 0 ? usg[x_row] : 0.0;
  const double x_rho = x_row >= 0 ? a.rhov[(size_t)b * m + x_row] : 1.0, x_rinv = 1.0 / x_rho, x_w = x_row >= 0 ? (double)a.w[(size_t)b * m + x_row] : 0.0;
  double x_z = x_row >= 0 && resume ? szg[x_row] : 0.0, x_y = x_row >= 0 && resume ? syg[x_row] : 0.0;
  // link slots (i = v LNK + s): constants and state; an empty slot is a row of zeros with l = u = 0, its z and y stay 0
  WvLinks<NV, LNK, LREG> lk;
  constexpr int NL1 = LNK > 0 ? LNK : 1;
  if constexpr (LNK > 0) {
    lk.lkl = lds + oCK + lane * 2;                                    // (!LREG: in the place of the constants of the test, CKG)
#pragma unroll
    for (int i = 0; i < NLK; i++) {
      const int lr = tab0[(oLROW + i) * 64 + lane], lph = tab0[(oLPHI + i) * 64 + lane];
      d2 ca, cb;
      // (a stacked row has no partner entry, lphi = -1: coefficient 0.  Every later use of the slot goes through this
      // constant, so the row's share of the link vector, of A'y and of A dx at the partner's place is an exact zero)
      ca.x = lr >= 0 ? As[tab0[(oLPLO + i) * 64 + lane]] : 0.0; ca.y = lr >= 0 && lph >= 0 ? As[lph] : 0.0;
      cb.x = lr >= 0 ? lsg[lr] : 0.0; cb.y = lr >= 0 ? usg[lr] : 0.0;
      if constexpr (LREG) { lk.alo[i] = ca.x; lk.ahi[i] = ca.y; lk.l[i] = cb.x; lk.u[i] = cb.y; }
      else { *(d2 *)(lk.lkl + (2 * i) * 128) = ca; *(d2 *)(lk.lkl + (2 * i + 1) * 128) = cb; }
      lk.z[i] = lr >= 0 && resume ? szg[lr] : 0.0; lk.y[i] = lr >= 0 && resume ? syg[lr] : 0.0;
    }
  }
  // sweep roles: DPP row 0 (and its copy, row 2) runs chain A, row 1 (and 3) chain B; lane k of a row holds component k
  // (GRES: rows 0 and 1 hold the first HS positions of the two chains, rows 2 and 3 the rest: pos0 is slot 0 of the lane)
  const int srow = lane >> 4, k8 = lane & 7, chain = srow & 1, half = GRES ? srow >> 1 : 0;
  const bool sw_store = (GRES || srow < 2) && (lane & 15) < 8;
  const int pos0 = (chain ? NSTEP + 1 : 0) + half * HS;
  const WvGresSlot sl0 = wv_gres_slot(NSTEP, pos0);                                    // (the next block: + 2 in a vector, + 8 in the couplings)
  const double *const sw_g = lds + oG + pos0 * 64 + k8 * 2 + (chain ? 16 : 0);        // row k8 of the chain's first block, piece 0
  const double *const sw_gd = lds + oG + pos0 * 64 + k8 * 2 + (chain ? 0 : 48);       // ... its piece 3
  double *const sw_v = lds + oR + sl0.vidx + wv_vidx(NPOS, 0, k8);                      // r of the chain's first block (next block: + 2)
  const double *const sw_e = lds + oEF + sl0.eidx + k8;                                // couplings of the chain's first block
  const double *const md_g = lds + oG + NSTEP * 64 + k8 * 2;
  double *const md_v = lds + oR + wv_vidx(NPOS, NSTEP, k8);
  const double *const md_e = lds + oEF + NSTEP * 8 + k8;
  // GRES: the lane's rows of G, read from the LDS image in front of every run of plain iterations, i.e. once per termination
  // test: held across the test as well, they would sit on top of its peak of live registers (the certificates' delta
  // vectors, the scalings) and push the kernel into scratch.  24 reads per `check` iterations instead of 39 per iteration.
  WvRow<BS> gr[GRES ? HS : 1], gmd;
  auto load_g = [&]() {
    static_assert(!GRES || H2 == HS, "the second half recomputes the first on its idle rows: both halves need the same step count");
#pragma unroll
    for (int s = 0; s < HS; s++) gr[s] = wv_row<BS>(sw_g + s * 64, sw_gd + s * 64);
    gmd = wv_row<BS>(md_g, md_g + 48);
  };
  WV_SYNC();

  // accumulators of the termination test that ride along in the checked step
  double c_ndy = 0.0, c_lhs = 0.0, c_ndx = 0.0, c_qdx = 0.0;
  // Row / variable indices and scaling constants that only a checked iteration needs.  They are fetched from global memory
  // at the START of that iteration, in front of the sweeps, so that the round trip (L2 or HBM: 68 x 512 B per problem) runs
  // under the iteration's own arithmetic; kept for the whole solve they would cost ~170 registers.
  const int pdense = (ablate & 32) ? 1 : a.pflag[b];         // P has entries off the three diagonals the compact constants hold
  // delta_y (clipped) / delta_x of the checked iteration: kept in registers for the infeasibility certificates
  struct { double h[NS], b[NS], e[NS], r0[NV], var[NV], x; } dsv;
  // One pass over the lane's rows and variables.  MODE 0: initialise (right-hand side of the first iteration from the
  // current x, z, y); 1: a plain iteration; 2: a checked iteration (delta_y / delta_x terms of the infeasibility tests).
  auto rows = [&](auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
    // every LDS read of this phase is issued before its first store (the compiler keeps loads behind stores that may alias)
    double xt[8], xtx = 0.0, xtv[NV];
    if (MODE) {
      const d2 a0 = *(const d2 *)xt_p, a1 = *(const d2 *)(xt_p + 2 * NPOS), a2 = *(const d2 *)(xt_p + 4 * NPOS), a3 = *(const d2 *)(xt_p + 6 * NPOS);
      xtx = x_p[0];
#pragma unroll
      for (int v = 0; v < NV; v++) xtv[v] = v_p[v][0];
      xt[0] = a0.x; xt[1] = a0.y; xt[2] = a1.x; xt[3] = a1.y; xt[4] = a2.x; xt[5] = a2.y; xt[6] = a3.x; xt[7] = a3.y;
    }
    // link slots: x~ of the partner (block t + 1, same in-block index)
    if constexpr (LNK > 0) {
      if (MODE) {
#pragma unroll
        for (int v = 0; v < NV; v++) lk.xp[v] = lds[oXT + v_pkp[v]];
      }
    }
    double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    d2 jn0, jn1, jn2, jn3;                       // (rows in LDS) the NEXT slot's row is in flight while this one's arithmetic runs
    if (!JREG) { const d2 *jp = (const d2 *)jl_p; jn0 = jp[0]; jn1 = jp[64]; jn2 = jp[128]; jn3 = jp[192]; }
#pragma unroll
    for (int q = 0; q < NS; q++) {
      double J[8];
      if (JREG) {
#pragma unroll
        for (int k = 0; k < 8; k++) J[k] = hJ[q][k];
      } else {
        J[0] = jn0.x; J[1] = jn0.y; J[2] = jn1.x; J[3] = jn1.y; J[4] = jn2.x; J[5] = jn2.y; J[6] = jn3.x; J[7] = jn3.y;
        if (q + 1 < NS) { const d2 *jp = (const d2 *)(jl_p + (q + 1) * 512); jn0 = jp[0]; jn1 = jp[64]; jn2 = jp[128]; jn3 = jp[192]; }
      }
      const double ae = h_ae[q], ab = h_ab[q], kinv = h_kinv[q];
      const double c2 = rw * ae;
      if (MODE) {
        double s = J[0] * xt[0];
#pragma unroll
        for (int k = 1; k < BS; k++) if (WV_COL(q, k)) s = __builtin_fma(J[k], xt[k], s);
        const double xte = h_ge[q] - (kinv * c2) * s;
        const double zth = __builtin_fma(ae, xte, s), ztb = ab * xte;
        // hinge row: l = -inf
        {
          const double zr = alpha * zth + oma * h_z[q];
          const double zn = wv_min(zr + rinv0 * h_y[q], h_u[q]);
          const double dy = rho0 * (zr - zn);
          h_y[q] += dy; h_z[q] = zn;
          if (MODE == 2) {
            const double dc = fmax(dy, 0.0);              // clipped to the cone of the bounds (u finite, l = -inf)
            c_ndy = fmax(c_ndy, wv_recip(CKH(q, 0)) * fabs(dc)); c_lhs += wc * (h_u[q] * dc);
            dsv.h[q] = dc;
          }
        }
        // slack's bound row: [0, inf)
        {
          const double zr = alpha * ztb + oma * h_zb[q];
          const double zn = wv_max(zr + rinv0 * h_yb[q], 0.0);
          const double dy = rho0 * (zr - zn);
          h_yb[q] += dy; h_zb[q] = zn;
          if (MODE == 2) {
            const double dc = fmin(dy, 0.0);
            c_ndy = fmax(c_ndy, wv_recip(CKH(q, 1)) * fabs(dc));           // l = 0: nothing for u' dy+ + l' dy-
            dsv.b[q] = dc;
          }
        }
        const double xo = h_xe[q], xn = alpha * xte + oma * xo;
        h_xe[q] = xn;
        if (MODE == 2) {
          const double dx = xn - xo;
          c_ndx = fmax(c_ndx, wv_recip(CKH(q, 2)) * fabs(dx)); c_qdx += h_q[q] * dx;
          dsv.e[q] = dx;
        }
      }
      const double th = wc * (rho0 * h_z[q] - h_y[q]);
      const double tb = rho0 * h_zb[q] - h_yb[q];
      const double rhs = ae * th + ab * tb + (sigma * h_xe[q] - h_q[q]);
      const double ge = rhs * kinv;
      h_ge[q] = ge;
      const double tp = th - c2 * ge;
#pragma unroll
      for (int k = 0; k < BS; k++) if (WV_COL(q, k)) part[k] = __builtin_fma(J[k], tp, part[k]);
    }
    {
      d2 v0, v1, v2, v3;
      v0.x = part[0]; v0.y = part[1]; v1.x = part[2]; v1.y = part[3]; v2.x = part[4]; v2.y = part[5]; v3.x = part[6]; v3.y = BS > 7 ? part[7] : 0.0;
      *(d2 *)part_p = v0; *(d2 *)(part_p + nslot2) = v1; *(d2 *)(part_p + 2 * nslot2) = v2; *(d2 *)(part_p + 3 * nslot2) = v3;
    }
    // extra rows
    {
      if (MODE) {
        const double xtc = xtx;
        const double zt = x_a * xtc, zr = alpha * zt + oma * x_z;
        const double zn = wv_min(wv_max(zr + x_rinv * x_y, x_l), x_u);
        const double dy = x_rho * (zr - zn);
        x_y += dy; x_z = zn;
        if (MODE == 2) {
          const double d1 = upper_is_infinite(x_u) ? fmin(dy, 0.0) : dy, dc = lower_is_infinite(x_l) ? fmax(d1, 0.0) : d1;
          c_ndy = fmax(c_ndy, wv_recip(CKX) * fabs(dc)); c_lhs += x_w * (x_u * fmax(dc, 0.0) + x_l * fmin(dc, 0.0));
          dsv.x = dc;
        }
      }
      const double t = x_w * (x_rho * x_z - x_y);
      if (x_row >= 0) x_p[oEX - oXT] = x_a * t;
    }
    // EARLY: every read of the sums is issued here, back to back, and the scheduler may move nothing of the variable loop in
    // front of them, nor them behind it: the loop's ~60 instructions run while the reads are on their way
    double s_ex[NV], s_pt[NV][LPB > 0 ? LPB : 1];
    if constexpr (EARLY) {
      WV_SYNC();
#pragma unroll
      for (int v = 0; v < NV; v++) {
        s_ex[v] = v_p[v][oEX - oXT];
#pragma unroll
        for (int s2 = 0; s2 < LPB; s2++) s_pt[v][s2] = v_pp[v][s2 * 2];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // core variables: box row, x update, own part of the right-hand side
    double own[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
      if (MODE) {
        const double xtc = xtv[v];
        const double zt = v_a[v] * xtc, zr = alpha * zt + oma * v_z[v];
        const double zn = wv_min(wv_max(zr + rinv0 * v_y[v], v_l[v]), v_u[v]);
        const double dy = rho0 * (zr - zn);
        v_y[v] += dy; v_z[v] = zn;
        const double xo = v_x[v], xn = alpha * xtc + oma * xo;
        v_x[v] = xn;
        if (MODE == 2) {
          const double d1 = upper_is_infinite(v_u[v]) ? fmin(dy, 0.0) : dy, dc = lower_is_infinite(v_l[v]) ? fmax(d1, 0.0) : d1;
          if (v_r0on[v]) { c_ndy = fmax(c_ndy, wv_recip(CKV(v, 1)) * fabs(dc)); c_lhs += v_u[v] * fmax(dc, 0.0) + v_l[v] * fmin(dc, 0.0); }
          dsv.r0[v] = dc;
          const double dx = xn - xo;
          if (v_on[v]) { c_ndx = fmax(c_ndx, wv_recip(CKV(v, 0)) * fabs(dx)); c_qdx += v_q[v] * dx; }
          dsv.var[v] = dx;
        }
      }
      const double t0 = rho0 * v_z[v] - v_y[v];
      own[v] = v_a[v] * t0 + (sigma * v_x[v] - v_q[v]);
      if constexpr (LNK > 0) {
        // the variable's link rows: the update of a box row on a row with two entries; the own end's share joins own[v], the
        // partner's goes to its place in the link vector (a lane without a partner: zeros into the dummy block)
        double ps = 0.0, la[NL1], lh[NL1], ll[NL1], lu[NL1];
        lk.consts(v, la, lh, ll, lu);
#pragma unroll
        for (int s = 0; s < LNK; s++) {
          const int i = v * LNK + s;
          if (MODE) {
            const double zt = __builtin_fma(lh[s], lk.xp[v], la[s] * xtv[v]), zr = alpha * zt + oma * lk.z[i];
            const double zn = wv_min(wv_max(zr + rinv0 * lk.y[i], ll[s]), lu[s]);
            const double dy = rho0 * (zr - zn);
            lk.y[i] += dy; lk.z[i] = zn;
            if (MODE == 2) {
              const double d1 = upper_is_infinite(lu[s]) ? fmin(dy, 0.0) : dy, dc = lower_is_infinite(ll[s]) ? fmax(d1, 0.0) : d1;
              c_ndy = fmax(c_ndy, wv_recip(CKL(i)) * fabs(dc)); c_lhs += lu[s] * fmax(dc, 0.0) + ll[s] * fmin(dc, 0.0);
              lk.d[i] = dc;
            }
          }
          const double t = rho0 * lk.z[i] - lk.y[i];
          own[v] = __builtin_fma(la[s], t, own[v]); ps = __builtin_fma(lh[s], t, ps);
        }
        lds[oLK + v_pkp[v]] = ps;
      }
    }
    if constexpr (EARLY) __builtin_amdgcn_sched_barrier(0); else WV_SYNC();
    // core right-hand side = own part + the extra row's (+ the link rows' share from block t - 1) + the block's partial
    // column sums
    double rsum[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
      double r = own[v] + (EARLY ? s_ex[v] : v_p[v][oEX - oXT]);
      if constexpr (LNK > 0) r += v_p[v][oLK - oXT];
      const double *pp = v_pp[v];
      if (EARLY) {
#pragma unroll
        for (int s2 = 0; s2 < LPB; s2++) r += s_pt[v][s2];
      } else if (LPB > 0) {
#pragma unroll
        for (int s2 = 0; s2 < LPB; s2++) r += pp[s2 * 2];
      } else {
        for (int s2 = 0; s2 < lpb; s2++) r += pp[s2 * 2];
      }
      rsum[v] = r;
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
      v_p[v][oR - oXT] = v_on[v] ? rsum[v] : 0.0;
      if (MODE == 2) v_p[v][oXC - oXT] = v_x[v];
    }
    WV_SYNC();
  };

  // x~_C = S^-1 r by the twisted block factorisation: forward sweeps of both chains, the middle block, backward sweeps.
  // Nothing is stored inside the sweeps: the NSTEP intermediate vectors of a chain stay in registers.
  auto sweep_lds = [&]() {
    // only the 16 lanes that hold a component of one of the two chains take part: the others would fetch the same rows of
    // G again (four wavefronts share a CU's LDS pipe).
    // A block step is ~60 cycles of arithmetic (seven dependent v_fmac_f64_dpp in two chains, one fma, one add) and an LDS
    // read comes back after ~130 (scripts/microbench/wave_cost.hip): the rows of G, the right-hand sides and the couplings
    // are asked for WV_PD block steps ahead (r04: one step ahead left the sweeps waiting for LDS, 176 cycles per step).
    constexpr int PD = WV_PD < NSTEP ? WV_PD : NSTEP;
    // The sweeps are bound by the CU's LDS pipe, not by their arithmetic (r04: plain v_fmac_f64 in place of the DPP broadcasts
    // changes nothing, scripts/build_ablate.py wv:WV_VARIANT=1; four wavefronts x 21 steps x 16 lanes x 64 B of G per pass):
    // rows of G the forward pass has read stay in registers for the backward pass (16 VGPRs per block) where the
    // instantiation has room.
    constexpr int KEEPN = NSTEP <= 10 ? (WV_KEEP < NSTEP ? WV_KEEP : NSTEP) : 0;      // the forward pass's last KEEPN blocks
    constexpr int K0 = NSTEP - KEEPN;
    WvRow<BS> gk[KEEPN > 0 ? KEEPN : 1];
    double vs[NSTEP];
    WvRow<BS> gq[PD]; double rq[PD], eq[PD];
    double emk = 0.0, vlast = 0.0;
    if (sw_store) {
      auto fetch_fwd = [&](int st, WvRow<BS> &g, double &r, double &e) {      // block st of the chain; st = NSTEP: the middle block
        if (st < NSTEP) { g = wv_row<BS>(sw_g + st * 64, sw_gd + st * 64); r = sw_v[st * 2]; e = sw_e[st * 8]; }
        else if (st == NSTEP) { g = wv_row<BS>(md_g, md_g + 48); r = md_v[0]; e = md_e[0]; }
      };
#pragma unroll
      for (int i = 0; i < PD; i++) fetch_fwd(i, gq[i], rq[i], eq[i]);
      double vprev = 0.0;
#pragma unroll
      for (int st = 0; st < NSTEP; st++) {
        const WvRow<BS> g = gq[st % PD]; const double rr = rq[st % PD], ee = eq[st % PD];
        fetch_fwd(st + PD, gq[st % PD], rq[st % PD], eq[st % PD]);
        const double w = __builtin_fma(-ee, vprev, rr);
        vprev = wv_matvec<BS, true, (SL & 1) != 0>(0.0, w, g);
        vs[st] = vprev;
        if (st >= K0) gk[st - K0] = g;
      }
      emk = lds[oEM + k8];
      vlast = vs[NSTEP - 1];
    }
    // the middle block needs the last vector of BOTH chains: DPP row 0 holds chain A's, row 1 chain B's.  One
    // v_permlane16_swap per register half hands each row the other's (through LDS the exchange was a store, a wait and a
    // read: ~250 cycles of the ~3000 of a sweep).  All lanes take part in the swap; only the sweep lanes use the result.
    double vA, vB;
    wv_meet<(SL & 4) != 0>(vlast, chain, vA, vB);
    if (sw_store) {
      // (slot NSTEP % PD of the ring holds the middle block: fetched PD steps before the end of the forward sweep)
      const WvRow<BS> gm = gq[NSTEP % PD]; const double rm = rq[NSTEP % PD], em_ = eq[NSTEP % PD];
      // backward sweep: block st of the chain and its coupling towards the middle, again PD steps ahead
      WvRow<BS> gb[PD]; double eb[PD];
      auto fetch_bwd = [&](int st, WvRow<BS> &g, double &e) {
        if (st >= 0) { if (st < K0) g = wv_row<BS>(sw_g + st * 64, sw_gd + st * 64); e = sw_e[st * 8 + (oEN - oEF)]; }
      };
#pragma unroll
      for (int i = 0; i < PD; i++) fetch_bwd(NSTEP - 1 - i, gb[i], eb[i]);
      double w = __builtin_fma(-em_, vA, rm);
      w = __builtin_fma(-emk, vB, w);
      double xn = wv_matvec<BS, true, (SL & 1) != 0>(0.0, w, gm);
      const double xmid = xn;
#pragma unroll
      for (int st = NSTEP - 1; st >= 0; st--) {
        const int slot = (NSTEP - 1 - st) % PD;
        const WvRow<BS> g = st >= K0 ? gk[st - K0] : gb[slot]; const double ee = eb[slot];
        fetch_bwd(st - PD, gb[slot], eb[slot]);
        const double u = -(ee * xn);
        xn = wv_matvec<BS, false, (SL & 1) != 0>(vs[st], u, g);
        vs[st] = xn;
      }
#pragma unroll
      for (int st = 0; st < NSTEP; st++) sw_v[st * 2 + (oXT - oR)] = vs[st];
      if (srow == 0) md_v[oXT - oR] = xmid;
    }
    WV_SYNC();
  };
  // The same sweeps with G resident (GRES).  A block step is issued once for the whole wavefront, NSTEP of them per pass as
  // before; slot s of a lane is position s of its half.  Forward: HS steps, live on rows 0 and 1; one v_permlane32_swap per
  // register half hands the last vector up to rows 2 and 3; HS steps on the same slots, live on rows 2 and 3; the middle
  // block between rows 2 and 3.  Backward: the reverse, with one hand-back.  The idle row pair of a half needs no
  // predication: rows 0 and 1 restart the second forward half from 0 as they started the first, and rows 2 and 3 restart
  // the second backward half from the middle block's x~, so each pair computes its own values again, on the same inputs with
  // the same instructions, while the other pair does its work (what rows 2 and 3 leave behind in the first forward half,
  // and rows 0 and 1 in the first backward half, is overwritten).  Right-hand sides and couplings come from LDS through
  // the lane's own addresses, 8 bytes per lane and step, asked for WV_PD steps ahead; all 64 lanes run the arithmetic
  // (lanes 8 .. 15 of a row mirror lanes 0 .. 7), the sweep lanes store.
  auto sweep_res = [&]() {
    constexpr int PD = WV_PD < NSTEP ? WV_PD : NSTEP;
    double vs[HS], xs[HS], rq[PD], eq[PD], eb[PD];
    auto fetch_fwd = [&](int i, double &r, double &e) {          // issue step i of the forward pass; i = NSTEP: the middle block
      if (i < NSTEP) { const int s = i < HS ? i : i - HS; r = sw_v[s * 2]; e = sw_e[s * 8]; }
      else if (i == NSTEP) { r = md_v[0]; e = md_e[0]; }
    };
    auto bslot = [&](int j) { return j < H2 ? H2 - 1 - j : NSTEP - 1 - j; };      // slot of issue step j of the backward pass
    auto fetch_bwd = [&](int j, double &e) { if (j < NSTEP) e = sw_e[bslot(j) * 8 + (oEN - oEF)]; };
#pragma unroll
    for (int i = 0; i < PD; i++) fetch_fwd(i, rq[i], eq[i]);
    double vprev = 0.0;
#pragma unroll
    for (int i = 0; i < NSTEP; i++) {
      if (i == HS) {
        // rows 2 and 3 take over the vector of their lanes in the LOWER half; rows 0 and 1 start again from 0.  The first
        // operand of the swap is that 0: its upper half receives the vector, its lower half stays.  (vprev itself is dead:
        // both row pairs write vs[] again in the second half.)
        double sx = (SL & 4) ? 0.0 : vprev, sy = vprev;
        lane_swap<32>(sx, sy);
        vprev = (SL & 4) ? sx : (half ? sx : 0.0);
      }
      const int s = i < HS ? i : i - HS;
      const double rr = rq[i % PD], ee = eq[i % PD];
      fetch_fwd(i + PD, rq[i % PD], eq[i % PD]);
      const double w = __builtin_fma(-ee, vprev, rr);
      vprev = wv_matvec<BS, true, (SL & 1) != 0>(0.0, w, gr[s]);
      vs[s] = vprev;
    }
    const double emk = lds[oEM + k8], vlast = vprev;
    // the middle block needs the last vector of both chains: row 2 holds chain A's, row 3 chain B's
    double vA, vB;
    wv_meet<(SL & 4) != 0>(vlast, chain, vA, vB);
    // (slot NSTEP % PD of the ring holds the middle block's right-hand side and coupling)
    const double rm = rq[NSTEP % PD], em_ = eq[NSTEP % PD];
#pragma unroll
    for (int j = 0; j < PD; j++) fetch_bwd(j, eb[j]);
    double w = __builtin_fma(-em_, vA, rm);
    w = __builtin_fma(-emk, vB, w);
    double xn = wv_matvec<BS, true, (SL & 1) != 0>(0.0, w, gmd);
    double xmid = xn;
#pragma unroll
    for (int j = 0; j < NSTEP; j++) {
      if (j == H2) {
        // rows 0 and 1 take over the vector of their lanes in the UPPER half; rows 2 and 3 start again from the middle
        // block.  The second operand of the swap is the middle block's x~: its lower half receives the vector, its upper
        // half stays -- and is still the middle block's x~ for the store of row 2 below.  (xn itself is dead: both row pairs
        // write xs[] again in the second half.)
        double sx = xn, sy = (SL & 4) ? xmid : xn;
        lane_swap<32>(sx, sy);
        xn = (SL & 4) ? sy : (half ? xmid : sy);
        if (SL & 4) xmid = sy;
      }
      const int s = bslot(j);
      const double ee = eb[j % PD];
      fetch_bwd(j + PD, eb[j % PD]);
      const double u = -(ee * xn);
      xn = wv_matvec<BS, false, (SL & 1) != 0>(vs[s], u, gr[s]);
      xs[s] = xn;
    }
    if (sw_store) {
#pragma unroll
      for (int s = 0; s < HS; s++) sw_v[s * 2 + (oXT - oR)] = xs[s];
      if (srow == 2) md_v[oXT - oR] = xmid;
    }
    WV_SYNC();
  };
  auto sweep = [&]() { if constexpr (GRES) sweep_res(); else sweep_lds(); };

  if ((EXT & 1) && a.warm && !resume) {
    // OSQP-style warm start from the previous solution of this handle (x, y unscaled in a.x / a.y), the formulas of the
    // row-local kernel:  x_s = x / D,  y_s = c y / (E w),  z = A_s x_s  (w: wc on the hinge rows, x_w on an extra row, 1 on
    // the bound and box rows -- the value test).  The block's x goes through its vector in LDS: every lane of the block
    // forms the products of its hinge rows from it.  rows(MODE 0) then builds the right-hand side as after a resume.
    const double *Dg = a.D + (size_t)b * n, *Eg = a.E + (size_t)b * m;
    const double *xg = a.x + (size_t)b * n, *yg = a.y + (size_t)b * m;
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const int var = tab0[(oVVAR + v) * 64 + lane], r0 = tab0[(oVROW + v) * 64 + lane];
      v_x[v] = var >= 0 ? xg[var] / Dg[var] : 0.0;
      v_z[v] = v_a[v] * v_x[v];
      v_y[v] = r0 >= 0 ? yg[r0] * cscale / Eg[r0] : 0.0;
      v_p[v][oXC - oXT] = v_x[v];                  // (a lane without a variable: a zero into the dummy block)
    }
    WV_SYNC();
    if (x_row >= 0) { x_z = x_a * x_p[oXC - oXT]; x_y = yg[x_row] * cscale / (Eg[x_row] * x_w); }
    if constexpr (LNK > 0) {
#pragma unroll
      for (int v = 0; v < NV; v++) {
        double la[NL1], lh[NL1], ll[NL1], lu[NL1];
        lk.consts(v, la, lh, ll, lu);
#pragma unroll
        for (int s = 0; s < LNK; s++) {
          const int i = v * LNK + s, lr = tab0[(oLROW + i) * 64 + lane];
          lk.z[i] = __builtin_fma(lh[s], lds[oXC + v_pkp[v]], la[s] * v_x[v]);
          lk.y[i] = lr >= 0 ? yg[lr] * cscale / Eg[lr] : 0.0;
        }
      }
    }
    const double *xq = xt_p + (oXC - oXT);
    const d2 a0 = *(const d2 *)xq, a1 = *(const d2 *)(xq + 2 * NPOS), a2 = *(const d2 *)(xq + 4 * NPOS), a3 = *(const d2 *)(xq + 6 * NPOS);
    const double xc[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
#pragma unroll
    for (int q = 0; q < NS; q++) {
      const int h = tab0[(oHROW + q) * 64 + lane], br = tab0[(oHBROW + q) * 64 + lane], ev = tab0[(oHEVAR + q) * 64 + lane];
      double J[8];
      if (JREG) {
#pragma unroll
        for (int k = 0; k < 8; k++) J[k] = hJ[q][k];
      } else {
        const d2 *jp = (const d2 *)(jl_p + q * 512);
        const d2 j0 = jp[0], j1 = jp[64], j2 = jp[128], j3 = jp[192];
        J[0] = j0.x; J[1] = j0.y; J[2] = j1.x; J[3] = j1.y; J[4] = j2.x; J[5] = j2.y; J[6] = j3.x; J[7] = j3.y;
      }
      double s = J[0] * xc[0];
#pragma unroll
      for (int k = 1; k < BS; k++) if (WV_COL(q, k)) s = __builtin_fma(J[k], xc[k], s);
      if (h >= 0) {
        h_xe[q] = xg[ev] / Dg[ev];
        h_z[q] = s + h_ae[q] * h_xe[q]; h_zb[q] = h_ab[q] * h_xe[q];
        h_y[q] = yg[h] * cscale / (Eg[h] * wc); h_yb[q] = yg[br] * cscale / Eg[br];
      }
    }
    WV_SYNC();
  }
  rows(std::integral_constant<int, 0>{});

  int status = 0, iter = it0;
  double pri = 0.0, dua = 0.0;
  double rho_new = 0.0;       // ADAPT: > 0 = park now, this is the rho to continue with
  const int stop = (a.slice > 0 && it0 + a.slice < a.max_iter) ? it0 + a.slice : a.max_iter;
  while (!status && iter < stop && !(ADAPT && rho_new > 0.0)) {
    int next = stop;
    if constexpr (GRES) load_g();
    if (a.check > 0) { next = (iter / a.check + 1) * a.check; if (next > stop) next = stop; }
    while (iter + 2 < next) { iter++; if (!(ablate & 1)) sweep(); if (!(ablate & 2)) rows(std::integral_constant<int, 1>{}); }
    if (iter + 1 < next) { iter++; if (!(ablate & 1)) sweep(); if (!(ablate & 2)) rows(std::integral_constant<int, 1>{}); }
    iter++;
    c_ndy = 0.0; c_lhs = 0.0; c_ndx = 0.0; c_qdx = 0.0;
    sweep(); rows(std::integral_constant<int, 2>{});
    if (ablate & 16) continue;
    // ADAPT, at an update point: the norms of the SCALED iterates that osqp_rho_estimate takes ride along in the test.
    // The estimate uses |z|, |Ax| and |q|, |A'y|, |Px| only through their maxima: four accumulators, not seven
    // (v_pri = |Ax - z|, v_pn = max(|z|, |Ax|), v_dua = |Px + q + A'y|, v_dn = max(|q|, |A'y|, |Px|)).
    const bool adapt_pt = ADAPT && iter % a.ad_interval == 0 && iter < a.max_iter;
    double v_pri = 0.0, v_pn = 0.0, v_dua = 0.0, v_dn = 0.0;
    // ---- termination test (the decisions of sco_admm_check.h) on the structured layout
    for (int approximate = 0; approximate < 2 && !status; approximate++) {
      if (approximate && iter < a.max_iter) break;
      double ea = a.eps_abs, er = a.eps_rel, epi = a.eps_prim_inf, edi = a.eps_dual_inf;
      if (approximate) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
      double w_pri = 0.0, w_pn = 0.0, w_dua = 0.0, w_dn = 0.0;
      // rows of the hinge slots; partial sums of A' (w y) over the block's columns
      {
        const double *xq = xt_p + (oXC - oXT);
        const d2 a0 = *(const d2 *)xq, a1 = *(const d2 *)(xq + 2 * NPOS), a2 = *(const d2 *)(xq + 4 * NPOS), a3 = *(const d2 *)(xq + 6 * NPOS);
        const double xc[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
        double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < NS; q++) {
          double J[8];
          if (JREG) {
#pragma unroll
            for (int k = 0; k < 8; k++) J[k] = hJ[q][k];
          } else {
            const d2 *jp = (const d2 *)(jl_p + q * 512);
            const d2 j0 = jp[0], j1 = jp[64], j2 = jp[128], j3 = jp[192];
            J[0] = j0.x; J[1] = j0.y; J[2] = j1.x; J[3] = j1.y; J[4] = j2.x; J[5] = j2.y; J[6] = j3.x; J[7] = j3.y;
          }
          double s = J[0] * xc[0];
#pragma unroll
          for (int k = 1; k < BS; k++) if (WV_COL(q, k)) s = __builtin_fma(J[k], xc[k], s);
          const double ax = s + h_ae[q] * h_xe[q], axb = h_ab[q] * h_xe[q];
          const double eh = CKH(q, 0), eb = CKH(q, 1), de = CKH(q, 2);
          w_pri = fmax(w_pri, fmax(eh * fabs(ax - h_z[q]), eb * fabs(axb - h_zb[q])));
          w_pn = fmax(w_pn, fmax(eh * fmax(fabs(h_z[q]), fabs(ax)), eb * fmax(fabs(h_zb[q]), fabs(axb))));
          const double wy = wc * h_y[q];
          const double aty = h_ae[q] * wy + h_ab[q] * h_yb[q];
          w_dua = fmax(w_dua, de * fabs(h_q[q] + aty));
          w_dn = fmax(w_dn, de * fmax(fabs(h_q[q]), fabs(aty)));
          if (ADAPT && adapt_pt) {
            v_pri = fmax(v_pri, fmax(fabs(ax - h_z[q]), fabs(axb - h_zb[q])));
            v_pn = fmax(v_pn, fmax(fmax(fabs(h_z[q]), fabs(h_zb[q])), fmax(fabs(ax), fabs(axb))));
            v_dua = fmax(v_dua, fabs(h_q[q] + aty)); v_dn = fmax(v_dn, fmax(fabs(h_q[q]), fabs(aty)));
          }
#pragma unroll
          for (int k = 0; k < BS; k++) if (WV_COL(q, k)) part[k] = __builtin_fma(J[k], wy, part[k]);
        }
        d2 v0, v1, v2, v3;
        v0.x = part[0]; v0.y = part[1]; v1.x = part[2]; v1.y = part[3]; v2.x = part[4]; v2.y = part[5]; v3.x = part[6]; v3.y = BS > 7 ? part[7] : 0.0;
        *(d2 *)part_p = v0; *(d2 *)(part_p + nslot2) = v1; *(d2 *)(part_p + 2 * nslot2) = v2; *(d2 *)(part_p + 3 * nslot2) = v3;
      }
      {
        const double xcv = x_p[oXC - oXT], ax = x_a * xcv, ex = CKX;
        w_pri = fmax(w_pri, ex * fabs(ax - x_z)); w_pn = fmax(w_pn, ex * fmax(fabs(x_z), fabs(ax)));
        if (ADAPT && adapt_pt) { v_pri = fmax(v_pri, fabs(ax - x_z)); v_pn = fmax(v_pn, fmax(fabs(x_z), fabs(ax))); }
        if (x_row >= 0) x_p[oEX - oXT] = x_a * (x_w * x_y);
      }
      // link rows: the partner's share of A'y through the link vector, as in the row phase
      if constexpr (LNK > 0) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
          double ps = 0.0, la[NL1], lh[NL1], ll[NL1], lu[NL1];
          lk.consts(v, la, lh, ll, lu);
#pragma unroll
          for (int s = 0; s < LNK; s++) ps = __builtin_fma(lh[s], lk.y[v * LNK + s], ps);
          lds[oLK + v_pkp[v]] = ps;
        }
      }
      WV_SYNC();
#pragma unroll
      for (int v = 0; v < NV; v++) {
        const double c[5] = {CKV(v, 0), CKV(v, 1), CKV(v, 2), CKV(v, 3), CKV(v, 4)};
        const int vix = (int)(v_p[v] - (lds + oXT)), p = (vix % (2 * NPOS)) >> 1;
        const double dj = c[0], e0 = c[1];
        const double ax = v_a[v] * v_x[v];
        w_pri = fmax(w_pri, e0 * fabs(ax - v_z[v])); w_pn = fmax(w_pn, e0 * fmax(fabs(v_z[v]), fabs(ax)));
        if (ADAPT && adapt_pt) { v_pri = fmax(v_pri, fabs(ax - v_z[v])); v_pn = fmax(v_pn, fmax(fabs(v_z[v]), fabs(ax))); }
        double aty = v_a[v] * v_y[v] + v_p[v][oEX - oXT];
        if constexpr (LNK > 0) {
          const double xp = lds[oXC + v_pkp[v]];
          double la[NL1], lh[NL1], ll[NL1], lu[NL1];
          lk.consts(v, la, lh, ll, lu);
          aty += v_p[v][oLK - oXT];
#pragma unroll
          for (int s = 0; s < LNK; s++) {
            const int i = v * LNK + s;
            const double axl = __builtin_fma(lh[s], xp, la[s] * v_x[v]), el = CKL(i);
            w_pri = fmax(w_pri, el * fabs(axl - lk.z[i])); w_pn = fmax(w_pn, el * fmax(fabs(lk.z[i]), fabs(axl)));
            aty = __builtin_fma(la[s], lk.y[i], aty);
          }
        }
        const double *pp = v_pp[v];
        if (LPB > 0) {
#pragma unroll
          for (int s2 = 0; s2 < LPB; s2++) aty += pp[s2 * 2];
        } else {
          for (int s2 = 0; s2 < lpb; s2++) aty += pp[s2 * 2];
        }
        double px = c[2] * lds[oXC + v_pkm[v]] + c[3] * lds[oXC + v_pkp[v]];
        if (pdense) {
          const double *cd = wv_opaque(cstg0) + (size_t)(wv_cst_v(NS, v) + 5) * 64;
#pragma unroll
          for (int k2 = 0; k2 < BS; k2++) px = __builtin_fma(cd[k2 * 64], lds[oXC + wv_vidx(NPOS, p, k2)], px);
        } else {
          px = __builtin_fma(c[4], v_x[v], px);
        }
        if (v_on[v]) {
          w_dua = fmax(w_dua, dj * fabs(v_q[v] + px + aty));
          w_dn = fmax(w_dn, dj * fmax(fabs(v_q[v]), fmax(fabs(aty), fabs(px))));
          if (ADAPT && adapt_pt) {
            v_dua = fmax(v_dua, fabs(v_q[v] + px + aty));
            v_dn = fmax(v_dn, fmax(fabs(v_q[v]), fmax(fabs(aty), fabs(px))));
          }
        }
      }
      WV_SYNC();       // (the next pass over the rows rewrites the two buffers the test has borrowed)
      w_pri = wv_wmax(w_pri); w_pn = wv_wmax(w_pn); w_dua = wv_wmax(w_dua); w_dn = wv_wmax(w_dn);
      const double ndy = wv_wmax(c_ndy), ndx = wv_wmax(c_ndx), lhs = wv_wsum(c_lhs), qdx = wv_wsum(c_qdx);
      pri = w_pri; dua = cinv * w_dua;
      if (!(pri <= SCO_INFTY) || !(dua <= SCO_INFTY)) { status = SCO_QP_NON_CVX; break; }
      const double eps_p = ea + er * w_pn, eps_d = ea + er * cinv * w_dn;
      const bool prim_ok = (m == 0) || (pri < eps_p), dual_ok = dua < eps_d;
      if (prim_ok && dual_ok) { status = approximate ? SCO_QP_SOLVED_INACCURATE : SCO_QP_SOLVED; break; }
      // The two infeasibility certificates, on the structured layout as well (r04: stiff penalty QPs -- the compounded
      // penalty of quirk Q1 -- meet their cheap preconditions at most checks; as generic loops over the CSC pattern in
      // global memory they cost 8 % of the solve, scripts/gpu_wv_time.py).  Same quantities as osqp_check in sco_admm_check.h:
      //   primal:  || D^-1 A' (w dy) ||inf < eps_prim_inf || E dy ||inf                  (dy clipped to the cone of the bounds)
      //   dual:    || D^-1 P dx ||inf < c eps_dual_inf || D dx ||inf  and no row of E^-1 A dx leaves its finite bounds' cone
      // delta_y / delta_x of the checked iteration are in registers (dsv); column sums go through the two buffers the
      // test above has borrowed already.
      if ((ablate & 64) == 0 && !prim_ok && ndy > epi && lhs < -epi * ndy) {
        double nat = 0.0;
        {
          double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int q = 0; q < NS; q++) {
            double J[8];
            if (JREG) {
#pragma unroll
              for (int k = 0; k < 8; k++) J[k] = hJ[q][k];
            } else {
              const d2 *jp = (const d2 *)(jl_p + q * 512);
              const d2 j0 = jp[0], j1 = jp[64], j2 = jp[128], j3 = jp[192];
              J[0] = j0.x; J[1] = j0.y; J[2] = j1.x; J[3] = j1.y; J[4] = j2.x; J[5] = j2.y; J[6] = j3.x; J[7] = j3.y;
            }
            const double wd = wc * dsv.h[q];
            nat = fmax(nat, CKH(q, 2) * fabs(h_ae[q] * wd + h_ab[q] * dsv.b[q]));      // the slack's column
#pragma unroll
            for (int k = 0; k < BS; k++) if (WV_COL(q, k)) part[k] = __builtin_fma(J[k], wd, part[k]);
          }
          d2 v0, v1, v2, v3;
          v0.x = part[0]; v0.y = part[1]; v1.x = part[2]; v1.y = part[3]; v2.x = part[4]; v2.y = part[5]; v3.x = part[6]; v3.y = BS > 7 ? part[7] : 0.0;
          *(d2 *)part_p = v0; *(d2 *)(part_p + nslot2) = v1; *(d2 *)(part_p + 2 * nslot2) = v2; *(d2 *)(part_p + 3 * nslot2) = v3;
        }
        if (x_row >= 0) x_p[oEX - oXT] = x_a * (x_w * dsv.x);
        if constexpr (LNK > 0) {
#pragma unroll
          for (int v = 0; v < NV; v++) {
            double ps = 0.0, la[NL1], lh[NL1], ll[NL1], lu[NL1];
            lk.consts(v, la, lh, ll, lu);
#pragma unroll
            for (int s = 0; s < LNK; s++) ps = __builtin_fma(lh[s], lk.d[v * LNK + s], ps);
            lds[oLK + v_pkp[v]] = ps;
          }
        }
        WV_SYNC();
#pragma unroll
        for (int v = 0; v < NV; v++) {
          double aty = v_a[v] * dsv.r0[v] + v_p[v][oEX - oXT];
          if constexpr (LNK > 0) {
            double la[NL1], lh[NL1], ll[NL1], lu[NL1];
            lk.consts(v, la, lh, ll, lu);
            aty += v_p[v][oLK - oXT];
#pragma unroll
            for (int s = 0; s < LNK; s++) aty = __builtin_fma(la[s], lk.d[v * LNK + s], aty);
          }
          const double *pp = v_pp[v];
          if (LPB > 0) {
#pragma unroll
            for (int s2 = 0; s2 < LPB; s2++) aty += pp[s2 * 2];
          } else {
            for (int s2 = 0; s2 < lpb; s2++) aty += pp[s2 * 2];
          }
          if (v_on[v]) nat = fmax(nat, CKV(v, 0) * fabs(aty));
        }
        WV_SYNC();
        nat = wv_wmax(nat);
        if ((status = osqp_primal_inf_status(nat, ndy, epi, approximate))) break;
      }
      if ((ablate & 64) == 0 && !dual_ok && ndx > edi && qdx < -cscale * edi * ndx) {
        // delta_x of the core variables takes the place of x in its block vector (the next checked pass rewrites it)
#pragma unroll
        for (int v = 0; v < NV; v++) v_p[v][oXC - oXT] = dsv.var[v];
        WV_SYNC();
        double npx = 0.0;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const double c[5] = {CKV(v, 0), CKV(v, 1), CKV(v, 2), CKV(v, 3), CKV(v, 4)};
          const int vix = (int)(v_p[v] - (lds + oXT)), p = (vix % (2 * NPOS)) >> 1;
          double px = c[2] * lds[oXC + v_pkm[v]] + c[3] * lds[oXC + v_pkp[v]];
          if (pdense) {
            const double *cd = wv_opaque(cstg0) + (size_t)(wv_cst_v(NS, v) + 5) * 64;
#pragma unroll
            for (int k2 = 0; k2 < BS; k2++) px = __builtin_fma(cd[k2 * 64], lds[oXC + wv_vidx(NPOS, p, k2)], px);
          } else {
            px = __builtin_fma(c[4], dsv.var[v], px);
          }
          if (v_on[v]) npx = fmax(npx, c[0] * fabs(px));
        }
        npx = wv_wmax(npx);
        if (npx < cscale * edi * ndx) {
          const double thr = edi * ndx;
          double badv = 0.0;
          const double *xq = xt_p + (oXC - oXT);
          const d2 a0 = *(const d2 *)xq, a1 = *(const d2 *)(xq + 2 * NPOS), a2 = *(const d2 *)(xq + 4 * NPOS), a3 = *(const d2 *)(xq + 6 * NPOS);
          const double dxb[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
#pragma unroll
          for (int q = 0; q < NS; q++) {
            double J[8];
            if (JREG) {
#pragma unroll
              for (int k = 0; k < 8; k++) J[k] = hJ[q][k];
            } else {
              const d2 *jp = (const d2 *)(jl_p + q * 512);
              const d2 j0 = jp[0], j1 = jp[64], j2 = jp[128], j3 = jp[192];
              J[0] = j0.x; J[1] = j0.y; J[2] = j1.x; J[3] = j1.y; J[4] = j2.x; J[5] = j2.y; J[6] = j3.x; J[7] = j3.y;
            }
            double s2 = J[0] * dxb[0];
#pragma unroll
            for (int k = 1; k < BS; k++) if (WV_COL(q, k)) s2 = __builtin_fma(J[k], dxb[k], s2);
            const double adh = CKH(q, 0) * (s2 + h_ae[q] * dsv.e[q]), adb = CKH(q, 1) * (h_ab[q] * dsv.e[q]);
            if (h_on[q] && ((h_u[q] < WV_BIG && adh > thr) || adb < -thr)) badv = 1.0;     // hinge: l = -inf; its slack's bound row: [0, inf)
          }
#pragma unroll
          for (int v = 0; v < NV; v++) {
            const double adx = CKV(v, 1) * (v_a[v] * dsv.var[v]);
            if (v_r0on[v] && ((v_u[v] < WV_BIG && adx > thr) || (v_l[v] > -WV_BIG && adx < -thr))) badv = 1.0;
            if constexpr (LNK > 0) {
              const double dxp = lds[oXC + v_pkp[v]];          // delta_x of the partner (an empty slot: 0 inside [0, 0])
              double la[NL1], lh[NL1], ll[NL1], lu[NL1];
              lk.consts(v, la, lh, ll, lu);
#pragma unroll
              for (int s = 0; s < LNK; s++) {
                const double adl = CKL(v * LNK + s) * __builtin_fma(lh[s], dxp, la[s] * dsv.var[v]);
                if (osqp_row_leaves_cone(adl, ll[s], lu[s], thr)) badv = 1.0;
              }
            }
          }
          if (x_row >= 0) {
            const double adx = CKX * (x_a * x_p[oXC - oXT]);
            if ((x_u < WV_BIG && adx > thr) || (x_l > -WV_BIG && adx < -thr)) badv = 1.0;
          }
          badv = wv_wmax(badv);
          if ((status = osqp_dual_inf_status(badv, approximate))) break;
        }
        WV_SYNC();
#pragma unroll
        for (int v = 0; v < NV; v++) v_p[v][oXC - oXT] = v_x[v];       // x back in its place (the test at max_iter runs twice)
        WV_SYNC();
      }
    }
    if (ADAPT && adapt_pt && !status) {
      const double vs[7] = {wv_wmax(v_pri), wv_wmax(v_pn), 0.0, wv_wmax(v_dua), wv_wmax(v_dn), 0.0, 0.0};    // (maxima of norms: 0 is neutral)
      const double est = osqp_rho_estimate(vs, rho0);
      if (osqp_rho_must_change(est, rho0, a.ad_tol)) rho_new = est;
    }
  }
  if (!status && iter < a.max_iter) {
    if (ADAPT && rho_new > 0.0 && lane == 0) { a.rho_b[b] = rho_new; a.rflag[b] = 1; a.smask[b] = 1; a.nupd[b] += 1; }
    // the slice is used up (or rho changes): park the solve (scaled x, z, y in natural order; t', g_e and the right-hand side are rebuilt
    // from them by the next launch with the same formulas, i.e. bit for bit).  t' and g_e are written too, in the form
    // the row-local kernel resumes from (sco_admm_rl.hip: t'_i = t_i - rw_i a_ie g_e): the SQP loop hands the tail of a
    // step, when fewer problems are alive than this tier needs to fill the chip, to that kernel.
    double *sx = a.sx + (size_t)b * n, *sz = a.sz + (size_t)b * m, *sy = a.sy + (size_t)b * m;
    double *stp = a.st + (size_t)b * m, *sgp = a.sg + (size_t)b * a.n_e;
    const int *tab = wv_opaque(tab0);
#pragma unroll
    for (int q = 0; q < NS; q++) {
      const int h = tab[(oHROW + q) * 64 + lane], br = tab[(oHBROW + q) * 64 + lane], ev = tab[(oHEVAR + q) * 64 + lane];
      if (h >= 0) {
        sz[h] = h_z[q]; sy[h] = h_y[q]; sz[br] = h_zb[q]; sy[br] = h_yb[q]; sx[ev] = h_xe[q];
        const double th = wc * (rho0 * h_z[q] - h_y[q]), tb = rho0 * h_zb[q] - h_yb[q];
        stp[h] = th - (rw * h_ae[q]) * h_ge[q]; stp[br] = tb - (rho0 * h_ab[q]) * h_ge[q];
        sgp[tab[(oHEIDX + q) * 64 + lane]] = h_ge[q];
      }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const int var = tab[(oVVAR + v) * 64 + lane], r0 = tab[(oVROW + v) * 64 + lane];
      if (var >= 0) sx[var] = v_x[v];
      if (r0 >= 0) { sz[r0] = v_z[v]; sy[r0] = v_y[v]; stp[r0] = rho0 * v_z[v] - v_y[v]; }
    }
    if (x_row >= 0) { sz[x_row] = x_z; sy[x_row] = x_y; stp[x_row] = x_w * (x_rho * x_z - x_y); }
    if constexpr (LNK > 0) {
#pragma unroll
      for (int i = 0; i < NLK; i++) {
        const int lr = tab[(oLROW + i) * 64 + lane];
        if (lr >= 0) { sz[lr] = lk.z[i]; sy[lr] = lk.y[i]; stp[lr] = rho0 * lk.z[i] - lk.y[i]; }
      }
    }
    if (lane == 0) { a.prog[b] = iter; a.status[b] = 0; a.iters[b] = iter; atomicAdd(a.it_count, (unsigned long long)(iter - it0)); }
    return;
  }
  if (a.slice > 0 && lane == 0) a.prog[b] = 0;
  if (!status) status = SCO_QP_MAX_ITER_REACHED;
  if (iter > a.max_iter) iter = a.max_iter;
  {
    const double *Dg = a.D + (size_t)b * n, *Eg = a.E + (size_t)b * m;
    double *xo = a.x + (size_t)b * n, *yo = a.y + (size_t)b * m;
    const int *tab = wv_opaque(tab0);
#pragma unroll
    for (int q = 0; q < NS; q++) {
      const int h = tab[(oHROW + q) * 64 + lane], br = tab[(oHBROW + q) * 64 + lane], ev = tab[(oHEVAR + q) * 64 + lane];
      if (h >= 0) {
        xo[ev] = Dg[ev] * h_xe[q];
        yo[h] = cinv * Eg[h] * h_y[q] * wc;
        yo[br] = cinv * Eg[br] * h_yb[q];
      }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const int var = tab[(oVVAR + v) * 64 + lane], r0 = tab[(oVROW + v) * 64 + lane];
      if (var >= 0) xo[var] = Dg[var] * v_x[v];
      if (r0 >= 0) yo[r0] = cinv * Eg[r0] * v_y[v];
    }
    if (x_row >= 0) yo[x_row] = cinv * Eg[x_row] * x_y * x_w;
    if constexpr (LNK > 0) {
#pragma unroll
      for (int i = 0; i < NLK; i++) {
        const int lr = tab[(oLROW + i) * 64 + lane];
        if (lr >= 0) yo[lr] = cinv * Eg[lr] * lk.y[i];
      }
    }
    if (lane == 0) {
      a.status[b] = status; a.iters[b] = iter; a.resid[2 * (size_t)b] = pri; a.resid[2 * (size_t)b + 1] = dua;
      atomicAdd(a.it_count, (unsigned long long)(iter - it0));
    }
  }
}
#undef WV_COL

// ---------------------------------------------------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------------------------------------------------
// The width profile a launch with these settings runs: the plan's, where an instantiation of it exists -- the parity kernel
// and the one that may start warm; adaptive rho keeps the generic kernel (its 7-wide instantiations sit at the register limit
// as they are: wv_gres_fits).  The factor kernel tests the values against the same answer.
// A profiled kernel keeps its Jacobian rows in registers (wv_jreg: a -DWV_JREG=0 build has none and runs the generic one).
static int wv_launch_jw(const WvHost &wh, const AdmmArgs &aa) {
  return (WV_JWIDTH != 0 && wv_jreg(wh.NS, wh.BS) && !aa.adaptive) ? wh.jw_profile : 0;
}

static void wv_fill_args(const AdmmArgs &aa, const WvHost &wh, const WvDev &wd, const int *setup_mask, WvArgs &a) {
  const QpDev &d = aa.d;
  a.n = d.n; a.m = d.m; a.n_e = d.n_e; a.n_c = d.n_c; a.nnzA = d.nnzA; a.nnzP = d.nnzP;
  a.max_iter = aa.max_iter; a.check = aa.check; a.slice = aa.slice; a.b0 = d.b0; a.list = d.list;
  a.bs = wh.bs; a.nb = wh.nb; a.mid = wh.mid; a.lpb = wh.lpb; a.n_extra = wh.n_extra; a.NS = wh.NS; a.NV = wh.NV; a.NSTEP = wh.NSTEP;
  a.cst_slots = wh.cst_slots; a.NL = wh.NL; a.g_doubles = wh.g_doubles;
  a.rho = aa.rho; a.sigma = aa.sigma; a.alpha = aa.alpha; a.eps_abs = aa.eps_abs; a.eps_rel = aa.eps_rel;
  a.eps_prim_inf = aa.eps_prim_inf; a.eps_dual_inf = aa.eps_dual_inf;
  a.tab = wd.tab; a.G = wd.G; a.cst = wd.cst; a.wc = wd.wc; a.scr = wd.scr; a.ok = wd.ok; a.rl_need = wd.rl_need; a.w_ready = wd.w_ready; a.pflag = wd.pflag; a.it_count = wd.it_count;
  a.As = d.As; a.Ps = d.Ps; a.qs = d.qs; a.ls = d.ls; a.us = d.us; a.rhov = d.rho; a.kee_inv = d.kee_inv; a.cscale = d.cscale;
  a.D = d.D; a.E = d.E; a.S = d.W; a.w = d.w; a.active = d.active; a.setup_active = setup_mask;
  a.Ap = d.Ap; a.Ai = d.Ai; a.Rp = d.Rp; a.Rj = d.Rj; a.Rpos = d.Rpos; a.Fp = d.Fp; a.Fi = d.Fi; a.Fpos = d.Fpos;
  a.x = d.x; a.y = d.y; a.resid = d.resid; a.status = d.status; a.iters = d.iters; a.prog = d.prog;
  a.sx = d.sx; a.sz = d.sz; a.sy = d.sy; a.st = d.st; a.sg = d.sg;
  a.warm = aa.warm; a.ad_interval = aa.adaptive ? aa.ad_interval : 0; a.ad_tol = aa.ad_tol;
  // (null without adaptive rho: only the ADAPT instantiation and the factor kernel's value test read them)
  a.rho_b = aa.adaptive ? d.rho_b : nullptr; a.rflag = aa.adaptive ? d.rflag : nullptr;
  a.smask = aa.adaptive ? d.smask : nullptr; a.nupd = aa.adaptive ? d.nupd : nullptr;
  a.jw = wv_launch_jw(wh, aa);
#ifdef WV_ABLATE
  { const char *ab = getenv("SCO_WV_ABLATE"); a.ablate = ab ? atoi(ab) : 0; }
#else
  a.ablate = 0;
#endif
}

// need[b] = the problem starts a QP, or it is active on a QP the wavefront tier factored (W buffer still holds S)
__global__ void qp_wv_need_kernel(int b0, const int *list, int nb, const int *setup_mask, const int *active, int *w_ready, int *need) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nb) return;
  const int b = list ? list[g + b0] : g + b0;
  if (b < 0) return;
  const int nd = (setup_mask ? setup_mask[b] != 0 : 1) || ((!active || active[b]) && !w_ready[b]);
  need[b] = nd;
  if (nd) w_ready[b] = 1;
}

int wv_launch_need(const AdmmArgs &aa, const int *setup_mask, const WvDev &wd, hipStream_t st) {
  const int nwg = qp_launch_nwg(aa.d);
  hipLaunchKernelGGL(qp_wv_need_kernel, dim3((nwg + 255) / 256), dim3(256), 0, st, aa.d.b0, aa.d.list, nwg, setup_mask, aa.d.active,
                     wd.w_ready, wd.rl_need);
  SCO_HIP(hipGetLastError());
  return SCO_OK;
}

int wv_launch_factor(const AdmmArgs &aa, const int *setup_mask, const WvHost &wh, const WvDev &wd, hipStream_t st) {
  WvArgs a; wv_fill_args(aa, wh, wd, setup_mask, a);
  const int nwg = qp_launch_nwg(aa.d);
  if (wh.NL) hipLaunchKernelGGL(qp_wv_factor_kernel<WV_NL>, dim3(nwg), dim3(WV_T), 0, st, a);
  else hipLaunchKernelGGL(qp_wv_factor_kernel<0>, dim3(nwg), dim3(WV_T), 0, st, a);
  SCO_HIP(hipGetLastError());
  return SCO_OK;
}

template <int BS, int NS, int NV, int NSTEP, int LPB, int EXT, int LNK, int JW = 0>
static int wv_launch_k(const WvArgs &a, int nwg, size_t lds, hipStream_t st) {
  static bool attr_done[64] = {};
  SCO_LDS_ATTR((qp_admm_wv_kernel<BS, NS, NV, NSTEP, LPB, EXT, LNK, JW>), 64 * 1024, attr_done);
  hipLaunchKernelGGL((qp_admm_wv_kernel<BS, NS, NV, NSTEP, LPB, EXT, LNK, JW>), dim3(nwg), dim3(WV_T), lds, st, a);
  SCO_HIP(hipGetLastError());
  return SCO_OK;
}

template <int BS, int NS, int NV, int NSTEP, int LPB, int JW = 0>
static int wv_launch_one(const WvArgs &a, int nwg, size_t lds, hipStream_t st) {
  // a width profile: a link-free plan with fixed rho (wv_plan_widths, wv_launch_jw), cold or warm
  if constexpr (JW != 0) return a.warm ? wv_launch_k<BS, NS, NV, NSTEP, LPB, 1, 0, JW>(a, nwg, lds, st) : wv_launch_k<BS, NS, NV, NSTEP, LPB, 0, 0, JW>(a, nwg, lds, st);
  // parity mode runs the instantiation without any code of the extensions; the adaptive one can start warm as well
  // (a plan with link rows has no adaptive instantiation: qp_launch_plan keeps such launches on the row-local kernel)
  if (a.NL) {
    // (nor one with compile-time lanes per block: wv_launch)
    if (LPB > 0 || a.ad_interval > 0) { sco_set_error("wv_launch: no instantiation with link rows for this launch"); return SCO_ERR_STATE; }
    // (the 7-wide parity instantiation with link rows, <7,4,3,10,0,0,2>, comes out with 28 B of scratch where the one that
    // may start warm has none: a cold launch runs on that one, which then takes the same path, a.warm = 0)
    if constexpr (LPB == 0 && BS == 7) return wv_launch_k<BS, NS, NV, NSTEP, LPB, 1, WV_NL>(a, nwg, lds, st);
    else if constexpr (LPB == 0) return a.warm ? wv_launch_k<BS, NS, NV, NSTEP, LPB, 1, WV_NL>(a, nwg, lds, st) : wv_launch_k<BS, NS, NV, NSTEP, LPB, 0, WV_NL>(a, nwg, lds, st);
  }
  if (a.ad_interval > 0) return wv_launch_k<BS, NS, NV, NSTEP, LPB, 3, 0>(a, nwg, lds, st);
  return a.warm ? wv_launch_k<BS, NS, NV, NSTEP, LPB, 1, 0>(a, nwg, lds, st) : wv_launch_k<BS, NS, NV, NSTEP, LPB, 0, 0>(a, nwg, lds, st);
}

int wv_launch(const AdmmArgs &aa, const WvHost &wh, const WvDev &wd, hipStream_t st) {
  WvArgs a; wv_fill_args(aa, wh, wd, nullptr, a);
  const int nwg = qp_launch_nwg(aa.d);
  // the LDS request also fixes how many problems share a CU: at most 4 (one wavefront per SIMD)
  const size_t lds = std::max(wh.lds_bytes, (size_t)36 * 1024);      // (36 KB: never a fifth workgroup on a CU)
  // (link rows at three lanes per block run on the run-time-lpb instantiation: <7,4,3,10,3> with link rows needs scratch,
  // profiles/wv_link_rows.md)
  if (wh.NSTEP == 10 && wh.NS == 4 && wh.lpb == 3 && !wh.NL) {                                                          // 7-DOF, 17 .. 20 timesteps
    // The width profiles of this kernel: one instantiation pair (cold, warm) per line of WV_JW_PROFILES (layout_wv.h), the one
    // table the planner picks from (wv_plan_widths) and this switch is made of.  To add a profile, add its line there, then
    // read the compiler's resource report for the two new kernels (-Rpass-analysis=kernel-resource-usage): no scratch, the
    // occupancy of the generic twin, no more accumulation registers than it -- else the plans it would take stay generic.
    if constexpr (wv_jreg(4, 7)) {
      switch (a.jw) {
#define X(w0, w1, w2, w3) case WV_JW_PACK(w0, w1, w2, w3): return wv_launch_one<7, 4, 3, 10, 3, WV_JW_PACK(w0, w1, w2, w3)>(a, nwg, lds, st);
        WV_JW_PROFILES(X)
#undef X
        default: break;
      }
    }
    if (a.jw) { sco_set_error("wv_launch: no instantiation of the plan's width profile"); return SCO_ERR_STATE; }
    return wv_launch_one<7, 4, 3, 10, 3>(a, nwg, lds, st);
  }
  if (a.jw) { sco_set_error("wv_launch: no instantiation of the plan's width profile"); return SCO_ERR_STATE; }
  if (wh.NSTEP == 10 && wh.NS == 4) return wv_launch_one<7, 4, 3, 10, 0>(a, nwg, lds, st);
  if (wh.NSTEP == 10) return wv_launch_one<8, 2, 2, 10, 0>(a, nwg, lds, st);
  if (wh.NSTEP == 4) return wv_launch_one<8, 1, 1, 4, 0>(a, nwg, lds, st);
  return wv_launch_one<8, 2, 2, 8, 0>(a, nwg, lds, st);
}
