// sco_admm_check.h -- what every ADMM kernel tier shares: the workgroup reductions and OSQP's termination
// test (check_termination of osqp 0.6 as restated by oracle/osqp_ref.c: convergence, the primal and dual
// infeasibility certificates, the 10x "approximate" pass at max_iter) with the adaptive-rho estimate.
//
//   * the workgroup reduction block_reduce / block_reduce_sm, used by every tier and by sco_sqp.hip (what happens
//     inside a wavefront is sco_lanes.h);
//   * OSQP's decisions on scalars (no memory access): OsqpTol, osqp_clip_dy, the bound predicates, osqp_converged,
//     the certificates' status choice, osqp_rho_estimate / osqp_rho_must_change;
//   * osqp_check: the decision tree and the order of its reductions for the kernels that walk rows and columns with
//     loops (sco_qp.hip, sco_qp_big.hip).  A kernel hands in an `Ops` object that says how a thread reaches its rows,
//     columns and dot products.
// The kernels that keep rows and columns in registers write the test on those registers.  sco_admm_fast.hip and
// sco_admm_reg.hip follow the skeleton of osqp_check statement by statement (instantiating it cost them registers and
// scratch) with the reductions and the scalar helpers; fast alone spells out the convergence decision (osqp_converged
// adds scratch to five of its instantiations).  sco_admm_rl.hip and sco_admm_wv.hip fuse the reductions of the test
// and take what leaves their machine code as it was: rl the reductions, wv the bound predicates and the
// certificates' status choice.  profiles/r08_check_refactor_resources.txt has the measurements.
//
// Everything here is __device__ __forceinline__: no translation unit of its own, no ABI.
#pragma once
#include "sco_internal.h"
#include "sco_lanes.h"

// --------------------------------------------------------------------------
// reductions.  Fixed trees and orders: results are run-to-run deterministic.
// --------------------------------------------------------------------------
// Sums of v[0 .. NS) and maxima of v[NS .. NS + NM) over a workgroup of NWAVES wavefronts; every thread gets the
// results.  `red` is NWAVES * (NS + NM) doubles of LDS; the first barrier protects it against a previous use.  Across
// the wavefronts the partial results combine in the order red[0], red[1], ...  DPP_MAX: maxima by wave_scan63 (lane 63
// publishes, and NS must be 0) instead of the shuffles (lane 0); sums always go through the shuffles.
template <int NS, int NM, int NWAVES, bool DPP_MAX = false>
__device__ __forceinline__ void block_reduce_sm(double (&v)[NS + NM], double *red) {
  static_assert(!DPP_MAX || NS == 0, "one lane publishes: 63 for the DPP maxima, 0 for the shuffles");
  constexpr int NR = NS + NM;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; k++) v[k] = wave_sum(v[k]);
#pragma unroll
  for (int k = NS; k < NR; k++) v[k] = DPP_MAX ? wave_scan63<true>(v[k]) : wave_max(v[k]);
  __syncthreads();
  if (lane == (DPP_MAX ? 63 : 0)) {
#pragma unroll
    for (int k = 0; k < NR; k++) red[wv * NR + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NR; k++) {
    double r = red[k];
#pragma unroll
    for (int w = 1; w < NWAVES; w++) {
      const double o = red[w * NR + k];
      r = k < NS ? r + o : fmax(r, o);
    }
    v[k] = r;
  }
}
// NR values of one kind
template <int NR, bool IS_MAX, int NWAVES, bool DPP_MAX = false>
__device__ __forceinline__ void block_reduce(double (&v)[NR], double *red) {
  block_reduce_sm<IS_MAX ? 0 : NR, IS_MAX ? NR : 0, NWAVES, IS_MAX && DPP_MAX>(v, red);
}

__device__ __forceinline__ double limit_scaling(double v) {
  v = v < SCO_MIN_SCALING ? 1.0 : v;
  return v > SCO_MAX_SCALING ? SCO_MAX_SCALING : v;
}

// --------------------------------------------------------------------------
// OSQP's decisions on scalars
// --------------------------------------------------------------------------
struct OsqpTol { double ea, er, epi, edi; };     // eps_abs, eps_rel, eps_prim_inf, eps_dual_inf
// From the fields of AdmmArgs / BigArgs.  The approximate test at max_iter runs on ten times every tolerance.
__device__ __forceinline__ OsqpTol osqp_tol(double eps_abs, double eps_rel, double eps_prim_inf, double eps_dual_inf, int approximate) {
  OsqpTol t{eps_abs, eps_rel, eps_prim_inf, eps_dual_inf};
  if (approximate) { t.ea *= 10; t.er *= 10; t.epi *= 10; t.edi *= 10; }
  return t;
}

// a bound of the SCALED problem counts as infinite beyond SCO_INFTY * SCO_MIN_SCALING
__device__ __forceinline__ bool upper_is_infinite(double u) { return u > SCO_INFTY * SCO_MIN_SCALING; }
__device__ __forceinline__ bool lower_is_infinite(double l) { return l < -SCO_INFTY * SCO_MIN_SCALING; }

// delta_y projected on the cone of the bounds: no upper bound -> dy <= 0, no lower bound -> dy >= 0, neither -> 0
__device__ __forceinline__ double osqp_clip_dy(double dy, double l, double u) {
  if (upper_is_infinite(u)) {
    if (lower_is_infinite(l)) dy = 0.0; else dy = fmin(dy, 0.0);
  } else if (lower_is_infinite(l)) dy = fmax(dy, 0.0);
  return dy;
}

// Convergence.  pri, dua: unscaled residual norms (dua with the cost scaling taken out); pscale, dscale: the largest
// of the norms each is relative to (dscale still carries the cost scaling).  Returns a final status, or 0 = go on
// to the certificate of every residual that is not small (prim_ok / dual_ok).
__device__ __forceinline__ int osqp_converged(double pri, double dua, double pscale, double dscale, double cinv, int m,
                                              const OsqpTol &t, int approximate, bool &prim_ok, bool &dual_ok) {
  prim_ok = dual_ok = false;
  if (!(pri <= SCO_INFTY) || !(dua <= SCO_INFTY)) return SCO_QP_NON_CVX;
  const double eps_p = t.ea + t.er * pscale;
  const double eps_d = t.ea + t.er * cinv * dscale;
  prim_ok = (m == 0) || (pri < eps_p);
  dual_ok = dua < eps_d;
  if (prim_ok && dual_ok) return approximate ? SCO_QP_SOLVED_INACCURATE : SCO_QP_SOLVED;
  return 0;
}
// Primal infeasibility, last condition: nat = || D^-1 A' (w dy) ||inf against ndy = || E dy ||inf
__device__ __forceinline__ int osqp_primal_inf_status(double nat, double ndy, double epi, int approximate) {
  if (nat < epi * ndy) return approximate ? SCO_QP_PRIMAL_INFEASIBLE_INACCURATE : SCO_QP_PRIMAL_INFEASIBLE;
  return 0;
}
// Dual infeasibility: row i of adx = E^-1 A dx must stay in the cone of its finite bounds (thr = eps_dual_inf || D dx ||inf) ...
// (A bound is finite here when it lies strictly inside the limit: not the negation of upper_is_infinite /
// lower_is_infinite, which differs for a bound equal to the limit and for a NaN.  OSQP has both forms; keep both.)
__device__ __forceinline__ bool osqp_row_leaves_cone(double adx, double l, double u, double thr) {
  return (u < SCO_INFTY * SCO_MIN_SCALING && adx > thr) || (l > -SCO_INFTY * SCO_MIN_SCALING && adx < -thr);
}
// ... and, last condition, no row may leave it (bad = 1.0 where one does, maximum over the rows)
__device__ __forceinline__ int osqp_dual_inf_status(double bad, int approximate) {
  if (bad == 0.0) return approximate ? SCO_QP_DUAL_INFEASIBLE_INACCURATE : SCO_QP_DUAL_INFEASIBLE;
  return 0;
}

// OSQP's rho estimate (compute_rho_estimate of osqp 0.6, as recalled; the library is not available here, see
// oracle/osqp_ref.c) from the infinity norms of the SCALED iterates,
//   v = |Ax - z|, |z|, |Ax|, |Px + q + A'y|, |q|, |A'y|, |Px|:
//   rho sqrt( (v0 / (max(v1, v2) + 1e-10)) / (v3 / (max(v4, v5, v6) + 1e-10) + 1e-10) )  clipped to [SCO_RHO_MIN, 1e6]
__device__ __forceinline__ double osqp_rho_estimate(const double (&v)[7], double rho) {
  const double pri = v[0] / (fmax(v[1], v[2]) + 1e-10);
  const double dua = v[3] / (fmax(v[4], fmax(v[5], v[6])) + 1e-10);
  return fmin(fmax(rho * sqrt(pri / (dua + 1e-10)), SCO_RHO_MIN), 1e6);
}
// rho changes (the solve parks, setup refactors) only when the estimate leaves [rho / tol, rho tol]
__device__ __forceinline__ bool osqp_rho_must_change(double est, double rho, double tol) {
  return est > rho * tol || est < rho / tol;
}

// --------------------------------------------------------------------------
// the termination test of the tiers that make one block reduction per norm
// --------------------------------------------------------------------------
// One pass of the test on the iterate (x, z, y) with delta_x, delta_y of the same iteration; all threads of the
// workgroup take part and return the same value: 0 = keep iterating, otherwise an SCO_QP_* status.  pri / dua get
// the residual norms.
//
// Ops (r: a row handle, c: a column handle, whatever the tier iterates over):
//   rows(f) / cols(f)        call f(r) / f(c) for the calling thread's rows / columns, in a fixed order
//   Ax(r) Adx(r)             row r of A x, A dx
//   l(r) u(r) w(r) z(r) E(r) bounds, row weight (0 / 1 as a double), z and the row scaling
//   dy(r) set_dy(r, v)       delta_y (the test leaves the clipped value there)
//   Px(c) Pdx(c) Aty(c)      column c of P x, P dx, A' (w y); the term order of Aty is the tier's own and differs from the
//                            one of its rho estimate (a (y w) here, a (w y) there), which is why the sums live in Ops
//   Atdy(c)                  column c of A' (w dy) with the clipped dy
//   q(c) D(c) dx(c)          cost, column scaling, delta_x
template <int NWAVES, class Ops>
__device__ __forceinline__ int osqp_check(Ops &o, const OsqpTol &t, int approximate, int m, double cscale, double *red,
                                          double &pri, double &dua) {
  const double cinv = 1.0 / cscale;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  o.rows([&](auto r) __attribute__((always_inline)) {      // primal residual and its scale
    const double ax = o.Ax(r), z = o.z(r), ei = 1.0 / o.E(r);
    v[0] = fmax(v[0], fabs(ei * (ax - z))); v[1] = fmax(v[1], fabs(ei * z)); v[2] = fmax(v[2], fabs(ei * ax));
  });
  o.cols([&](auto c) __attribute__((always_inline)) {      // dual residual and its scale
    const double px = o.Px(c), aty = o.Aty(c), q = o.q(c), dj = 1.0 / o.D(c);
    v[3] = fmax(v[3], fabs(dj * (q + px + aty))); v[4] = fmax(v[4], fabs(dj * q));
    v[5] = fmax(v[5], fabs(dj * aty)); v[6] = fmax(v[6], fabs(dj * px));
  });
  block_reduce<7, true, NWAVES>(v, red);
  pri = v[0]; dua = cinv * v[3];
  bool prim_ok, dual_ok;
  if (const int st = osqp_converged(pri, dua, fmax(v[1], v[2]), fmax(v[4], fmax(v[5], v[6])), cinv, m, t, approximate, prim_ok, dual_ok))
    return st;
  if (!prim_ok) {           // primal infeasibility certificate from delta_y
    double r1[1] = {0.0};
    o.rows([&](auto r) __attribute__((always_inline)) {
      const double dy = osqp_clip_dy(o.dy(r), o.l(r), o.u(r));
      o.set_dy(r, dy);
      r1[0] = fmax(r1[0], fabs(o.E(r) * dy));
    });
    block_reduce<1, true, NWAVES>(r1, red);
    const double ndy = r1[0];
    if (ndy > t.epi) {
      double lhs[1] = {0.0};
      o.rows([&](auto r) __attribute__((always_inline)) {
        const double dy = o.dy(r);
        lhs[0] += o.w(r) * (o.u(r) * fmax(dy, 0.0) + o.l(r) * fmin(dy, 0.0));
      });
      block_reduce<1, false, NWAVES>(lhs, red);
      if (lhs[0] < -t.epi * ndy) {
        double nat[1] = {0.0};
        o.cols([&](auto c) __attribute__((always_inline)) { nat[0] = fmax(nat[0], fabs(o.Atdy(c) / o.D(c))); });
        block_reduce<1, true, NWAVES>(nat, red);
        if (const int st = osqp_primal_inf_status(nat[0], ndy, t.epi, approximate)) return st;
      }
    }
  }
  if (!dual_ok) {           // dual infeasibility certificate from delta_x
    double r1[1] = {0.0};
    o.cols([&](auto c) __attribute__((always_inline)) { r1[0] = fmax(r1[0], fabs(o.D(c) * o.dx(c))); });
    block_reduce<1, true, NWAVES>(r1, red);
    const double ndx = r1[0];
    if (ndx > t.edi) {
      double qdx[1] = {0.0};
      o.cols([&](auto c) __attribute__((always_inline)) { qdx[0] += o.q(c) * o.dx(c); });
      block_reduce<1, false, NWAVES>(qdx, red);
      if (qdx[0] < -cscale * t.edi * ndx) {
        double npx[1] = {0.0};
        o.cols([&](auto c) __attribute__((always_inline)) { npx[0] = fmax(npx[0], fabs(o.Pdx(c) / o.D(c))); });
        block_reduce<1, true, NWAVES>(npx, red);
        if (npx[0] < cscale * t.edi * ndx) {
          double bad[1] = {0.0};
          o.rows([&](auto r) __attribute__((always_inline)) {
            if (osqp_row_leaves_cone(o.Adx(r) / o.E(r), o.l(r), o.u(r), t.edi * ndx)) bad[0] = 1.0;
          });
          block_reduce<1, true, NWAVES>(bad, red);
          if (const int st = osqp_dual_inf_status(bad[0], approximate)) return st;
        }
      }
    }
  }
  return 0;
}

// The test as an ADMM loop calls it after iteration `iter`: once, and at max_iter a second time on ten times the
// tolerances when the first pass came back empty.
template <int NWAVES, class Args, class Ops>
__device__ __forceinline__ int osqp_check_at(Ops &o, const Args &a, int iter, int m, double cscale, double *red,
                                             double &pri, double &dua) {
  int status = 0;
  for (int approximate = 0; approximate < 2 && !status; approximate++) {
    if (approximate && iter < a.max_iter) break;
    const OsqpTol t = osqp_tol(a.eps_abs, a.eps_rel, a.eps_prim_inf, a.eps_dual_inf, approximate);
    status = osqp_check<NWAVES>(o, t, approximate, m, cscale, red, pri, dua);
  }
  return status;
}
