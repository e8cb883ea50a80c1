// sco_sqp.hip -- device-resident penalty-SQP loop for a batch of trajectory
// problems (SQP layer of libsco_hip).
//
// Per problem this is Solver.solve(prob, method="penalty_sqp") of the reference
// (/root/reference/sco_py/sco_osqp/solver.py:30-253) together with the Prob methods
// it drives (prob.py:369-652), restated as a per-problem state machine so that a
// whole batch advances in lock-step "rounds", one QP solve per active problem per
// round:
//
//   round 0   projection QP           find_closest_feasible_point (prob.py:369-412)
//   round r   sqp_pre_kernel          convexify (prob.py:522-544, expr.py:130-142,
//                                     353-371) with finite-difference Jacobians
//                                     (expr.py:61-69), update_obj (prob.py:414-512,
//                                     incl. quirks Q1/Q2), get_value (prob.py:571-579),
//                                     save (prob.py:639-645), add_trust_region
//                                     (variable.py:37-45), all written straight into the
//                                     QP value arrays (no dense P/A as in
//                                     osqp_utils.py:146-193)
//             qp setup + ADMM         sco_qp.hip
//             sqp_post_kernel         get_approx_value / get_value (prob.py:605-630,
//                                     571-579), the accept / shrink / converge decisions
//                                     (solver.py:151-251), penalty escalation
//                                     (solver.py:84-105)
//
// One workgroup of 256 threads per problem; problems are independent, so there is
// no inter-workgroup communication.  The host only reads one "active problems"
// counter per round.
//
// This file holds the round kernels, the handle, the loaders and the round loop.  What a row or an objective term of a
// family IS (value, gradient, violation) lives in sqp_rows.h; which descriptors and programs are accepted, every
// dimension, the QP patterns and the position tables are host arithmetic in sqp_layout.{h,cpp}.
#include "sco_admm_check.h"
#include "sqp_layout.h"
#include "sqp_rows.h"
#include "sqp_sched.h"

#include <algorithm>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

enum { ST_PROJECT = 0, ST_CONVEXIFY = 1, ST_TRIAL = 2, ST_DONE = 3 };
enum { STEP_PROJECT = 0, STEP_ACCEPT = 1, STEP_SHRINK = 2, STEP_YCONV = 3, STEP_XCONV = 4, STEP_BAD = 5, STEP_GROUP = 6 };

#define TRACE_W 8

struct SqpScalars {
  double penalty, trust, slack_cost, merit, merit_viol;
  long long admm_iters;
  int state, k, sqp_iters, qp_solves, success, escalations, n_trace, spawned;
  int flags;      // SCO_SQP_FLAG_*
};

// Events of a handle: created on demand behind a cursor, handed out in the same order by every solve, destroyed with the
// handle.
struct EventPool {
  std::vector<hipEvent_t> ev;
  size_t cur = 0;
  unsigned flags = hipEventDefault;
  int next(hipEvent_t *out) {
    if (cur == ev.size()) { hipEvent_t e; SCO_HIP(hipEventCreateWithFlags(&e, flags)); ev.push_back(e); }
    *out = ev[cur++];
    return SCO_OK;
  }
  void rewind() { cur = 0; }
  void destroy() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); cur = 0; }
};

struct SqpDev {
  int b0;            // launch window of a stream group: workgroup g of the round kernels works on problem b0 + g
  int batch, d, T, K, O, R, n_x, n_slack, n, m_lin, m_nl, m, prox_count, analytic_jac, trace_cap;
  // SCO_FAM_ARM_REACH: NE = 2 equality rows (end-effector x, y) on the last timestep, block index T;
  // NB = number of constraint blocks (T or T + 1), RM = widest block (history strides)
  int NE, NB, RM;
  // constraint blocks of the state families: block t covers the S (span) timesteps t .. t + S - 1, its state is the
  // ds = S d numbers x[t d .. t d + ds) (consecutive timesteps are contiguous), there are NBt = T - S + 1 of them, and the
  // last Req of a block's R rows are equalities (r03).  Arm / point families: S = 1, ds = d, NBt = T, Req = 0.
  int S, ds, NBt, Req;
  int point;         // RowFamily (sqp_layout.h): which model the non-linear rows follow
  double *qQ, *qa, *qc;   // ROWS_QUADRATIC: [B][O][d*d], [B][O][d], [B][O]
                     // ROWS_PROGRAM: words, row starts and constants (shared), parameters per problem
  const int *pw, *pptr; const double *pconst; const double *ppar; int n_par;
  int R1;            // r04 (SCO_FAM_STATE_PROGRAM): the first R1 rows of a block are keep-out rows of the point (x[0], x[1]) against
                     // obstacles[b][0 .. R1) as in SCO_FAM_POINT_CIRCLES -- a SECOND kind of non-linear rows on the same Variable
                     // (sco_sqp_set_circle_rows); programs supply the remaining O - R1 rows
  int par_step;      // r04: 0 = one parameter vector per problem; n_par = one per problem AND timestep (sco_sqp_load_program_steps:
                     // block t and the objective term of timestep t read params[problem][t])
  int acc;                // r04 (SCO_FAM_FLAG_ACC_COST): P holds the second super-diagonal block too
  const double *accw;     // r04: [B][d] weights of the acceleration term sum_t sum_j a_j (x[t+2][j] - 2 x[t+1][j] + x[t][j])^2, nullptr = all 0
  const double *objw;     // r04: [B][d] weights of the smoothing objective sum_t sum_j w_j (x[t+1][j] - x[t][j])^2, nullptr = all 1
  // linear rows: m_pin pins (start, and goal unless reach), then m_vel velocity-limit rows, then m_jl joint-limit
  // rows (theta <= hi for every trajectory variable, then -theta <= -lo)
  int m_pin, m_vel, m_jl;
  // r04: m_gen GENERAL affine rows behind them (a shared CSR pattern over the trajectory variables, values and right-hand
  // sides per problem: sco_sqp_create_rows / sco_sqp_load_linear_rows): row r is an equality (gen_eq[r]) a x = rhs or an
  // inequality a x <= rhs; gpos0 / gpos1: where entry k of the pattern sits in the A values of the projection / penalty QP
  int m_gen, nnz_gen;
  const int *gen_eq, *gpos0, *gpos1;
  const double *gen_rhs, *gen_val;      // [B][m_gen], [B][nnz_gen]
  // SCO_FAM_FLAG_EE_COST: non-quadratic objective term weight * ||ee(theta_t) - target||^2 per timestep, convexified to
  // degree 2 every SQP iteration (expr.py:143-153): oH = Hessian after the eigenvalue shift, oA, ob = the model's
  // linear and constant part; ppos = position in qp1's P values of entry (row (t, 0), column (t, j))
  int cost;          // ObjKind (sqp_layout.h)
  double *cw, *ctgt, *oH, *oA, *ob;   // [B], [B][2], [B][NO][dO*dO], [B][NO][dO], [B][NO] (NO, dO = T, d or NBt, ds)
  const int *ppos;                    // [n_x]; OBJ_BLOCK: entry (r, c) of the dense band sits at ppos[c] + r
  const double *a0c, *a1c;      // constant parts of the A values of the projection / penalty QP (shared)
  double *vmax;                 // [B]
  double *jlo, *jhi;            // [B][d]
  // problem data
  double *x0, *start, *goal, *link_len, *obstacles, *target;   // [B][...]
  const int *point_link; const double *point_frac;    // [K]
  // SCO_FAM_ARM_SPATIAL (sco_sqp_load_spatial): joint offsets and unit axes, link points and their radii, sphere obstacles
  double *sp_off, *sp_axis, *sp_pos, *sp_rad, *sp_sph;   // [B][d][3], [B][d][3], [B][K][3], [B][K], [B][O][4]
  // SQP state
  double *x, *x_saved, *gsave, *J, *bmod, *trace;
  unsigned char *mask;
  SqpScalars *sc;
  int *active, *n_active;
  int *newqp;        // [B] 1 = this round's pre kernel prepared a new QP for the problem (setup mask)
  const int *list;   // [B] or null: workgroup g of a round kernel works on problem list[g] (< 0: none) -- the problems
                     // sqp_select_kernel lets take part in this round; the others are not visited at all
  int *list_buf;     // [B] storage of `list`
  const int *jpos;   // [T*d] CSC position of J[t][0][j] in qp1's A values
  const int *epos;   // [d]   CSC position of the first equality-row entry of column (T-1, j)
  // constraint groups (prob.py:81-86, 135-142): G = 0 means the default single group "all"
  int G;
  const unsigned int *gmask;      // [NB] groups of every constraint block
  const unsigned int *goverlap;   // [32] groups sharing a block with group g
  double *mvec;                   // [B][32] per-group violation at the convexification point
  unsigned int *nonconv;          // [B] prob.nonconverged_groups: the violated groups under the y threshold (solver.py:232-234)
  unsigned int *stalled;          // [B] the groups that ended the minimisation (solver.py:209-228); the reference lists them first
  // Q3 emulation: per timestep block, the points already seen (keys = rint(x * 1e6), the
  // reference's tuple(x.round(6))) with their f values, and the points already
  // convexified with their affine model
  int H, HC;
  double *hkey, *hval, *ckey, *cJ, *cb;   // [B][NB][H][d], [B][NB][H][RM], [B][NB][HC][d], [B][NB][HC][RM*d], [B][NB][HC][RM]
  int *hn, *cn;                            // [B][NB]
};

struct sco_sqp {
  int device = 0;
  sco_trajopt_desc desc{};
  sco_qp *qp0 = nullptr, *qp1 = nullptr;
  SqpDev d{};
  hipStream_t stream = nullptr;
  // stream groups of the round loop (sco_sqp_solve): group 0 runs on `stream`, group g > 0 on gstream[g - 1]
  hipStream_t gstream[SQP_MAX_GROUPS - 1] = {};
  EventPool events, gevents[SQP_MAX_GROUPS];          // stage marks of the main stream and of every group's rounds (timed)
  EventPool done{{}, 0, hipEventDisableTiming};       // per (group, slot): the round's read-back has landed
  EventPool mix_events{{}, 0, hipEventDisableTiming}; // three per mixed round (QpGroup::side_ev)
  int xcds = 0;                      // sqp_xcds of the device, looked up by the first solve that needs it
  double *fetch_buf = nullptr;       // [2][B] merit and max violation of sco_sqp_fetch
  int *host_active = nullptr;        // pinned: [SQP_MAX_GROUPS][SQP_DEPTH] active counts read back per round
  int groups_used = 1;
  std::vector<void *> allocs;
  void *prog_buf[4] = {nullptr, nullptr, nullptr, nullptr};   // sco_sqp_load_program: words, row starts, constants, parameters
  void *objw_buf = nullptr;                                    // sco_sqp_load_obj_weights
  void *accw_buf = nullptr;                                    // sco_sqp_load_acc_weights
  bool gen_loaded = false;
  size_t prog_bytes[4] = {0, 0, 0, 0};
  bool loaded = false, solved = false, target_loaded = false, vel_loaded = false, jl_loaded = false, cost_loaded = false, quad_loaded = false, prog_loaded = false, spatial_loaded = false;
  double last_ms[5] = {0, 0, 0, 0, 0};
  int rounds = 0;          // 1 (projection) + the rounds of the group that needed most
  int launches = 0;        // round launches over all stream groups
  int wv_rounds = 0;       // of them on the wavefront tier
  double wv_ms = 0.0;      // ADMM time of those rounds (part of last_ms[2])
  int mixed_rounds = 0, mixed_side = 0;   // of the wavefront rounds the mixed ones, and their side-window sizes summed
};

// --------------------------------------------------------------------------
// device helpers
// --------------------------------------------------------------------------
// index of the stored point whose rounded key equals that of x (d coordinates), or -1
__device__ __forceinline__ int memo_find(const double *keys, int count, int d, const double *x) {
  for (int h = 0; h < count; h++) {
    const double *k = keys + (size_t)h * d;
    bool same = true;
    for (int j = 0; j < d; j++) same = same && (k[j] == rint(x[j] * 1e6));
    if (same) return h;
  }
  return -1;
}

// w: the problem's objective weights (r04, QuadExpr with per-joint weights, prob.py:348-367) or nullptr = all 1
__device__ __forceinline__ double traj_obj_partial(const double *x, int d, int T, int tid, const double *w, const double *aw) {
  double s = 0.0;
  for (int e = tid; e < (T - 1) * d; e += SCO_BLOCK) {
    const double df = x[e + d] - x[e];
    s += w ? w[e % d] * (df * df) : df * df;
  }
  if (aw)                                  // acceleration term (r04): second differences
    for (int e = tid; e < (T - 2) * d; e += SCO_BLOCK) {
      const double dd = (x[e + 2 * d] - 2.0 * x[e + d]) + x[e];
      s += aw[e % d] * (dd * dd);
    }
  return s;
}
// entries of the objective's P = Q (0.5 x'Qx form) in column (t, j): (t - 2, j), (t - 1, j), (t, j); wv / wa the joint's weights
__device__ __forceinline__ double obj_p_diag(int t, int T, double wv, double wa) {
  double v = ((t == 0 || t == T - 1) ? 2.0 : 4.0) * wv;
  if (wa != 0.0) {
    if (t <= T - 3) v += 2.0 * wa;                    // first point of window t
    if (t >= 1 && t <= T - 2) v += 8.0 * wa;          // middle point of window t - 1
    if (t >= 2) v += 2.0 * wa;                        // last point of window t - 2
  }
  return v;
}
__device__ __forceinline__ double obj_p_off1(int t, int T, double wv, double wa) {      // entry ((t - 1, j), (t, j)), t >= 1
  double v = -2.0 * wv;
  if (wa != 0.0) {
    if (t <= T - 2) v -= 4.0 * wa;                    // (first, middle) of window t - 1
    if (t >= 2) v -= 4.0 * wa;                        // (middle, last) of window t - 2
  }
  return v;
}

// upper bound of linear inequality row i (m_pin <= i < m_lin): velocity rows, then theta <= hi, then -theta <= -lo, then the
// general affine rows (prob.py:329-338: lb = -inf, ub = val - b; an equality among the general rows: lb = ub, prob.py:339-346)
__device__ __forceinline__ bool lin_row_is_eq(const SqpDev &s, int i) {
  return i >= s.m_lin - s.m_gen && s.gen_eq[i - (s.m_lin - s.m_gen)] != 0;
}
__device__ __forceinline__ double lin_ineq_hi(const SqpDev &s, int b, int i) {
  if (i >= s.m_lin - s.m_gen) return s.gen_rhs[(size_t)b * s.m_gen + (i - (s.m_lin - s.m_gen))];      // general rows (r04)
  const int v = i - s.m_pin;
  if (v < s.m_vel) return s.vmax[b];
  const int k = v - s.m_vel;
  return k < s.n_x ? s.jhi[(size_t)b * s.d + k % s.d] : -s.jlo[(size_t)b * s.d + (k - s.n_x) % s.d];
}
// bounds of linear row i < m_lin, the same in both QPs: the pins, then the inequality rows
__device__ __forceinline__ void lin_row_bounds(const SqpDev &s, int b, int i, double *lo, double *hi) {
  if (i < s.d) *lo = *hi = s.start[(size_t)b * s.d + i];
  else if (i < s.m_pin) *lo = *hi = s.goal[(size_t)b * s.d + (i - s.d)];
  else { *hi = lin_ineq_hi(s, b, i); *lo = lin_row_is_eq(s, i) ? *hi : -INFINITY; }
}

// what the row and objective models (sqp_rows.h) need of problem b
__device__ __forceinline__ RowCtx row_ctx(const SqpDev &s, int b) {
  return RowCtx{s.link_len + (size_t)b * s.d, s.obstacles + (size_t)b * s.O * 3, s.target + (size_t)b * 2, s.point_link, s.point_frac,
                s.ds, s.O, s.point,
                s.qQ + (size_t)b * s.O * s.ds * s.ds, s.qa + (size_t)b * s.O * s.ds, s.qc + (size_t)b * s.O,
                s.pw, s.pptr, s.pconst, s.ppar + (size_t)b * s.n_par * (s.par_step ? s.T : 1), s.par_step, s.R1,
                s.sp_off + (size_t)b * s.d * 3, s.sp_axis + (size_t)b * s.d * 3, s.sp_pos + (size_t)b * s.K * 3, s.sp_rad + (size_t)b * s.K,
                s.sp_sph + (size_t)b * s.O * 4};
}
__device__ __forceinline__ ObjCtx obj_ctx(const SqpDev &s, int b) {
  return ObjCtx{s.cost, s.link_len + (size_t)b * s.d, s.d, s.ctgt[(size_t)b * 2], s.ctgt[(size_t)b * 2 + 1], s.cw[b]};
}

// Q3 emulation.  A history holds, per constraint block, up to H rounded points (keys, ds numbers each) and how many
// (count).  memo_lookup: hit[t] = the stored point block t's state at x rounds onto, or -1 (always -1 without `memo`).
// Block NBt (the reach equality rows) lives on the last timestep.
__device__ __forceinline__ void memo_lookup(const SqpDev &s, bool memo, const double *keys, const int *count, int H, const double *x,
                                            int *hit) {
  for (int t = threadIdx.x; t < s.NB; t += SCO_BLOCK)
    hit[t] = memo ? memo_find(keys + (size_t)t * H * s.ds, count[t], s.ds, x + (t < s.NBt ? t : s.T - 1) * s.d) : -1;
}
// memo_commit: every block that missed gets its key stored and its counter bumped -- after all its values have been
// written -- or, when its history is full, raises SCO_SQP_FLAG_MEMO_FULL
__device__ __forceinline__ void memo_commit(const SqpDev &s, SqpScalars &sc, double *keys, int *count, int H, const double *x,
                                            const int *hit) {
  for (int t = threadIdx.x; t < s.NB; t += SCO_BLOCK) {
    if (hit[t] >= 0) continue;
    if (count[t] < H) {
      const double *xb = x + (t < s.NBt ? t : s.T - 1) * s.d;
      for (int j = 0; j < s.ds; j++) keys[((size_t)t * H + count[t]) * s.ds + j] = rint(xb[j] * 1e6);
      count[t] += 1;
    } else atomicOr(&sc.flags, SCO_SQP_FLAG_MEMO_FULL);
  }
}

// d f / d x_j by central differences on a halving ladder + Richardson extrapolation (expr.py:61-69, numdiff.py);
// f(j, h) = the function with coordinate j moved by h, xj = that coordinate
template <typename F>
__device__ __forceinline__ double central_diff(double xj, int j, F f) {
  const double h0 = FD_BASE * fmax(1.0, fabs(xj));
  double tab[FD_LEVELS];
#pragma unroll
  for (int lv = 0; lv < FD_LEVELS; lv++) {
    const double h = h0 / (double)(1 << lv);
    const double fp = f(j, h);
    const double fm = f(j, -h);
    tab[lv] = (fp - fm) / (2.0 * h);
  }
  return richardson(tab);
}

// row e of the affine model applied to x: sum_j J[e][j] x[q.t d + j] in j order (a reach row lives on one timestep)
__device__ __forceinline__ double model_row(const double *J, const double *x, const RowRef &q, int e, int d, int ds) {
  const int nj = q.eq == ROW_REACH_EQ ? d : ds;
  double acc = 0.0;
  for (int j = 0; j < nj; j++) acc += J[(size_t)e * ds + j] * x[q.t * d + j];
  return acc;
}

// get_value(vectorize=True) (prob.py:558-570): per-block sums of what a row contributes, viol(e, q), then per-group sums
// in block order, handed to out(g, sum)
template <typename F, typename G>
__device__ __forceinline__ void group_sums(const SqpDev &s, const RowLay &L, F viol, G out) {
  __shared__ double bsum[260];
  for (int blk = threadIdx.x; blk < s.NB; blk += SCO_BLOCK) {
    const int e0 = blk < s.NBt ? blk * s.R : s.NBt * s.R, cnt = blk < s.NBt ? s.R : s.NE;
    double acc = 0.0;
    for (int e = e0; e < e0 + cnt; e++) acc += viol(e, row_ref(e, L));
    bsum[blk] = acc;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < s.G; g += SCO_BLOCK) {
    double acc = 0.0;
    for (int blk = 0; blk < s.NB; blk++) if ((s.gmask[blk] >> g) & 1u) acc += bsum[blk];
    out(g, acc);
  }
  __syncthreads();
}

// --------------------------------------------------------------------------
// round 0: projection QP values  (prob.py:369-412)
//   P_ii = 2 c, q_i = -2 c x0_i  (c = number of Variables holding atom i),
//   rows = [pins ; bound rows (-inf, inf)]
// --------------------------------------------------------------------------
__global__ __launch_bounds__(SCO_BLOCK) void sqp_proj_assemble_kernel(SqpDev s, QpDev q0) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_x = s.n_x, d = s.d, m0 = q0.m;
  const double *x0 = s.x0 + (size_t)b * n_x;
  for (int i = tid; i < n_x; i += SCO_BLOCK) {
    // one (x_i - x0_i)^2 per Variable that holds the atom (prob.py:381-404): the descriptor's count is that of an atom
    // covered by one block Variable; with blocks of S > 1 timesteps timestep t sits in `nblk` of them
    const int ts = i / d, nblk = (ts < s.NBt - 1 ? ts : s.NBt - 1) - (ts - s.S + 1 > 0 ? ts - s.S + 1 : 0) + 1;
    const double c = (double)(s.prox_count - 1 + nblk);
    // entries whose initial value is unknown (NaN) take no part in the distance (prob.py:394-404)
    const bool known = !isnan(x0[i]);
    q0.Pval[(size_t)b * q0.nnzP + i] = known ? 2.0 * c : 0.0;
    q0.q[(size_t)b * n_x + i] = known ? (-2.0 * x0[i]) * c : 0.0;
    s.x[(size_t)b * n_x + i] = x0[i];
  }
  for (int t = tid; t < q0.nnzA; t += SCO_BLOCK) q0.Aval[(size_t)b * q0.nnzA + t] = s.a0c[t];
  if (s.nnz_gen) {                       // per-problem coefficients of the general affine rows over the shared constants
    __syncthreads();
    for (int k = tid; k < s.nnz_gen; k += SCO_BLOCK) q0.Aval[(size_t)b * q0.nnzA + s.gpos0[k]] = s.gen_val[(size_t)b * s.nnz_gen + k];
  }
  for (int i = tid; i < m0; i += SCO_BLOCK) {
    double lo, hi;
    if (i < s.m_lin) lin_row_bounds(s, b, i, &lo, &hi);
    else { lo = -INFINITY; hi = INFINITY; }
    q0.l[(size_t)b * m0 + i] = lo; q0.u[(size_t)b * m0 + i] = hi;
    q0.w[(size_t)b * m0 + i] = 1;
  }
  if (tid == 0) {
    SqpScalars &sc = s.sc[b];
    sc.state = ST_PROJECT; sc.k = 0; sc.sqp_iters = 0; sc.qp_solves = 0; sc.success = 0;
    sc.escalations = 0; sc.n_trace = 0; sc.spawned = 0; sc.admm_iters = 0; sc.flags = 0;
    sc.slack_cost = 1.0; sc.merit = 0.0; sc.merit_viol = 0.0;
    s.active[b] = 1; s.nonconv[b] = 0u; s.stalled[b] = 0u;
  }
  for (int t = tid; t < s.NB; t += SCO_BLOCK) { s.hn[(size_t)b * s.NB + t] = 0; s.cn[(size_t)b * s.NB + t] = 0; }
}

struct SqpParamsDev {
  double improve_ratio_threshold, min_trust_region_size, min_approx_improve, trust_shrink_ratio,
      trust_expand_ratio, cnt_tolerance, merit_coeff_increase_ratio, initial_trust_region_size,
      initial_penalty_coeff;
  int max_merit_coeff_increases, compound_penalty, duplicate_rows, max_qp_solves, memo;
};

__device__ __forceinline__ void trace_row(const SqpDev &s, int b, SqpScalars &sc, int kind, double merit,
                                          double model, double newm, double trust, double pen, int status,
                                          int iters) {
  if (sc.n_trace < s.trace_cap) {
    double *r = s.trace + ((size_t)b * s.trace_cap + sc.n_trace) * TRACE_W;
    r[0] = kind; r[1] = merit; r[2] = model; r[3] = newm; r[4] = trust; r[5] = pen; r[6] = status; r[7] = iters;
  }
  sc.n_trace++;
}

__global__ __launch_bounds__(SCO_BLOCK) void sqp_proj_post_kernel(SqpDev s, QpDev q0, QpDev q1, SqpParamsDev p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_x = s.n_x, n = s.n, m = s.m, d = s.d;
  const int status = q0.status[b];
  const bool ok = (status == 1 || status == 2);
  if (ok) for (int i = tid; i < n_x; i += SCO_BLOCK) s.x[(size_t)b * n_x + i] = q0.x[(size_t)b * n_x + i];
  // constant parts of the penalty QP (prob.py:251-278, 348-367; osqp_utils.py:185-189)
  {
    double *Pv = q1.Pval + (size_t)b * q1.nnzP;
    // pattern built on the host: column (t, j) holds [super-diagonal (-2) if t > 0, diagonal]
    // (with SCO_FAM_FLAG_EE_COST the column also holds rows (t, 0 .. j - 1) of its diagonal block: the Hessian of the
    // objective term, written by every convexify)
    int pos = 0;
    for (int col = 0; col < n_x; col++) {   // cheap: n_x entries, one thread
      if (tid == 0) {
        const int t = col / d;
        const double wj = s.objw ? s.objw[(size_t)b * d + col % d] : 1.0;
        const double aj = s.accw ? s.accw[(size_t)b * d + col % d] : 0.0;
        if (s.cost == OBJ_BLOCK) {                    // block terms: the dense band of rows max(0, t - S + 1) d .. col
          if (s.acc && s.S == 2 && t > 1) Pv[pos++] = 2.0 * aj;
          for (int r = (t - s.S + 1 > 0 ? t - s.S + 1 : 0) * d; r <= col; r++)
            Pv[pos++] = r == col ? obj_p_diag(t, s.T, wj, aj) : r == col - d ? obj_p_off1(t, s.T, wj, aj) :
                        (s.acc && r == col - 2 * d) ? 2.0 * aj : 0.0;
          continue;
        }
        if (s.acc && t > 1) Pv[pos++] = 2.0 * aj;                            // ((t - 2, j), (t, j)): first x last of window t - 2
        if (t > 0) Pv[pos++] = obj_p_off1(t, s.T, wj, aj);
        if (s.cost) for (int i = 0; i < col % d; i++) Pv[pos++] = 0.0;
        Pv[pos++] = obj_p_diag(t, s.T, wj, aj);
      }
    }
    double *qv = q1.q + (size_t)b * n;
    for (int i = tid; i < n; i += SCO_BLOCK) qv[i] = 0.0;
    double *Av = q1.Aval + (size_t)b * q1.nnzA;
    // constant entries (pins, velocity rows, slack and bound entries; zeros where convexify writes the
    // Jacobian), built once on the host (sco_sqp_create)
    for (int t = tid; t < q1.nnzA; t += SCO_BLOCK) Av[t] = s.a1c[t];
    if (s.nnz_gen) {
      __syncthreads();
      for (int k = tid; k < s.nnz_gen; k += SCO_BLOCK) Av[s.gpos1[k]] = s.gen_val[(size_t)b * s.nnz_gen + k];
    }
    double *l = q1.l + (size_t)b * m, *u = q1.u + (size_t)b * m;
    int *w = q1.w + (size_t)b * m;
    for (int i = tid; i < m; i += SCO_BLOCK) {
      double lo, hi;
      if (i < s.m_lin) lin_row_bounds(s, b, i, &lo, &hi);
      else if (i < s.m_lin + s.m_nl) {                                  // hinge rows; equality rows are set by convexify
        const RowRef qr = row_ref(i - s.m_lin, RowLay{s.T, s.NBt, s.R, s.Req});
        lo = qr.eq != ROW_HINGE ? 0.0 : -INFINITY; hi = 0.0;
      }
      else if (i < s.m_lin + s.m_nl + n_x) { lo = -INFINITY; hi = INFINITY; }
      else { lo = 0.0; hi = INFINITY; }
      l[i] = lo; u[i] = hi; w[i] = 1;
    }
  }
  if (tid == 0) {
    SqpScalars &sc = s.sc[b];
    sc.qp_solves = 1; sc.admm_iters = q0.iters[b];
    sc.penalty = p.initial_penalty_coeff; sc.trust = p.initial_trust_region_size;
    trace_row(s, b, sc, STEP_PROJECT, 0.0, 0.0, 0.0, sc.trust, sc.penalty, status, q0.iters[b]);
    if (ok) { sc.state = ST_CONVEXIFY; atomicAdd(s.n_active, 1); }
    else { sc.state = ST_DONE; sc.success = 0; s.active[b] = 0; }   // solver.py:81-82
  }
}

// SCO_FAM_FLAG_OBJ_WIDE: eigenvalue shift and degree-2 model of the objective terms (n <= 32 numbers each), ONE WAVEFRONT per
// term.  The term's matrix sits in dynamic LDS with row stride WIDE_LD = 33 doubles, so lane k's column entry (k, p) and a row
// (p, 0 .. n-1) are both free of bank conflicts.  The cyclic Jacobi sweep is min_eig_jacobi's, rotation for rotation (12
// sweeps, the 1e-300 skip, the 1e150 guard): every lane reads the rotation's scalars from LDS and computes c, s itself; lanes
// k < n rotate the column pair (k, p), (k, q), then -- after a wavefront-scope fence -- the row pair (p, k), (q, k).  Every
// element sees the same operations in the same order as in the per-thread sweep.  The model: lane j forms (x'H)_j and
// A_j = g_j - (x'H)_j; lane 0 sums x'Hx and g.x in j order, as the per-thread path does.  No workgroup barrier inside.
#define WIDE_LD 33
#define WIDE_WAVE_LDS (SCO_STATE_MAX * WIDE_LD + 2 * SCO_STATE_MAX)     // doubles per wavefront: the matrix, x'H, g
#define WIDE_LDS_BYTES (NWAVE * WIDE_WAVE_LDS * sizeof(double))
__device__ void obj_shift_model_wide(double *oH, double *oA, double *ob, const double *of0, const double *x, int d, int n,
                                     int NO, int tid) {
  extern __shared__ double wide_lds[];
  const int lane = tid & 63, wave = tid >> 6;
  double *A = wide_lds + wave * WIDE_WAVE_LDS, *xh = A + SCO_STATE_MAX * WIDE_LD, *gl = xh + SCO_STATE_MAX;
  for (int t = wave; t < NO; t += NWAVE) {
    double *Ht = oH + (size_t)t * n * n;
    const double *th = x + t * d;
    for (int e = lane; e < n * n; e += 64) A[(e / n) * WIDE_LD + e % n] = Ht[e];
    wave_lds_fence();
    for (int sweep = 0; sweep < 12; sweep++)
      for (int p = 0; p < n - 1; p++)
        for (int q = p + 1; q < n; q++) {
          const double apq = A[p * WIDE_LD + q];
          if (fabs(apq) < 1e-300) continue;
          const double theta = (A[q * WIDE_LD + q] - A[p * WIDE_LD + p]) / (2.0 * apq);
          const double at = fabs(theta);
          const double tr = (theta >= 0.0 ? 1.0 : -1.0) / (at + (at > 1e150 ? at : sqrt(theta * theta + 1.0)));
          const double c = 1.0 / sqrt(tr * tr + 1.0), sn = tr * c;
          if (lane < n) {                                   // columns p, q
            const double rp = A[lane * WIDE_LD + p], rq = A[lane * WIDE_LD + q];
            A[lane * WIDE_LD + p] = c * rp - sn * rq; A[lane * WIDE_LD + q] = sn * rp + c * rq;
          }
          wave_lds_fence();
          if (lane < n) {                                   // rows p, q
            const double rp = A[p * WIDE_LD + lane], rq = A[q * WIDE_LD + lane];
            A[p * WIDE_LD + lane] = c * rp - sn * rq; A[q * WIDE_LD + lane] = sn * rp + c * rq;
          }
          wave_lds_fence();
        }
    double lam = A[0];
    for (int i = 1; i < n; i++) lam = fmin(lam, A[i * WIDE_LD + i]);
    if (lane < n) {
      if (lam < 0.0) Ht[lane * n + lane] -= lam;           // (lane j touches only its own diagonal entry)
      const double g = oA[t * n + lane];
      double acc = 0.0;
      for (int i = 0; i < n; i++) acc += th[i] * Ht[i * n + lane];
      xh[lane] = acc; gl[lane] = g;
      oA[t * n + lane] = g - acc;
    }
    wave_lds_fence();
    if (lane == 0) {
      double xHx = 0.0, gx = 0.0;
      for (int j = 0; j < n; j++) { xHx += xh[j] * th[j]; gx += gl[j] * th[j]; }
      ob[t] = (0.5 * xHx - gx) + of0[t];
    }
    wave_lds_fence();                                       // the next term overwrites A, x'H and g
  }
}

// --------------------------------------------------------------------------
// sqp_pre: convexify + update_obj + merit + save (for problems that start a new
// SQP iteration), then the trust-region bounds (for every active problem).
// WIDE (SCO_FAM_FLAG_OBJ_WIDE, sqp_pre_wide_kernel): the objective terms' shift and model by obj_shift_model_wide
// --------------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ void sqp_pre_body(SqpDev &s, QpDev &q1, SqpParamsDev &p) {
  const int g = blockIdx.x + s.b0, tid = threadIdx.x;
  const int b = s.list ? s.list[g] : g;        // round selection: only the listed problems are visited
  if (b < 0) return;
  SqpScalars &sc = s.sc[b];
  const int state = sc.state;
  // a problem whose QP is parked between two ADMM slices keeps its QP untouched
  const bool parked = q1.prog && q1.prog[b] > 0;
  if (tid == 0) s.newqp[b] = (state != ST_DONE && !parked) ? 1 : 0;
  if (state == ST_DONE || parked) return;
  __shared__ double red[NWAVE * 4];
  __shared__ double of0[260];           // f of the non-quadratic objective terms at the convexification point
  const int n_x = s.n_x, d = s.d, T = s.T, R = s.R, n = s.n, m = s.m;
  const int ds = s.ds, NBt = s.NBt;             // state dimension of a block, number of timestep blocks
  const int NO = s.cost == OBJ_BLOCK ? NBt : T;         // objective terms: one per timestep, or one per block (OBJ_BLOCK)
  const RowLay L{T, NBt, R, s.Req};
  double *x = s.x + (size_t)b * n_x, *xs = s.x_saved + (size_t)b * n_x;
  double *gs = s.gsave + (size_t)b * s.m_nl, *J = s.J + (size_t)b * s.m_nl * ds, *bm = s.bmod + (size_t)b * s.m_nl;
  unsigned char *mask = s.mask + (size_t)b * s.m_nl * ds;
  const double penalty = sc.penalty, trust = sc.trust;
  const int spawned = sc.spawned;
  int k_rows = sc.k;
  double slack_cost = sc.slack_cost;

  if (state == ST_CONVEXIFY) {
    // Q3: which blocks sit on an already-seen / already-convexified rounded point
    __shared__ int ev_hit[260], cv_hit[260];
    const int H = s.H, HC = s.HC, NB = s.NB, RM = s.RM, m_nl = s.m_nl;
    const RowCtx rc = row_ctx(s, b);
    double *hkey = s.hkey + (size_t)b * NB * H * ds, *hval = s.hval + (size_t)b * NB * H * RM;
    double *ckey = s.ckey + (size_t)b * NB * HC * ds, *cJ = s.cJ + (size_t)b * NB * HC * RM * ds, *cb = s.cb + (size_t)b * NB * HC * RM;
    int *hn = s.hn + (size_t)b * NB, *cn = s.cn + (size_t)b * NB;
    memo_lookup(s, p.memo, hkey, hn, H, x, ev_hit);
    memo_lookup(s, p.memo, ckey, cn, HC, x, cv_hit);
    __syncthreads();
    // S1: f(x) per row, memoised on the rounded point (expr.py:34-41)
    for (int e = tid; e < m_nl; e += SCO_BLOCK) {
      const RowRef q = row_ref(e, L);
      double g;
      if (ev_hit[q.blk] >= 0) g = hval[((size_t)q.blk * H + ev_hit[q.blk]) * RM + q.r];
      else {
        g = row_value(rc, q, x + q.t * d, -1, 0.0);
        if (p.memo && hn[q.blk] < H) hval[((size_t)q.blk * H + hn[q.blk]) * RM + q.r] = g;
      }
      gs[e] = g;
    }
    // S1/S2: Jacobian entry per thread (expr.py:61-69 numeric / :88 analytic); a block whose
    // rounded point was convexified before reuses that affine model (expr.py:362-365, 323-332)
    for (int e = tid; e < m_nl * ds; e += SCO_BLOCK) {
      const int j = e % ds;
      const RowRef q = row_ref(e / ds, L);
      const double *th = x + q.t * d;
      double val;
      if (q.eq == ROW_REACH_EQ && j >= d) {
        val = 0.0;                               // (a reach row lives on ONE timestep; its entry slots beyond dof do not exist)
      } else if (cv_hit[q.blk] >= 0) {
        val = cJ[(((size_t)q.blk * HC + cv_hit[q.blk]) * RM + q.r) * ds + j];
      } else if (s.analytic_jac) {
        val = row_grad(rc, q, th, j);
      } else if (row_ignores(rc, q, j)) {
        val = 0.0;                               // (the central differences of a row that does not see coordinate j: 0 on the host too)
      } else {
        val = central_diff(th[j], j, [&](int jj, double h) { return row_value(rc, q, th, jj, h); });
      }
      J[e] = val;
      if (p.memo && cv_hit[q.blk] < 0 && cn[q.blk] < HC) cJ[(((size_t)q.blk * HC + cn[q.blk]) * RM + q.r) * ds + j] = val;
      if (!spawned) mask[e] = (val != 0.0) ? 1 : 0;   // creation-time pattern (prob.py:264, 440)
    }
    __syncthreads();
    // S2: affine model b = f - J x - val (expr.py:141, 367 / 328);  S3: rows
    if (p.duplicate_rows) k_rows += 1; else k_rows = 1;
    slack_cost = p.compound_penalty ? slack_cost * penalty : penalty;
    double *Av = q1.Aval + (size_t)b * q1.nnzA;
    double *l = q1.l + (size_t)b * m, *u = q1.u + (size_t)b * m;
    int *w = q1.w + (size_t)b * m;
    for (int e = tid; e < m_nl; e += SCO_BLOCK) {
      const RowRef q = row_ref(e, L);
      double bb = (gs[e] - model_row(J, x, q, e, d, ds)) - row_rhs(rc, q);
      if (cv_hit[q.blk] >= 0) bb = cb[((size_t)q.blk * HC + cv_hit[q.blk]) * RM + q.r];
      else if (p.memo && cn[q.blk] < HC) cb[((size_t)q.blk * HC + cn[q.blk]) * RM + q.r] = bb;
      bm[e] = bb;
      u[s.m_lin + e] = -bb;            // hinge: -inf <= a x - t <= -b  (prob.py:265-275, 486)
      if (q.eq != ROW_HINGE) l[s.m_lin + e] = -bb;  // abs:   a x - p + n = -b        (prob.py:303-312, 480-484)
      w[s.m_lin + e] = k_rows;         // row present k times (prob.py:508-509)
    }
    for (int e = tid; e < m_nl * ds; e += SCO_BLOCK) {
      const int j = e % ds;
      const RowRef q = row_ref(e / ds, L);
      if (q.eq == ROW_REACH_EQ && j >= d) continue;
      // column c = (timestep q.t + j / d, coordinate j % d) holds, below its linear entries, the R slots of every block
      // that covers its timestep, in block order (sco_sqp_create)
      const int c = q.t * d + j, tfirst = (c / d - s.S + 1 > 0) ? c / d - s.S + 1 : 0;
      const int pos = q.eq == ROW_REACH_EQ ? s.epos[j] + q.r : s.jpos[c] + (q.blk - tfirst) * R + q.r;
      Av[pos] = mask[e] ? J[e] : 0.0;   // prob.py:493-504
    }
    double *qv = q1.q + (size_t)b * n;
    for (int i = tid; i < s.n_slack; i += SCO_BLOCK) qv[n_x + i] = slack_cost;   // prob.py:424-426
    if (s.cost) {
      // ---- non-quadratic objective terms: Expr.convexify(degree 2) (expr.py:143-153) per timestep block, or per constraint
      // block of S timesteps (OBJ_BLOCK: NO = NBt terms on dO = ds numbers; block t's state starts at x[t d] as well)
      const ObjCtx oc = obj_ctx(s, b);
      const int dO = s.cost == OBJ_BLOCK ? ds : d;
      double *oH = s.oH + (size_t)b * NO * dO * dO, *oA = s.oA + (size_t)b * NO * dO, *ob = s.ob + (size_t)b * NO;
      // f(x), memoised on the rounded point like every Expr.eval (expr.py:34-41); the term shares the point history of
      // its constraint block (same Variable, same evaluation points): its value is the block's last column
      for (int t = tid; t < NO; t += SCO_BLOCK) {
        double f;
        if (ev_hit[t] >= 0) f = hval[((size_t)t * H + ev_hit[t]) * RM + (RM - 1)];
        else {
          f = obj_value(oc, rc, t, x + t * d, -1, 0.0, -1, 0.0);
          if (p.memo && hn[t] < H) hval[((size_t)t * H + hn[t]) * RM + (RM - 1)] = f;
        }
        of0[t] = f;
      }
      __syncthreads();
      // numeric Hessian (expr.py:102-109; second central differences on the halving ladder, Richardson: numdiff.py)
      const int npair = dO * (dO + 1) / 2;
      for (int e = tid; e < NO * npair; e += SCO_BLOCK) {
        const int t = e / npair;
        int k = e % npair, i = 0;
        while (k >= dO - i) { k -= dO - i; i++; }
        const int j = i + k;
        const double *th = x + t * d;
        const double si = FD_BASE * fmax(1.0, fabs(th[i])), sj = FD_BASE * fmax(1.0, fabs(th[j]));
        double tab[FD_LEVELS];
#pragma unroll
        for (int lv = 0; lv < FD_LEVELS; lv++) {
          const double hi = si / (double)(1 << lv), hj = sj / (double)(1 << lv);
          if (i == j) {
            const double fp = obj_value(oc, rc, t, th, i, hi, -1, 0.0);
            const double fm = obj_value(oc, rc, t, th, i, -hi, -1, 0.0);
            tab[lv] = (fp - 2.0 * of0[t] + fm) / (hi * hi);
          } else {
            const double fpp = obj_value(oc, rc, t, th, i, hi, j, hj);
            const double fpm = obj_value(oc, rc, t, th, i, hi, j, -hj);
            const double fmp = obj_value(oc, rc, t, th, i, -hi, j, hj);
            const double fmm = obj_value(oc, rc, t, th, i, -hi, j, -hj);
            tab[lv] = (fpp - fpm - fmp + fmm) / (4.0 * hi * hj);
          }
        }
        const double hv = richardson(tab);
        oH[(size_t)t * dO * dO + i * dO + j] = hv; oH[(size_t)t * dO * dO + j * dO + i] = hv;
      }
      // numeric gradient (expr.py:61-69), parked in oA until the block's thread turns it into the model's A
      for (int e = tid; e < NO * dO; e += SCO_BLOCK) {
        const int t = e / dO, j = e % dO;
        const double *th = x + t * d;
        oA[e] = central_diff(th[j], j, [&](int jj, double h) { return obj_value(oc, rc, t, th, jj, h, -1, 0.0); });
      }
      __syncthreads();
      // eigenvalue shift, then Q = H, A = g - x'H, b = 1/2 x'Hx - g.x + f (expr.py:145-152)
      if constexpr (WIDE) obj_shift_model_wide(oH, oA, ob, of0, x, d, dO, NO, tid);
      else
      for (int t = tid; t < NO; t += SCO_BLOCK) {
        double *Ht = oH + (size_t)t * dO * dO;
        const double *th = x + t * d;
        const double lam = min_eig_jacobi(Ht, dO);
        if (lam < 0.0) for (int i = 0; i < dO; i++) Ht[i * dO + i] -= lam;
        double xHx = 0.0, gx = 0.0, g[OBJ_DMAX], xH[OBJ_DMAX];
        for (int j = 0; j < dO; j++) {
          g[j] = oA[t * dO + j];
          double acc = 0.0;
          for (int i = 0; i < dO; i++) acc += th[i] * Ht[i * dO + j];
          xH[j] = acc;
        }
        for (int j = 0; j < dO; j++) { xHx += xH[j] * th[j]; gx += g[j] * th[j]; oA[t * dO + j] = g[j] - xH[j]; }
        ob[t] = (0.5 * xHx - gx) + of0[t];
      }
      __syncthreads();
      // QuadExpr lowering (prob.py:348-367; osqp_utils.py:153-163): Q into the upper triangle of P, A into q
      double *Pv = q1.Pval + (size_t)b * q1.nnzP;
      if (s.cost == OBJ_BLOCK) {
        // blocks overlap: every entry of the band is written by one thread, which adds, in the reference's order, the
        // smoothing QuadExpr first, then each covering block's Q in block order -- an off-diagonal pair as its two halves
        // 0.5 Q_ij + 0.5 Q_ji, the diagonal whole (osqp_utils.py:153-163); q likewise (osqp_utils.py:146-148)
        const int S = s.S;
        for (int e = tid; e < n_x * ds; e += SCO_BLOCK) {
          const int c = e / ds, tc = c / d, j = c % d, tlo = tc - S + 1 > 0 ? tc - S + 1 : 0, r = tlo * d + e % ds;
          if (r > c) continue;
          const int thi = r / d < NBt - 1 ? r / d : NBt - 1;
          const double wj = s.objw ? s.objw[(size_t)b * d + j] : 1.0, aj = s.accw ? s.accw[(size_t)b * d + j] : 0.0;
          double v = r == c ? obj_p_diag(tc, T, wj, aj) : r == c - d ? obj_p_off1(tc, T, wj, aj) : (s.acc && r == c - 2 * d) ? 2.0 * aj : 0.0;
          for (int t = tlo; t <= thi; t++) {
            const double h = oH[(size_t)t * ds * ds + (r - t * d) * ds + (c - t * d)];
            if (r == c) v += h;
            else { v += 0.5 * h; v += 0.5 * h; }
          }
          Pv[s.ppos[c] + r] = v;
        }
        for (int i = tid; i < n_x; i += SCO_BLOCK) {
          const int ti = i / d, thi = ti < NBt - 1 ? ti : NBt - 1;
          double acc = 0.0;
          for (int t = ti - S + 1 > 0 ? ti - S + 1 : 0; t <= thi; t++) acc += oA[t * ds + (i - t * d)];
          qv[i] = acc;
        }
      } else {
      for (int e = tid; e < T * npair; e += SCO_BLOCK) {
        const int t = e / npair;
        int k = e % npair, i = 0;
        while (k >= d - i) { k -= d - i; i++; }
        const int j = i + k;
        const double base = (i == j) ? obj_p_diag(t, T, s.objw ? s.objw[(size_t)b * d + i] : 1.0, s.accw ? s.accw[(size_t)b * d + i] : 0.0) : 0.0;
        Pv[s.ppos[t * d + j] + i] = base + oH[(size_t)t * d * d + i * d + j];
      }
      for (int e = tid; e < n_x; e += SCO_BLOCK) qv[e] = oA[e];
      }
    }
    // S7: merit at the convexification point (prob.py:571-579), S4 prerequisite: save
    double v[2] = {traj_obj_partial(x, d, T, tid, s.objw ? s.objw + (size_t)b * d : nullptr, s.accw ? s.accw + (size_t)b * d : nullptr) + ((s.cost && tid < NO) ? of0[tid] : 0.0), 0.0};
    for (int e = tid; e < m_nl; e += SCO_BLOCK) {
      const RowRef q = row_ref(e, L);
      v[1] += row_viol(q, gs[e] - row_rhs(rc, q));
    }
    block_reduce_sm<2, 0, NWAVE>(v, red);
    if (s.G > 0) {
      // per-group violation at the saved point
      group_sums(s, L, [&](int e, const RowRef &q) { return row_viol(q, gs[e] - row_rhs(rc, q)); },
                 [&](int g, double sum) { s.mvec[(size_t)b * 32 + g] = sum; });
    }
    for (int i = tid; i < n_x; i += SCO_BLOCK) xs[i] = x[i];
    // commit the new history entries (keys last, after every value has been written)
    if (p.memo) {
      memo_commit(s, sc, hkey, hn, H, x, ev_hit);
      memo_commit(s, sc, ckey, cn, HC, x, cv_hit);
    }
    if (tid == 0) {
      sc.merit_viol = v[1];
      sc.merit = v[0] + penalty * v[1];
      sc.k = k_rows; sc.slack_cost = slack_cost; sc.spawned = 1;
      sc.sqp_iters += 1;
      sc.state = ST_TRIAL;
    }
    __syncthreads();
  }
  // S4: trust box around the saved point (variable.py:43-45)
  {
    double *l = q1.l + (size_t)b * m, *u = q1.u + (size_t)b * m;
    const int base = s.m_lin + s.m_nl;
    for (int i = tid; i < n_x; i += SCO_BLOCK) { l[base + i] = xs[i] - trust; u[base + i] = xs[i] + trust; }
  }
}
__global__ __launch_bounds__(SCO_BLOCK) void sqp_pre_kernel(SqpDev s, QpDev q1, SqpParamsDev p) { sqp_pre_body<false>(s, q1, p); }
// launched with WIDE_LDS_BYTES of dynamic LDS
__global__ __launch_bounds__(SCO_BLOCK) void sqp_pre_wide_kernel(SqpDev s, QpDev q1, SqpParamsDev p) { sqp_pre_body<true>(s, q1, p); }

// --------------------------------------------------------------------------
// sqp_post: model merit, new merit, decision
// --------------------------------------------------------------------------
__global__ __launch_bounds__(SCO_BLOCK) void sqp_post_kernel(SqpDev s, QpDev q1, SqpParamsDev p) {
  const int g = blockIdx.x + s.b0, tid = threadIdx.x;
  const int b = s.list ? s.list[g] : g;
  if (b < 0) return;
  SqpScalars &sc = s.sc[b];
  if (sc.state != ST_TRIAL) return;
  if (q1.prog && q1.prog[b] > 0) {             // its QP is parked between two ADMM slices: nothing to decide yet
    if (tid == 0) atomicAdd(s.n_active, 1);
    return;
  }
  __shared__ double red[NWAVE * 6];
  const int n_x = s.n_x, d = s.d, T = s.T, R = s.R, n = s.n;
  const int ds = s.ds, NBt = s.NBt;
  const RowLay L{T, NBt, R, s.Req};
  double *x = s.x + (size_t)b * n_x, *xs = s.x_saved + (size_t)b * n_x;
  const double *gs = s.gsave + (size_t)b * s.m_nl, *J = s.J + (size_t)b * s.m_nl * ds, *bm = s.bmod + (size_t)b * s.m_nl;
  const int status = q1.status[b], iters = q1.iters[b];
  // every scalar is read BEFORE the reduction's barriers; thread 0 rewrites them afterwards
  const double pen = sc.penalty, trust = sc.trust, merit = sc.merit, merit_viol0 = sc.merit_viol;
  const int qp_solves0 = sc.qp_solves;
  const bool ok = (status == 1 || status == 2);                 // prob.py:197
  const double *xq = ok ? (q1.x + (size_t)b * n) : xs;          // failed QP leaves the variables alone
  // Q3: blocks of the trial point that round onto an already-seen point reuse its f values
  __shared__ int ev_hit[260];
  const int H = s.H, NB = s.NB, RM = s.RM, m_nl = s.m_nl;
  const RowCtx rc = row_ctx(s, b);
  double *hkey = s.hkey + (size_t)b * NB * H * ds, *hval = s.hval + (size_t)b * NB * H * RM;
  int *hn = s.hn + (size_t)b * NB;
  memo_lookup(s, p.memo, hkey, hn, H, xq, ev_hit);
  __syncthreads();
  // model violation uses the FULL Jacobian (prob.py:627-628), new violation f at the new point (prob.py:575-577)
  // v: quadratic objective, model violation, new violation, objective MODELS at the new point (prob.py:625-626),
  //    objective terms at the new point (prob.py:571-573), max violation at the saved point
  double v[6] = {traj_obj_partial(xq, d, T, tid, s.objw ? s.objw + (size_t)b * d : nullptr, s.accw ? s.accw + (size_t)b * d : nullptr), 0.0, 0.0, 0.0, 0.0, 0.0};
  if (s.cost) {
    const int NO = s.cost == OBJ_BLOCK ? NBt : T, dO = s.cost == OBJ_BLOCK ? ds : d;     // per timestep, or per block (OBJ_BLOCK)
    const double *oH = s.oH + (size_t)b * NO * dO * dO, *oA = s.oA + (size_t)b * NO * dO, *ob = s.ob + (size_t)b * NO;
    for (int t = tid; t < NO; t += SCO_BLOCK) {
      const double *th = xq + t * d, *Ht = oH + (size_t)t * dO * dO;
      double xHx = 0.0, ax = 0.0;
      for (int i = 0; i < dO; i++) {
        double acc = 0.0;
        for (int j = 0; j < dO; j++) acc += Ht[i * dO + j] * th[j];
        xHx += th[i] * acc; ax += oA[t * dO + i] * th[i];
      }
      v[3] += (0.5 * xHx + ax) + ob[t];                        // QuadExpr.eval (expr.py:205-206)
      double f;
      if (ev_hit[t] >= 0) f = hval[((size_t)t * H + ev_hit[t]) * RM + (RM - 1)];
      else {
        f = obj_value(obj_ctx(s, b), rc, t, th, -1, 0.0, -1, 0.0);
        if (p.memo && hn[t] < H) hval[((size_t)t * H + hn[t]) * RM + (RM - 1)] = f;
      }
      v[4] += f;
    }
  }
  for (int e = tid; e < m_nl; e += SCO_BLOCK) {
    const RowRef q = row_ref(e, L);
    const double rhs = row_rhs(rc, q);
    v[1] += row_viol(q, model_row(J, xq, q, e, d, ds) + bm[e]);
    double g;
    if (ev_hit[q.blk] >= 0) g = hval[((size_t)q.blk * H + ev_hit[q.blk]) * RM + q.r];
    else {
      g = row_value(rc, q, xq + q.t * d, -1, 0.0);
      if (p.memo && hn[q.blk] < H) hval[((size_t)q.blk * H + hn[q.blk]) * RM + q.r] = g;
    }
    v[2] += row_viol(q, g - rhs);
    v[5] = fmax(v[5], row_viol(q, gs[e] - rhs));                 // max violation at the SAVED point
  }
  __syncthreads();
  if (p.memo) memo_commit(s, sc, hkey, hn, H, xq, ev_hit);
  block_reduce_sm<5, 1, NWAVE>(v, red);
  // constraint groups: which violated groups stopped improving, and do their overlapping groups too
  // (solver.py:155-161, 209-235)
  __shared__ unsigned int g_stalled, g_report;
  if (s.G > 0) {
    __shared__ double gimp[32];
    // per-group model violation at the trial point -> approx_improve_vec
    group_sums(s, L, [&](int e, const RowRef &q) { return row_viol(q, model_row(J, xq, q, e, d, ds) + bm[e]); },
               [&](int g, double sum) { gimp[g] = s.mvec[(size_t)b * 32 + g] - sum; });
    if (tid == 0) {
      unsigned int stalled = 0, report = 0;
      for (int g = 0; g < s.G; g++) {
        const bool viol_g = s.mvec[(size_t)b * 32 + g] > p.cnt_tolerance;
        if (!(viol_g && gimp[g] < p.min_approx_improve)) continue;
        report |= 1u << g;
        bool overlap_improve = false;
        for (int h = 0; h < s.G; h++)
          if (((s.goverlap[g] >> h) & 1u) && gimp[h] > p.min_approx_improve) overlap_improve = true;
        if (!overlap_improve) stalled |= 1u << g;
      }
      g_stalled = stalled; g_report = report;
    }
    __syncthreads();
  }
  const double model_merit = (v[0] + v[3]) + pen * v[1], new_merit = (v[0] + v[4]) + pen * v[2];
  double approx = merit - model_merit;
  if (approx == 0.0) approx += 1e-12;                           // solver.py:152-153
  const double exact = merit - new_merit;
  const double ratio = exact / approx;
  const double approx_vec = merit_viol0 - v[1];               // single group "all" (prob.py:135-136)
  const bool violated = merit_viol0 > p.cnt_tolerance;
  int kind, ret = -1;   // ret: -1 continue, 0/1 = _min_merit_fn returned False/True
  double new_trust = trust;
  if (approx < -1e-5) { kind = STEP_BAD; ret = 0; }                               // solver.py:185-198
  else if (approx < p.min_approx_improve) { kind = STEP_YCONV; ret = 1; }         // solver.py:200-204
  else if (s.G > 0 ? g_stalled != 0u : (violated && approx_vec < p.min_approx_improve)) { kind = STEP_GROUP; ret = 1; }   // solver.py:209-235
  else if (exact < 0.0 || ratio < p.improve_ratio_threshold) {                   // solver.py:237-241
    kind = STEP_SHRINK; new_trust = trust * p.trust_shrink_ratio;
    if (new_trust < p.min_trust_region_size) { kind = STEP_XCONV; ret = 1; }      // solver.py:248-251
  } else { kind = STEP_ACCEPT; new_trust = trust * p.trust_expand_ratio; }        // solver.py:242-246
  const int qp_solves = qp_solves0 + 1;
  const bool capped = (ret < 0) && (qp_solves >= p.max_qp_solves);
  if (kind == STEP_ACCEPT) for (int i = tid; i < n_x; i += SCO_BLOCK) x[i] = xq[i];
  // every other outcome restores the saved point (solver.py:197, 203, 229, 238); x == xs already
  if (tid == 0) {
    // prob.nonconverged_groups is rewritten by every trust-region trial that gets past the
    // y-convergence test (solver.py:209, 233-235)
    if (kind != STEP_BAD && kind != STEP_YCONV)
    {
      s.nonconv[b] = (kind == STEP_GROUP) ? (s.G > 0 ? g_report : 1u) : 0u;
      s.stalled[b] = (kind == STEP_GROUP) ? (s.G > 0 ? g_stalled : 1u) : 0u;
    }
    sc.qp_solves = qp_solves; sc.admm_iters += iters;
    if (capped) atomicOr(&sc.flags, SCO_SQP_FLAG_CAPPED);
    if (sc.n_trace >= s.trace_cap) atomicOr(&sc.flags, SCO_SQP_FLAG_TRACE_FULL);
    trace_row(s, b, sc, kind, merit, model_merit, new_merit, trust, pen, status, iters);
    sc.trust = new_trust;
    if (ret < 0 && !capped) {
      sc.state = (kind == STEP_ACCEPT) ? ST_CONVEXIFY : ST_TRIAL;
      atomicAdd(s.n_active, 1);
    } else {
      // _min_merit_fn returned: outer loop of _penalty_sqp (solver.py:84-105)
      const double max_viol = v[5];
      sc.escalations += 1;
      if (!capped && max_viol > p.cnt_tolerance && sc.escalations < p.max_merit_coeff_increases) {
        sc.penalty = pen * p.merit_coeff_increase_ratio;
        sc.trust = p.initial_trust_region_size;
        sc.state = ST_CONVEXIFY;
        atomicAdd(s.n_active, 1);
      } else {
        sc.success = (!capped && max_viol <= p.cnt_tolerance) ? ret : 0;
        sc.state = ST_DONE; s.active[b] = 0;
      }
    }
  }
}

// final merit / max violation at the returned point (prob.py:571-603)
__global__ __launch_bounds__(SCO_BLOCK) void sqp_final_kernel(SqpDev s, double *merit_out, double *viol_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[NWAVE * 4];
  const int n_x = s.n_x, d = s.d, T = s.T, R = s.R;
  const double *x = s.x + (size_t)b * n_x;
  const RowCtx rc = row_ctx(s, b);
  const RowLay L{T, s.NBt, R, s.Req};
  double v[3] = {traj_obj_partial(x, d, T, tid, s.objw ? s.objw + (size_t)b * d : nullptr, s.accw ? s.accw + (size_t)b * d : nullptr), 0.0, 0.0};
  if (s.cost)
    for (int t = tid; t < (s.cost == OBJ_BLOCK ? s.NBt : T); t += SCO_BLOCK)
      v[0] += obj_value(obj_ctx(s, b), rc, t, x + t * d, -1, 0.0, -1, 0.0);
  for (int e = tid; e < s.m_nl; e += SCO_BLOCK) {
    const RowRef q = row_ref(e, L);
    const double g = row_viol(q, row_value(rc, q, x + q.t * d, -1, 0.0) - row_rhs(rc, q));
    v[1] += g; v[2] = fmax(v[2], g);
  }
  block_reduce_sm<2, 1, NWAVE>(v, red);
  if (tid == 0) { merit_out[b] = v[0] + s.sc[b].penalty * v[1]; viol_out[b] = v[2]; }
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
extern "C" void sco_sqp_default_params(sco_sqp_params *p) {
  if (!p) return;
  p->improve_ratio_threshold = 0.25; p->min_trust_region_size = 1e-4; p->min_approx_improve = 1e-8;
  p->trust_shrink_ratio = 0.1; p->trust_expand_ratio = 1.5; p->cnt_tolerance = 1e-4;
  p->merit_coeff_increase_ratio = 10.0; p->initial_trust_region_size = 1.0; p->initial_penalty_coeff = 1e3;
  p->max_merit_coeff_increases = 1; p->compound_penalty = 1; p->duplicate_rows = 1; p->max_sqp_iters = 0;
  p->memoize_rounded = 1; p->warm_start_qps = 0; p->admm_slice = 0;
}

template <typename T>
static int sq_alloc(sco_sqp *h, size_t count, T **out) {
  void *p = nullptr;
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  SCO_HIP(hipMalloc(&p, bytes));
  SCO_HIP(hipMemset(p, 0, bytes));
  h->allocs.push_back(p);
  *out = (T *)p;
  return SCO_OK;
}
// allocate and upload this vector
template <typename T>
static int sq_upload(sco_sqp *h, const std::vector<T> &v, const T **out) {
  T *p = nullptr;
  if (int rc = sq_alloc(h, v.size(), &p)) return rc;
  if (!v.empty()) SCO_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return SCO_OK;
}

static int sqp_create_impl(sco_sqp *h, int device, const SqpLayout &L);

// r04: sco_sqp_create with n_rows GENERAL affine rows over the trajectory variables behind the built-in linear rows -- what a
// caller of the reference adds with prob.add_cnt_expr(BoundExpr(EqExpr / LEqExpr(AffExpr(A, b), val), traj)) (prob.py:126-131,
// 317-346): a shared CSR pattern (row_ptr[n_rows + 1], col_idx strictly increasing inside a row, columns = name-sorted
// trajectory atoms t * dof + j), row_is_eq[r] != 0: a x = rhs, else a x <= rhs; coefficients and right-hand sides per problem
// through sco_sqp_load_linear_rows.  Which descriptors and patterns are accepted: sqp_check_desc (sqp_layout.cpp).
extern "C" int sco_sqp_create_rows(int device, const sco_trajopt_desc *desc, int n_rows, const int *row_ptr, const int *col_idx,
                                   const int *row_is_eq, sco_sqp **out) {
  if (!desc || !out) { sco_set_error("sco_sqp_create: null pointer"); return SCO_ERR_ARG; }
  const char *err = "";
  if (int rc = sqp_check_desc(desc, n_rows, row_ptr, col_idx, row_is_eq, &err)) { sco_set_error(err); return rc; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    sco_set_error("sco_sqp_create: no HIP device visible (this library has no CPU fallback)");
    return SCO_ERR_NO_GPU;
  }
  if (device < 0 || device >= ndev) { sco_set_error("sco_sqp_create: bad device index"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(device);
  sco_sqp *h = new sco_sqp();
  h->device = device; h->desc = *desc;
  const int rc = sqp_create_impl(h, device, sqp_layout_build(*desc, n_rows, row_ptr, col_idx, row_is_eq));
  if (rc) { sco_sqp_destroy(h); return rc; }       // frees whatever had been allocated
  *out = h;
  return SCO_OK;
}

extern "C" int sco_sqp_create(int device, const sco_trajopt_desc *desc, sco_sqp **out) {
  return sco_sqp_create_rows(device, desc, 0, nullptr, nullptr, nullptr, out);
}

// stream and allocations, the two QP handles fed from the layout (sqp_layout_build), and the uploads
static int sqp_create_impl(sco_sqp *h, int device, const SqpLayout &L) {
  const sco_trajopt_desc *desc = &h->desc;
  SCO_HIP(hipStreamCreate(&h->stream));
  SCO_HIP(hipHostMalloc((void **)&h->host_active, SQP_MAX_GROUPS * SQP_DEPTH * sizeof(int)));
  {
    void *fb = nullptr;
    SCO_HIP(hipMalloc(&fb, 2 * (size_t)desc->batch * sizeof(double)));
    h->allocs.push_back(fb); h->fetch_buf = (double *)fb;
  }
  const int B = desc->batch, d = desc->dof, T = desc->horizon, K = desc->n_points, O = desc->n_obstacles;
  const int n_x = L.n_x, m_nl = L.m_nl, ds = L.ds, NBt = L.NBt;
  const bool cost = L.cost != OBJ_NONE, oblk = L.cost == OBJ_BLOCK;
  int rc = sco_qp_create_on_stream(device, B, n_x, L.m_lin + n_x, L.qp0.Pp.data(), L.qp0.Pi.data(), L.qp0.Ap.data(), L.qp0.Ai.data(),
                                   h->stream, &h->qp0);
  if (rc) return rc;
  rc = sco_qp_create_on_stream(device, B, L.n, L.m, L.qp1.Pp.data(), L.qp1.Pi.data(), L.qp1.Ap.data(), L.qp1.Ai.data(), h->stream, &h->qp1);
  if (rc) return rc;
  SqpDev &s = h->d;
  s.batch = B; s.d = d; s.T = T; s.K = K; s.O = O; s.R = L.R; s.n_x = n_x; s.n_slack = L.n_slack; s.n = L.n;
  s.m_lin = L.m_lin; s.m_nl = m_nl; s.m = L.m; s.prox_count = desc->prox_count > 0 ? desc->prox_count : 1;
  s.analytic_jac = desc->analytic_jac; s.trace_cap = 64;
  s.point = L.point;
  s.NE = L.NE; s.NB = L.NB; s.RM = L.RM;
  s.S = L.S; s.ds = ds; s.NBt = NBt; s.Req = L.Req;
  s.m_gen = L.m_gen; s.nnz_gen = L.nnz_gen;
  s.acc = L.acc;
  s.m_pin = L.m_pin; s.m_vel = L.m_vel; s.m_jl = L.m_jl; s.cost = L.cost;
#define AL(f, cnt) if ((rc = sq_alloc(h, (cnt), &s.f))) return rc;
  AL(x0, (size_t)B * n_x) AL(start, (size_t)B * d) AL(goal, (size_t)B * d) AL(link_len, (size_t)B * d)
  AL(obstacles, (size_t)B * O * 3) AL(target, (size_t)B * 2) AL(vmax, (size_t)B) AL(jlo, (size_t)B * d) AL(jhi, (size_t)B * d)
  {
    const bool quadf = L.point == ROWS_QUADRATIC;
    AL(qQ, quadf ? (size_t)B * O * ds * ds : 1) AL(qa, quadf ? (size_t)B * O * ds : 1) AL(qc, quadf ? (size_t)B * O : 1)
  }
  {
    const bool spf = L.point == ROWS_SPATIAL;
    AL(sp_off, spf ? (size_t)B * d * 3 : 1) AL(sp_axis, spf ? (size_t)B * d * 3 : 1) AL(sp_pos, spf ? (size_t)B * K * 3 : 1)
    AL(sp_rad, spf ? (size_t)B * K : 1) AL(sp_sph, spf ? (size_t)B * O * 4 : 1)
  }
  AL(x, (size_t)B * n_x) AL(x_saved, (size_t)B * n_x) AL(gsave, (size_t)B * m_nl) AL(J, (size_t)B * m_nl * ds)
  AL(bmod, (size_t)B * m_nl) AL(trace, (size_t)B * s.trace_cap * TRACE_W) AL(mask, (size_t)B * m_nl * ds)
  AL(sc, (size_t)B) AL(active, (size_t)B) AL(n_active, SQP_MAX_GROUPS) AL(newqp, (size_t)B) AL(list_buf, (size_t)B)
  s.H = 40; s.HC = 24;
  AL(hkey, (size_t)B * s.NB * s.H * ds) AL(hval, (size_t)B * s.NB * s.H * s.RM) AL(ckey, (size_t)B * s.NB * s.HC * ds)
  AL(cJ, (size_t)B * s.NB * s.HC * s.RM * ds) AL(cb, (size_t)B * s.NB * s.HC * s.RM) AL(hn, (size_t)B * s.NB)
  AL(cn, (size_t)B * s.NB)
  AL(cw, (size_t)B) AL(ctgt, (size_t)B * 2)
  {
    const size_t NO = oblk ? NBt : T, dO = oblk ? ds : d;     // objective terms and their state
    if (desc->family & SCO_FAM_FLAG_OBJ_WIDE) {
      // a wide term's Hessians: B * NO * dO^2 doubles (2.1 GB at B = 1024, T = 256, dO = 32), refused when they do not fit
      void *p = nullptr;
      const size_t bytes = (size_t)B * NO * dO * dO * sizeof(double);
      if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        char buf[200];
        snprintf(buf, sizeof buf, "sco_sqp_create: the objective terms' Hessians (batch x terms x n^2 doubles) need %zu bytes of "
                 "device memory; use a smaller batch", bytes);
        sco_set_error(buf); return SCO_ERR_CAPACITY;
      }
      h->allocs.push_back(p); s.oH = (double *)p;
      SCO_HIP(hipMemset(p, 0, bytes));
    } else {
      AL(oH, cost ? (size_t)B * NO * dO * dO : 1)
    }
    AL(oA, cost ? (size_t)B * NO * dO : 1) AL(ob, cost ? (size_t)B * NO : 1)
  }
  AL(mvec, (size_t)B * 32) AL(nonconv, (size_t)B) AL(stalled, (size_t)B)
#undef AL
  { int *p; if ((rc = sq_alloc(h, (size_t)K, &p))) return rc; s.point_link = p; }
  { double *p; if ((rc = sq_alloc(h, (size_t)K, &p))) return rc; s.point_frac = p; }
  { unsigned int *p; if ((rc = sq_alloc(h, (size_t)s.NB, &p))) return rc; s.gmask = p; }
  { unsigned int *p; if ((rc = sq_alloc(h, (size_t)32, &p))) return rc; s.goverlap = p; }
  s.G = 0;
  if ((rc = sq_upload(h, L.ppos, &s.ppos)) || (rc = sq_upload(h, L.jpos, &s.jpos)) || (rc = sq_upload(h, L.epos, &s.epos)) ||
      (rc = sq_upload(h, L.a0c, &s.a0c)) || (rc = sq_upload(h, L.a1c, &s.a1c))) return rc;
  s.gen_eq = s.gpos0 = s.gpos1 = nullptr; s.gen_rhs = s.gen_val = nullptr;
  if (L.m_gen) {
    double *q;
    if ((rc = sq_upload(h, L.gen_eq, &s.gen_eq)) || (rc = sq_upload(h, L.gpos0, &s.gpos0)) || (rc = sq_upload(h, L.gpos1, &s.gpos1))) return rc;
    if ((rc = sq_alloc(h, (size_t)B * L.m_gen, &q))) return rc; s.gen_rhs = q;
    if ((rc = sq_alloc(h, (size_t)B * L.nnz_gen, &q))) return rc; s.gen_val = q;
  }
  return SCO_OK;
}

extern "C" int sco_sqp_destroy(sco_sqp *h) {
  if (!h) return SCO_OK;
  ScoDeviceGuard sco_guard_(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->qp0) sco_qp_destroy(h->qp0);
  if (h->qp1) sco_qp_destroy(h->qp1);
  for (void *p : h->allocs) (void)hipFree(p);
  for (void *p : h->prog_buf) if (p) (void)hipFree(p);
  if (h->objw_buf) (void)hipFree(h->objw_buf);
  if (h->accw_buf) (void)hipFree(h->accw_buf);
  h->events.destroy(); h->done.destroy(); h->mix_events.destroy();
  for (auto &ge : h->gevents) ge.destroy();
  for (auto gs : h->gstream) if (gs) { (void)hipStreamSynchronize(gs); (void)hipStreamDestroy(gs); }
  if (h->host_active) (void)hipHostFree(h->host_active);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return SCO_OK;
}

extern "C" int sco_sqp_load(sco_sqp *h, const double *x0, const double *start, const double *goal,
                            const double *link_len, const int *point_link, const double *point_frac,
                            const double *obstacles) {
  if (!h || !x0 || !start || !goal || !link_len || !point_link || !point_frac || !obstacles) {
    sco_set_error("sco_sqp_load: null pointer"); return SCO_ERR_ARG;
  }
  const SqpDev &s = h->d;
  for (int k = 0; k < s.K; k++)
    if (point_link[k] < 0 || point_link[k] >= s.d) { sco_set_error("sco_sqp_load: point_link out of range"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  const size_t B = s.batch;
  SCO_HIP(hipMemcpyAsync(s.x0, x0, B * s.n_x * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(s.start, start, B * s.d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(s.goal, goal, B * s.d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(s.link_len, link_len, B * s.d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(s.obstacles, obstacles, B * s.O * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync((void *)s.point_link, point_link, s.K * sizeof(int), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync((void *)s.point_frac, point_frac, s.K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  {
    // the serial-arm families promise the penalty QP the widths of their hinge rows (sqp_row_widths); any other family
    // withdraws what an earlier load may have promised
    std::vector<int> w;
    const bool hint = sqp_row_widths(s.point, s.S, s.d, s.O, s.R, s.NBt, s.m_lin, s.m, point_link, w);
    if (int rc = sco_qp_set_row_widths(h->qp1, hint ? w.data() : nullptr)) return rc;
  }
  h->loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_ee_cost(sco_sqp *h, const double *weight, const double *target) {
  if (!h || !weight || !target) { sco_set_error("sco_sqp_load_ee_cost: null pointer"); return SCO_ERR_ARG; }
  if (!(h->desc.family & SCO_FAM_FLAG_EE_COST)) { sco_set_error("sco_sqp_load_ee_cost: family has no objective term"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_ee_cost: call sco_sqp_load first"); return SCO_ERR_STATE; }
  for (int b = 0; b < h->d.batch; b++)
    if (!(weight[b] >= 0.0)) { sco_set_error("sco_sqp_load_ee_cost: weight must be >= 0"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpyAsync(h->d.cw, weight, (size_t)h->d.batch * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(h->d.ctgt, target, (size_t)h->d.batch * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->cost_loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_target(sco_sqp *h, const double *target) {
  if (!h || !target) { sco_set_error("sco_sqp_load_target: null pointer"); return SCO_ERR_ARG; }
  if ((h->desc.family & 15) != SCO_FAM_ARM_REACH) { sco_set_error("sco_sqp_load_target: family has no target"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_target: call sco_sqp_load first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpyAsync(h->d.target, target, (size_t)h->d.batch * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->target_loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_vel_limit(sco_sqp *h, const double *vmax) {
  if (!h || !vmax) { sco_set_error("sco_sqp_load_vel_limit: null pointer"); return SCO_ERR_ARG; }
  if (!(h->desc.family & SCO_FAM_FLAG_VEL_LIMITS)) { sco_set_error("sco_sqp_load_vel_limit: family has no velocity limits"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_vel_limit: call sco_sqp_load first"); return SCO_ERR_STATE; }
  for (int b = 0; b < h->d.batch; b++)
    if (!(vmax[b] > 0.0)) { sco_set_error("sco_sqp_load_vel_limit: vmax must be positive"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpyAsync(h->d.vmax, vmax, (size_t)h->d.batch * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->vel_loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_joint_limits(sco_sqp *h, const double *lo, const double *hi) {
  if (!h || !lo || !hi) { sco_set_error("sco_sqp_load_joint_limits: null pointer"); return SCO_ERR_ARG; }
  if (!(h->desc.family & SCO_FAM_FLAG_JOINT_LIMITS)) { sco_set_error("sco_sqp_load_joint_limits: family has no joint limits"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_joint_limits: call sco_sqp_load first"); return SCO_ERR_STATE; }
  const size_t cnt = (size_t)h->d.batch * h->d.d;
  for (size_t k = 0; k < cnt; k++)
    if (!(lo[k] < hi[k])) { sco_set_error("sco_sqp_load_joint_limits: need lo < hi"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpyAsync(h->d.jlo, lo, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(h->d.jhi, hi, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->jl_loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_quadratic(sco_sqp *h, const double *Q, const double *a, const double *c) {
  if (!h || !Q || !a || !c) { sco_set_error("sco_sqp_load_quadratic: null pointer"); return SCO_ERR_ARG; }
  if ((h->desc.family & 15) != SCO_FAM_STATE_QUADRATIC) { sco_set_error("sco_sqp_load_quadratic: family has no quadratic rows"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_quadratic: call sco_sqp_load first"); return SCO_ERR_STATE; }
  const size_t B = h->d.batch, O = h->d.O, d = h->d.d;
  for (size_t k = 0; k < B * O; k++)
    for (size_t i = 0; i < d; i++)
      for (size_t j = 0; j < i; j++)
        if (Q[k * d * d + i * d + j] != Q[k * d * d + j * d + i]) { sco_set_error("sco_sqp_load_quadratic: Q must be symmetric"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpyAsync(h->d.qQ, Q, B * O * d * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(h->d.qa, a, B * O * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipMemcpyAsync(h->d.qc, c, B * O * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->quad_loaded = true; h->solved = false;
  return SCO_OK;
}

// SCO_FAM_ARM_SPATIAL: the arm's geometry and the sphere obstacles of every problem, into buffers the handle owns since its
// creation (the call may be repeated).  Everything is checked before anything is copied.
extern "C" int sco_sqp_load_spatial(sco_sqp *h, const double *joint_off, const double *joint_axis, const double *point_pos,
                                    const double *point_rad, const double *spheres) {
  if (!h || !joint_off || !joint_axis || !point_pos || !point_rad || !spheres) { sco_set_error("sco_sqp_load_spatial: null pointer"); return SCO_ERR_ARG; }
  if ((h->desc.family & 15) != SCO_FAM_ARM_SPATIAL) { sco_set_error("sco_sqp_load_spatial: family has no spatial arm"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_spatial: call sco_sqp_load first"); return SCO_ERR_STATE; }
  const SqpDev &s = h->d;
  const size_t B = s.batch, d = s.d, K = s.K, O = s.O;
  const double *arr[5] = {joint_off, joint_axis, point_pos, point_rad, spheres};
  const size_t cnt[5] = {B * d * 3, B * d * 3, B * K * 3, B * K, B * O * 4};
  for (int a = 0; a < 5; a++)
    for (size_t k = 0; k < cnt[a]; k++)
      if (!std::isfinite(arr[a][k])) { sco_set_error("sco_sqp_load_spatial: non-finite number"); return SCO_ERR_ARG; }
  for (size_t k = 0; k < B * d; k++) {
    const double *a = joint_axis + 3 * k;
    if (fabs(sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) - 1.0) > 1e-9) { sco_set_error("sco_sqp_load_spatial: joint axes must be unit vectors"); return SCO_ERR_ARG; }
  }
  for (size_t k = 0; k < B * K; k++)
    if (point_rad[k] < 0.0) { sco_set_error("sco_sqp_load_spatial: negative radius"); return SCO_ERR_ARG; }
  for (size_t k = 0; k < B * O; k++)
    if (spheres[4 * k + 3] < 0.0) { sco_set_error("sco_sqp_load_spatial: negative radius"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  double *dst[5] = {s.sp_off, s.sp_axis, s.sp_pos, s.sp_rad, s.sp_sph};
  for (int a = 0; a < 5; a++) SCO_HIP(hipMemcpyAsync(dst[a], arr[a], cnt[a] * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  h->spatial_loaded = true; h->solved = false;
  return SCO_OK;
}

static int load_program_impl(sco_sqp *h, int n_words, const int *words, const int *row_ptr, int n_consts, const double *consts,
                             int n_params, const double *params, bool per_step) {
  if (!h || !words || !row_ptr || (n_consts > 0 && !consts) || (n_params > 0 && !params)) {
    sco_set_error("sco_sqp_load_program: null pointer"); return SCO_ERR_ARG;
  }
  if ((h->desc.family & 15) != SCO_FAM_STATE_PROGRAM) { sco_set_error("sco_sqp_load_program: family has no row programs"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_program: call sco_sqp_load first"); return SCO_ERR_STATE; }
  // the rows of a block (behind its R1 circle rows), then the objective term's program: layout, stack depth, operands
  const char *err = "";
  if (int rc = sqp_check_program(h->d.O - h->d.R1, h->d.cost, h->d.ds, h->d.d, n_words, words, row_ptr, n_consts, n_params, &err)) {
    sco_set_error(err); return rc;
  }
  const int R = h->d.O - h->d.R1 + (obj_is_program(h->d.cost) ? 1 : 0);
  SCO_ON_DEVICE(h->device);
  SqpDev &s = h->d;
  // the four buffers belong to the handle: a reload of the same sizes (new parameters per solve) reuses them, another
  // size frees the old ones first
  const size_t need[4] = {(size_t)2 * n_words * sizeof(int), ((size_t)R + 1) * sizeof(int), (size_t)std::max(n_consts, 1) * sizeof(double),
                          std::max<size_t>((size_t)s.batch * (per_step ? s.T : 1) * n_params, 1) * sizeof(double)};
  // From here until every buffer is in place and filled the handle has NO program: a failed hipMalloc / hipMemcpy below
  // returns early, and the kernels of a later sco_sqp_solve must not read freed or half-written buffers (solve refuses
  // while prog_loaded is false).
  h->prog_loaded = false; h->solved = false;
  s.pw = nullptr; s.pptr = nullptr; s.pconst = nullptr; s.ppar = nullptr; s.n_par = 0; s.par_step = 0;
  for (int k = 0; k < 4; k++)
    if (h->prog_bytes[k] != need[k]) {
      if (h->prog_buf[k]) { (void)hipFree(h->prog_buf[k]); h->prog_buf[k] = nullptr; h->prog_bytes[k] = 0; }
      SCO_HIP(hipMalloc(&h->prog_buf[k], need[k]));
      h->prog_bytes[k] = need[k];
    }
  SCO_HIP(hipMemcpy(h->prog_buf[0], words, (size_t)2 * n_words * sizeof(int), hipMemcpyHostToDevice));
  SCO_HIP(hipMemcpy(h->prog_buf[1], row_ptr, ((size_t)R + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (n_consts) SCO_HIP(hipMemcpy(h->prog_buf[2], consts, (size_t)n_consts * sizeof(double), hipMemcpyHostToDevice));
  if (n_params) SCO_HIP(hipMemcpy(h->prog_buf[3], params, (size_t)s.batch * (per_step ? s.T : 1) * n_params * sizeof(double), hipMemcpyHostToDevice));
  s.pw = (const int *)h->prog_buf[0]; s.pptr = (const int *)h->prog_buf[1];
  s.pconst = (const double *)h->prog_buf[2]; s.ppar = (const double *)h->prog_buf[3]; s.n_par = n_params;
  s.par_step = per_step ? n_params : 0;
  h->prog_loaded = true; h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_load_program(sco_sqp *h, int n_words, const int *words, const int *row_ptr, int n_consts, const double *consts,
                                    int n_params, const double *params) {
  return load_program_impl(h, n_words, words, row_ptr, n_consts, consts, n_params, params, false);
}
// r04: parameters per problem AND timestep, params[batch][horizon][n_params]: block t (the Variable of timesteps t .. t + span - 1)
// and the objective term of timestep t are evaluated with params[problem][t] -- what a caller of the reference gets by closing
// each timestep's Expr over its own data (moving obstacles, time-varying references; expr.py:22-41, prob.py:112-144)
extern "C" int sco_sqp_load_program_steps(sco_sqp *h, int n_words, const int *words, const int *row_ptr, int n_consts,
                                          const double *consts, int n_params, const double *params) {
  return load_program_impl(h, n_words, words, row_ptr, n_consts, consts, n_params, params, true);
}

// r04 (SCO_FAM_FLAG_ACC_COST): weights a[batch][dof] >= 0 of the acceleration term of the quadratic objective,
//     sum_t sum_j a_j (theta[t+2][j] - 2 theta[t+1][j] + theta[t][j])^2,
// next to the (weighted) velocity term -- the QuadExpr a caller builds from first AND second difference matrices (prob.py:88-104,
// 348-367).  P gets its second super-diagonal block (pattern fixed at sco_sqp_create by the flag).  After sco_sqp_load; nullptr = 0.
extern "C" int sco_sqp_load_acc_weights(sco_sqp *h, const double *a) {
  if (!h) { sco_set_error("sco_sqp_load_acc_weights: null pointer"); return SCO_ERR_ARG; }
  if (!h->d.acc) { sco_set_error("sco_sqp_load_acc_weights: the handle was created without SCO_FAM_FLAG_ACC_COST"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_acc_weights: call sco_sqp_load first"); return SCO_ERR_STATE; }
  SqpDev &s = h->d;
  if (!a) { s.accw = nullptr; h->solved = false; return SCO_OK; }
  for (size_t i = 0; i < (size_t)s.batch * s.d; i++)
    if (!(a[i] >= 0.0) || !(a[i] < 1e30)) { sco_set_error("sco_sqp_load_acc_weights: weights must be finite and >= 0"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  s.accw = nullptr;
  if (!h->accw_buf) SCO_HIP(hipMalloc(&h->accw_buf, (size_t)s.batch * s.d * sizeof(double)));
  SCO_HIP(hipMemcpy(h->accw_buf, a, (size_t)s.batch * s.d * sizeof(double), hipMemcpyHostToDevice));
  s.accw = (const double *)h->accw_buf;
  h->solved = false;
  return SCO_OK;
}

// r04: two kinds of non-linear rows in one problem.  SCO_FAM_STATE_PROGRAM, span 1, before sco_sqp_load_program: the first n_rows
// rows of every block are keep-out rows r_o - || x[0:2] - c_o || of the point (x[0], x[1]) against obstacles[b][0 .. n_rows) of
// sco_sqp_load (SCO_FAM_POINT_CIRCLES' rows); the program supplies the remaining n_obstacles - n_rows rows.  In the reference: two
// BoundExprs on the same timestep Variable, the circle Expr added first (prob.py:112-144).  0 restores the plain program family.
extern "C" int sco_sqp_set_circle_rows(sco_sqp *h, int n_rows) {
  if (!h) { sco_set_error("sco_sqp_set_circle_rows: null pointer"); return SCO_ERR_ARG; }
  if ((h->desc.family & 15) != SCO_FAM_STATE_PROGRAM || h->d.S != 1 || h->d.d < 2) {
    sco_set_error("sco_sqp_set_circle_rows: program family on single timesteps with dof >= 2 only"); return SCO_ERR_ARG;
  }
  if (n_rows < 0 || n_rows >= h->d.O || n_rows > h->d.O - h->d.Req - 1 + 1) { sco_set_error("sco_sqp_set_circle_rows: 0 <= n_rows < rows per block, equality rows belong to the program"); return SCO_ERR_ARG; }
  if (n_rows != h->d.R1) { h->prog_loaded = false; h->solved = false; }       // the program's row count changes with it
  h->d.R1 = n_rows;
  return SCO_OK;
}

// r04: coefficients vals[batch][nnz] (CSR order of the pattern given to sco_sqp_create_rows) and right-hand sides
// rhs[batch][n_rows] of the general affine rows; after sco_sqp_load, before sco_sqp_solve; may be called again.
extern "C" int sco_sqp_load_linear_rows(sco_sqp *h, const double *vals, const double *rhs) {
  if (!h || !vals || !rhs) { sco_set_error("sco_sqp_load_linear_rows: null pointer"); return SCO_ERR_ARG; }
  SqpDev &s = h->d;
  if (!s.m_gen) { sco_set_error("sco_sqp_load_linear_rows: the handle was created without general affine rows"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_linear_rows: call sco_sqp_load first"); return SCO_ERR_STATE; }
  for (size_t i = 0; i < (size_t)s.batch * s.nnz_gen; i++)
    if (!(fabs(vals[i]) < 1e30)) { sco_set_error("sco_sqp_load_linear_rows: coefficients must be finite"); return SCO_ERR_ARG; }
  for (size_t i = 0; i < (size_t)s.batch * s.m_gen; i++)
    if (!(fabs(rhs[i]) < 1e30)) { sco_set_error("sco_sqp_load_linear_rows: right-hand sides must be finite"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpy((void *)s.gen_val, vals, (size_t)s.batch * s.nnz_gen * sizeof(double), hipMemcpyHostToDevice));
  SCO_HIP(hipMemcpy((void *)s.gen_rhs, rhs, (size_t)s.batch * s.m_gen * sizeof(double), hipMemcpyHostToDevice));
  h->gen_loaded = true; h->solved = false;
  return SCO_OK;
}

// r04: weights of the smoothing objective, w[batch][dof] >= 0: sum_t sum_j w_j (theta[t+1][j] - theta[t][j])^2 -- the QuadExpr a
// caller of the reference builds with a weighted difference matrix (prob.py:88-104, 348-367).  After sco_sqp_load; nullptr
// restores the unweighted objective.
extern "C" int sco_sqp_load_obj_weights(sco_sqp *h, const double *w) {
  if (!h) { sco_set_error("sco_sqp_load_obj_weights: null pointer"); return SCO_ERR_ARG; }
  if (!h->loaded) { sco_set_error("sco_sqp_load_obj_weights: call sco_sqp_load first"); return SCO_ERR_STATE; }
  SqpDev &s = h->d;
  if (!w) { s.objw = nullptr; h->solved = false; return SCO_OK; }
  for (size_t i = 0; i < (size_t)s.batch * s.d; i++)
    if (!(w[i] >= 0.0) || !(w[i] < 1e30)) { sco_set_error("sco_sqp_load_obj_weights: weights must be finite and >= 0"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(h->device);
  s.objw = nullptr;
  if (!h->objw_buf) SCO_HIP(hipMalloc(&h->objw_buf, (size_t)s.batch * s.d * sizeof(double)));
  SCO_HIP(hipMemcpy(h->objw_buf, w, (size_t)s.batch * s.d * sizeof(double), hipMemcpyHostToDevice));
  s.objw = (const double *)h->objw_buf;
  h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_set_groups(sco_sqp *h, int n_groups, const unsigned int *block_mask) {
  if (!h || !block_mask) { sco_set_error("sco_sqp_set_groups: null pointer"); return SCO_ERR_ARG; }
  if (n_groups < 1 || n_groups > 32) { sco_set_error("sco_sqp_set_groups: 1..32 groups"); return SCO_ERR_ARG; }
  SqpDev &s = h->d;
  const unsigned int all = n_groups == 32 ? 0xffffffffu : ((1u << n_groups) - 1u);
  unsigned int overlap[32] = {0};
  for (int blk = 0; blk < s.NB; blk++) {
    const unsigned int mk = block_mask[blk];
    if (mk == 0u || (mk & ~all)) { sco_set_error("sco_sqp_set_groups: every block needs a group < n_groups"); return SCO_ERR_ARG; }
    for (int g = 0; g < n_groups; g++) if ((mk >> g) & 1u) overlap[g] |= mk & ~(1u << g);    // prob.py:139-142
  }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpy((void *)s.gmask, block_mask, (size_t)s.NB * sizeof(unsigned int), hipMemcpyHostToDevice));
  SCO_HIP(hipMemcpy((void *)s.goverlap, overlap, sizeof overlap, hipMemcpyHostToDevice));
  s.G = n_groups;
  h->solved = false;
  return SCO_OK;
}

extern "C" int sco_sqp_fetch_flags(sco_sqp *h, int *flags) {
  if (!h || !flags) return SCO_ERR_ARG;
  if (!h->solved) { sco_set_error("sco_sqp_fetch_flags: call sco_sqp_solve first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  const size_t B = h->d.batch;
  std::vector<SqpScalars> sc(B);
  SCO_HIP(hipMemcpy(sc.data(), h->d.sc, B * sizeof(SqpScalars), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; b++) flags[b] = sc[b].flags;
  return SCO_OK;
}

extern "C" int sco_sqp_fetch_groups(sco_sqp *h, unsigned int *nonconverged) {
  if (!h || !nonconverged) return SCO_ERR_ARG;
  if (!h->solved) { sco_set_error("sco_sqp_fetch_groups: call sco_sqp_solve first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpy(nonconverged, h->d.nonconv, (size_t)h->d.batch * sizeof(unsigned int), hipMemcpyDeviceToHost));
  return SCO_OK;
}

extern "C" int sco_sqp_fetch_stalled_groups(sco_sqp *h, unsigned int *stalled) {
  if (!h || !stalled) return SCO_ERR_ARG;
  if (!h->solved) { sco_set_error("sco_sqp_fetch_stalled_groups: call sco_sqp_solve first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  SCO_HIP(hipMemcpy(stalled, h->d.stalled, (size_t)h->d.batch * sizeof(unsigned int), hipMemcpyDeviceToHost));
  return SCO_OK;
}

// Which problems take part in the next round.  A workgroup of the ADMM kernels fills a CU and the hardware deals the
// workgroups of a launch to XCDs and shader engines in a fixed rotation, waiting for the engine whose turn it is: a
// workgroup that finds its problem inactive and exits at once still takes its turn, so a launch of 1024 workgroups of
// which 768 have work costs four passes of the chip, not three (measured, profiles/r02_rounds.txt), and
// once problems start to finish the last pass of every lock-step round is partly empty.  With more active problems
// than CUs a round therefore runs P = floor(active / CUs) whole passes as a COMPACT launch: this kernel lists the
// P x CUs problems with most in front of them as far as the device can tell -- the slices their current QP has left if
// it runs to max_iter, one more QP for a problem still in its first penalty QP (a step is normally followed by at
// least one more), ties by index -- and workgroup g of the round's kernels takes problem list[g].  The host sizes the
// launch from the active count it read back SQP_DEPTH rounds earlier (`cap`, never too small: the count only falls);
// surplus workgroups find -1 and exit.  The others are not visited: per problem the sequence of kernels and every
// result is unchanged, only the round it happens in moves (model on the measured chains, 1024 problems at 7x20:
// 667 -> 636 ms per step; choosing by the true remaining work would give 629, profiles/r02_slice_model.txt).
// n_active starts the round at the number of live problems left out (sqp_post_kernel adds those that ran and go on).
// `order` (mixed rounds, at most SEL_T listed problems): the list is then sorted by that estimate, most in front first, ties by
// index -- its head is the side window of the round.
#define SEL_T 1024
#define SEL_BUCKETS 1024
static_assert(SEL_T == SQP_SEL_MAX && SCO_WV_PER_CU == SQP_WV_PER_CU, "sqp_sched.h plans with the kernels' sizes");
// (r03: the kernel works on the problems [s.b0, s.b0 + nb) of a stream group and fills that group's part of the list, so
// selection and stream groups combine: SCO_SQP_GROUPS)
__global__ __launch_bounds__(SEL_T) void sqp_select_kernel(SqpDev s, QpDev q1, int cus, int slice, int max_iter, int cap, int nb, int order) {
  __shared__ int hist[SEL_BUCKETS];
  __shared__ int part[SEL_T], part2[SEL_T];
  __shared__ int s_active, s_thr, s_take;
  const int tid = threadIdx.x, B = nb, gb0 = s.b0;
  int *list = s.list_buf + gb0;
  for (int k = tid; k < SEL_BUCKETS; k += SEL_T) hist[k] = 0;
  if (tid == 0) s_active = 0;
  __syncthreads();
  const int per_qp = slice > 0 ? (max_iter + slice - 1) / slice : 1;
  // bucket 0 = most in front of it; -1 = finished
  auto key_of = [&](int b) -> int {
    const SqpScalars &sc = s.sc[b];
    if (sc.state == ST_DONE) return -1;
    const int done = (q1.prog && slice > 0) ? q1.prog[b] / slice : 0;
    const int est = max(per_qp - done, 0) + (sc.qp_solves <= 1 ? per_qp : 0);
    return max(SEL_BUCKETS - 1 - est, 0);
  };
  const int per = (B + SEL_T - 1) / SEL_T, b0 = gb0 + min(B, tid * per), b1 = min(gb0 + B, b0 + per);
  int mine = 0;
  for (int b = b0; b < b1; b++) {
    const int k = key_of(b);
    if (k >= 0) { atomicAdd(&hist[k], 1); mine++; }
  }
  if (mine) atomicAdd(&s_active, mine);
  __syncthreads();
  const int A = s_active;
  const int quota = min(cap, (cus <= 0 || A <= cus) ? A : (A / cus) * cus);
  if (tid == 0) {
    int acc = 0, k = 0;
    for (; k < SEL_BUCKETS; k++) { if (acc + hist[k] > quota) break; acc += hist[k]; }
    s_thr = k; s_take = quota - acc;           // every bucket below s_thr runs; of bucket s_thr the first s_take by index
    *s.n_active = A - quota;
  }
  __syncthreads();
  const int thr = s_thr, take = s_take;
  // two exclusive scans over the threads' consecutive chunks: members of bucket thr (ties), then chosen problems
  int cnt = 0;
  for (int b = b0; b < b1; b++) cnt += key_of(b) == thr ? 1 : 0;
  part[tid] = cnt;
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int t = 0; t < SEL_T; t++) { const int v = part[t]; part[t] = acc; acc += v; } }
  __syncthreads();
  int seen = part[tid], chosen = 0;
  for (int b = b0; b < b1; b++) {
    const int k = key_of(b);
    if (k >= 0 && k < thr) chosen++;
    else if (k == thr) { if (seen < take) chosen++; seen++; }
  }
  part2[tid] = chosen;
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int t = 0; t < SEL_T; t++) { const int v = part2[t]; part2[t] = acc; acc += v; } }
  __syncthreads();
  int pos = part2[tid];
  seen = part[tid];
  for (int b = b0; b < b1; b++) {
    const int k = key_of(b);
    bool r = false;
    if (k >= 0 && k < thr) r = true;
    else if (k == thr) { r = seen < take; seen++; }
    if (r) list[pos++] = b;
  }
  for (int g = quota + tid; g < cap; g += SEL_T) list[g] = -1;
  if (order && quota <= SEL_T) {
    // rank of every listed problem among the listed ones by (bucket, position): a stable counting sort, one problem per thread
    __syncthreads();
    const int mine_b = tid < quota ? list[tid] : -1, mine_k = tid < quota ? key_of(mine_b) : SEL_BUCKETS;
    part[tid] = mine_k;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < quota; j++) { const int kj = part[j]; rank += (kj < mine_k || (kj == mine_k && j < tid)) ? 1 : 0; }
    __syncthreads();
    if (tid < quota) list[rank] = mine_b;
  }
}

// problems the host loop's launch cap left unfinished: failed + SCO_SQP_FLAG_CAPPED
__global__ void sqp_cap_kernel(SqpDev s) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.batch) return;
  SqpScalars &sc = s.sc[b];
  if (sc.state != ST_DONE) { sc.state = ST_DONE; sc.success = 0; sc.flags |= SCO_SQP_FLAG_CAPPED; s.active[b] = 0; }
}

// XCDs the device deals the workgroups of a launch to (qp_mix_split).  HIP has no attribute for it: eight on the CDNA3 / CDNA4
// parts whose CU count they divide, else one (SCO_SQP_XCDS overrides: sqp_sched.cpp).
static int sqp_xcds(int device, int cus) {
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, device) != hipSuccess) { (void)hipGetLastError(); return 1; }
  const bool multi = !strncmp(pr.gcnArchName, "gfx94", 5) || !strncmp(pr.gcnArchName, "gfx95", 5);
  return (multi && cus > 0 && cus % 8 == 0) ? 8 : 1;
}

// Timed events of one stream: event i ends the interval that is charged to stage[i] (0 convexify, 1 QP setup, 2 ADMM, 5 ADMM
// on the wavefront tier, 3 decisions; < 0: nobody)
struct StageMarks {
  EventPool *pool = nullptr; hipStream_t st = nullptr;
  std::vector<int> stage;
  int take(int stg, hipEvent_t *e) { stage.push_back(stg); return pool->next(e); }      // an event the callee records
  int mark(int stg) {
    hipEvent_t e; SCO_TRY(take(stg, &e)); SCO_HIP(hipEventRecord(e, st));
    return SCO_OK;
  }
};

struct SqpGroupRun {                                   // one stream group of the round loop
  int b0 = 0, nb = 0; hipStream_t st = nullptr;
  int issued = 0, retired = 0, last_active = 1;        // rounds enqueued / read back; active count of the last one read
  StageMarks marks;
};
struct SqpLoop {                                       // state of the round loop of one sco_sqp_solve
  sco_sqp *h = nullptr;
  SqpParamsDev p{};
  sco_qp_settings qsl{};
  SqpSchedule sc;
  StageMarks main;                                     // the main stream: projection round, start of the stream groups
  SqpGroupRun grp[SQP_MAX_GROUPS];
  hipEvent_t done[SQP_MAX_GROUPS * SQP_DEPTH] = {};    // per (group, slot): the round's read-back has landed
  int wv_rounds = 0, mixed_rounds = 0, mixed_side = 0;
  std::vector<int> round_k;                            // per round of group 0: -1 row-local, 0 wavefront, k > 0 mixed (SCO_SQP_TRACE_ROUNDS)
  bool capped = false;
};

static int sqp_check_state(const sco_sqp *h, const sco_sqp_params *params, const sco_qp_settings *qs) {
  if (!h || !params || !qs) { sco_set_error("sco_sqp_solve: null pointer"); return SCO_ERR_ARG; }
  const int fam = h->desc.family;
  const char *missing = !h->loaded ? "sco_sqp_load"
      : ((fam & 15) == SCO_FAM_ARM_REACH && !h->target_loaded) ? "sco_sqp_load_target"
      : ((fam & SCO_FAM_FLAG_VEL_LIMITS) && !h->vel_loaded) ? "sco_sqp_load_vel_limit"
      : ((fam & SCO_FAM_FLAG_EE_COST) && !h->cost_loaded) ? "sco_sqp_load_ee_cost"
      : ((fam & SCO_FAM_FLAG_JOINT_LIMITS) && !h->jl_loaded) ? "sco_sqp_load_joint_limits"
      : (h->d.m_gen && !h->gen_loaded) ? "sco_sqp_load_linear_rows"
      : ((fam & 15) == SCO_FAM_STATE_PROGRAM && !h->prog_loaded) ? "sco_sqp_load_program"
      : ((fam & 15) == SCO_FAM_STATE_QUADRATIC && !h->quad_loaded) ? "sco_sqp_load_quadratic"
      : ((fam & 15) == SCO_FAM_ARM_SPATIAL && !h->spatial_loaded) ? "sco_sqp_load_spatial" : nullptr;
  if (missing) { sco_set_error(std::string("sco_sqp_solve: call ") + missing + " first"); return SCO_ERR_STATE; }
  return SCO_OK;
}

// settings are checked before the first launch: nothing on the device is touched by a call that is going to fail
static int sqp_check_settings(const sco_sqp *h, const sco_sqp_params *params, const sco_qp_settings *qs) {
  if (qs->max_iter <= 0 || !(qs->rho > 0) || !(qs->sigma > 0) || qs->scaling < 0 || !(qs->alpha > 0) || !(qs->alpha < 2)) {
    sco_set_error("sco_sqp_solve: bad QP settings (max_iter, rho, sigma > 0; 0 < alpha < 2; scaling >= 0)"); return SCO_ERR_ARG;
  }
  if (!(params->initial_trust_region_size > 0) || !(params->initial_penalty_coeff > 0) ||
      !(params->trust_shrink_ratio > 0) || !(params->trust_expand_ratio > 0) || !(params->merit_coeff_increase_ratio > 0) ||
      params->max_merit_coeff_increases < 0) {
    sco_set_error("sco_sqp_solve: bad SQP parameters"); return SCO_ERR_ARG;
  }
  if (qs->adaptive_rho) {
    if (!(qs->adaptive_rho_tolerance > 1.0) || qs->check_termination <= 0) {
      sco_set_error("sco_sqp_solve: adaptive_rho needs adaptive_rho_tolerance > 1 and check_termination > 0"); return SCO_ERR_ARG;
    }
    if (!sco_qp_can_adapt(h->qp1)) {
      sco_set_error("sco_sqp_solve: adaptive_rho: the dense form of the global-memory tier cannot park a solve");
      return SCO_ERR_CAPACITY;
    }
  }
  return SCO_OK;
}

// ---- round 0: projection onto the linear constraints, DEFAULT QP settings (Q7); *n_active: the problems that go on
static int sqp_projection_round(sco_sqp *h, const SqpParamsDev &p, StageMarks &main, int *n_active) {
  const SqpDev &s = h->d;
  const dim3 grid(s.batch), block(SCO_BLOCK);
  SCO_TRY(main.mark(-1));
  SCO_HIP(hipMemsetAsync(s.n_active, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(sqp_proj_assemble_kernel, grid, block, 0, h->stream, s, h->qp0->d);
  SCO_HIP(hipGetLastError());
  SCO_TRY(main.mark(0));
  sco_qp_settings q0s; sco_qp_default_settings(&q0s);
  hipEvent_t mid;
  SCO_TRY(main.take(1, &mid));
  SCO_TRY(sco_qp_launch(h->qp0, &q0s, nullptr, mid));
  SCO_TRY(main.mark(2));
  hipLaunchKernelGGL(sqp_proj_post_kernel, grid, block, 0, h->stream, s, h->qp0->d, h->qp1->d, p);
  SCO_HIP(hipGetLastError());
  SCO_TRY(main.mark(3));
  SCO_HIP(hipMemcpyAsync(n_active, s.n_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SCO_HIP(hipStreamSynchronize(h->stream));
  return SCO_OK;
}

// the penalty QP's handle before the first round: settings of the rounds' QPs (*qsl), nothing parked, counters at zero
static int sqp_reset_penalty_qp(sco_sqp *h, const sco_sqp_params *params, const sco_qp_settings *qs, sco_qp_settings *qsl) {
  *qsl = *qs;
  if (params->warm_start_qps) {
    // beyond parity: every penalty QP starts from the previous one's solution; the first one from zero
    qsl->warm_start = 1;
    const QpDev &q1 = h->qp1->d;
    SCO_HIP(hipMemsetAsync(q1.x, 0, (size_t)q1.batch * q1.n * sizeof(double), h->stream));
    SCO_HIP(hipMemsetAsync(q1.y, 0, (size_t)q1.batch * q1.m * sizeof(double), h->stream));
    h->qp1->solved_once = true;
  }
  SCO_HIP(hipMemsetAsync(h->qp1->d.prog, 0, (size_t)h->d.batch * sizeof(int), h->stream));
  sco_qp_wv_iters_reset(h->qp1, h->stream);
  return SCO_OK;
}

static SqpSchedule sqp_plan(sco_sqp *h, int admm_slice, const sco_qp_settings &qsl, int max_qp_solves, int n_active) {
  SqpSchedIn in;
  in.batch = h->d.batch;
  (void)hipDeviceGetAttribute(&in.cus, hipDeviceAttributeMultiprocessorCount, h->device);
  in.admm_slice = admm_slice; in.max_qp_solves = max_qp_solves; in.n_active = n_active;
  in.adaptive_rho = qsl.adaptive_rho; in.max_iter = qsl.max_iter;
  in.adaptive_interval = qsl.adaptive_rho ? sco_qp_adaptive_interval(&qsl) : 0;
  in.supports_groups = sco_qp_supports_groups(h->qp1, &qsl);
  // (link rows have no adaptive-rho instantiation on the wavefront tier: the QP layer keeps such launches off it)
  in.handle_wv = sco_qp_has_wv(h->qp1) && !(qsl.adaptive_rho && sco_qp_wv_links(h->qp1));
  in.wv_min = sco_wv_min_live(in.cus, qsl.adaptive_rho != 0);
  if (in.handle_wv) {                           // (mixed rounds need the wavefront tier; the device is asked once per handle)
    if (!h->xcds) h->xcds = sqp_xcds(h->device, in.cus);
    in.xcds = h->xcds;
  }
  in.env = sqp_sched_env();
  return sqp_schedule_plan(in);
}

static int sqp_loop_start(SqpLoop &L) {
  sco_sqp *h = L.h;
  const SqpSchedule &sc = L.sc;
  if (sc.trace) fprintf(stderr, "sco_sqp_solve: %d CUs, %d stream group(s), round selection %s, slice %d\n", sc.cus, sc.G, sc.select ? "on" : "off", sc.slice);
  if (sc.mix_on && !h->gstream[0]) SCO_HIP(hipStreamCreate(&h->gstream[0]));
  h->groups_used = sc.G;
  for (int g = 1; g < sc.G; g++)
    if (!h->gstream[g - 1]) SCO_HIP(hipStreamCreate(&h->gstream[g - 1]));
  for (int g = 0; g < sc.G; g++) {
    SqpGroupRun &r = L.grp[g];
    r.b0 = sc.grp[g].b0; r.nb = sc.grp[g].nb; r.last_active = sc.grp[g].live;
    r.st = g == 0 ? h->stream : h->gstream[g - 1];
    h->gevents[g].rewind();
    r.marks.pool = &h->gevents[g]; r.marks.st = r.st;
  }
  h->done.rewind(); h->mix_events.rewind();
  for (int i = 0; i < sc.G * SQP_DEPTH; i++)
    SCO_TRY(h->done.next(&L.done[i]));
  if (sc.G > 1) {
    // the other groups' streams start behind the memsets queued on the main stream above (prog reset, warm-start zeroing)
    hipEvent_t ready;
    SCO_TRY(L.main.take(-2, &ready));
    SCO_HIP(hipEventRecord(ready, h->stream));
    for (int g = 1; g < sc.G; g++) SCO_HIP(hipStreamWaitEvent(L.grp[g].st, ready, 0));
  }
  return SCO_OK;
}

// one round of stream group g: [selection ->] pre -> QP setup + ADMM slice -> post -> read-back of the active count
static int sqp_enqueue_round(SqpLoop &L, int g) {
  sco_sqp *h = L.h;
  const SqpSchedule &sc = L.sc;
  const SqpDev &s = h->d;
  SqpGroupRun &r = L.grp[g];
  const SqpRound rp = sqp_round_plan(sc, r.nb, r.last_active, r.issued);
  const dim3 block(SCO_BLOCK);
  SqpDev sg = s; sg.b0 = r.b0; sg.n_active = s.n_active + g;
  if (r.issued == 0) SCO_TRY(r.marks.mark(-1));
  if (!sc.select) SCO_HIP(hipMemsetAsync(sg.n_active, 0, sizeof(int), r.st));
  sg.list = nullptr;
  if (sc.select) {
    hipLaunchKernelGGL(sqp_select_kernel, dim3(1), dim3(SEL_T), 0, r.st, sg, h->qp1->d, rp.pass, sc.slice, L.qsl.max_iter, rp.nwg, r.nb, rp.mix_k > 0 ? 1 : 0);
    SCO_HIP(hipGetLastError());
    sg.list = s.list_buf;
  }
  if (h->desc.family & SCO_FAM_FLAG_OBJ_WIDE)   // the objective terms' sweep on one wavefront per term, matrices in LDS
    hipLaunchKernelGGL(sqp_pre_wide_kernel, dim3(rp.nwg), block, WIDE_LDS_BYTES, r.st, sg, h->qp1->d, L.p);
  else
    hipLaunchKernelGGL(sqp_pre_kernel, dim3(rp.nwg), block, 0, r.st, sg, h->qp1->d, L.p);
  SCO_HIP(hipGetLastError());
  SCO_TRY(r.marks.mark(0));
  hipEvent_t gm;
  SCO_TRY(r.marks.take(1, &gm));
  QpGroup win{r.b0, rp.nwg, r.st, sg.list, rp.tier};
  if (rp.mix_k > 0) {
    win.side_nb = rp.mix_k; win.side_slices = sc.mix_slices; win.side_stream = h->gstream[0];
    win.side_b0 = r.b0 + rp.side_off;
    for (int e = 0; e < 3; e++)
      SCO_TRY(h->mix_events.next(&win.side_ev[e]));
    L.mixed_rounds++; L.mixed_side += rp.mix_k;
  }
  if (g == 0) L.round_k.push_back(rp.mix_k > 0 ? rp.mix_k : (rp.wv_round ? 0 : -1));
  if (rp.counts_as_wv) L.wv_rounds++;
  SCO_TRY(sco_qp_launch_sliced(h->qp1, &L.qsl, s.newqp, s.active, sc.slice, gm, nullptr, rp.window ? &win : nullptr));
  SCO_TRY(r.marks.mark(rp.counts_as_wv ? 5 : 2));
  hipLaunchKernelGGL(sqp_post_kernel, dim3(rp.nwg), block, 0, r.st, sg, h->qp1->d, L.p);
  SCO_HIP(hipGetLastError());
  SCO_TRY(r.marks.mark(3));
  const int slot = r.issued % SQP_DEPTH;
  SCO_HIP(hipMemcpyAsync(h->host_active + g * SQP_DEPTH + slot, sg.n_active, sizeof(int), hipMemcpyDeviceToHost, r.st));
  SCO_HIP(hipEventRecord(L.done[g * SQP_DEPTH + slot], r.st));
  r.issued++;
  return SCO_OK;
}

// SCO_SQP_TRACE_ROUNDS: the first 40 rounds of a group and every 100th (2: every round)
static void sqp_trace_round(const SqpLoop &L, int g) {
  const SqpGroupRun &r = L.grp[g];
  if (!L.sc.trace || !(r.retired < 40 || r.retired % 100 == 0 || L.sc.trace >= 2)) return;
  const int rk = (g == 0 && L.sc.has_wv) ? L.round_k[r.retired - 1] : -2;
  char kind[48] = "";
  if (rk > 0) snprintf(kind, sizeof kind, " (mixed round, k = %d)", rk);
  else if (rk > -2) snprintf(kind, sizeof kind, rk == 0 ? " (wavefront round)" : " (row-local round)");
  fprintf(stderr, "sco_sqp_solve: group %d round %d, %d problems active%s\n", g, r.retired, r.last_active, kind);
}

// ---- rounds: one QP solve (or one slice of it) per active problem, sc.depth rounds of every group enqueued ahead
static int sqp_run_rounds(SqpLoop &L) {
  const SqpSchedule &sc = L.sc;
  for (int k = 0; k < sc.depth; k++)
    for (int g = 0; g < sc.G; g++)
      SCO_TRY(sqp_enqueue_round(L, g));
  for (bool busy = true; busy;) {
    busy = false;
    for (int g = 0; g < sc.G; g++) {
      SqpGroupRun &r = L.grp[g];
      if (r.retired == r.issued) continue;
      busy = true;
      const int slot = r.retired % SQP_DEPTH;
      SCO_HIP(hipEventSynchronize(L.done[g * SQP_DEPTH + slot]));
      r.last_active = L.h->host_active[g * SQP_DEPTH + slot];
      r.retired++;
      sqp_trace_round(L, g);
      if (r.last_active > 0) {
        if (r.issued + 1 < sc.round_cap) SCO_TRY(sqp_enqueue_round(L, g));
        else if (r.retired == r.issued) L.capped = true;
      }
    }
  }
  return SCO_OK;
}

// the counters the ABI reports; problems the launch cap left running are marked
static int sqp_store_counters(SqpLoop &L) {
  sco_sqp *h = L.h;
  int total_rounds = 0;
  h->launches = 0;
  for (int g = 0; g < L.sc.G; g++) { total_rounds = std::max(total_rounds, L.grp[g].retired); h->launches += L.grp[g].retired; }
  h->rounds = 1 + total_rounds;
  h->wv_rounds = L.wv_rounds; h->mixed_rounds = L.mixed_rounds; h->mixed_side = L.mixed_side;
  if (L.capped) {
    // the launch cap ended the loop with problems still running (it is sized so that this cannot happen while every
    // problem respects max_sqp_iters): they are reported as capped failures, never silently as finished
    hipLaunchKernelGGL(sqp_cap_kernel, dim3((h->d.batch + SCO_BLOCK - 1) / SCO_BLOCK), dim3(SCO_BLOCK), 0, h->stream, h->d);
    SCO_HIP(hipGetLastError());
    SCO_HIP(hipStreamSynchronize(h->stream));
  }
  return SCO_OK;
}

// ---- timing: sum the event intervals by stage.  With one stream group the intervals follow each other; the rounds of
// several groups overlap and go through sqp_stage_sweep (every instant charged to one stage, so that the stages add up
// to the wall time of the call).
static void sqp_stage_times(SqpLoop &L) {
  sco_sqp *h = L.h;
  double ms[5] = {0, 0, 0, 0, 0}, wv_ms = 0.0;
  // an ADMM launch on the wavefront tier (stage 5) is ADMM time, summed on the side as well (sco_sqp_last_tiers)
  auto admm_stage = [&wv_ms](int stg, double dt) { if (stg != 5) return stg; wv_ms += dt; return 2; };
  auto sum_consecutive = [&](const StageMarks &mk) {
    for (size_t i = 1; i < mk.pool->cur; i++) {
      float t = 0; (void)hipEventElapsedTime(&t, mk.pool->ev[i - 1], mk.pool->ev[i]);
      const int stg = admm_stage(mk.stage[i], t);
      if (stg >= 0) ms[stg] += t;
      ms[4] += t;
    }
  };
  sum_consecutive(L.main);
  if (L.sc.G == 1) sum_consecutive(L.grp[0].marks);
  else {
    // milliseconds after the first event of the call
    std::vector<double> t0, t1; std::vector<int> stg;
    for (int g = 0; g < L.sc.G; g++) {
      const std::vector<int> &stage = L.grp[g].marks.stage;
      double prev = 0.0;
      for (size_t i = 0; i < h->gevents[g].cur; i++) {
        float t = 0; (void)hipEventElapsedTime(&t, h->events.ev[0], h->gevents[g].ev[i]);
        if (i > 0) { t0.push_back(prev); t1.push_back(t); stg.push_back(admm_stage(stage[i], t - prev)); }
        prev = t;
      }
    }
    sqp_stage_sweep(t0.data(), t1.data(), stg.data(), (int)stg.size(), ms);
  }
  memcpy(h->last_ms, ms, sizeof ms);
  h->wv_ms = wv_ms;
}

extern "C" int sco_sqp_solve(sco_sqp *h, const sco_sqp_params *params, const sco_qp_settings *qs) {
  SCO_TRY(sqp_check_state(h, params, qs));
  h->solved = false;            // a failed call must not leave an older result readable through fetch / trace
  SCO_TRY(sqp_check_settings(h, params, qs));
  SCO_ON_DEVICE(h->device);
  SqpLoop L;
  L.h = h;
  L.p = SqpParamsDev{params->improve_ratio_threshold, params->min_trust_region_size, params->min_approx_improve,
                     params->trust_shrink_ratio, params->trust_expand_ratio, params->cnt_tolerance,
                     params->merit_coeff_increase_ratio, params->initial_trust_region_size, params->initial_penalty_coeff,
                     params->max_merit_coeff_increases, params->compound_penalty, params->duplicate_rows,
                     params->max_sqp_iters > 0 ? params->max_sqp_iters : 10000, params->memoize_rounded ? 1 : 0};
  h->events.rewind();
  L.main.pool = &h->events; L.main.st = h->stream;
  int n_active = 0;
  SCO_TRY(sqp_projection_round(h, L.p, L.main, &n_active));
  h->rounds = 1;
  SCO_TRY(sqp_reset_penalty_qp(h, params, qs, &L.qsl));
  L.sc = sqp_plan(h, params->admm_slice, L.qsl, L.p.max_qp_solves, n_active);
  SCO_TRY(sqp_loop_start(L));
  if (n_active > 0) SCO_TRY(sqp_run_rounds(L));
  SCO_TRY(sqp_store_counters(L));
  sqp_stage_times(L);
  h->solved = true;
  return SCO_OK;
}

extern "C" int sco_sqp_fetch(sco_sqp *h, double *x, int *success, int *sqp_iters, int *qp_solves,
                             long long *admm_iters, double *merit, double *max_violation) {
  if (!h) return SCO_ERR_ARG;
  if (!h->solved) { sco_set_error("sco_sqp_fetch: call sco_sqp_solve first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  const SqpDev &s = h->d; const size_t B = s.batch;
  if (x) SCO_HIP(hipMemcpy(x, s.x, B * s.n_x * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<SqpScalars> sc(B);
  SCO_HIP(hipMemcpy(sc.data(), s.sc, B * sizeof(SqpScalars), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; b++) {
    if (success) success[b] = sc[b].success;
    if (sqp_iters) sqp_iters[b] = sc[b].sqp_iters;
    if (qp_solves) qp_solves[b] = sc[b].qp_solves;
    if (admm_iters) admm_iters[b] = sc[b].admm_iters;
  }
  if (merit || max_violation) {
    // result buffers of the handle (an allocation per call cost a device-wide synchronisation and now and then 70 ms)
    double *dm = h->fetch_buf, *dv = h->fetch_buf + B;
    hipLaunchKernelGGL(sqp_final_kernel, dim3(s.batch), dim3(SCO_BLOCK), 0, h->stream, s, dm, dv);
    SCO_HIP(hipGetLastError());
    SCO_HIP(hipStreamSynchronize(h->stream));
    if (merit) SCO_HIP(hipMemcpy(merit, dm, B * sizeof(double), hipMemcpyDeviceToHost));
    if (max_violation) SCO_HIP(hipMemcpy(max_violation, dv, B * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SCO_OK;
}

extern "C" int sco_sqp_trace(sco_sqp *h, int cap, double *trace, int *n_entries) {
  if (!h || !trace || !n_entries || cap <= 0) return SCO_ERR_ARG;
  if (!h->solved) { sco_set_error("sco_sqp_trace: call sco_sqp_solve first"); return SCO_ERR_STATE; }
  SCO_ON_DEVICE(h->device);
  const SqpDev &s = h->d; const size_t B = s.batch;
  std::vector<double> tr(B * s.trace_cap * TRACE_W);
  std::vector<SqpScalars> sc(B);
  SCO_HIP(hipMemcpy(tr.data(), s.trace, tr.size() * sizeof(double), hipMemcpyDeviceToHost));
  SCO_HIP(hipMemcpy(sc.data(), s.sc, B * sizeof(SqpScalars), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; b++) {
    n_entries[b] = sc[b].n_trace;
    const int rows = std::min(std::min(sc[b].n_trace, s.trace_cap), cap);
    for (int r = 0; r < rows; r++)
      memcpy(trace + (b * cap + r) * TRACE_W, tr.data() + (b * s.trace_cap + r) * TRACE_W, TRACE_W * sizeof(double));
  }
  return SCO_OK;
}

extern "C" int sco_sqp_last_rounds(const sco_sqp *h, int *rounds) {
  if (!h || !rounds) return SCO_ERR_ARG;
  *rounds = h->rounds;
  return SCO_OK;
}

// The layout and the program check on plain numbers (include/sco_hip.h): no device is touched
extern "C" int sco_debug_sqp_layout(const sco_trajopt_desc *desc, int n_rows, const int *row_ptr, const int *col_idx, const int *row_is_eq,
                                    int dims[22], int sizes[15], int *ints, double *vals) {
  if (!dims || !sizes) { sco_set_error("sco_debug_sqp_layout: null pointer"); return SCO_ERR_ARG; }
  const char *err = "";
  if (int rc = sqp_check_desc(desc, n_rows, row_ptr, col_idx, row_is_eq, &err)) { sco_set_error(err); return rc; }
  const SqpLayout L = sqp_layout_build(*desc, n_rows, row_ptr, col_idx, row_is_eq);
  const int dm[22] = {L.NE, L.S, L.ds, L.NBt, L.Req, L.m_pin, L.m_vel, L.m_jl, L.m_gen, L.nnz_gen, L.R, L.n_x, L.n_slack, L.n,
                      L.m_lin, L.m_nl, L.m, L.NB, L.RM, L.point, L.cost, L.acc};
  memcpy(dims, dm, sizeof dm);
  const std::vector<int> *iv[13] = {&L.qp0.Pp, &L.qp0.Pi, &L.qp0.Ap, &L.qp0.Ai, &L.qp1.Pp, &L.qp1.Pi, &L.qp1.Ap, &L.qp1.Ai,
                                    &L.jpos, &L.epos, &L.ppos, &L.gpos0, &L.gpos1};
  const std::vector<double> *dv[2] = {&L.a0c, &L.a1c};
  for (int k = 0; k < 13; k++) {
    sizes[k] = (int)iv[k]->size();
    if (ints) ints = std::copy(iv[k]->begin(), iv[k]->end(), ints);
  }
  for (int k = 0; k < 2; k++) {
    sizes[13 + k] = (int)dv[k]->size();
    if (vals) vals = std::copy(dv[k]->begin(), dv[k]->end(), vals);
  }
  return SCO_OK;
}
extern "C" int sco_debug_sqp_row_widths(const sco_trajopt_desc *desc, const int *point_link, int *out) {
  const char *err = "";
  if (int rc = sqp_check_desc(desc, 0, nullptr, nullptr, nullptr, &err)) { sco_set_error(err); return rc; }
  if (!point_link || !out) { sco_set_error("sco_debug_sqp_row_widths: null pointer"); return SCO_ERR_ARG; }
  const SqpLayout L = sqp_layout_build(*desc, 0, nullptr, nullptr, nullptr);
  std::vector<int> w;
  const bool hint = sqp_row_widths(L.point, L.S, desc->dof, desc->n_obstacles, L.R, L.NBt, L.m_lin, L.m, point_link, w);
  std::copy(w.begin(), w.end(), out);
  return hint ? 1 : 0;
}
extern "C" int sco_debug_sqp_check_program(const sco_trajopt_desc *desc, int n_circle_rows, int n_words, const int *words,
                                           const int *row_ptr, int n_consts, int n_params) {
  const char *err = "";
  if (int rc = sqp_check_desc(desc, 0, nullptr, nullptr, nullptr, &err)) { sco_set_error(err); return rc; }
  if (!words || !row_ptr) { sco_set_error("sco_sqp_load_program: null pointer"); return SCO_ERR_ARG; }
  if ((desc->family & 15) != SCO_FAM_STATE_PROGRAM) { sco_set_error("sco_sqp_load_program: family has no row programs"); return SCO_ERR_ARG; }
  const SqpLayout L = sqp_layout_build(*desc, 0, nullptr, nullptr, nullptr);
  if (n_circle_rows < 0 || n_circle_rows >= desc->n_obstacles) { sco_set_error("sco_debug_sqp_check_program: bad circle-row count"); return SCO_ERR_ARG; }
  const int rc = sqp_check_program(desc->n_obstacles - n_circle_rows, L.cost, L.ds, desc->dof, n_words, words, row_ptr, n_consts, n_params, &err);
  if (rc) sco_set_error(err);
  return rc;
}

extern "C" int sco_debug_sqp_wv_rounds(const sco_sqp *h) { return h ? h->wv_rounds : -1; }
extern "C" int sco_debug_sqp_mixed(const sco_sqp *h, int out[2]) {
  if (!h || !out) return SCO_ERR_ARG;
  out[0] = h->mixed_rounds; out[1] = h->mixed_side;
  return SCO_OK;
}
extern "C" int sco_sqp_last_tiers(const sco_sqp *h, double ms[2], long long iters[2], int launches[2]) {
  if (!h || !ms || !iters || !launches) return SCO_ERR_ARG;
  SCO_ON_DEVICE(h->device);
  unsigned long long wv_it = 0;
  if (sco_qp_wv_iters(h->qp1, &wv_it)) return SCO_ERR_DEVICE;
  ms[0] = h->wv_ms; ms[1] = h->last_ms[2] - h->wv_ms;
  iters[0] = (long long)wv_it; iters[1] = -1;          // the other kernels': total (sco_sqp_fetch: admm_iters) minus these
  launches[0] = h->wv_rounds; launches[1] = h->launches - h->wv_rounds + h->mixed_rounds;    // (a mixed round launches on both)
  return SCO_OK;
}
extern "C" int sco_sqp_last_launches(const sco_sqp *h, int *launches, int *groups) {
  if (!h) return SCO_ERR_ARG;
  if (launches) *launches = h->launches;
  if (groups) *groups = h->groups_used;
  return SCO_OK;
}

extern "C" int sco_sqp_last_timing(const sco_sqp *h, double ms[5]) {
  if (!h || !ms) return SCO_ERR_ARG;
  memcpy(ms, h->last_ms, 5 * sizeof(double));
  return SCO_OK;
}
