// sqp_rows.h -- device models of every non-linear row and objective family of the SQP layer, included only by sco_sqp.hip.
//
// What a row IS lives here: its value, its analytic gradient, its right-hand side and its violation, per family
// (RowFamily, sqp_layout.h) and per kind (RowKind); the non-quadratic objective terms (ObjKind); and the numeric tools the
// convexification applies to them (the finite-difference ladder's constants, Richardson extrapolation, the Jacobi
// eigenvalue sweep).  A new family is added here; the round kernels in sco_sqp.hip only call row_value, row_grad,
// obj_value, row_rhs and row_viol.
#pragma once
#include <hip/hip_runtime.h>

#include "sqp_layout.h"

#define FD_LEVELS 4
#define FD_BASE (1.0 / 64.0)

// SCO_FAM_ARM_CIRCLES: row (k, o) of one timestep block,
//   g = r_o - || p_k(theta) - c_o ||,  p_k = planar forward kinematics.
// `pert` >= 0 adds `h` to joint `pert` (finite differences).
__device__ __forceinline__ double arm_row(const double *th, const double *len, int lk, double frac,
                                          double cx, double cy, double rad, int pert, double h) {
  double phi = 0.0, px = 0.0, py = 0.0;
  for (int i = 0; i <= lk; i++) {
    double a = th[i];
    if (i == pert) a += h;
    phi += a;
    double s, c;
    sincos(phi, &s, &c);
    const double L = (i == lk) ? frac * len[i] : len[i];
    px += L * c; py += L * s;
  }
  const double dx = px - cx, dy = py - cy;
  return rad - sqrt(dx * dx + dy * dy);
}

// analytic d g / d theta_j of the same row
__device__ __forceinline__ double arm_row_grad(const double *th, const double *len, int lk, double frac,
                                               double cx, double cy, int j) {
  if (j > lk) return 0.0;
  double phi = 0.0, px = 0.0, py = 0.0, sx = 0.0, sy = 0.0;
  for (int i = 0; i <= lk; i++) {
    phi += th[i];
    double s, c;
    sincos(phi, &s, &c);
    const double L = (i == lk) ? frac * len[i] : len[i];
    px += L * c; py += L * s;
    if (i >= j) { sx += -L * s; sy += L * c; }
  }
  const double dx = px - cx, dy = py - cy;
  return -(dx * sx + dy * sy) / sqrt(dx * dx + dy * dy);
}

// SCO_FAM_ARM_REACH: component `comp` (0 = x, 1 = y) of the end-effector position
__device__ __forceinline__ double arm_ee(const double *th, const double *len, int d, int comp, int pert, double h) {
  double phi = 0.0, p = 0.0;
  for (int i = 0; i < d; i++) {
    double a = th[i];
    if (i == pert) a += h;
    phi += a;
    double sn, cs;
    sincos(phi, &sn, &cs);
    p += len[i] * (comp == 0 ? cs : sn);
  }
  return p;
}
__device__ __forceinline__ double arm_ee_grad(const double *th, const double *len, int d, int comp, int j) {
  double phi = 0.0, g = 0.0;
  for (int i = 0; i < d; i++) {
    phi += th[i];
    double sn, cs;
    sincos(phi, &sn, &cs);
    if (i >= j) g += comp == 0 ? -(len[i] * sn) : len[i] * cs;
  }
  return g;
}

// SCO_FAM_FLAG_EE_COST: weight * ||ee(theta) - target||^2 with up to two perturbed coordinates (finite differences)
__device__ __forceinline__ double arm_ee_cost(const double *th, const double *len, int d, double tx, double ty, double w,
                                              int pi, double hi, int pj, double hj) {
  double phi = 0.0, ex = 0.0, ey = 0.0;
  for (int i = 0; i < d; i++) {
    double a = th[i];
    if (i == pi) a += hi;
    if (i == pj) a += hj;
    phi += a;
    double sn, cs;
    sincos(phi, &sn, &cs);
    ex += len[i] * cs; ey += len[i] * sn;
  }
  ex -= tx; ey -= ty;
  return w * (ex * ex + ey * ey);
}

// SCO_FAM_ARM_SPATIAL: forward kinematics of a spatial serial arm of revolute joints up to link point (lk, pos).  Joint i:
//   p <- p + R off_i;   R <- R Rod(ax_i, theta_i),  Rod = I + sin K + (1 - cos) K^2,  K = skew(ax_i)
// and the point rides on the frame of joint lk behind that joint's rotation, p_k = p + R pos.  Every sum and product is the
// one sco_py_amd/workloads.py:_spatial_chain writes, in its order and without fused multiply-adds (NumPy has none): a
// Jacobian entry that differs in its last bit can move the iteration count of a slowly converging QP by many termination
// checks.  `pert` >= 0 adds `h` to joint `pert`; jg >= 0 also returns that joint's world axis and origin (aj, oj).
struct Vec3 { double x, y, z; };
__device__ __forceinline__ Vec3 spatial_point(const double *th, const double *off, const double *axis, int lk, const double *pos,
                                              int pert, double h, int jg, Vec3 *aj, Vec3 *oj) {
#pragma clang fp contract(off)
  double r00 = 1.0, r01 = 0.0, r02 = 0.0, r10 = 0.0, r11 = 1.0, r12 = 0.0, r20 = 0.0, r21 = 0.0, r22 = 1.0;
  double px = 0.0, py = 0.0, pz = 0.0;
  for (int i = 0; i <= lk; i++) {
    const double ox = off[3 * i], oy = off[3 * i + 1], oz = off[3 * i + 2];
    const double ax = axis[3 * i], ay = axis[3 * i + 1], az = axis[3 * i + 2];
    px = px + ((r00 * ox + r01 * oy) + r02 * oz);
    py = py + ((r10 * ox + r11 * oy) + r12 * oz);
    pz = pz + ((r20 * ox + r21 * oy) + r22 * oz);
    if (i == jg) {
      aj->x = (r00 * ax + r01 * ay) + r02 * az; aj->y = (r10 * ax + r11 * ay) + r12 * az; aj->z = (r20 * ax + r21 * ay) + r22 * az;
      oj->x = px; oj->y = py; oj->z = pz;
    }
    double a = th[i];
    if (i == pert) a += h;
    double s, c;
    sincos(a, &s, &c);
    const double v = 1.0 - c;
    const double xy = v * (ax * ay), xz = v * (ax * az), yz = v * (ay * az);
    const double sx = s * ax, sy = s * ay, sz = s * az;
    const double m00 = 1.0 - v * (ay * ay + az * az), m01 = xy - sz, m02 = xz + sy;
    const double m10 = xy + sz, m11 = 1.0 - v * (ax * ax + az * az), m12 = yz - sx;
    const double m20 = xz - sy, m21 = yz + sx, m22 = 1.0 - v * (ax * ax + ay * ay);
    const double n00 = (r00 * m00 + r01 * m10) + r02 * m20, n01 = (r00 * m01 + r01 * m11) + r02 * m21, n02 = (r00 * m02 + r01 * m12) + r02 * m22;
    const double n10 = (r10 * m00 + r11 * m10) + r12 * m20, n11 = (r10 * m01 + r11 * m11) + r12 * m21, n12 = (r10 * m02 + r11 * m12) + r12 * m22;
    const double n20 = (r20 * m00 + r21 * m10) + r22 * m20, n21 = (r20 * m01 + r21 * m11) + r22 * m21, n22 = (r20 * m02 + r21 * m12) + r22 * m22;
    r00 = n00; r01 = n01; r02 = n02; r10 = n10; r11 = n11; r12 = n12; r20 = n20; r21 = n21; r22 = n22;
  }
  Vec3 p;
  p.x = px + ((r00 * pos[0] + r01 * pos[1]) + r02 * pos[2]);
  p.y = py + ((r10 * pos[0] + r11 * pos[1]) + r12 * pos[2]);
  p.z = pz + ((r20 * pos[0] + r21 * pos[1]) + r22 * pos[2]);
  return p;
}
// row (k, o) of one timestep block: g = (r_o + rad_k) - || p_k(theta) - c_o ||, sphere = (cx, cy, cz, r)
__device__ __forceinline__ double spatial_row(const double *th, const double *off, const double *axis, int lk, const double *pos,
                                              double rad, const double *sphere, int pert, double h) {
#pragma clang fp contract(off)
  const Vec3 p = spatial_point(th, off, axis, lk, pos, pert, h, -1, nullptr, nullptr);
  const double dx = p.x - sphere[0], dy = p.y - sphere[1], dz = p.z - sphere[2];
  return (sphere[3] + rad) - sqrt((dx * dx + dy * dy) + dz * dz);
}
// analytic d g / d theta_j of the same row from the geometric Jacobian: d p_k / d theta_j = a_j x (p_k - o_j) with joint j's
// world axis a_j and world origin o_j; exactly 0 for a joint behind the point's link
__device__ __forceinline__ double spatial_row_grad(const double *th, const double *off, const double *axis, int lk, const double *pos,
                                                   const double *sphere, int j) {
#pragma clang fp contract(off)
  if (j > lk) return 0.0;
  Vec3 a, o;
  const Vec3 p = spatial_point(th, off, axis, lk, pos, -1, 0.0, j, &a, &o);
  const double ex = p.x - o.x, ey = p.y - o.y, ez = p.z - o.z;
  const double cx = a.y * ez - a.z * ey, cy = a.z * ex - a.x * ez, cz = a.x * ey - a.y * ex;
  const double dx = p.x - sphere[0], dy = p.y - sphere[1], dz = p.z - sphere[2];
  return -((dx * cx + dy * cy) + dz * cz) / sqrt((dx * dx + dy * dy) + dz * dz);
}

// Richardson extrapolation of a central-difference ladder (halving steps): sco_py_amd/numdiff.py:_richardson
__device__ __forceinline__ double richardson(double (&tab)[FD_LEVELS]) {
  double p4 = 4.0;
#pragma unroll
  for (int i = 1; i < FD_LEVELS; i++) {
    const double fac = 1.0 / (p4 - 1.0);
#pragma unroll
    for (int lv = FD_LEVELS - 1; lv >= i; lv--) tab[lv] = tab[lv] + (tab[lv] - tab[lv - 1]) * fac;
    p4 *= 4.0;
  }
  return tab[FD_LEVELS - 1];
}

// smallest eigenvalue of the symmetric d x d matrix H (d <= 16) by cyclic Jacobi rotations on a private copy
// (the reference calls scipy.linalg.eigvalsh, expr.py:145; oracle/sco_ref.py:min_eig_jacobi is this sweep)
__device__ double min_eig_jacobi(const double *H, int d) {
  double A[OBJ_DMAX * OBJ_DMAX];
  for (int i = 0; i < d * d; i++) A[i] = H[i];
  for (int sweep = 0; sweep < 12; sweep++)
    for (int p = 0; p < d - 1; p++)
      for (int q = p + 1; q < d; q++) {
        const double apq = A[p * d + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (A[q * d + q] - A[p * d + p]) / (2.0 * apq);
        // |theta| beyond 1e150 would overflow theta^2: there sqrt(theta^2 + 1) = |theta| to the last bit
        const double at = fabs(theta);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (at + (at > 1e150 ? at : sqrt(theta * theta + 1.0)));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < d; k++) {            // columns p, q
          const double rp = A[k * d + p], rq = A[k * d + q];
          A[k * d + p] = c * rp - sn * rq; A[k * d + q] = sn * rp + c * rq;
        }
        for (int k = 0; k < d; k++) {            // rows p, q
          const double rp = A[p * d + k], rq = A[q * d + k];
          A[p * d + k] = c * rp - sn * rq; A[q * d + k] = sn * rp + c * rq;
        }
      }
  double lam = A[0];
  for (int i = 1; i < d; i++) lam = fmin(lam, A[i * d + i]);
  return lam;
}

// Non-linear row e of a problem: hinge rows (timestep-major, R per timestep) first, then the NE
// equality rows of the reach variant on the last timestep (constraint block index T).
enum RowKind {
  ROW_HINGE = 0,        // inequality row: violation max(g, 0)
  ROW_REACH_EQ = 1,     // equality row of the reach variant (block NBt = T on the last timestep, arm kinematics)
  ROW_BLOCK_EQ = 2      // equality row inside a block of the state families (the last Req rows of the block, r03)
};
struct RowRef { int blk, t, r, eq; };      // eq: RowKind
struct RowLay { int T, NBt, R, Req; };
__device__ __forceinline__ RowRef row_ref(int e, const RowLay &L) {
  RowRef q;
  if (e < L.NBt * L.R) { q.blk = e / L.R; q.t = q.blk; q.r = e % L.R; q.eq = (q.r >= L.R - L.Req) ? ROW_BLOCK_EQ : ROW_HINGE; }
  else { q.blk = L.NBt; q.t = L.T - 1; q.r = e - L.NBt * L.R; q.eq = ROW_REACH_EQ; }
  return q;
}

struct RowCtx { const double *len, *obs, *target; const int *point_link; const double *point_frac; int d, O, point;      // point: RowFamily
                const double *qQ, *qa, *qc;         // SCO_FAM_STATE_QUADRATIC: this problem's row coefficients (ROWS_QUADRATIC)
                const int *pw, *pptr; const double *pconst, *ppar; int par_step, R1;     // SCO_FAM_STATE_PROGRAM (ROWS_PROGRAM): words, row starts, constants, this problem's parameters (block t: ppar + t * par_step)
                const double *joff, *jaxis, *ppos, *prad, *sph; };   // SCO_FAM_ARM_SPATIAL (ROWS_SPATIAL): this problem's joint offsets and axes [d][3], link points [K][3] and their radii [K], spheres [O][4]
// (for the state families `d` is the dimension of a BLOCK's state, span x dof)

// SCO_FAM_STATE_PROGRAM: value of program `o` at th, up to two coordinates perturbed (finite differences)
__device__ __forceinline__ double prog_eval(const RowCtx &c, const double *par, int o, const double *th, int pi, double hi, int pj, double hj) {
  double st[SCO_PROGRAM_STACK];
  int sp = 0;
  for (int w = c.pptr[o];; w++) {
    const int op = c.pw[2 * w], arg = c.pw[2 * w + 1];
    if (op == SCO_OP_END) break;
    switch (op) {
      case SCO_OP_X: st[sp++] = th[arg] + (arg == pi ? hi : 0.0) + (arg == pj ? hj : 0.0); break;
      case SCO_OP_P: st[sp++] = par[arg]; break;
      case SCO_OP_C: st[sp++] = c.pconst[arg]; break;
      case SCO_OP_ADD: sp--; st[sp - 1] = st[sp - 1] + st[sp]; break;
      case SCO_OP_SUB: sp--; st[sp - 1] = st[sp - 1] - st[sp]; break;
      case SCO_OP_MUL: sp--; st[sp - 1] = st[sp - 1] * st[sp]; break;
      case SCO_OP_DIV: sp--; st[sp - 1] = st[sp - 1] / st[sp]; break;
      case SCO_OP_NEG: st[sp - 1] = -st[sp - 1]; break;
      case SCO_OP_SIN: st[sp - 1] = sin(st[sp - 1]); break;
      case SCO_OP_COS: st[sp - 1] = cos(st[sp - 1]); break;
      case SCO_OP_SQRT: st[sp - 1] = sqrt(st[sp - 1]); break;
      case SCO_OP_EXP: st[sp - 1] = exp(st[sp - 1]); break;
      default: st[sp - 1] = st[sp - 1] * st[sp - 1]; break;       // SCO_OP_SQUARE
    }
  }
  return st[0];
}
// d(program o) / d x_j by forward-mode differentiation: every stack slot carries (value, derivative along e_j); the rules,
// in this order of operations, are the ones sco_py_amd/rowexpr.py:Program.jacobian applies on the host (the `grad` a caller
// hands to the reference's Expr, expr.py:86-100), so host and device agree to rounding
__device__ __forceinline__ double prog_dual(const RowCtx &c, const double *par, int o, const double *th, int j) {
  // no fused multiply-adds here: the host applies the rules operation by operation (NumPy), and a derivative that differs in
  // its last bit can move the iteration count of a slowly converging QP by many termination checks
#pragma clang fp contract(off)
  double sv[SCO_PROGRAM_STACK], sd[SCO_PROGRAM_STACK];
  int sp = 0;
  for (int w = c.pptr[o];; w++) {
    const int op = c.pw[2 * w], arg = c.pw[2 * w + 1];
    if (op == SCO_OP_END) break;
    switch (op) {
      case SCO_OP_X: sv[sp] = th[arg]; sd[sp++] = (arg == j) ? 1.0 : 0.0; break;
      case SCO_OP_P: sv[sp] = par[arg]; sd[sp++] = 0.0; break;
      case SCO_OP_C: sv[sp] = c.pconst[arg]; sd[sp++] = 0.0; break;
      case SCO_OP_ADD: sp--; sv[sp - 1] = sv[sp - 1] + sv[sp]; sd[sp - 1] = sd[sp - 1] + sd[sp]; break;
      case SCO_OP_SUB: sp--; sv[sp - 1] = sv[sp - 1] - sv[sp]; sd[sp - 1] = sd[sp - 1] - sd[sp]; break;
      case SCO_OP_MUL: sp--; sd[sp - 1] = sd[sp - 1] * sv[sp] + sv[sp - 1] * sd[sp]; sv[sp - 1] = sv[sp - 1] * sv[sp]; break;
      case SCO_OP_DIV: { sp--; const double qv = sv[sp - 1] / sv[sp]; sd[sp - 1] = (sd[sp - 1] - qv * sd[sp]) / sv[sp]; sv[sp - 1] = qv; break; }
      case SCO_OP_NEG: sv[sp - 1] = -sv[sp - 1]; sd[sp - 1] = -sd[sp - 1]; break;
      case SCO_OP_SIN: sd[sp - 1] = cos(sv[sp - 1]) * sd[sp - 1]; sv[sp - 1] = sin(sv[sp - 1]); break;
      case SCO_OP_COS: sd[sp - 1] = -(sin(sv[sp - 1]) * sd[sp - 1]); sv[sp - 1] = cos(sv[sp - 1]); break;
      case SCO_OP_SQRT: { const double r = sqrt(sv[sp - 1]); sd[sp - 1] = sd[sp - 1] / (2.0 * r); sv[sp - 1] = r; break; }
      case SCO_OP_EXP: { const double ev = exp(sv[sp - 1]); sd[sp - 1] = ev * sd[sp - 1]; sv[sp - 1] = ev; break; }
      default: sd[sp - 1] = (2.0 * sv[sp - 1]) * sd[sp - 1]; sv[sp - 1] = sv[sp - 1] * sv[sp - 1]; break;       // SCO_OP_SQUARE
    }
  }
  return sd[0];
}
// f of row q at th (the raw function value: the right-hand side val is 0 for hinge rows and the equality rows of the state
// families and target[r] for the reach rows and is applied by the callers, in the reference's order)
__device__ __forceinline__ double row_value(const RowCtx &c, const RowRef &q, const double *th, int pert, double h) {
  if (q.eq == ROW_REACH_EQ) return arm_ee(th, c.len, c.d, q.r, pert, h);
  const int kp = q.r / c.O, o = q.r % c.O;
  if (c.point == ROWS_SPATIAL)                            // SCO_FAM_ARM_SPATIAL: link sphere kp against sphere o
    return spatial_row(th, c.joff, c.jaxis, c.point_link[kp], c.ppos + 3 * kp, c.prad[kp], c.sph + 4 * o, pert, h);
  if (c.point == ROWS_PROGRAM) {                          // SCO_FAM_STATE_PROGRAM: the row's postfix program; r04: behind R1 circle rows of the point x[0:2]
    if (q.r < c.R1) {
      const double dx = th[0] + (pert == 0 ? h : 0.0) - c.obs[3 * q.r], dy = th[1] + (pert == 1 ? h : 0.0) - c.obs[3 * q.r + 1];
      return c.obs[3 * q.r + 2] - sqrt(dx * dx + dy * dy);
    }
    return prog_eval(c, c.ppar + q.t * c.par_step, q.r - c.R1, th, pert, h, -1, 0.0);
  }
  if (c.point == ROWS_QUADRATIC) {                          // SCO_FAM_STATE_QUADRATIC: 1/2 x' Q x + a' x + c of row o
    const double *Q = c.qQ + (size_t)o * c.d * c.d, *av = c.qa + (size_t)o * c.d;
    double val = c.qc[o];
    for (int i = 0; i < c.d; i++) {
      const double xi = th[i] + (i == pert ? h : 0.0);
      double qx = 0.0;
      for (int j2 = 0; j2 < c.d; j2++) qx += Q[i * c.d + j2] * (th[j2] + (j2 == pert ? h : 0.0));
      val += xi * (av[i] + 0.5 * qx);
    }
    return val;
  }
  if (c.point == ROWS_POINT) {                               // SCO_FAM_POINT_CIRCLES: r_o - || x[0:2] - c_o ||
    const double dx = th[0] + (pert == 0 ? h : 0.0) - c.obs[3 * o], dy = th[1] + (pert == 1 ? h : 0.0) - c.obs[3 * o + 1];
    return c.obs[3 * o + 2] - sqrt(dx * dx + dy * dy);
  }
  return arm_row(th, c.len, c.point_link[kp], c.point_frac[kp], c.obs[3 * o], c.obs[3 * o + 1], c.obs[3 * o + 2], pert, h);
}
__device__ __forceinline__ double row_grad(const RowCtx &c, const RowRef &q, const double *th, int j) {
  if (q.eq == ROW_REACH_EQ) return arm_ee_grad(th, c.len, c.d, q.r, j);
  const int kp = q.r / c.O, o = q.r % c.O;
  if (c.point == ROWS_SPATIAL) return spatial_row_grad(th, c.joff, c.jaxis, c.point_link[kp], c.ppos + 3 * kp, c.sph + 4 * o, j);
  if (c.point == ROWS_PROGRAM) {                          // forward-mode differentiation of the row's program (r03); circle rows in closed form
    if (q.r < c.R1) {
      if (j > 1) return 0.0;
      const double dx = th[0] - c.obs[3 * q.r], dy = th[1] - c.obs[3 * q.r + 1];
      return -(j == 0 ? dx : dy) / sqrt(dx * dx + dy * dy);
    }
    return prog_dual(c, c.ppar + q.t * c.par_step, q.r - c.R1, th, j);
  }
  if (c.point == ROWS_QUADRATIC) {                          // a_j + sum_i Q_ji x_i  (Q symmetric)
    const double *Q = c.qQ + (size_t)o * c.d * c.d;
    double g = c.qa[(size_t)o * c.d + j];
    for (int i = 0; i < c.d; i++) g += Q[j * c.d + i] * th[i];
    return g;
  }
  if (c.point == ROWS_POINT) {
    if (j > 1) return 0.0;
    const double dx = th[0] - c.obs[3 * o], dy = th[1] - c.obs[3 * o + 1];
    return -(j == 0 ? dx : dy) / sqrt(dx * dx + dy * dy);
  }
  return arm_row_grad(th, c.len, c.point_link[kp], c.point_frac[kp], c.obs[3 * o], c.obs[3 * o + 1], j);
}
// THE SERIAL-ARM GUARANTEE (stated here once; sqp_row_widths of sqp_layout.cpp turns it into the width hint of the penalty
// QP, the wavefront ADMM tier skips the columns it empties): in the planar and the spatial arm family the Jacobian entry of
// a hinge row of link point k at a joint j > point_link[k] is EXACTLY 0.0 on every route.  Analytic: arm_row_grad and
// spatial_row_grad return 0.0 there.  Central differences: arm_row never reads a joint behind the point's link, so both
// ends of every difference are the same number and Richardson extrapolates zeros; the spatial arm's ladder is not run at
// all (row_ignores).  The memo (cJ) hands back what one of these routes stored.  The reach rows see every joint: no
// promise.  A family that cannot say this gives no hint.

// true when row q does not depend on coordinate j at all, so that its central differences are exactly 0 and need not be
// run: a joint behind the link a point of the spatial arm rides on
__device__ __forceinline__ bool row_ignores(const RowCtx &c, const RowRef &q, int j) {
  return c.point == ROWS_SPATIAL && j > c.point_link[q.r / c.O];
}
// non-quadratic objective term of a timestep with up to two perturbed coordinates: the arm's end-effector term
// (SCO_FAM_FLAG_EE_COST) or the objective program (SCO_FAM_FLAG_OBJ_PROGRAM / SCO_FAM_FLAG_OBJ_BLOCK: program index O; for a
// block term `t` is the block and th its span * dof state)
struct ObjCtx { int kind /* ObjKind */; const double *len; int d; double tx, ty, w; };
__device__ __forceinline__ double obj_value(const ObjCtx &oc, const RowCtx &c, int t, const double *th, int pi, double hi, int pj, double hj) {
  if (obj_is_program(oc.kind)) return prog_eval(c, c.ppar + t * c.par_step, c.O - c.R1, th, pi, hi, pj, hj);
  return arm_ee_cost(th, oc.len, oc.d, oc.tx, oc.ty, oc.w, pi, hi, pj, hj);
}
__device__ __forceinline__ double row_rhs(const RowCtx &c, const RowRef &q) { return q.eq == ROW_REACH_EQ ? c.target[q.r] : 0.0; }
// violation of a row with value g = f - val: |g| for equality rows, max(g, 0) for hinge rows (prob.py:582-590)
__device__ __forceinline__ double row_viol(const RowRef &q, double g) { return q.eq != ROW_HINGE ? fabs(g) : fmax(g, 0.0); }
