// sqp_layout.cpp -- problem layout of the SQP layer: see sqp_layout.h.
#include "sqp_layout.h"

#include <algorithm>
#include <utility>

int sqp_check_desc(const sco_trajopt_desc *desc, int n_rows, const int *row_ptr, const int *col_idx, const int *row_is_eq,
                   const char **err) {
  auto refuse = [&](const char *text) { *err = text; return SCO_ERR_ARG; };
  if (!desc) return refuse("sco_sqp_create: null pointer");
  if (n_rows < 0 || n_rows > 65536 || (n_rows > 0 && (!row_ptr || !col_idx || !row_is_eq))) return refuse("sco_sqp_create_rows: bad row pattern");
  if (n_rows > 0) {
    if (row_ptr[0] != 0) return refuse("sco_sqp_create_rows: bad row pattern");
    const long long nx = (long long)desc->dof * desc->horizon;
    for (int r = 0; r < n_rows; r++) {
      if (row_ptr[r + 1] <= row_ptr[r] || row_ptr[r + 1] - row_ptr[r] > nx) return refuse("sco_sqp_create_rows: bad row pattern (empty row or row_ptr not increasing)");
      for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++)
        if (col_idx[k] < 0 || col_idx[k] >= nx || (k > row_ptr[r] && col_idx[k] <= col_idx[k - 1]))
          return refuse("sco_sqp_create_rows: column indices must lie in [0, dof * horizon) and increase inside a row");
    }
  }
  const int family = desc->family, fam = family & 15, span = desc->span > 0 ? desc->span : 1, dof = desc->dof;
  const bool arm = fam == SCO_FAM_ARM_CIRCLES || fam == SCO_FAM_ARM_REACH, pointfam = fam == SCO_FAM_POINT_CIRCLES;
  const bool spatial = fam == SCO_FAM_ARM_SPATIAL;
  const bool progfam = fam == SCO_FAM_STATE_PROGRAM, statefam = fam == SCO_FAM_STATE_QUADRATIC || progfam;
  const bool ee = (family & SCO_FAM_FLAG_EE_COST) != 0, objprog = (family & SCO_FAM_FLAG_OBJ_PROGRAM) != 0;
  const bool objblk = (family & SCO_FAM_FLAG_OBJ_BLOCK) != 0, objwide = (family & SCO_FAM_FLAG_OBJ_WIDE) != 0;
  // widest objective term: the per-thread eigenvalue sweep's, or with SCO_FAM_FLAG_OBJ_WIDE the wavefront's
  const int objmax = objwide ? SCO_STATE_MAX : OBJ_DMAX;
  const int known_flags = 15 | SCO_FAM_FLAG_VEL_LIMITS | SCO_FAM_FLAG_JOINT_LIMITS | SCO_FAM_FLAG_EE_COST | SCO_FAM_FLAG_OBJ_PROGRAM |
                          SCO_FAM_FLAG_ACC_COST | SCO_FAM_FLAG_OBJ_BLOCK | SCO_FAM_FLAG_OBJ_WIDE;
  const bool refused[] = {
      // sizes
      desc->batch <= 0 || dof <= 0 || desc->n_points <= 0 || desc->n_obstacles <= 0,
      desc->horizon < 2 || desc->horizon > 256,
      // family and flags
      (family & ~known_flags) != 0,
      !arm && !pointfam && !statefam && !spatial,
      // the spatial arm: obstacle rows and the linear-row flags only (no 3-D reach equality or end-effector term)
      spatial && (dof > SPATIAL_DMAX || ee),
      ee && dof > OBJ_DMAX,
      (family & SCO_FAM_FLAG_ACC_COST) && desc->horizon < 3,
      pointfam && (desc->n_points != 1 || dof < 2 || ee),
      statefam && (desc->n_points != 1 || ee),
      fam == SCO_FAM_STATE_QUADRATIC && dof > OBJ_DMAX,
      // blocks of `span` timesteps, equality rows and objective programs: the state families' extensions
      desc->span < 0 || desc->span > 4 || (span > 1 && !progfam),
      desc->n_eq_rows < 0 || desc->n_eq_rows > desc->n_obstacles || (desc->n_eq_rows > 0 && !statefam),
      progfam && (span * dof > SCO_STATE_MAX || span >= desc->horizon),
      objprog && (!progfam || span != 1 || dof > objmax),
      // an objective program per constraint block: span 2 .. 4, the block's state fits the eigenvalue sweep
      objblk && (!progfam || span < 2 || span * dof > objmax || objprog || ee),
      // SCO_FAM_FLAG_OBJ_WIDE: opt-in, the program family with exactly one of its two objective flags
      objwide && (!progfam || ee || objprog == objblk),
  };
  for (bool r : refused)
    if (r) return refuse("sco_sqp_create: bad descriptor");
  return SCO_OK;
}

SqpLayout sqp_layout_build(const sco_trajopt_desc &desc, int m_gen, const int *gen_ptr, const int *gen_col, const int *gen_iseq) {
  SqpLayout L;
  const int d = desc.dof, T = desc.horizon, K = desc.n_points, O = desc.n_obstacles, fam = desc.family & 15;
  const bool reach = fam == SCO_FAM_ARM_REACH, vel = (desc.family & SCO_FAM_FLAG_VEL_LIMITS) != 0;
  const bool jl = (desc.family & SCO_FAM_FLAG_JOINT_LIMITS) != 0;
  const bool cost = (desc.family & (SCO_FAM_FLAG_EE_COST | SCO_FAM_FLAG_OBJ_PROGRAM | SCO_FAM_FLAG_OBJ_BLOCK)) != 0;
  const bool oblk = (desc.family & SCO_FAM_FLAG_OBJ_BLOCK) != 0;
  const bool acc = (desc.family & SCO_FAM_FLAG_ACC_COST) != 0;
  const int NE = reach ? 2 : 0;                  // equality rows (end-effector x, y) on the last timestep
  const int S = desc.span > 0 ? desc.span : 1, ds = S * d, NBt = T - S + 1, Req = desc.n_eq_rows;
  const int m_pin = reach ? d : 2 * d, dT1 = d * (T - 1), m_vel = vel ? 2 * dT1 : 0;
  const int m_jl = jl ? 2 * d * T : 0;
  // general affine rows: column lists of the CSR pattern; entry k of the pattern = (row, column) in CSR order
  const int nnz_gen = m_gen ? gen_ptr[m_gen] : 0;
  std::vector<std::vector<std::pair<int, int>>> gen_of_col(d * T);       // (row, k), rows ascending
  for (int r = 0; r < m_gen; r++)
    for (int k = gen_ptr[r]; k < gen_ptr[r + 1]; k++) gen_of_col[gen_col[k]].push_back({r, k});
  L.gpos0.assign(nnz_gen, 0); L.gpos1.assign(nnz_gen, 0);
  for (int r = 0; r < m_gen; r++) L.gen_eq.push_back(gen_iseq[r] ? 1 : 0);
  // a hinge row has one slack, an equality row two (prob.py:258, 285-286); block-major, hinge rows of a block first
  const int R = K * O, n_x = d * T, SB = R + Req, n_slack = NBt * SB + 2 * NE, n = n_x + n_slack, m_lin = m_pin + m_vel + m_jl + m_gen;
  const int m_nl = NBt * R + NE, m = m_lin + m_nl + n;
  L.NE = NE; L.S = S; L.ds = ds; L.NBt = NBt; L.Req = Req;
  L.m_pin = m_pin; L.m_vel = m_vel; L.m_jl = m_jl; L.m_gen = m_gen; L.nnz_gen = nnz_gen;
  L.R = R; L.n_x = n_x; L.n_slack = n_slack; L.n = n; L.m_lin = m_lin; L.m_nl = m_nl; L.m = m;
  L.NB = NBt + (reach ? 1 : 0); L.RM = std::max(R, NE) + (cost ? 1 : 0);     // + the objective term's value
  L.point = fam == SCO_FAM_POINT_CIRCLES ? ROWS_POINT : fam == SCO_FAM_STATE_QUADRATIC ? ROWS_QUADRATIC :
            fam == SCO_FAM_STATE_PROGRAM ? ROWS_PROGRAM : fam == SCO_FAM_ARM_SPATIAL ? ROWS_SPATIAL : ROWS_ARM;
  L.cost = oblk ? OBJ_BLOCK : (desc.family & SCO_FAM_FLAG_OBJ_PROGRAM) ? OBJ_PROGRAM : cost ? OBJ_EE : OBJ_NONE;
  L.acc = acc ? 1 : 0;
  // linear rows of column (t, j), ascending: pin, velocity rows "theta[t] - theta[t-1] <= vmax" (+1),
  // "theta[t+1] - theta[t] <= vmax" (-1), then the two negated rows
  auto linear_entries = [&](int t, int j, std::vector<int> &Ai, std::vector<double> &Av, std::vector<int> &gpos) {
    if (t == 0) { Ai.push_back(j); Av.push_back(1.0); }
    if (t == T - 1 && !reach) { Ai.push_back(d + j); Av.push_back(1.0); }
    if (vel) {
      if (t >= 1) { Ai.push_back(m_pin + (t - 1) * d + j); Av.push_back(1.0); }
      if (t <= T - 2) { Ai.push_back(m_pin + t * d + j); Av.push_back(-1.0); }
      if (t >= 1) { Ai.push_back(m_pin + dT1 + (t - 1) * d + j); Av.push_back(-1.0); }
      if (t <= T - 2) { Ai.push_back(m_pin + dT1 + t * d + j); Av.push_back(1.0); }
    }
    if (jl) {
      Ai.push_back(m_pin + m_vel + t * d + j); Av.push_back(1.0);
      Ai.push_back(m_pin + m_vel + d * T + t * d + j); Av.push_back(-1.0);
    }
    for (const auto &rk : gen_of_col[t * d + j]) {        // values per problem (sco_sqp_load_linear_rows): 0 in the constants
      gpos[rk.second] = (int)Ai.size();
      Ai.push_back(m_pin + m_vel + m_jl + rk.first); Av.push_back(0.0);
    }
  };
  // ---- projection QP pattern: P = diag, A = [linear rows ; I]
  {
    std::vector<int> &Pp = L.qp0.Pp, &Pi = L.qp0.Pi, &Ap = L.qp0.Ap, &Ai = L.qp0.Ai;
    Pp.resize(n_x + 1); Pi.resize(n_x); Ap.resize(n_x + 1);
    for (int i = 0; i < n_x; i++) { Pp[i] = i; Pi[i] = i; }
    Pp[n_x] = n_x;
    for (int col = 0; col < n_x; col++) {
      Ap[col] = (int)Ai.size();
      const int t = col / d, j = col % d;
      linear_entries(t, j, Ai, L.a0c, L.gpos0);
      Ai.push_back(m_lin + col); L.a0c.push_back(1.0);
    }
    Ap[n_x] = (int)Ai.size();
  }
  // ---- penalty QP pattern (prob.py:251-278 rows, osqp_utils.py:185-189 bound rows)
  L.jpos.assign(n_x, 0); L.epos.assign(d, 0); L.ppos.assign(n_x, 0);
  {
    std::vector<int> &Pp = L.qp1.Pp, &Pi = L.qp1.Pi, &Ap = L.qp1.Ap, &Ai = L.qp1.Ai;
    std::vector<int> &jpos = L.jpos, &epos = L.epos, &ppos = L.ppos;
    std::vector<double> &a1c = L.a1c;
    Pp.resize(n + 1); Ap.resize(n + 1);
    for (int col = 0; col < n; col++) {
      Pp[col] = (int)Pi.size();
      if (col < n_x && oblk) {
        // block terms (SCO_FAM_FLAG_OBJ_BLOCK): a block's Hessian couples all its S timesteps, so column (t, j) holds the
        // dense band of rows max(0, t - S + 1) d .. col -- with the acceleration term's (t - 2, j) in front when S = 2
        const int t = col / d, r0 = std::max(0, t - S + 1) * d;
        if (acc && S == 2 && t > 1) Pi.push_back(col - 2 * d);
        ppos[col] = (int)Pi.size() - r0;           // entry (r, col) sits at ppos + r
        for (int r = r0; r <= col; r++) Pi.push_back(r);
      } else if (col < n_x) {
        if (acc && col / d > 1) Pi.push_back(col - 2 * d);       // acceleration term: second super-diagonal block
        if (col / d > 0) Pi.push_back(col - d);
        ppos[col] = (int)Pi.size();
        // a non-quadratic objective term fills the upper triangle of its timestep's diagonal block
        if (cost) for (int i = 0; i < col % d; i++) Pi.push_back(col - col % d + i);
        else ppos[col] -= col % d;                 // entry (i, j) sits at ppos + i; only i == j exists
        Pi.push_back(col);
      }
    }
    Pp[n] = (int)Pi.size();
    for (int col = 0; col < n; col++) {
      Ap[col] = (int)Ai.size();
      if (col < n_x) {
        const int t = col / d, j = col % d;
        linear_entries(t, j, Ai, a1c, L.gpos1);
        jpos[col] = (int)Ai.size();
        // Jacobian slots: the R rows of every block that covers timestep t (blocks t - S + 1 .. t), in block order
        for (int blk = std::max(0, t - S + 1); blk <= std::min(t, NBt - 1); blk++)
          for (int r = 0; r < R; r++) { Ai.push_back(m_lin + blk * R + r); a1c.push_back(0.0); }
        if (t == T - 1 && reach) {
          epos[j] = (int)Ai.size();
          for (int r = 0; r < NE; r++) { Ai.push_back(m_lin + NBt * R + r); a1c.push_back(0.0); }
        }
        Ai.push_back(m_lin + m_nl + col); a1c.push_back(1.0);
      } else {
        // slack columns block-major: per block its R - Req hinge slacks (-1 in their hinge row), then (p, n) of each of its
        // Req equality rows (-1, +1); behind the blocks (p, n) of the reach rows (prob.py:265-275, 303-312); then the
        // slack's bound row
        const int sidx = col - n_x;
        int row; double sgn = -1.0;
        if (sidx < NBt * SB) {
          const int blk = sidx / SB, k = sidx % SB, nh = R - Req;
          if (k < nh) row = blk * R + k;
          else { row = blk * R + nh + (k - nh) / 2; if ((k - nh) & 1) sgn = 1.0; }
        } else {
          const int ke = sidx - NBt * SB;
          row = NBt * R + ke / 2; if (ke & 1) sgn = 1.0;
        }
        Ai.push_back(m_lin + row); a1c.push_back(sgn);
        Ai.push_back(m_lin + m_nl + col); a1c.push_back(1.0);
      }
    }
    Ap[n] = (int)Ai.size();
  }
  return L;
}

bool sqp_row_widths(int point, int S, int dof, int O, int R, int NBt, int m_lin, int m, const int *point_link, std::vector<int> &out) {
  out.assign(m, 0);
  if ((point != ROWS_ARM && point != ROWS_SPATIAL) || S != 1 || O <= 0 || !point_link) return false;
  // hinge rows block-major behind the linear rows, row (k, o) of a block at k O + o (the reach rows behind them: no promise)
  for (int blk = 0; blk < NBt; blk++)
    for (int r = 0; r < R; r++) {
      const int lk = point_link[r / O];
      out[m_lin + blk * R + r] = (lk >= 0 && lk < dof) ? lk + 1 : 0;
    }
  return true;
}

int sqp_check_program(int n_prog_rows, int cost, int ds, int dof, int n_words, const int *words, const int *row_ptr,
                      int n_consts, int n_params, const char **err) {
  auto refuse = [&](const char *text) { *err = text; return SCO_ERR_ARG; };
  // the rows of a block, then (OBJ_PROGRAM) the objective term of a timestep or (OBJ_BLOCK) of a block
  const int R = n_prog_rows + (obj_is_program(cost) ? 1 : 0);
  if (n_words <= 0 || n_consts < 0 || n_params < 0) return refuse("sco_sqp_load_program: bad program layout");
  // the whole of row_ptr is checked BEFORE any word is read through it: 0 = first entry, strictly increasing, last = n_words
  if (row_ptr[0] != 0) return refuse("sco_sqp_load_program: bad program layout");
  for (int r = 0; r < R; r++)
    if (row_ptr[r + 1] <= row_ptr[r] || row_ptr[r + 1] > n_words) return refuse("sco_sqp_load_program: bad program layout");
  if (row_ptr[R] != n_words) return refuse("sco_sqp_load_program: bad program layout");
  // every row's program is run on the host once, symbolically: stack depth and operand indices
  for (int r = 0; r < R; r++) {
    if (words[2 * (row_ptr[r + 1] - 1)] != SCO_OP_END) return refuse("sco_sqp_load_program: a row's program must end with SCO_OP_END");
    const int nx = (r < n_prog_rows || cost == OBJ_BLOCK) ? ds : dof;      // the objective term sees one timestep (a block's: ds)
    int sp = 0;
    for (int w = row_ptr[r]; w < row_ptr[r + 1] - 1; w++) {
      const int op = words[2 * w], arg = words[2 * w + 1];
      bool ok = true;
      if (op == SCO_OP_X) { ok = arg >= 0 && arg < nx; sp++; }
      else if (op == SCO_OP_P) { ok = arg >= 0 && arg < n_params; sp++; }
      else if (op == SCO_OP_C) { ok = arg >= 0 && arg < n_consts; sp++; }
      else if (op >= SCO_OP_ADD && op <= SCO_OP_DIV) { ok = sp >= 2; sp--; }
      else if (op >= SCO_OP_NEG && op <= SCO_OP_SQUARE) ok = sp >= 1;
      else ok = false;
      if (!ok || sp > SCO_PROGRAM_STACK) return refuse("sco_sqp_load_program: malformed program (operand index, stack depth or opcode)");
    }
    if (sp != 1) return refuse("sco_sqp_load_program: a row's program must leave exactly one value");
  }
  return SCO_OK;
}
