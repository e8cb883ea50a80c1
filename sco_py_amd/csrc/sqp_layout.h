// sqp_layout.h -- problem layout of the SQP layer (sco_sqp.hip): host arithmetic only, no device types.
//
// What a trajectory descriptor means -- which descriptors and row programs are accepted, every dimension of the two QPs,
// their CSC patterns, the constant A values and where the kernels write the per-iteration values -- is decided here from
// plain numbers, so that it can be read, and tested, without a GPU (tests/test_sqp_layout.py, through
// sco_debug_sqp_layout and sco_debug_sqp_check_program; scripts/sanitize/sqp_layout_sweep.cpp).  sco_sqp.hip allocates,
// uploads and launches what the layout says and derives nothing again.
#pragma once
#include "../../include/sco_hip.h"

#include <vector>

#define OBJ_DMAX 16           // widest objective term of the per-thread eigenvalue sweep (min_eig_jacobi)
#define SPATIAL_DMAX 16       // most joints of SCO_FAM_ARM_SPATIAL
#define SCO_STATE_MAX 32      // widest state of a constraint block of the program family (span x dof)

// SqpDev::point -- the family of the non-linear rows (sco_trajopt_desc::family & 15)
enum RowFamily {
  ROWS_ARM = 0,               // SCO_FAM_ARM_CIRCLES / SCO_FAM_ARM_REACH: link points of the planar arm against circles
  ROWS_POINT = 1,             // SCO_FAM_POINT_CIRCLES: distances of the point x[0:2] itself (no arm kinematics)
  ROWS_QUADRATIC = 2,         // SCO_FAM_STATE_QUADRATIC: general quadratic rows with per-problem coefficients
  ROWS_PROGRAM = 3,           // SCO_FAM_STATE_PROGRAM: rows as postfix programs (shared) over the state and per-problem parameters
  ROWS_SPATIAL = 4            // SCO_FAM_ARM_SPATIAL: link spheres of a spatial serial arm against sphere obstacles
};
// SqpDev::cost -- the non-quadratic objective term
enum ObjKind {
  OBJ_NONE = 0,
  OBJ_EE = 1,                 // SCO_FAM_FLAG_EE_COST: the arm's end-effector term
  OBJ_PROGRAM = 2,            // SCO_FAM_FLAG_OBJ_PROGRAM: an objective program per timestep (program index R)
  OBJ_BLOCK = 3               // SCO_FAM_FLAG_OBJ_BLOCK: an objective program per constraint block (state ds, NBt terms)
};
constexpr bool obj_is_program(int kind) { return kind >= OBJ_PROGRAM; }      // either of the two program objectives

// The descriptor rules of sco_sqp_create_rows and the CSR pattern check of its general affine rows.  SCO_OK, or
// SCO_ERR_ARG with *err set to the text for sco_set_error.
int sqp_check_desc(const sco_trajopt_desc *desc, int n_rows, const int *row_ptr, const int *col_idx, const int *row_is_eq,
                   const char **err);

struct SqpQpPattern { std::vector<int> Pp, Pi, Ap, Ai; };      // CSC: upper triangle of P, and A

struct SqpLayout {
  // NE = 2 equality rows (end-effector x, y) of SCO_FAM_ARM_REACH on the last timestep; constraint block t covers the S
  // timesteps t .. t + S - 1 (state: ds = S d numbers), NBt = T - S + 1 of them, the last Req of a block's R rows are
  // equalities; NB = blocks with the reach block, RM = widest block plus the objective term's value (history strides)
  int NE, S, ds, NBt, Req;
  int m_pin, m_vel, m_jl, m_gen, nnz_gen;      // linear rows: pins, velocity limits, joint limits, general affine rows
  int R, n_x, n_slack, n, m_lin, m_nl, m, NB, RM;
  int point, cost, acc;                         // RowFamily, ObjKind, SCO_FAM_FLAG_ACC_COST
  SqpQpPattern qp0, qp1;                        // projection QP (n_x x (m_lin + n_x)), penalty QP (n x m)
  std::vector<double> a0c, a1c;                 // constant parts of their A values
  // positions in the penalty QP's values: jpos[t d + j] first Jacobian slot of column (t, j) in A, epos[j] first reach-row
  // entry of column (T - 1, j) in A, ppos[c] + r entry (r, c) of the objective term's block in P; gpos0 / gpos1: entry k of
  // the general rows' pattern in the A values of the projection / penalty QP
  std::vector<int> jpos, epos, ppos, gpos0, gpos1;
  std::vector<int> gen_eq;                      // [m_gen] 1 = the general row is an equality
};
// `desc` and the general rows' pattern (gen_ptr[m_gen + 1], gen_col, gen_iseq[m_gen]; m_gen may be 0) have passed sqp_check_desc
SqpLayout sqp_layout_build(const sco_trajopt_desc &desc, int m_gen, const int *gen_ptr, const int *gen_col, const int *gen_iseq);

// The Jacobian width hint of the penalty QP (sco_qp_set_row_widths): for the serial-arm families -- the planar arm with or
// without the reach rows, the spatial arm -- the hinge row of link point k holds non-zeros only at the joints 0 ..
// point_link[k] of its timestep (the family guarantee: sqp_rows.h), so its width is point_link[k] + 1.  out[m]: that for
// every hinge row, 0 (no promise) for every other row; false and all 0 for a family without the guarantee.
// (plain numbers of the layout: point = RowFamily, S = span, R = rows per block, NBt = blocks)
bool sqp_row_widths(int point, int S, int dof, int O, int R, int NBt, int m_lin, int m, const int *point_link, std::vector<int> &out);

// The programs of sco_sqp_load_program{,_steps}: n_prog_rows = n_obstacles - circle rows programs of a block's rows over
// its ds numbers, then, for a program objective (`cost`), the objective term over ds (OBJ_BLOCK) or dof (OBJ_PROGRAM)
// numbers.  All of row_ptr is checked before any word is read through it; every program is then run once symbolically
// (stack depth, operand indices, opcodes).  SCO_OK, or SCO_ERR_ARG with *err set.
int sqp_check_program(int n_prog_rows, int cost, int ds, int dof, int n_words, const int *words, const int *row_ptr,
                      int n_consts, int n_params, const char **err);
