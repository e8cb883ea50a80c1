// Stand-alone sweep of the SQP problem layout (csrc/sqp_layout.cpp) for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       scripts/sanitize/sqp_layout_sweep.cpp sco_py_amd/csrc/sqp_layout.cpp -o sqp_layout_sweep && ./sqp_layout_sweep
// Every family (the spatial arm included) x flag set x dof 1 .. 4 x horizon 2 .. 6 and 256 x span 0 .. 4 x n_eq_rows 0 .. 2, with and without general
// rows: sqp_check_desc, and for every accepted descriptor sqp_layout_build -- every index of Pi / Ai in range, Pp / Ap
// monotone and ending at the vector sizes, every position table entry inside its value array.  Then sqp_check_program on
// truncated and random word streams: whatever it accepts stays inside the stack and the operand arrays.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sco_py_amd/csrc/sqp_layout.h"

static bool pattern_ok(const std::vector<int> &ptr, const std::vector<int> &idx, int cols, int rows, bool upper) {
  if ((int)ptr.size() != cols + 1 || ptr[0] != 0 || ptr[cols] != (int)idx.size()) return false;
  for (int c = 0; c < cols; c++) {
    if (ptr[c + 1] < ptr[c]) return false;
    for (int k = ptr[c]; k < ptr[c + 1]; k++)
      if (idx[k] < 0 || idx[k] >= rows || (upper && idx[k] > c) || (k > ptr[c] && idx[k] <= idx[k - 1])) return false;
  }
  return true;
}

static bool layout_ok(const SqpLayout &L, int d) {
  if (!pattern_ok(L.qp0.Pp, L.qp0.Pi, L.n_x, L.n_x, true) || !pattern_ok(L.qp0.Ap, L.qp0.Ai, L.n_x, L.m_lin + L.n_x, false)) return false;
  if (!pattern_ok(L.qp1.Pp, L.qp1.Pi, L.n, L.n, true) || !pattern_ok(L.qp1.Ap, L.qp1.Ai, L.n, L.m, false)) return false;
  if (L.a0c.size() != L.qp0.Ai.size() || L.a1c.size() != L.qp1.Ai.size()) return false;
  if ((int)L.jpos.size() != L.n_x || (int)L.ppos.size() != L.n_x || (int)L.epos.size() != d) return false;
  if ((int)L.gpos0.size() != L.nnz_gen || (int)L.gpos1.size() != L.nnz_gen || (int)L.gen_eq.size() != L.m_gen) return false;
  const int nnzA0 = (int)L.a0c.size(), nnzA1 = (int)L.a1c.size(), nnzP1 = (int)L.qp1.Pi.size();
  for (int c = 0; c < L.n_x; c++) {
    const int t = c / d, slots = (std::min(t, L.NBt - 1) - std::max(0, t - L.S + 1) + 1) * L.R;      // blocks that cover timestep t
    if (L.jpos[c] < L.qp1.Ap[c] || L.jpos[c] + slots >= L.qp1.Ap[c + 1]) return false;
    // the entries convexify writes through ppos: the band of a block objective, else the timestep's diagonal block
    const int lo = L.cost == OBJ_BLOCK ? std::max(0, t - L.S + 1) * d : L.cost ? 0 : c % d, hi = L.cost == OBJ_BLOCK ? c : c % d;
    if (L.ppos[c] + lo < L.qp1.Pp[c] || L.ppos[c] + hi >= L.qp1.Pp[c + 1] || L.ppos[c] + hi >= nnzP1) return false;
  }
  for (int j = 0; j < d; j++)
    if (L.NE && (L.epos[j] < L.qp1.Ap[L.n_x - d + j] || L.epos[j] + L.NE >= L.qp1.Ap[L.n_x - d + j + 1])) return false;
  for (int k = 0; k < L.nnz_gen; k++)
    if (L.gpos0[k] < 0 || L.gpos0[k] >= nnzA0 || L.gpos1[k] < 0 || L.gpos1[k] >= nnzA1) return false;
  return true;
}

int main() {
  const int flag_bits[] = {SCO_FAM_FLAG_VEL_LIMITS, SCO_FAM_FLAG_JOINT_LIMITS, SCO_FAM_FLAG_EE_COST, SCO_FAM_FLAG_OBJ_PROGRAM,
                           SCO_FAM_FLAG_ACC_COST, SCO_FAM_FLAG_OBJ_BLOCK, SCO_FAM_FLAG_OBJ_WIDE, 2048};
  const int horizons[] = {2, 3, 4, 5, 6, 256};
  long long descs = 0, accepted = 0, spatial = 0;
  for (int fam = 0; fam <= 7; fam++)
    for (int fl = 0; fl < 256; fl++) {
      int family = fam;
      for (int k = 0; k < 8; k++) if ((fl >> k) & 1) family |= flag_bits[k];
      for (int dof = 1; dof <= 4; dof++)
        for (int T : horizons)
          for (int span = 0; span <= 4; span++)
            for (int neq = 0; neq <= 2; neq++)
              for (int gen = 0; gen < 2; gen++) {
                const sco_trajopt_desc desc = {3, dof, T, (fam <= 2 || fam == SCO_FAM_ARM_SPATIAL) ? 2 : 1, 2, family, 0, 0, span, neq};
                // general rows: an equality over the first and last variable, an inequality on the middle one
                const int nx = dof * T, row_ptr[3] = {0, 2, 3}, col[3] = {0, nx - 1, nx / 2}, iseq[2] = {1, 0};
                const char *err = nullptr;
                const int rc = sqp_check_desc(&desc, gen ? 2 : 0, row_ptr, col, iseq, &err);
                descs++;
                if (rc != SCO_OK) {
                  if (rc != SCO_ERR_ARG || !err || !err[0]) { printf("refusal without a text\n"); return 1; }
                  continue;
                }
                accepted++;
                const SqpLayout L = sqp_layout_build(desc, gen ? 2 : 0, row_ptr, col, iseq);
                if (fam == SCO_FAM_ARM_SPATIAL) {      // the planar arm's layout under another row model; linear-row flags and the acceleration term only
                  spatial++;
                  if (L.point != ROWS_SPATIAL || L.NE != 0 || L.cost != OBJ_NONE || span > 1 || neq != 0 ||
                      (family & ~(15 | SCO_FAM_FLAG_VEL_LIMITS | SCO_FAM_FLAG_JOINT_LIMITS | SCO_FAM_FLAG_ACC_COST))) { printf("spatial family: accepted %d\n", family); return 1; }
                }
                if (!layout_ok(L, dof)) { printf("bad layout: family %d dof %d T %d span %d neq %d gen %d\n", family, dof, T, span, neq, gen); return 1; }
              }
    }
  printf("%lld descriptors, %lld accepted: every index, pointer and position of their layouts is in range\n", descs, accepted);
  if (accepted == 0 || spatial == 0) return 1;
  {   // the spatial arm's widest accepted arm, and one joint more
    const sco_trajopt_desc wide = {1, SPATIAL_DMAX, 4, 3, 2, SCO_FAM_ARM_SPATIAL, 0, 0, 0, 0}, wider = {1, SPATIAL_DMAX + 1, 4, 3, 2, SCO_FAM_ARM_SPATIAL, 0, 0, 0, 0};
    const char *err = nullptr;
    if (sqp_check_desc(&wide, 0, nullptr, nullptr, nullptr, &err) != SCO_OK || sqp_check_desc(&wider, 0, nullptr, nullptr, nullptr, &err) != SCO_ERR_ARG ||
        !layout_ok(sqp_layout_build(wide, 0, nullptr, nullptr, nullptr), SPATIAL_DMAX)) { printf("spatial family: joint limit\n"); return 1; }
  }

  // malformed general-row patterns (each array as long as the well-formed one, so a refusal never reads past it)
  {
    const sco_trajopt_desc desc = {1, 2, 3, 1, 2, SCO_FAM_ARM_CIRCLES, 0, 0, 0, 0};
    const int ptrs[][3] = {{0, 2, 3}, {1, 2, 3}, {0, 0, 3}, {0, 3, 2}, {0, 2, 2}}, cols[][3] = {{0, 5, 2}, {5, 5, 2}, {0, 6, 2}, {-1, 5, 2}, {5, 0, 2}};
    const int iseq[2] = {1, 0};
    int ok = 0;
    for (const auto &p : ptrs)
      for (const auto &c : cols) {
        const char *err = nullptr;
        ok += sqp_check_desc(&desc, 2, p, c, iseq, &err) == SCO_OK;
      }
    const char *err = nullptr;
    if (ok != 1 || sqp_check_desc(&desc, 65537, ptrs[0], cols[0], iseq, &err) != SCO_ERR_ARG || sqp_check_desc(&desc, 2, nullptr, cols[0], iseq, &err) != SCO_ERR_ARG) {
      printf("general-row patterns: %d accepted\n", ok); return 1;
    }
  }

  // programs: a well-formed two-row program truncated at every length, then random streams.  The arrays hold exactly the
  // words and row pointers announced, so a read through an unchecked row_ptr is a sanitizer finding.
  unsigned long long rng = 88172645463325252ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (unsigned)(rng >> 11); };
  long long progs = 0, prog_ok = 0;
  const int good[] = {SCO_OP_X, 0, SCO_OP_P, 1, SCO_OP_MUL, 0, SCO_OP_C, 0, SCO_OP_ADD, 0, SCO_OP_END, 0,
                      SCO_OP_X, 3, SCO_OP_SQUARE, 0, SCO_OP_X, 1, SCO_OP_SUB, 0, SCO_OP_SQRT, 0, SCO_OP_END, 0};
  for (int n_words = 0; n_words <= 12; n_words++)
    for (int split = 0; split <= 13; split++)
      for (int cost = OBJ_NONE; cost <= OBJ_BLOCK; cost++) {
        const std::vector<int> words(good, good + 2 * n_words);
        const int rows = obj_is_program(cost) ? 1 : 2;
        const std::vector<int> row_ptr = {0, split, n_words};
        const char *err = nullptr;
        const int rc = sqp_check_program(rows, cost, 4, 2, n_words, words.data(), row_ptr.data(), 1, 2, &err);
        progs++; prog_ok += rc == SCO_OK;
        if (rc != SCO_OK && (!err || !err[0])) { printf("refusal without a text\n"); return 1; }
        // the whole program, split where its first row ends: accepted unless the second row is a per-timestep objective
        // (X(3) is beyond dof = 2)
        if ((rc == SCO_OK) != (n_words == 12 && split == 6 && cost != OBJ_PROGRAM)) { printf("truncated program: %d %d %d -> %d\n", n_words, split, cost, rc); return 1; }
      }
  for (int it = 0; it < 200000; it++) {
    const int R = 1 + next() % 3, cost = next() % 4, n_words = 1 + next() % 24, n_consts = next() % 3, n_params = next() % 3;
    const int total = R + (obj_is_program(cost) ? 1 : 0);
    std::vector<int> words(2 * n_words), row_ptr(total + 1);
    for (int w = 0; w < n_words; w++) {
      words[2 * w] = next() % 8 == 0 ? (int)(next() % 40) - 10 : (int)(next() % 14);
      words[2 * w + 1] = (int)(next() % 7) - 1;
    }
    // half of the streams get sorted row pointers and, per row, a random walk that respects the stack and ends on one
    // value; one in four of those then has one word overwritten at random
    const bool tidy = next() % 2;
    for (int r = 0; r <= total; r++) row_ptr[r] = tidy ? (int)((long long)n_words * r / total) : (int)(next() % (n_words + 3)) - 1;
    if (tidy) {
      for (int r = 0; r < total; r++) {
        int sp = 0;
        for (int w = row_ptr[r]; w < row_ptr[r + 1] - 1; w++) {
          const int rem = row_ptr[r + 1] - 1 - w, pick = next() % 3;       // words left in the row before its END
          if (sp == 0 || (pick == 0 && sp < rem)) { words[2 * w] = SCO_OP_X + next() % 3; words[2 * w + 1] = next() % 3; sp++; }
          else if (sp >= 2 && (pick == 1 || sp > rem)) { words[2 * w] = SCO_OP_ADD + next() % 4; sp--; }
          else words[2 * w] = SCO_OP_NEG + next() % 6;
        }
        if (row_ptr[r + 1] > 0) words[2 * (row_ptr[r + 1] - 1)] = SCO_OP_END;
      }
      if (next() % 4 == 0) { const int w = next() % n_words; words[2 * w] = (int)(next() % 18) - 2; words[2 * w + 1] = (int)(next() % 7) - 1; }
    }
    const char *err = nullptr;
    const int rc = sqp_check_program(R, cost, 4, 2, n_words, words.data(), row_ptr.data(), n_consts, n_params, &err);
    progs++; prog_ok += rc == SCO_OK;
    if (rc != SCO_OK) continue;
    // an accepted program runs inside the stack and the operand arrays
    for (int r = 0; r < total; r++) {
      const int nx = (r < R || cost == OBJ_BLOCK) ? 4 : 2;
      int sp = 0;
      for (int w = row_ptr[r]; w < row_ptr[r + 1] - 1; w++) {
        const int op = words[2 * w], arg = words[2 * w + 1];
        if (op == SCO_OP_X || op == SCO_OP_P || op == SCO_OP_C) {
          if (arg < 0 || arg >= (op == SCO_OP_X ? nx : op == SCO_OP_P ? n_params : n_consts) || sp >= SCO_PROGRAM_STACK) { printf("accepted a bad operand\n"); return 1; }
          sp++;
        } else if (op >= SCO_OP_ADD && op <= SCO_OP_DIV) { if (sp < 2) { printf("accepted a stack underflow\n"); return 1; } sp--; }
        else if (op < SCO_OP_NEG || op > SCO_OP_SQUARE || sp < 1) { printf("accepted a bad opcode\n"); return 1; }
      }
      if (sp != 1 || words[2 * (row_ptr[r + 1] - 1)] != SCO_OP_END) { printf("accepted a bad row end\n"); return 1; }
    }
  }
  printf("%lld programs, %lld accepted: every accepted one stays inside the stack and the operand arrays\n", progs, prog_ok);
  return prog_ok > 1000 ? 0 : 1;
}
