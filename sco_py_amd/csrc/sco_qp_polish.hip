// sco_qp_polish.hip -- OSQP's polish step on the result of a sco_qp_solve (include/sco_hip.h: sco_qp_polish).
//
// Per problem with status SCO_QP_SOLVED, on the unscaled data of the handle:
//   1. polish_active_kernel    z = A x; row i is `low` if z_i - l_i < -y_i / w_i, `upp` if u_i - z_i < y_i / w_i; index
//                              lists by a workgroup prefix sum (low rows first, then upp rows), k = their number
//   2. polish_assemble_kernel  lower triangle of [[P + delta I, Ar'], [Ar, -delta I]] (order N = n + k, column-major, leading
//                              dimension ld = the batch's largest N rounded up to 16; padding: unit diagonal)
//   3. polish_factor_kernel    blocked right-looking LDL' without pivoting: a 16-column panel through LDS, the trailing
//                              update C -= (L_p D) L_p' on 16 x 16 tiles with v_mfma_f64_16x16x4 (or the vector ALU)
//   4. polish_solve_kernel     L D L' s = [-q; l_low; u_upp], refine_iter steps of iterative refinement against the
//                              unregularised matrix applied from the sparse P and A, residuals of the polished point,
//                              OSQP's acceptance rule, write-back of x, y, resid when accepted
// A row of multiplicity w enters once.  The y of the handle is the multiplier of the logical row, the sum over its w copies
// (what sco_qp_solve returns and a warm start reads), so OSQP's tests on one copy see y_i / w_i, the unknown of the reduced
// system is y_i itself and the dual residual is |P x + q + A' y|.  One workgroup per problem, kernels 2 .. 4 per chunk of
// the batch (csrc/qp_polish_plan.h).  No floating-point atomics: two runs give the same bits.
#include "sco_internal.h"
#include "qp_polish_plan.h"

#define POLISH_BLOCK 256       // threads of the active-set, assemble and solve kernels
#define POLISH_FBLOCK 512      // threads of the factor kernel (8 wavefronts share the tiles of a trailing update)
#define PT SCO_POLISH_TILE

struct QpPolishBuf {
  int *pos = nullptr, *act = nullptr, *kcnt = nullptr, *kmax = nullptr, *pstat = nullptr;
  double *ws = nullptr;
  size_t ws_bytes = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

struct PolishArgs {
  QpDev d;
  const int *Pp, *Pi;          // upper-triangular CSC pattern of P
  double delta;
  int refine;
  int ld, b0, nb;              // leading dimension of an image; the chunk: problems b0 .. b0 + nb - 1
  double *ws;                  // [nb][ld * ld]
  int *pos;                    // [batch][m] row -> index among the active rows, or -1
  int *act;                    // [batch][m] index -> row (the first k entries)
  int *kcnt;                   // [batch][2] k (-1: status not SCO_QP_SOLVED, polish does not run) and the number of low rows
  int *kmax;                   // [1] largest k of the batch
  int *pstat;                  // [batch] SCO_QP_POLISH_*
};

// The reduced order of problem b against the workspace the host allocated: false = nothing to do for this workgroup (not
// solved, or an order the images cannot hold -- the host sized them from the same k, so that is a guard, not a path).
__device__ inline bool polish_order(const PolishArgs &a, int b, int *k, int *N, int *Np) {
  const int kk = a.kcnt[2 * b];
  if (kk < 0 || kk > a.d.m) return false;
  const int nn = a.d.n + kk, np = (nn + PT - 1) / PT * PT;
  if (np > a.ld || np > SCO_POLISH_MAX_ORDER) return false;
  *k = kk; *N = nn; *Np = np;
  return true;
}

// ---- 1. active sets ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POLISH_BLOCK) void polish_active_kernel(PolishArgs a) {
  const QpDev &d = a.d;
  const int b = blockIdx.x, tid = threadIdx.x, n = d.n, m = d.m;
  __shared__ int s_lo[POLISH_BLOCK], s_up[POLISH_BLOCK];
  int *pos = a.pos + (size_t)b * m, *act = a.act + (size_t)b * m;
  if (d.status[b] != SCO_QP_SOLVED) {
    for (int i = tid; i < m; i += POLISH_BLOCK) pos[i] = -1;
    if (tid == 0) { a.kcnt[2 * b] = -1; a.kcnt[2 * b + 1] = 0; a.pstat[b] = SCO_QP_POLISH_NOT_RUN; }
    return;
  }
  const double *x = d.x + (size_t)b * n, *y = d.y + (size_t)b * m, *Av = d.Aval + (size_t)b * d.nnzA;
  const double *l = d.l + (size_t)b * m, *u = d.u + (size_t)b * m;
  const int *w = d.w + (size_t)b * m;
  // a thread owns a run of consecutive rows, so that the lists come out in row order
  const int per = (m + POLISH_BLOCK - 1) / POLISH_BLOCK;
  const int i0 = min(m, tid * per), i1 = min(m, i0 + per);
  int nlo = 0, nup = 0;
  for (int i = i0; i < i1; i++) {
    double z = 0.0;
    for (int t = d.Rp[i]; t < d.Rp[i + 1]; t++) z += Av[d.Rpos[t]] * x[d.Rj[t]];
    const double yc = y[i] / (double)max(w[i], 1);     // the multiplier of one copy of the row
    int c = 0;
    if (z - l[i] < -yc) c = 1;
    else if (u[i] - z < yc) c = 2;
    pos[i] = c;
    nlo += c == 1; nup += c == 2;
  }
  s_lo[tid] = nlo; s_up[tid] = nup;
  __syncthreads();
  for (int off = 1; off < POLISH_BLOCK; off <<= 1) {
    const int vl = tid >= off ? s_lo[tid - off] : 0, vu = tid >= off ? s_up[tid - off] : 0;
    __syncthreads();
    s_lo[tid] += vl; s_up[tid] += vu;
    __syncthreads();
  }
  const int klo = s_lo[POLISH_BLOCK - 1], k = klo + s_up[POLISH_BLOCK - 1];
  int olo = s_lo[tid] - nlo, oup = klo + s_up[tid] - nup;
  for (int i = i0; i < i1; i++) {
    const int c = pos[i];
    if (c == 1) { pos[i] = olo; act[olo++] = i; }
    else if (c == 2) { pos[i] = oup; act[oup++] = i; }
    else pos[i] = -1;
  }
  if (tid == 0) {
    a.kcnt[2 * b] = k; a.kcnt[2 * b + 1] = klo;
    a.pstat[b] = SCO_QP_POLISH_FAILED;          // until the solve kernel accepts the polished point
    atomicMax(a.kmax, k);
  }
}

// ---- 2. assembly ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POLISH_BLOCK) void polish_assemble_kernel(PolishArgs a) {
  const QpDev &d = a.d;
  const int b = a.b0 + blockIdx.x, tid = threadIdx.x, n = d.n, ld = a.ld;
  int k, N, Np;
  if (blockIdx.x >= a.nb || !polish_order(a, b, &k, &N, &Np)) return;
  double *K = a.ws + (size_t)blockIdx.x * ld * ld;
  for (int c = 0; c < Np; c++) {
    const double dg = c < n ? a.delta : c < N ? -a.delta : 1.0;
    for (int r = c + tid; r < Np; r += POLISH_BLOCK) K[(size_t)c * ld + r] = r == c ? dg : 0.0;
  }
  __syncthreads();
  const double *Pv = d.Pval + (size_t)b * d.nnzP, *Av = d.Aval + (size_t)b * d.nnzA;
  const int *pos = a.pos + (size_t)b * d.m;
  for (int j = tid; j < n; j += POLISH_BLOCK) {
    // P_ij, i <= j, sits at row j of column i of the lower triangle; A_ij of an active row at row n + pos of column j
    for (int t = a.Pp[j]; t < a.Pp[j + 1]; t++) {
      const int i = a.Pi[t];
      if (i >= 0 && i <= j) K[(size_t)i * ld + j] += Pv[t];
    }
    for (int t = d.Ap[j]; t < d.Ap[j + 1]; t++) {
      const int p = pos[d.Ai[t]];
      if (p >= 0 && p < k) K[(size_t)j * ld + n + p] = Av[t];
    }
  }
}

// ---- 3. factorisation ----------------------------------------------------------------------------------------------------
// Column-major lower triangle in, L (unit diagonal implied) below the diagonal and D on it out.  Panel p holds columns
// 16 p .. 16 p + 15 for rows >= 16 p as Lp[column][row] in LDS.  Inside the panel the columns go one by one (the pivot
// column's unscaled entries of the diagonal block are parked in piv first, so that every row can be scaled and can update
// its 15 other entries without reading a row another thread is scaling).  Then every 16 x 16 tile (I, J), p < J <= I, of the
// trailing matrix gets  C[r][c] -= sum_k L[r][k] d_k L[c][k]:  one wavefront per tile, D = A B + C with
// A[i][k] = -L[16 J + i][k], B[k][j] = d_k L[16 I + j][k]; lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16] and holds
// D[4 v + l / 16][l % 16], i.e. column 16 J + 4 v + l / 16 at row 16 I + l % 16: sixteen lanes on consecutive rows of a column.
typedef double polish_d4 __attribute__((ext_vector_type(4)));

template <bool MFMA>
__global__ __launch_bounds__(POLISH_FBLOCK) void polish_factor_kernel(PolishArgs a) {
  extern __shared__ double polish_sm[];
  const int b = a.b0 + blockIdx.x, tid = threadIdx.x, ld = a.ld;
  int k_, N_, Np;
  if (blockIdx.x >= a.nb || !polish_order(a, b, &k_, &N_, &Np)) return;
  double *K = a.ws + (size_t)blockIdx.x * ld * ld;
  double *Lp = polish_sm, *piv = polish_sm + (size_t)PT * ld, *dd = piv + PT;
  const int nt = Np / PT;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  for (int p = 0; p < nt; p++) {
    const int p0 = PT * p;
    for (int kk = 0; kk < PT; kk++)
      for (int r = p0 + tid; r < Np; r += POLISH_FBLOCK) Lp[kk * ld + r] = K[(size_t)(p0 + kk) * ld + r];
    __syncthreads();
    for (int kk = 0; kk < PT; kk++) {
      if (tid < PT) piv[tid] = Lp[kk * ld + p0 + tid];
      __syncthreads();
      const double dk = piv[kk];
      if (tid == 0) dd[kk] = dk;
      for (int r = p0 + kk + 1 + tid; r < Np; r += POLISH_FBLOCK) {
        const double lv = Lp[kk * ld + r] / dk;
        Lp[kk * ld + r] = lv;
        const int jend = min(PT - 1, r - p0);
        for (int j = kk + 1; j <= jend; j++) Lp[j * ld + r] -= lv * piv[j];
      }
      __syncthreads();
    }
    for (int kk = 0; kk < PT; kk++)
      for (int r = p0 + kk + tid; r < Np; r += POLISH_FBLOCK) K[(size_t)(p0 + kk) * ld + r] = Lp[kk * ld + r];
    const int t = nt - p - 1, ntile = t * (t + 1) / 2;
    for (int q = wave; q < ntile; q += POLISH_FBLOCK / 64) {
      int ti = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
      while ((ti + 1) * (ti + 2) / 2 <= q) ti++;
      while (ti * (ti + 1) / 2 > q) ti--;
      const int tj = q - ti * (ti + 1) / 2;
      const int r = PT * (p + 1 + ti) + li, c0 = PT * (p + 1 + tj);
      polish_d4 acc;
#pragma unroll
      for (int v = 0; v < 4; v++) { const int c = c0 + 4 * v + lk; acc[v] = r >= c ? K[(size_t)c * ld + r] : 0.0; }
      if (MFMA) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int kk = 4 * s + lk;
          const double av = -Lp[kk * ld + c0 + li], bv = dd[kk] * Lp[kk * ld + r];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
      } else {
#pragma unroll 2
        for (int kk = 0; kk < PT; kk++) {
          const double bv = dd[kk] * Lp[kk * ld + r];
#pragma unroll
          for (int v = 0; v < 4; v++) acc[v] = fma(-Lp[kk * ld + c0 + 4 * v + lk], bv, acc[v]);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; v++) { const int c = c0 + 4 * v + lk; if (r >= c) K[(size_t)c * ld + r] = acc[v]; }
    }
    __syncthreads();
  }
}

// ---- 4. solves, refinement, decision ---------------------------------------------------------------------------------------
// v <- (L D L')^-1 v for a vector of Np entries in LDS, 16 columns at a time: the diagonal block by one wavefront from an LDS
// copy, the rows below (forward) / the column sums (backward) by the whole workgroup.
__device__ inline void polish_ldl_solve(const double *K, int ld, int Np, double *v, double *tile, double *red) {
  const int tid = threadIdx.x, nt = Np / PT;
  for (int p = 0; p < nt; p++) {
    const int p0 = PT * p;
    { const int kk = tid >> 4, i = tid & 15; tile[kk * PT + i] = i > kk ? K[(size_t)(p0 + kk) * ld + p0 + i] : 0.0; }
    __syncthreads();
    if (tid < 64) {
      double val = tid < PT ? v[p0 + tid] : 0.0;
      for (int kk = 0; kk < PT - 1; kk++) {
        const double wk = __shfl(val, kk);
        if (tid < PT && tid > kk) val -= tile[kk * PT + tid] * wk;
      }
      if (tid < PT) v[p0 + tid] = val;
    }
    __syncthreads();
    for (int r = p0 + PT + tid; r < Np; r += POLISH_BLOCK) {
      double acc = v[r];
      for (int kk = 0; kk < PT; kk++) acc -= K[(size_t)(p0 + kk) * ld + r] * v[p0 + kk];
      v[r] = acc;
    }
    __syncthreads();
  }
  for (int i = tid; i < Np; i += POLISH_BLOCK) v[i] /= K[(size_t)i * ld + i];
  __syncthreads();
  for (int p = nt - 1; p >= 0; p--) {
    const int p0 = PT * p;
    {
      const int c = tid >> 4, s = tid & 15;
      double sum = 0.0;
      for (int r = p0 + PT + s; r < Np; r += PT) sum += K[(size_t)(p0 + c) * ld + r] * v[r];
      sum += __shfl_xor(sum, 8); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 1);
      if (s == 0) red[c] = v[p0 + c] - sum;
      tile[c * PT + s] = s > c ? K[(size_t)(p0 + c) * ld + p0 + s] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      double val = tid < PT ? red[tid] : 0.0;
      for (int kk = PT - 1; kk > 0; kk--) {
        const double vk = __shfl(val, kk);
        if (tid < kk) val -= tile[tid * PT + kk] * vk;
      }
      if (tid < PT) v[p0 + tid] = val;
    }
    __syncthreads();
  }
}

// max that keeps a NaN (fmax would drop it and a broken factorisation would pass for a small residual)
__device__ inline double polish_nanmax(double cur, double v) { return (v > cur || v != v) ? v : cur; }

__device__ inline double polish_block_max(double v, double *red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int off = POLISH_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] = polish_nanmax(red[tid], red[tid + off]);
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(POLISH_BLOCK) void polish_solve_kernel(PolishArgs a) {
  const QpDev &d = a.d;
  const int b = a.b0 + blockIdx.x, tid = threadIdx.x, n = d.n, m = d.m, ld = a.ld;
  int k, N, Np;
  if (blockIdx.x >= a.nb || !polish_order(a, b, &k, &N, &Np)) return;
  __shared__ double rhs[SCO_POLISH_MAX_ORDER], sol[SCO_POLISH_MAX_ORDER], wrk[SCO_POLISH_MAX_ORDER];
  __shared__ double tile[PT * PT], red[POLISH_BLOCK];
  const double *K = a.ws + (size_t)blockIdx.x * ld * ld;
  const double *Pv = d.Pval + (size_t)b * d.nnzP, *Av = d.Aval + (size_t)b * d.nnzA, *q = d.q + (size_t)b * n;
  const double *l = d.l + (size_t)b * m, *u = d.u + (size_t)b * m;
  const int *pos = a.pos + (size_t)b * m, *act = a.act + (size_t)b * m;
  const int klo = a.kcnt[2 * b + 1];
  for (int i = tid; i < Np; i += POLISH_BLOCK) {
    double v = 0.0;
    if (i < n) v = -q[i];
    else if (i < N) { const int row = min(max(act[i - n], 0), m - 1); v = i - n < klo ? l[row] : u[row]; }
    rhs[i] = v; sol[i] = v;
  }
  __syncthreads();
  polish_ldl_solve(K, ld, Np, sol, tile, red);
  for (int it = 0; it < a.refine; it++) {
    // wrk = rhs - [[P, Ar'], [Ar, 0]] sol from the sparse data, then sol += (L D L')^-1 wrk
    for (int i = tid; i < Np; i += POLISH_BLOCK) {
      double v = 0.0;
      if (i < n) {
        for (int t = d.Fp[i]; t < d.Fp[i + 1]; t++) v += Pv[d.Fpos[t]] * sol[d.Fi[t]];
        for (int t = d.Ap[i]; t < d.Ap[i + 1]; t++) { const int p = pos[d.Ai[t]]; if (p >= 0 && p < k) v += Av[t] * sol[n + p]; }
      } else if (i < N) {
        const int row = min(max(act[i - n], 0), m - 1);
        for (int t = d.Rp[row]; t < d.Rp[row + 1]; t++) v += Av[d.Rpos[t]] * sol[d.Rj[t]];
      }
      wrk[i] = i < N ? rhs[i] - v : 0.0;
    }
    __syncthreads();
    polish_ldl_solve(K, ld, Np, wrk, tile, red);
    for (int i = tid; i < Np; i += POLISH_BLOCK) sol[i] += wrk[i];
    __syncthreads();
  }
  // residuals of the polished point: pri = |A x - clip(A x, l, u)|_inf, dua = |P x + q + A' y|_inf
  double pri = 0.0, dua = 0.0;
  for (int i = tid; i < m; i += POLISH_BLOCK) {
    double z = 0.0;
    for (int t = d.Rp[i]; t < d.Rp[i + 1]; t++) z += Av[d.Rpos[t]] * sol[d.Rj[t]];
    double v = fmax(fmax(l[i] - z, z - u[i]), 0.0);
    if (z != z) v = z;
    pri = polish_nanmax(pri, v);
  }
  for (int j = tid; j < n; j += POLISH_BLOCK) {
    double g = q[j];
    for (int t = d.Fp[j]; t < d.Fp[j + 1]; t++) g += Pv[d.Fpos[t]] * sol[d.Fi[t]];
    for (int t = d.Ap[j]; t < d.Ap[j + 1]; t++) { const int p = pos[d.Ai[t]]; if (p >= 0 && p < k) g += Av[t] * sol[n + p]; }
    dua = polish_nanmax(dua, fabs(g));
  }
  pri = polish_block_max(pri, red);
  dua = polish_block_max(dua, red);
  double *resid = d.resid + 2 * (size_t)b;
  const double pa = resid[0], da = resid[1];
  const bool ok = (pri < pa && dua < da) || (pri < pa && da < 1e-10) || (dua < da && pa < 1e-10);
  __syncthreads();                                  // every thread has read the solve's residuals
  if (!ok) return;                                  // x, y, resid stay what the solve left; the status stays FAILED
  double *x = d.x + (size_t)b * n, *y = d.y + (size_t)b * m;
  for (int j = tid; j < n; j += POLISH_BLOCK) x[j] = sol[j];
  for (int i = tid; i < m; i += POLISH_BLOCK) {
    const int p = pos[i];
    y[i] = (p >= 0 && p < k) ? sol[n + p] : 0.0;
  }
  if (tid == 0) { resid[0] = pri; resid[1] = dua; a.pstat[b] = SCO_QP_POLISH_OK; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
extern "C" void sco_qp_default_polish_settings(sco_qp_polish_settings *s) {
  if (!s) return;
  s->delta = 1e-6;          // OSQP 0.6 defaults (delta, polish_refine_iter)
  s->refine_iter = 3;
}

void qp_polish_free(sco_qp *qp) {
  QpPolishBuf *pb = qp->pol;
  if (!pb) return;
  for (void *p : {(void *)pb->pos, (void *)pb->act, (void *)pb->kcnt, (void *)pb->kmax, (void *)pb->pstat, (void *)pb->ws})
    if (p) (void)hipFree(p);
  for (auto &e : pb->ev) if (e) (void)hipEventDestroy(e);
  delete pb;
  qp->pol = nullptr;
}

static int polish_buffers(sco_qp *qp) {
  if (qp->pol) return SCO_OK;
  QpPolishBuf *pb = qp->pol = new QpPolishBuf();      // (sco_qp_destroy frees whatever a failure below leaves)
  const size_t B = qp->d.batch, m = std::max(qp->d.m, 1);
  SCO_HIP(hipMalloc((void **)&pb->pos, B * m * sizeof(int)));
  SCO_HIP(hipMalloc((void **)&pb->act, B * m * sizeof(int)));
  SCO_HIP(hipMalloc((void **)&pb->kcnt, B * 2 * sizeof(int)));
  SCO_HIP(hipMalloc((void **)&pb->kmax, sizeof(int)));
  SCO_HIP(hipMalloc((void **)&pb->pstat, B * sizeof(int)));
  for (auto &e : pb->ev) SCO_HIP(hipEventCreate(&e));
  return SCO_OK;
}

template <bool MFMA>
static int polish_launch_factor(const PolishArgs &pa, int lds_bytes, hipStream_t st) {
  static bool attr_done[64];
  const int lds_max = (PT * SCO_POLISH_MAX_ORDER + 2 * PT) * (int)sizeof(double);
  SCO_LDS_ATTR(polish_factor_kernel<MFMA>, lds_max, attr_done);
  hipLaunchKernelGGL(polish_factor_kernel<MFMA>, dim3(pa.nb), dim3(POLISH_FBLOCK), lds_bytes, st, pa);
  SCO_HIP(hipGetLastError());
  return SCO_OK;
}

extern "C" int sco_qp_polish(sco_qp *qp, const sco_qp_polish_settings *s, double *x, double *y, int *polish_status,
                             double *resid) {
  if (!qp) { sco_set_error("sco_qp_polish: null handle"); return SCO_ERR_ARG; }
  sco_qp_polish_settings def;
  sco_qp_default_polish_settings(&def);
  if (!s) s = &def;
  if (!(s->delta > 0) || s->refine_iter < 0 || s->refine_iter > 100) { sco_set_error("sco_qp_polish: bad settings"); return SCO_ERR_ARG; }
  const QpDev &d = qp->d;
  // a property of the pattern, so it is answered first: such a handle never polishes, solved or not
  if (!qp_polish_order_fits(d.n, d.m)) { sco_set_error(qp_polish_err_text(QP_POLISH_ERR_ORDER)); return SCO_ERR_CAPACITY; }
  if (!qp->polish_ready) {
    sco_set_error("sco_qp_polish: no sco_qp_solve result on the loaded values (solve first; loading values or bounds discards it)");
    return SCO_ERR_STATE;
  }
  SCO_ON_DEVICE(qp->device);
  SCO_TRY(polish_buffers(qp));
  QpPolishBuf *pb = qp->pol;
  hipStream_t st = qp->stream;
  const int B = d.batch;
  PolishArgs pa{};
  pa.d = d; pa.d.b0 = 0; pa.d.nb = 0; pa.d.list = nullptr; pa.d.active = nullptr;
  pa.Pp = qp->Pp_dev; pa.Pi = qp->Pi_dev; pa.delta = s->delta; pa.refine = s->refine_iter;
  pa.pos = pb->pos; pa.act = pb->act; pa.kcnt = pb->kcnt; pa.kmax = pb->kmax; pa.pstat = pb->pstat;
  for (double &t : qp->polish_ms) t = 0.0;
  SCO_HIP(hipMemsetAsync(pb->kmax, 0, sizeof(int), st));
  SCO_HIP(hipEventRecord(pb->ev[0], st));
  hipLaunchKernelGGL(polish_active_kernel, dim3(B), dim3(POLISH_BLOCK), 0, st, pa);
  SCO_HIP(hipGetLastError());
  SCO_HIP(hipEventRecord(pb->ev[1], st));
  int kmax = 0;
  SCO_HIP(hipMemcpyAsync(&kmax, pb->kmax, sizeof(int), hipMemcpyDeviceToHost, st));
  SCO_HIP(hipStreamSynchronize(st));
  float ms = 0;
  SCO_HIP(hipEventElapsedTime(&ms, pb->ev[0], pb->ev[1]));
  qp->polish_ms[0] = ms;
  const QpPolishPlan pl = qp_polish_plan(d.n, d.m, B, kmax, 0);
  if (pl.rc) { sco_set_error(qp_polish_err_text(pl.err)); return pl.rc; }
  if (pb->ws_bytes < (size_t)pl.ws_bytes) {
    if (pb->ws) { (void)hipFree(pb->ws); pb->ws = nullptr; pb->ws_bytes = 0; }
    SCO_HIP(hipMalloc((void **)&pb->ws, (size_t)pl.ws_bytes));
    pb->ws_bytes = (size_t)pl.ws_bytes;
  }
  pa.ld = pl.ld; pa.ws = pb->ws;
  const bool mfma = qp_polish_use_mfma();
  for (int c = 0; c < pl.chunks; c++) {
    pa.b0 = c * pl.per_chunk; pa.nb = std::min(pl.per_chunk, B - pa.b0);
    SCO_HIP(hipEventRecord(pb->ev[0], st));
    hipLaunchKernelGGL(polish_assemble_kernel, dim3(pa.nb), dim3(POLISH_BLOCK), 0, st, pa);
    SCO_HIP(hipGetLastError());
    SCO_HIP(hipEventRecord(pb->ev[1], st));
#ifdef SCO_QP_POLISH_NO_MFMA
    SCO_TRY(polish_launch_factor<false>(pa, pl.lds_bytes, st));
#else
    if (mfma) SCO_TRY(polish_launch_factor<true>(pa, pl.lds_bytes, st));
    else SCO_TRY(polish_launch_factor<false>(pa, pl.lds_bytes, st));
#endif
    SCO_HIP(hipEventRecord(pb->ev[2], st));
    hipLaunchKernelGGL(polish_solve_kernel, dim3(pa.nb), dim3(POLISH_BLOCK), 0, st, pa);
    SCO_HIP(hipGetLastError());
    SCO_HIP(hipEventRecord(pb->ev[3], st));
    SCO_HIP(hipStreamSynchronize(st));            // the next chunk reuses the workspace and the events
    for (int e = 0; e < 3; e++) {
      SCO_HIP(hipEventElapsedTime(&ms, pb->ev[e], pb->ev[e + 1]));
      qp->polish_ms[1 + e] += ms;
    }
  }
  (void)mfma;
  const size_t Bs = (size_t)B;
  if (x) SCO_HIP(hipMemcpyAsync(x, d.x, Bs * d.n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (y && d.m) SCO_HIP(hipMemcpyAsync(y, d.y, Bs * d.m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (polish_status) SCO_HIP(hipMemcpyAsync(polish_status, pb->pstat, Bs * sizeof(int), hipMemcpyDeviceToHost, st));
  if (resid) SCO_HIP(hipMemcpyAsync(resid, d.resid, Bs * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  SCO_HIP(hipStreamSynchronize(st));
  return SCO_OK;
}

// ---- diagnostics (not in the public header) --------------------------------------------------------------------------------
// out = {return code, refusal (QpPolishErr), ld, problems per chunk, chunks, LDS bytes of the factor kernel, workspace bytes}
extern "C" int sco_debug_polish_plan(int n, int m, int batch, int max_k, long long budget, long long *out) {
  if (!out) return SCO_ERR_ARG;
  const QpPolishPlan p = qp_polish_plan(n, m, batch, max_k, budget);
  out[0] = p.rc; out[1] = p.err; out[2] = p.ld; out[3] = p.per_chunk; out[4] = p.chunks; out[5] = p.lds_bytes; out[6] = p.ws_bytes;
  return p.rc;
}
// HIP-event milliseconds of the last sco_qp_polish by kernel, summed over its chunks: active sets, assembly, factorisation,
// solves + decision; k[batch] (may be null): active rows per problem, -1 where polish did not run
extern "C" int sco_debug_polish_info(sco_qp *qp, double ms[4], int *k) {
  if (!qp || !ms) return SCO_ERR_ARG;
  for (int i = 0; i < 4; i++) ms[i] = qp->polish_ms[i];
  if (k) {
    if (!qp->pol) return SCO_ERR_STATE;
    SCO_ON_DEVICE(qp->device);
    std::vector<int> kc(2 * (size_t)qp->d.batch);
    SCO_HIP(hipMemcpy(kc.data(), qp->pol->kcnt, kc.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < qp->d.batch; b++) k[b] = kc[2 * (size_t)b];
  }
  return SCO_OK;
}
