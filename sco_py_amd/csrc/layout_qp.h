// layout_qp.h -- what the host planners and the kernels of the QP layer must agree on, generic part: the workgroup of the
// generic kernels (sco_qp.hip) and their LDS sizes, the LDS of a CU, and the macro the layout_*.h headers mark their
// functions with.  No HIP header: the planners (qp_tier.cpp, *_plan.cpp) are plain C++.
#pragma once
#include <cstddef>

#include "qp_plan.h"

// a function of a layout header: callable from kernels under hipcc, an ordinary function under a host compiler
#ifdef __HIP__
#define SCO_HD __host__ __device__
#else
#define SCO_HD
#endif

#define SCO_LDS_CAP (160 * 1024)   // LDS of a CU, bytes: no plan asks for more

#define SCO_BLOCK 256   // threads per workgroup (4 wavefronts of 64)
#define NWAVE (SCO_BLOCK / 64)

SCO_HD inline size_t admm_lds_doubles(int n, int m, int nnzA, int n_e, int n_c, int ncpl) {
  return (size_t)nnzA + n + 2 * (size_t)m + m + n + 2 * (size_t)m + m + n + n_e + 2 * (size_t)n_c + n_e + ncpl + m + n + NWAVE * 8;
}

inline size_t setup_lds_doubles(const QpPlan &pl) {
  return (size_t)pl.nnzP + pl.nnzA + 2 * (size_t)pl.n + pl.m + pl.n + pl.m + pl.ncpl + NWAVE * 2 +
         (size_t)pl.n_c * (pl.n_c + 1) / 2;
}
