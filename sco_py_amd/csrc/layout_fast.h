// layout_fast.h -- what fast_plan_build (reg_fast_plan.cpp) and qp_admm_fast_kernel (sco_admm_fast.hip) must agree on:
// the workgroup and the tiling of W.  No HIP header.
#pragma once
#include "layout_qp.h"    // SCO_HD

#define FT 512            // threads per workgroup
#define FW (FT / 64)      // wavefronts per workgroup
#define GJ 16             // column groups of the W tiling
#define GI (FT / GJ)      // row groups (32)

// Rows per thread (the kernel's NQ): two up to 2 x 512 rows, three beyond (fast_plan_build refuses m > 3 x 512).  The
// three-row instantiation has the looping dots only: patterns this large have wide columns anyway.
SCO_HD inline int fast_rows_per_thread(int m) { return m > 2 * FT ? 3 : 2; }
