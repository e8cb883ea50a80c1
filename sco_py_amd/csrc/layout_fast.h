// layout_fast.h -- what fast_plan_build (reg_fast_plan.cpp) and qp_admm_fast_kernel (sco_admm_fast.hip) must agree on:
// the workgroup and the tiling of W.  No HIP header.
#pragma once

#define FT 512            // threads per workgroup
#define FW (FT / 64)      // wavefronts per workgroup
#define GJ 16             // column groups of the W tiling
#define GI (FT / GJ)      // row groups (32)
