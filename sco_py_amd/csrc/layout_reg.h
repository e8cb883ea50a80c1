// layout_reg.h -- what reg_plan_build (reg_fast_plan.cpp) and qp_admm_reg_kernel (sco_admm_reg.hip) must agree on: the
// workgroup, the tiling of W, the caps of the vectors in static LDS and that LDS's size.  No HIP header.
#pragma once

#define RT 512
#define RWV (RT / 64)
#define RGJ 16
#define RGI (RT / RGJ)
#define CAP_N 512
#define CAP_M 1024
#define CAP_NC 160
// static LDS of qp_admm_reg_kernel: its seven __shared__ arrays (s_xt, s_tv, s_ge, s_xc, s_rv, s_scr, s_red)
#define REG_STATIC_LDS (8 * (4 * CAP_N + 3 * CAP_M + 2 * CAP_NC + RWV * 8))
static_assert(REG_STATIC_LDS == 44032, "static LDS of qp_admm_reg_kernel");
