// layout_big.h -- what bt_plan_build (big_plan.cpp) and the kernels of the structured global-memory form
// (sco_qp_big.hip) must agree on.  No HIP header.
#pragma once

// chunk descriptor of the structured form (bt_plan_build): 16 ints per chunk
#define CH_STRIDE 16      // kind, nact, ncols, r0, c0, pos0, col stride, e0, j0, r1, ep0, ep0 stride, ep1, ep1 stride, partial base, pad
#define BT_MAXBS 16       // largest block order (half-bandwidth of the core's Schur complement) the structured form takes
