// layout_rl.h -- what rl_plan_build (rl_plan.cpp) and qp_admm_rl_kernel (sco_admm_rl.hip) must agree on: workgroup and
// W tiling, caps, slot widths of the packed offsets, the rows of the role table.  No HIP header.
#pragma once
#include "layout_qp.h"

#define LT 512
#define LWV (LT / 64)
#define LGJ 16
#define LGI (LT / LGJ)
#define LCAP_M 1280
#define LCAP_NC 160
#define LCW 12          // value slots of a core variable's column = 2 x operand pairs (default; 16 for the widest instantiation)
#define LCW_MAX 16
#define LCW_MAX3 20       // three-row-slot instantiation: 10 operand pairs per column
#define LNS_MAX 3
#define LRW 8           // value slots of a row's core entries (4 aligned pairs); the wide instantiation (CW = 16) takes 10
#define LRW_MAX 10
#define RL_ROLES 29
// aligned closed assignment: core index of the thread's W tile rows (3) and of the mat-vec total it stores (-1: none)
#define ROLE_WROW(rr) (25 + (rr))
#define ROLE_XOUT 28
// tile of the aligned layout: 8 column groups (lane bits 0, 4, 5) x 8 row groups per wavefront (lane bits 1-3)
#define AL_TR 3
#define AL_TC 18
#define AL_ROWS (8 * AL_TR)       // W rows (core columns) a wavefront can own
// role-table rows of row slot q (slots 0, 1 keep their r01 places; slot 2 follows)
#define ROLE_ROW(q) ((q) < 2 ? 4 + (q) : 20)
#define ROLE_EPOS(q) ((q) < 2 ? 6 + (q) : 21)
#define ROLE_RBASE(q) ((q) < 2 ? 9 + (q) : 22)
#define ROLE_RWID(q) ((q) < 2 ? 14 + (q) : 23)
#define ROLE_POS(q) ((q) < 2 ? 16 + (q) : 24)

// The instantiations of qp_admm_rl_kernel<TR, TC, CW, ADAPT, NS, LAY> that exist (each with its ADAPT twin): what rl_launch
// dispatches on and what rl_plan_build may accept -- a plan outside this list is refused, so that the tier choice goes on to
// the next tier.  lay: 0 open assignment, 1 eight column groups (lay8), 2 aligned closed assignment.
//   NS 2, CW 12: the six W tiles <1,2> <2,4> <3,6> <4,8> <5,9> <5,10>;  NS 2, CW 16 (wide): <5,9> <5,10>;
//   NS 3, CW 12 or 20: <5,9> <5,10>;  lay 1 / 2: <3,18> at CW 12 or 16, NS 2.
SCO_HD constexpr bool rl_has_kernel(int TR, int TC, int CW, int NS, int lay) {
  return lay != 0 ? (lay == 1 || lay == 2) && NS == 2 && TR == AL_TR && TC == AL_TC && (CW == LCW || CW == LCW_MAX)
         : TR == 5 ? (TC == 9 || TC == 10) && (NS == 2 ? CW == LCW || CW == LCW_MAX : NS == 3 && (CW == LCW || CW == LCW_MAX3))
                   : TR >= 1 && TR <= 4 && TC == 2 * TR && NS == 2 && CW == LCW;
}

// What sco_qp_info adds to the handle's dynamic part (RlHost::lds_bytes) for the static LDS of qp_admm_rl_kernel.  NOT the
// kernel's static LDS of today: the figure is the one reported since the kernel was written and is kept as reported.  The
// kernel's __shared__ arrays take 36 480 bytes today (37 888 in the aligned form), which is what rl_plan_build budgets 40 KB
// for.
#define RL_REPORTED_STATIC_LDS 30208
