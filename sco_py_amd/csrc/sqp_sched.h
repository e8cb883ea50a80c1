// sqp_sched.h -- scheduling policy of the SQP round loop (sco_sqp_solve): host arithmetic only, no device types.
//
// Which rounds go where is decided here from plain numbers -- the batch, the CU count, the settings and the SCO_SQP_*
// environment variables -- so that it can be read, and tested, without a GPU (tests/test_sqp_schedule.py, through the
// sco_debug_sqp_* entry points).  Results never depend on any of it: per problem the sequence of kernels and every
// decision is the same under every schedule, only the round something happens in moves.
#pragma once

#define SQP_MAX_GROUPS 4
#define SQP_DEPTH 2        // rounds kept in flight per stream group
#define SQP_MIX_DEFAULT 1  // mixed ADMM rounds (SCO_SQP_MIX): on
#define SQP_WV_PER_CU 4    // problems the wavefront tier puts on a CU (SCO_WV_PER_CU)
#define SQP_SEL_MAX 1024   // most problems sqp_select_kernel can sort for a mixed round (SEL_T)

// The environment of one solve, read once (sqp_sched_env).  Values are as written (atoi); the planner clamps them.
struct SqpSchedEnv {
  int slice = 0;                 // SCO_SQP_SLICE > 0: the default slice (tuning aid; honoured only when admm_slice == 0)
  int groups = 1;                // SCO_SQP_GROUPS
  bool select = true;            // SCO_SQP_SELECT: off only when its first character is '0'
  int mix = SQP_MIX_DEFAULT;     // SCO_SQP_MIX
  int mix_slack = 1;             // SCO_SQP_MIX_SLACK
  int mix_slices = 2;            // SCO_SQP_MIX_SLICES
  bool mix_tail = false;         // SCO_SQP_MIX_PICK is exactly "tail"
  int xcds = 0;                  // SCO_SQP_XCDS > 0: overrides the device's XCD count
  int trace = 0;                 // SCO_SQP_TRACE_ROUNDS: 0 unset, 1 set (the first 40 rounds, then every 100th), 2 every round
};
SqpSchedEnv sqp_sched_env();

struct SqpSchedIn {
  int batch = 0, cus = 0;                    // cus: 0 = unknown
  int admm_slice = 0;                        // sco_sqp_params: < 0 unsliced, 0 default, > 0 iterations per launch
  int adaptive_rho = 0, max_iter = 0, adaptive_interval = 0;    // QP settings; the interval: sco_qp_adaptive_interval
  int max_qp_solves = 0;
  int n_active = 0;                          // problems alive after the projection round
  bool supports_groups = false;              // the penalty QP's tier takes launch windows and index lists
  bool handle_wv = false;                    // the penalty QP's handle holds the wavefront tier
  int wv_min = 0;                            // sco_wv_min_live
  int xcds = 1;                              // XCDs of the device (SqpSchedEnv::xcds overrides)
  SqpSchedEnv env;
};

struct SqpSchedule {
  int cus = 0;
  int slice = 0;                             // ADMM iterations per launch, 0 = every QP in one launch
  int G = 1;                                 // stream groups; group g works on the problems [b0, b0 + nb)
  struct { int b0, nb, live; } grp[SQP_MAX_GROUPS] = {};     // live: upper bound of the group's live problems at the start
  bool select = false;                       // round selection (sqp_select_kernel)
  bool has_wv = false, handle_wv = false;    // the loop chooses the tier per round / the handle holds the wavefront tier
  int wv_min = 0;
  bool mix_on = false, mix_tail = false;
  int mix_slack = 0, mix_slices = 1, xcds = 1;
  int depth = SQP_DEPTH;                     // rounds enqueued ahead of the host
  long long round_cap = 0;                   // launches per group after which the loop gives up (SCO_SQP_FLAG_CAPPED)
  int trace = 0;
};
SqpSchedule sqp_schedule_plan(const SqpSchedIn &in);

// One round of a stream group of `group_nb` problems, `live` of them alive as far as the host knows (the newest count read
// back; it only falls), the group's round_index-th.
struct SqpRound {
  bool wv_round = false;       // the loop asks for the wavefront tier
  int pass = 0;                // problems one pass of the chip holds on the round's tier
  int nwg = 0;                 // workgroups of the round's kernels
  int mix_k = 0;               // side window of a mixed round (0: none)
  int side_off = 0;            // where in the round's list the side window starts
  int tier = 0;                // QpGroup::tier
  bool window = false;         // the ADMM launch gets a launch window (QpGroup) at all
  bool counts_as_wv = false;   // the round's ADMM launch runs on the wavefront tier
};
SqpRound sqp_round_plan(const SqpSchedule &sc, int group_nb, int live, int round_index);

// Mixed ADMM rounds: how many of `live` problems leave the wavefront launch (per_cu problems on a CU) for the row-local
// kernel (one problem on a whole CU) so that both launches are resident at once.
// Workgroups are dealt to the XCDs in rotation and an XCD that receives one wavefront more than its free CUs hold would
// double the round, so the count is taken per XCD: the largest k with
//     ceil(k / xcds) + slack + ceil(ceil((live - k) / xcds) / per_cu) <= cus / xcds
// and 0 when there is none, or while the wavefront launch alone still needs every CU (live > per_cu (cus - 1)).
int qp_mix_split(int live, int cus, int xcds, int slack, int per_cu);

// Stage times of overlapping stream groups.  The rounds of different groups overlap, so their intervals
// [begin_ms[i], end_ms[i]) are laid on one time axis and every instant is charged to ONE stage (0 convexify, 1 QP setup,
// 2 ADMM, 3 decisions): the ADMM launch if any group is inside one, else QP setup, else convexify, else the decisions --
// the ADMM figure is then the wall time during which at least one ADMM launch was resident or queued behind another
// group's.  Adds to ms[0 .. 3] and the length of the intervals' union to ms[4]; an instant inside no interval is
// charged to nobody.
void sqp_stage_sweep(const double *begin_ms, const double *end_ms, const int *stage, int n, double ms[5]);
