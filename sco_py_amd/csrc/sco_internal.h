// sco_internal.h -- the device side shared by the kernel files of the QP layer (sco_qp.hip and the tier files) and the SQP
// layer (sco_sqp.hip): HIP error handling, QpDev, every tier's device image (*Dev), AdmmArgs, the upload and launch
// prototypes, the handle.  Not part of the public ABI (that is include/sco_hip.h).
// Everything without a device type -- the tiers' host plans (*Host), QpTiers, the planners' prototypes -- is
// qp_tier_plans.h, which a host compiler takes without a HIP header; no planner lives in a file that includes this one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sco_hip.h"
#include "qp_plan.h"
#include "qp_tier.h"
#include "qp_tier_plans.h"

#define SCO_INFTY 1e30
#define SCO_MIN_SCALING 1e-4
#define SCO_MAX_SCALING 1e4
#define SCO_RHO_MIN 1e-6
#define SCO_RHO_TOL 1e-4
#define SCO_RHO_EQ_OVER_RHO_INEQ 1e3

int sco_hip_fail(hipError_t e, const char *what);
#define SCO_HIP(call)                                                         \
  do {                                                                        \
    hipError_t _e = (call);                                                   \
    if (_e != hipSuccess) return sco_hip_fail(_e, #call);                     \
  } while (0)

#define SCO_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)     // pass an SCO_ERR_* on to the caller

// Every ABI entry point runs on its handle's device and puts the caller's current device back on return
// (a process that shares HIP with PyTorch or another library on a different device must not find its
// current device changed by a call into this one).
struct ScoDeviceGuard {
  int prev = -1; bool ok = false;
  explicit ScoDeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~ScoDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  ScoDeviceGuard(const ScoDeviceGuard &) = delete;
  ScoDeviceGuard &operator=(const ScoDeviceGuard &) = delete;
};
#define SCO_ON_DEVICE(dev)                                                    \
  ScoDeviceGuard sco_guard_(dev);                                             \
  if (!sco_guard_.ok) return sco_hip_fail(hipGetLastError(), "hipSetDevice")

// ---- host glue shared by the tier files -------------------------------------
// A vector as a device array, entered in `allocs` (freed with the handle); an empty vector still gets an allocation.
template <typename T>
inline int sco_upload(std::vector<void *> &allocs, const std::vector<T> &v, const T **out) {
  void *p = nullptr;
  size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  SCO_HIP(hipMalloc(&p, bytes));
  allocs.push_back(p);
  if (!v.empty()) SCO_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (const T *)p;
  return SCO_OK;
}
// A zeroed device array of `count` elements, entered in `allocs`.
template <typename T>
inline int sco_alloc_zeroed(std::vector<void *> &allocs, size_t count, T **out) {
  void *p = nullptr;
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  SCO_HIP(hipMalloc(&p, bytes));
  SCO_HIP(hipMemset(p, 0, bytes));
  allocs.push_back(p);
  *out = (T *)p;
  return SCO_OK;
}
// The dynamic-LDS limit of a kernel, raised once per device (hipFuncSetAttribute applies to the current device only).
// attr_done: a static array of the calling launch helper, one per kernel instantiation; `what`: the call as the error
// text of a failure names it (SCO_LDS_ATTR spells it the way the launch helpers' own SCO_HIP lines did).
inline int sco_lds_attr(const void *kernel, int bytes, bool (&attr_done)[64], const char *what) {
  int dev_ = 0;
  (void)hipGetDevice(&dev_);
  dev_ &= 63;
  if (!attr_done[dev_]) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return sco_hip_fail(e, what);
    attr_done[dev_] = true;
  }
  return SCO_OK;
}
#define SCO_LDS_ATTR(kernel, bytes, attr_done)                                                                             \
  SCO_TRY(sco_lds_attr((const void *)kernel, bytes, attr_done,                                                             \
                       "hipFuncSetAttribute((const void *)" #kernel ", hipFuncAttributeMaxDynamicSharedMemorySize, " #bytes ")"))

// Device-side view of one batched QP: plans (shared) + per-problem value arrays.
struct QpDev {
  int n, m, nnzP, nnzA, n_e, n_c, ncpl, nS, batch;
  // launch window (stream groups of the SQP loop): the kernels that honour it work on problem blockIdx.x + b0 and are
  // launched with nb workgroups (nb = 0: the whole batch from problem 0)
  int b0, nb;
  const int *list;   // or null: workgroup g works on problem list[g + b0] (< 0: none) instead of g + b0
  // shared index plans
  const int *Ap, *Ai, *Rp, *Rj, *Rpos, *Fp, *Fi, *Fpos, *Pdiag;
  const int *elim_var, *core_var, *elim_of, *core_of;
  const int *e_ptr, *pair_core, *pair_elim, *cp_ptr, *cp_row, *cp_pa, *cp_pe, *a_ptr, *a_pair;
  const int *s_a, *s_b, *s_ppos, *sa_ptr, *sa_row, *sa_pa, *sa_pb, *ss_ptr, *ss_k1, *ss_k2, *ss_e;
  // per-problem inputs (unscaled), problem-major
  double *Pval, *q, *Aval, *l, *u;
  int *w;
  // per-problem scaled data and factor, written by the setup kernel
  double *Ps, *As, *qs, *ls, *us, *D, *E, *cscale, *rho, *kee_inv, *cpl, *W;
  // per-problem outputs
  double *x, *y, *resid;
  int *status, *iters;
  // optional per-problem activity mask (NULL = all active); inactive problems
  // are skipped by both kernels
  const int *active;
  // parked solves of the row-local tier (time slicing): iterations done, scaled x / z / y / t' / g_e
  int *prog;
  double *sx, *sz, *sy, *st, *sg;
  // adaptive rho (opt-in): rho in use per problem, "rho changed: re-derive the cached right-hand sides on
  // resume" flag, "run setup" mask, number of updates
  double *rho_b;
  int *rflag, *smask, *nupd, *amask;   // amask: problems still parked (sco_qp_solve's own loop)
};
// workgroups of a per-problem kernel that honours the launch window
inline int qp_launch_nwg(const QpDev &d) { return d.nb > 0 ? d.nb : d.batch; }

// ---- the tiers' device images, upload and launch (host plans: qp_tier_plans.h) ----
// fast ADMM path (sco_admm_fast.hip): device copy of a SellHost
struct SellDev { const int *base, *width, *src; const unsigned short *idx; int total; };
struct FastDev { SellDev Ac, Ar, Ca, Ce; };

struct AdmmArgs {
  QpDev d;
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int max_iter, check;
  int warm;     // start from the previous solution in d.x / d.y (row-local and wavefront kernels, structured global-memory tier)
  int slice;    // > 0: at most this many ADMM iterations per launch (row-local and generic kernels), see RlArgs
  int adaptive; // adaptive rho: every ad_interval iterations the kernel estimates rho; when it must change the solve
                // parks with the new rho in d.rho_b[b] and d.smask[b] = d.rflag[b] = 1
  int ad_interval;
  double ad_tol;
  const int *skip;   // or null: problems with skip[b] != 0 are left alone (the wavefront tier has taken them)
};

int fast_upload(const FastHost &fh, std::vector<void *> &allocs, FastDev &fd);
int fast_launch(const AdmmArgs &a, const FastHost &fh, const FastDev &fd, hipStream_t st);

// register-resident ADMM path (sco_admm_reg.hip)
struct RegDev { const unsigned short *off; const int *role; const int *srcAc, *srcAr, *srcCa, *srcCe; };
int reg_upload(const RegHost &rh, std::vector<void *> &allocs, RegDev &rd);
int reg_launch(const AdmmArgs &a, const RegHost &rh, const RegDev &rd, hipStream_t st);

// row-local ADMM path (sco_admm_rl.hip)
struct RlDev { const unsigned short *off; const int *role, *srcAc, *srcAr[3], *pc_ptr, *pc_pos, *pc_core; };
int rl_upload(const RlHost &rh, std::vector<void *> &allocs, RlDev &rd);
int rl_launch(const AdmmArgs &a, const RlHost &rh, const RlDev &rd, hipStream_t st);

// wavefront tier (sco_admm_wv.hip)
// G: [batch][g_doubles] factor (pivot inverses, couplings); cst: [batch][cst_slots][64] constants of the termination test;
// wc: [batch] common weight of the hinge rows; ok: [batch] 1 = the problem's values have the penalty-QP structure (else the
// row-local kernel solves it: rl_need = its setup mask); scr: [batch][m + n] delta_y / delta_x of the last checked iteration
// w_ready: [batch] 1 = the problem's W buffer holds the dense inverse (the row-local kernel can run it), 0 = it still
// holds S (the wavefront tier factored this QP; qp_sweep_kernel has to run before the row-local kernel takes over)
// it_count: [1] ADMM iterations the tier's kernel has run since the last reset (diagnostics: per-tier rates of bench.py)
struct WvDev { const int *tab; double *G, *cst, *wc, *scr; int *ok, *rl_need, *w_ready, *pflag; unsigned long long *it_count; };
int wv_upload(const WvHost &wh, int batch, int n, int m, std::vector<void *> &allocs, WvDev &wd);
int wv_launch_factor(const AdmmArgs &a, const int *setup_mask, const WvHost &wh, const WvDev &wd, hipStream_t st);
int wv_launch(const AdmmArgs &a, const WvHost &wh, const WvDev &wd, hipStream_t st);
// row-local round on a handle that also holds the wavefront tier: need[b] = setup_mask[b] or (active and W not ready)
int wv_launch_need(const AdmmArgs &a, const int *setup_mask, const WvDev &wd, hipStream_t st);

// big tier (sco_qp_big.hip) and its structured variant
struct BigDev { const int *row_elim, *row_epos, *er_ptr, *er_row, *free_rows, *pc_ptr, *pc_pos, *pc_core; double *ws; };
int big_upload(const BigHost &bh, int batch, std::vector<void *> &allocs, BigDev &bd);
// park_part: [batch][npart] of a parked solve; cflag: [batch][nchunks] flags of the per-row constants that are known values
// for all rows of a dense chunk, ccon: [batch] the common row weight they refer to (written by qp_setup_big_kernel)
struct BtDev { const int *ch_desc, *it, *cent; double *blk, *ws, *park_part; int *cflag; double *ccon; const int *mf_id, *mf_h0, *mf_h1; };
int bt_upload(const BtHost &th, int batch, std::vector<void *> &allocs, BtDev &td);
// th/td null = dense route
// setup_mask: the problems whose setup + factorisation run (a.d.active: the ones whose ADMM runs); the structured
// form honours a.slice / a.adaptive (park and resume), the dense form runs every solve to the end
int big_launch(const AdmmArgs &a, const int *setup_mask, int scaling, const int *Pp, const int *Pi, const BigHost &bh,
               const BigDev &bd, const BtHost *th, const BtDev *td, hipStream_t st, hipEvent_t ev_mid, hipEvent_t mid2);

struct sco_qp : QpTiers {
  int device = 0;
  int cus = 0;                         // compute units of the device (tier choice by batch size)
  BigDev bigd{};
  BtDev btd{};
  RlDev rld{};
  WvDev wvd{};
  RegDev regd{};
  FastDev fastd{};
  QpDev d{};
  const int *Pp_dev = nullptr, *Pi_dev = nullptr;   // device copies of the P triu pattern
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  std::vector<void *> allocs;
  bool loaded = false, solved_once = false;
  double last_ms[2] = {0, 0};
  // polish (sco_qp_polish.hip): the handle holds the result of a sco_qp_solve on the values and bounds as loaded; the
  // call's device buffers (allocated by the first one); HIP-event time of the last call by kernel
  bool polish_ready = false;
  struct QpPolishBuf *pol = nullptr;
  double polish_ms[4] = {0, 0, 0, 0};
};
void qp_polish_free(sco_qp *qp);        // sco_qp_destroy: the polish buffers are not in `allocs` (the workspace is regrown)

// Internal (device-pointer) entry points used by the SQP layer.
int sco_qp_create_on_stream(int device, int batch, int n, int m, const int *Pp, const int *Pi,
                            const int *Ap, const int *Ai, hipStream_t stream, sco_qp **out);
// Launch setup + ADMM on the handle's stream for the problems whose active flag
// is non-zero; no host synchronisation.
// `mid` (may be null) is recorded between the two kernels so callers can split the time.
int sco_qp_launch(sco_qp *qp, const sco_qp_settings *st, const int *active_dev, hipEvent_t mid);
// Time-sliced variant for the SQP loop: setup runs for the problems flagged in `setup_mask` (those that start
// a new QP), ADMM for the ones in `active_dev` for at most `slice` iterations (0 = to the end); a problem whose
// solve is not finished keeps status 0 and is resumed by the next call.  Returns the slice actually used
// through *sliced (0 if the handle's tier cannot park a solve).
// With st->adaptive_rho the slice is the rho-update interval and `setup_mask` names the problems that START a
// QP (device array, or SCO_MASK_ALL / SCO_MASK_NONE); setup then also runs for parked problems whose rho changed.
#define SCO_MASK_ALL ((const int *)(uintptr_t)1)
#define SCO_MASK_NONE ((const int *)(uintptr_t)2)
// `grp` (may be null): run only problems [b0, b0 + nb) and on grp->stream instead of the handle's own (stream groups of
// the SQP loop; row-local tier with the Gauss-Jordan inversion only, see sco_qp_supports_groups)
// tier: 0 = the handle decides (wavefront tier when the batch has at least SCO_WV_MIN_PER_CU problems per CU), 1 = row-local
// kernel, 2 = wavefront tier (handles that hold it; others ignore the field), 3 = MIXED round (handles with the wavefront tier
// and an index list): the problems list[side_b0 .. side_b0 + side_nb) run on the row-local kernel for side_slices slices on
// side_stream, the rest of the window -- [b0, side_b0) and [side_b0 + side_nb, b0 + nb), one of them empty -- on the wavefront
// tier on `stream`, both launches resident at once (the side window on CUs the wavefront launch leaves free); the streams
// join before the call returns.  side_ev: three events of the caller's (no timing needed), not in use by an earlier round
// that may still be in flight.
struct QpGroup {                                                                      // list: see QpDev (null = none)
  int b0, nb; hipStream_t stream; const int *list; int tier;
  int side_b0 = 0, side_nb = 0, side_slices = 0; hipStream_t side_stream = nullptr; hipEvent_t side_ev[3] = {nullptr, nullptr, nullptr};
};
int sco_qp_launch_sliced(sco_qp *qp, const sco_qp_settings *st, const int *setup_mask, const int *active_dev,
                         int slice, hipEvent_t mid, int *sliced, const QpGroup *grp = nullptr);
bool sco_qp_supports_groups(const sco_qp *qp, const sco_qp_settings *st);
bool sco_qp_has_wv(const sco_qp *qp);
bool sco_qp_wv_links(const sco_qp *qp);   // the handle's wavefront plan holds link or stacked rows (NL > 0)
int sco_qp_wv_iters(const sco_qp *qp, unsigned long long *out);      // iterations run by the wavefront kernel since the reset
void sco_qp_wv_iters_reset(sco_qp *qp, hipStream_t st);   // the handle holds the wavefront tier and these settings can use it
bool sco_qp_can_adapt(const sco_qp *qp);   // false: this handle sits on the dense global-memory tier, which cannot park a solve
