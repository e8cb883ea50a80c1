// sco_lanes.h -- how a double moves between the 64 lanes of a wavefront: the one place where the kernel tiers spell out
// DPP controls, the gfx950 lane swaps and v_readlane.  Lanes are numbered 0 .. 63; a DPP "row" is 16 consecutive lanes
// (row r = lanes 16 r .. 16 r + 15), a "quad" four, a "pair" lanes l and l ^ 1.  Every reduction here has a fixed
// association order, so results are run-to-run deterministic, and every contract below is stated per lane;
// tests/test_lanes_gpu.py checks each against a model written from these sentences (sco_lanes_probe.hip runs them).
//
// Everything here is __device__ __forceinline__: no translation unit of its own, no ABI.
//
// Order of the halves.  A double moves as two 32-bit registers, and which half the source names first reaches the
// machine code (instruction order, in sco_qp_big.hip register numbers too).  The tiers grew up with two orders: the
// scans (row_scan15, wave_scan63) move the low half first, everything else the high half first.  lane_dpp keeps both
// behind its last template parameter (lane_scan_step hands it through) so that every kernel compiles to the code it
// had before this header existed; only row_scan15 and wave_scan63 set it, no caller outside this header should.
//
// Not here, on purpose: the variable-width __shfl_xor loops of qp_factor_kernel and sco_qp_polish.hip, the __shfl
// broadcasts, every readfirstlane, and the inline-assembly DPP chains of the wavefront sweep (WV_DPP_STEP,
// WV_FMAC_DPP in sco_admm_wv.hip), which fuse the move into an FMA.  WV_SYNC of sco_admm_wv.hip stays a second
// hand-over beside wave_lds_fence (one acq_rel fence, not a release / acquire pair): with wave_lds_fence in its
// place the wavefront kernels compile to different code.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned int lane_u2 __attribute__((ext_vector_type(2)));

// --------------------------------------------------------------------------
// the mover and the swap
// --------------------------------------------------------------------------
// v through the DPP control CTRL, in the rows of RMASK (bit r = row r): lane l gets v of the lane CTRL names as its
// source.  A lane without a source (shifted in from outside its row, or in a row RMASK leaves out) gets 0.0, or with
// KEEP its own v.  Controls in use: quad_perm [1,0,3,2] 0xb1 (l ^ 1), quad_perm [2,3,0,1] 0x4e (l ^ 2),
// row_half_mirror 0x141 (l ^ 7), row_mirror 0x140 (l ^ 15), row_shr:n 0x110 + n (l - n inside the row),
// row_bcast15 0x142 (lane 15 of the row below, for every lane of rows 1 .. 3), row_bcast31 0x143 (lane 31, for
// every lane of rows 2 and 3).
template <int CTRL, int RMASK = 0xf, bool KEEP = false, bool LOW_FIRST = false>
__device__ __forceinline__ double lane_dpp(double v) {
  auto half = [](int h) { return KEEP ? __builtin_amdgcn_update_dpp(h, h, CTRL, RMASK, 0xf, false) : __builtin_amdgcn_update_dpp(0, h, CTRL, RMASK, 0xf, true); };
  int lo = __double2loint(v), hi = __double2hiint(v);
  if (LOW_FIRST) { lo = half(lo); hi = half(hi); } else { hi = half(hi); lo = half(lo); }
  return __hiloint2double(hi, lo);
}
// v of lane LANE in every lane (v_readlane)
template <int LANE>
__device__ __forceinline__ double lane_bcast(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), LANE), __builtin_amdgcn_readlane(__double2loint(v), LANE));
}
// v_permlane32_swap (W = 32): the upper 32 lanes of a change places with the lower 32 lanes of b -- a ends as
// a[0..31] | b[0..31], b as a[32..63] | b[32..63].  v_permlane16_swap (W = 16): the odd rows of a change places with
// the even rows of b, row 1 with row 0 and row 3 with row 2 -- a ends as the rows a0 b0 a2 b2, b as a1 b1 a3 b3.
// lane_swap_halves leaves the four registers as they come out (.x: a's, .y: b's), for the one caller that rejoins only
// the double its lane needs (wv_meet of sco_admm_wv.hip without DIRECT: rejoining both first changed that file's code).
template <int W>
__device__ __forceinline__ void lane_swap_halves(double a, double b, lane_u2 &lo, lane_u2 &hi) {
  static_assert(W == 16 || W == 32, "there is a 16-lane and a 32-lane swap");
  const unsigned al = (unsigned)__double2loint(a), ah = (unsigned)__double2hiint(a), bl = (unsigned)__double2loint(b), bh = (unsigned)__double2hiint(b);
  lo = W == 16 ? __builtin_amdgcn_permlane16_swap(al, bl, false, false) : __builtin_amdgcn_permlane32_swap(al, bl, false, false);
  hi = W == 16 ? __builtin_amdgcn_permlane16_swap(ah, bh, false, false) : __builtin_amdgcn_permlane32_swap(ah, bh, false, false);
}
template <int W>
__device__ __forceinline__ void lane_swap(double &a, double &b) {
  lane_u2 lo, hi;
  lane_swap_halves<W>(a, b, lo, hi);
  a = __hiloint2double((int)hi.x, (int)lo.x); b = __hiloint2double((int)hi.y, (int)lo.y);
}
// The swap, then a + b or fmax(a, b) of what each lane holds: one instruction pair folds two values at once.
// W = 32: lane l < 32 gets a[l] op a[l + 32], lane l >= 32 gets b[l - 32] op b[l].  W = 16: the lanes of rows 0 and 2
// get row 0 op row 1 and row 2 op row 3 of a, the lanes of rows 1 and 3 the same of b.
template <int W, bool IS_MAX = false>
__device__ __forceinline__ double lane_fold(double a, double b) {
  lane_swap<W>(a, b);
  return IS_MAX ? fmax(a, b) : a + b;
}

// --------------------------------------------------------------------------
// scans: the result is valid in ONE lane, the others hold partial results
// --------------------------------------------------------------------------
// one step: v op (v moved by CTRL); a lane without a source keeps v (the sum adds 0.0, the maximum meets itself, so
// a NaN survives a maximum exactly when every lane taking part holds one)
template <int CTRL, bool IS_MAX, int RMASK = 0xf, bool LOW_FIRST = false>
__device__ __forceinline__ double lane_scan_step(double v) {
  const double s = lane_dpp<CTRL, RMASK, IS_MAX, LOW_FIRST>(v);
  return IS_MAX ? fmax(v, s) : v + s;
}
// sum or maximum of a row, valid in its lane 15: row_shr 1, 2, 4, 8.  Lane 15 ends with
// ((v15 + v14) + (v13 + v12)) + ((v11 + v10) + (v9 + v8)) + (the same of lanes 7 .. 0).
template <bool IS_MAX>
__device__ __forceinline__ double row_scan15(double v) {
  v = lane_scan_step<0x111, IS_MAX, 0xf, true>(v); v = lane_scan_step<0x112, IS_MAX, 0xf, true>(v);
  v = lane_scan_step<0x114, IS_MAX, 0xf, true>(v); v = lane_scan_step<0x118, IS_MAX, 0xf, true>(v);
  return v;
}
// sum or maximum of the wavefront, valid in lane 63: the row scan, then row_bcast15 into rows 1 and 3 (row mask 0xa)
// and row_bcast31 into rows 2 and 3 (0xc): lane 63 ends with (r3 + r2) + (r1 + r0) of the row results.  VALU only: the
// shuffles of wave_max go through the LDS permute path six dependent times per value and made the termination test's
// reductions cost 3.7 k cycles each (profiles/r01_check_stamps.txt).
template <bool IS_MAX>
__device__ __forceinline__ double wave_scan63(double v) {
  v = row_scan15<IS_MAX>(v);
  v = lane_scan_step<0x142, IS_MAX, 0xa, true>(v); v = lane_scan_step<0x143, IS_MAX, 0xc, true>(v);
  return v;
}

// --------------------------------------------------------------------------
// reductions whose result every lane taking part holds
// --------------------------------------------------------------------------
// both lanes of a pair end with v + (the other lane's v)
__device__ __forceinline__ double pair_sum(double v) { return v + lane_dpp<0xb1>(v); }
// all four lanes of a quad end with the quad's sum: the pair, then the other pair of the quad
__device__ __forceinline__ double quad_sum(double v) {
  v += lane_dpp<0xb1>(v);
  v += lane_dpp<0x4e>(v);
  return v;
}
// every lane ends with the sum or maximum of the wavefront, in registers: lane distances 1, 2, the half mirror, the
// row mirror, then the two folds (rows 0 op 1 and 2 op 3, then lower op upper half).  (__shfl_xor goes through
// ds_bpermute: an LDS round trip per step, 48 of them per termination test of the wavefront tier.)
template <bool IS_MAX>
__device__ __forceinline__ double wave_reduce_all(double v) {
  auto op = [](double a, double b) { return IS_MAX ? fmax(a, b) : a + b; };
  v = op(v, lane_dpp<0xb1>(v));
  v = op(v, lane_dpp<0x4e>(v));
  v = op(v, lane_dpp<0x141>(v));
  v = op(v, lane_dpp<0x140>(v));
  v = lane_fold<16, IS_MAX>(v, v);
  return lane_fold<32, IS_MAX>(v, v);
}
// the same through the shuffles, lane distances 32, 16, .. 1 (each step: v op v of lane l ^ distance); the summation
// order is part of the result
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// --------------------------------------------------------------------------
// hand-over through LDS inside ONE wavefront
// --------------------------------------------------------------------------
// What one lane wrote to LDS, another lane of the same wavefront reads behind this.  The LDS operations of one
// wavefront complete in the order they were issued, so no s_barrier is needed (and none is paid for); the fences and
// the wave barrier only keep the compiler from moving accesses across the hand-over.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
