// sco_lanes_probe.hip -- the cross-lane primitives of sco_lanes.h on ONE wavefront, one at a time, so that their lane
// contracts can be tested by themselves (tests/test_lanes_gpu.py) and not only through whole solves.  Diagnostics: no
// solver path calls this.
#include "sco_internal.h"
#include "sco_lanes.h"

// the ops of sco_debug_lanes (include/sco_hip.h lists them for callers: keep the two in step)
enum {
  LANES_DPP_XOR1 = 0, LANES_DPP_XOR2, LANES_DPP_HALF_MIRROR, LANES_DPP_MIRROR, LANES_DPP_SHR1_ZERO, LANES_DPP_SHR8_KEEP,
  LANES_DPP_BCAST15_ZERO, LANES_DPP_BCAST31_KEEP, LANES_BCAST23, LANES_SWAP16, LANES_SWAP32, LANES_FOLD16_SUM,
  LANES_FOLD16_MAX, LANES_FOLD32_SUM, LANES_FOLD32_MAX, LANES_STEP_SHR2_SUM, LANES_STEP_SHR4_MAX, LANES_ROW15_SUM,
  LANES_ROW15_MAX, LANES_WAVE63_SUM, LANES_WAVE63_MAX, LANES_PAIR_SUM, LANES_QUAD_SUM, LANES_ALL_SUM, LANES_ALL_MAX,
  LANES_SHFL_SUM, LANES_SHFL_MAX, LANES_LDS_REVERSE, LANES_N_OPS
};

__global__ __launch_bounds__(64) void lanes_probe_kernel(int op, const double *a_in, const double *b_in, double *a_out, double *b_out) {
  __shared__ double lds[64];
  const int lane = threadIdx.x;
  double a = a_in[lane], b = b_in[lane];
  switch (op) {
    case LANES_DPP_XOR1: a = lane_dpp<0xb1>(a); break;
    case LANES_DPP_XOR2: a = lane_dpp<0x4e>(a); break;
    case LANES_DPP_HALF_MIRROR: a = lane_dpp<0x141>(a); break;
    case LANES_DPP_MIRROR: a = lane_dpp<0x140>(a); break;
    case LANES_DPP_SHR1_ZERO: a = lane_dpp<0x111>(a); break;
    case LANES_DPP_SHR8_KEEP: a = lane_dpp<0x118, 0xf, true>(a); break;
    case LANES_DPP_BCAST15_ZERO: a = lane_dpp<0x142, 0xa>(a); break;
    case LANES_DPP_BCAST31_KEEP: a = lane_dpp<0x143, 0xc, true>(a); break;
    case LANES_BCAST23: a = lane_bcast<23>(a); break;
    case LANES_SWAP16: lane_swap<16>(a, b); break;
    case LANES_SWAP32: lane_swap<32>(a, b); break;
    case LANES_FOLD16_SUM: a = lane_fold<16>(a, b); break;
    case LANES_FOLD16_MAX: a = lane_fold<16, true>(a, b); break;
    case LANES_FOLD32_SUM: a = lane_fold<32>(a, b); break;
    case LANES_FOLD32_MAX: a = lane_fold<32, true>(a, b); break;
    case LANES_STEP_SHR2_SUM: a = lane_scan_step<0x112, false>(a); break;
    case LANES_STEP_SHR4_MAX: a = lane_scan_step<0x114, true>(a); break;
    case LANES_ROW15_SUM: a = row_scan15<false>(a); break;
    case LANES_ROW15_MAX: a = row_scan15<true>(a); break;
    case LANES_WAVE63_SUM: a = wave_scan63<false>(a); break;
    case LANES_WAVE63_MAX: a = wave_scan63<true>(a); break;
    case LANES_PAIR_SUM: a = pair_sum(a); break;
    case LANES_QUAD_SUM: a = quad_sum(a); break;
    case LANES_ALL_SUM: a = wave_reduce_all<false>(a); break;
    case LANES_ALL_MAX: a = wave_reduce_all<true>(a); break;
    case LANES_SHFL_SUM: a = wave_sum(a); break;
    case LANES_SHFL_MAX: a = wave_max(a); break;
    case LANES_LDS_REVERSE: lds[lane] = a; wave_lds_fence(); a = lds[63 - lane]; break;
    default: break;
  }
  a_out[lane] = a; b_out[lane] = b;
}

extern "C" int sco_debug_lanes(int device, int op, const double *a, const double *b, double *out_a, double *out_b) {
  if (op < 0 || op >= LANES_N_OPS || !a || !out_a) { sco_set_error("sco_debug_lanes: bad argument"); return SCO_ERR_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    sco_set_error("sco_debug_lanes: no HIP device visible (this library has no CPU fallback)");
    return SCO_ERR_NO_GPU;
  }
  if (device < 0 || device >= ndev) { sco_set_error("sco_debug_lanes: bad device index"); return SCO_ERR_ARG; }
  SCO_ON_DEVICE(device);
  struct Buf { double *p = nullptr; ~Buf() { if (p) (void)hipFree(p); } } d;      // a_in | b_in | a_out | b_out
  const size_t vec = 64 * sizeof(double);
  SCO_HIP(hipMalloc((void **)&d.p, 4 * vec));
  SCO_HIP(hipMemset(d.p, 0, 4 * vec));
  SCO_HIP(hipMemcpy(d.p, a, vec, hipMemcpyHostToDevice));
  if (b) SCO_HIP(hipMemcpy(d.p + 64, b, vec, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lanes_probe_kernel, dim3(1), dim3(64), 0, 0, op, d.p, d.p + 64, d.p + 128, d.p + 192);
  SCO_HIP(hipGetLastError());
  SCO_HIP(hipDeviceSynchronize());
  SCO_HIP(hipMemcpy(out_a, d.p + 128, vec, hipMemcpyDeviceToHost));
  if (out_b) SCO_HIP(hipMemcpy(out_b, d.p + 192, vec, hipMemcpyDeviceToHost));
  return SCO_OK;
}
