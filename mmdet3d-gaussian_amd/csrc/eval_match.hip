// eval_match.hip — the two remaining pieces of the reference's CPU evaluation helpers on gfx950:
//   * trans_bev   (ops/eval/affinity.cpp:83-105): BEV centre distance matrix, one thread per (det, gt);
//   * match_coco  (ops/eval/matcher.cpp:8-74):    COCO-style greedy matching per cost threshold.
// The matcher consumes the (D,G) affinity the IoU kernels of rbox.hip leave in HBM, so an evaluation pass moves only
// the (T,D) int32 result to the host.  Compiled with -ffp-contract=off (distances bit-equal to the CPU evaluation).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "eval_match_device.h"
#include "gd3d_fill.h"

namespace evalm {

__global__ __launch_bounds__(256) void trans_bev_kernel(const float* __restrict__ det, long long nd, int dcols,
                                                        const float* __restrict__ gt, long long ng, int gcols,
                                                        float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nd * ng) return;
  const long long di = idx / ng, gi = idx - di * ng;
  const float dx = det[di * dcols] - gt[gi * gcols], dy = det[di * dcols + 1] - gt[gi * gcols + 1];
  out[idx] = sqrtf(dx * dx + dy * dy);  // correctly rounded (hipcc default); __fsqrt_rn maps to the native approximation
}

// The matcher bodies (one wave, one threshold) live in eval_match_device.h, which eval_frames.hip shares.
template <bool REG, bool WIDE>
__global__ __launch_bounds__(64) void match_coco_kernel(const float* __restrict__ cost, const float* __restrict__ thrs,
                                                        const unsigned char* __restrict__ is_ignore,
                                                        const unsigned char* __restrict__ is_crowd, int nd, int ng,
                                                        int* __restrict__ matched) {
  extern __shared__ unsigned int taken[];  // ceil(ng / 32) words, this threshold's gt_matched row
  const int t = blockIdx.x;
  if (ng <= 0 || nd <= 0) return;  // host never launches these; the clamped loads of the body assume >= 1 row and column
  match_coco_wave<REG, WIDE>(cost, thrs[t], ByteFlags{is_ignore, is_crowd}, nd, ng, taken, matched + (size_t)t * nd);
}

template <int KBT>
__global__ __launch_bounds__(64) void match_coco_small_kernel(const float* __restrict__ cost,
                                                              const float* __restrict__ thrs,
                                                              const unsigned char* __restrict__ is_ignore,
                                                              const unsigned char* __restrict__ is_crowd, int nd, int ng,
                                                              int* __restrict__ matched) {
  const int t = blockIdx.x;
  if (ng <= 0 || nd <= 0) return;
  match_coco_small_wave<KBT>(cost, thrs[t], ByteFlags{is_ignore, is_crowd}, nd, ng, matched + (size_t)t * nd);
}

}  // namespace evalm

extern "C" {

int riou_eval_trans_bev(const float* det, int64_t nd, int32_t det_cols, const float* gt, int64_t ng, int32_t gt_cols,
                        float* dist, void* stream) {
  if (nd < 0 || ng < 0 || det_cols < 2 || gt_cols < 2) return GD3D_E_BADARG;
  if (nd == 0 || ng == 0) return 0;
  if (det == nullptr || gt == nullptr || dist == nullptr) return GD3D_E_BADARG;
  const long long total = (long long)nd * ng;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipLaunchKernelGGL(evalm::trans_bev_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, det, (long long)nd,
                     det_cols, gt, (long long)ng, gt_cols, dist);
  return (int)hipGetLastError();
}

int eval_match_coco(const float* cost, const float* cost_thrs, const uint8_t* is_ignore, const uint8_t* is_crowd,
                    int64_t nd, int64_t ng, int64_t nt, int32_t* matched, void* stream) {
  if (nd < 0 || ng < 0 || nt < 0) return GD3D_E_BADARG;
  if (nt == 0 || nd == 0) return 0;
  if (matched == nullptr || cost_thrs == nullptr) return GD3D_E_BADARG;
  if (ng == 0)  // no ground truth: every detection is unmatched (-1 = all-ones bytes); the kernels index gt ng - 1
    return gd3d::fill_words(matched, sizeof(int32_t) * (size_t)nt * (size_t)nd, 0xffffffffu, (hipStream_t)stream);
  if (cost == nullptr || is_ignore == nullptr || is_crowd == nullptr) return GD3D_E_BADARG;
  if (nd > 0x7fffffffLL || nt > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (ng > 1048576) return GD3D_E_TOOLARGE;  // taken bitmask: 128 KiB of the 160 KiB LDS
  const size_t lds = (size_t)((ng + 31) / 32 + 1) * sizeof(unsigned int);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)evalm::match_coco_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (ng <= 64)
    hipLaunchKernelGGL((evalm::match_coco_small_kernel<1>), dim3((unsigned)nt), dim3(64), 0, (hipStream_t)stream, cost,
                       cost_thrs, is_ignore, is_crowd, (int)nd, (int)ng, (int*)matched);
  else if (ng <= 256)
    hipLaunchKernelGGL((evalm::match_coco_small_kernel<4>), dim3((unsigned)nt), dim3(64), 0, (hipStream_t)stream, cost,
                       cost_thrs, is_ignore, is_crowd, (int)nd, (int)ng, (int*)matched);
  else if (ng <= 2048)
    hipLaunchKernelGGL((evalm::match_coco_kernel<true, true>), dim3((unsigned)nt), dim3(64), 16, (hipStream_t)stream, cost,
                       cost_thrs, is_ignore, is_crowd, (int)nd, (int)ng, (int*)matched);
  else
    hipLaunchKernelGGL((evalm::match_coco_kernel<false, true>), dim3((unsigned)nt), dim3(64), lds, (hipStream_t)stream, cost,
                       cost_thrs, is_ignore, is_crowd, (int)nd, (int)ng, (int*)matched);
  return (int)hipGetLastError();
}

}  // extern "C"
