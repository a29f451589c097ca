// eval_frames_common.h — what csrc/eval_frames.hip (gfx950 kernels) and csrc/eval_frames_cpu.cpp (the `_cpu` twin) share: the limits
// and the argument checks of eval_frames_records (include/gd3d.h "Flexible mAP, a batch of frames").
#pragma once
#include <stdint.h>

#include "../../include/gd3d.h"
#include "eval_ap_common.h"

namespace eval_frames {

constexpr int64_t MAX_GT = 2048;   // gts of one problem: the register-bit form of the matcher (one taken bit per 64-gt chunk and lane)
constexpr int64_t MAX_I32 = 0x7fffffffLL;

inline int check_frames(int32_t mode, const void* det, const void* score, const void* det_seg, int64_t ND, const void* gt, const void* gt_seg,
                        int64_t NG, const void* pair_off, int64_t pairs, int64_t max_gt, const void* det_flag, const void* gt_flag,
                        const void* group, const void* thrs, int32_t P, int32_t R, int32_t T, const void* o_group, const void* o_score,
                        const void* o_tp, const void* o_msk) {
  if (mode < 0 || mode > 2 || ND < 0 || NG < 0 || pairs < 0 || max_gt < 0 || P < 0 || R < 1 || T < 1 || T > eval_ap::MAX_T) return GD3D_E_BADARG;
  if (thrs == nullptr) return GD3D_E_BADARG;
  if (P > 0 && (det_seg == nullptr || gt_seg == nullptr || pair_off == nullptr || group == nullptr)) return GD3D_E_BADARG;
  if (P == 0 && (ND > 0 || NG > 0 || pairs > 0)) return GD3D_E_BADARG;
  if (ND > 0 && (det == nullptr || score == nullptr || det_flag == nullptr || o_group == nullptr || o_score == nullptr || o_tp == nullptr ||
                 o_msk == nullptr))
    return GD3D_E_BADARG;
  if (NG > 0 && (gt == nullptr || gt_flag == nullptr)) return GD3D_E_BADARG;
  if (pairs > 0 && (ND == 0 || NG == 0)) return GD3D_E_BADARG;
  if (max_gt > MAX_GT) return GD3D_E_TOOLARGE;
  if (pairs > MAX_I32 || NG > MAX_I32 || ND > MAX_I32 || (int64_t)R * ND > MAX_I32 || (int64_t)P * R > MAX_I32 ||
      (int64_t)P * R * T > MAX_I32)
    return GD3D_E_TOOLARGE;
  return 0;
}

}  // namespace eval_frames
