// roi_head_cpu.cpp — the `_cpu` twins of the RoI-head training slice (include/gd3d.h, gd3d_roi_head_*_cpu): plain loops over the
// per-row math of csrc/roi_head_common.h, the source csrc/roi_head.hip compiles for the device (both units with
// -ffp-contract=off).  The decisions — label, label_weights > 0, reg_mask — and the normalised weights are bit-identical to the
// kernels'; the values that pass through sin / cos / exp / log follow the host's libm.  The loss sums are fp64, taken in row
// order: the same bits on every run.  Host memory in and out, no stream, no HIP call, one thread (10^2..10^4 rows).
#define GD3D_HOST_TWIN 1
#include "roi_head_common.h"

#include "../../include/gd3d.h"

#include <vector>

using namespace roi_head;

extern "C" {

int gd3d_roi_head_targets_cpu(const float* pos_bboxes, const float* pos_gt_bboxes, const float* ious, const int32_t* pos_batch_cnt,
                              const int32_t* roi_batch_cnt, int32_t B, int64_t P, int64_t R, float cls_pos_thr, float cls_neg_thr,
                              int32_t clockwise, float* label, float* bbox_targets, int64_t* reg_mask, float* label_weights,
                              float* bbox_weights) {
  if (B < 0 || P < 0 || R < 0) return GD3D_E_BADARG;
  if (B > MAX_SAMPLES || P > MAX_ROWS || R > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (P == 0 && R == 0) return 0;
  if (B > 0 && (pos_batch_cnt == nullptr || roi_batch_cnt == nullptr)) return GD3D_E_BADARG;
  if (R > 0 && (ious == nullptr || label == nullptr || reg_mask == nullptr || label_weights == nullptr || bbox_weights == nullptr))
    return GD3D_E_BADARG;
  if (P > 0 && (pos_bboxes == nullptr || pos_gt_bboxes == nullptr || bbox_targets == nullptr)) return GD3D_E_BADARG;
  try {
    std::vector<int> rstart((size_t)B + 1, 0), pstart((size_t)B + 1, 0);
    int n_pos = 0;
    for (int b = 0; b < B; ++b) {
      const int rn = clamp_count(roi_batch_cnt[b], (int)R - rstart[b]), pn = clamp_count(pos_batch_cnt[b], (int)P - pstart[b]);
      n_pos += pn < rn ? pn : rn;
      rstart[b + 1] = rstart[b] + rn;
      pstart[b + 1] = pstart[b] + pn;
    }
    int n_label = 0;
    for (int i = 0; i < rstart[B]; ++i) n_label += label_of(ious[i], cls_pos_thr, cls_neg_thr) >= 0.0f ? 1 : 0;
    const float lden = n_label > 1 ? (float)n_label : 1.0f;
    const float bden = n_pos > 1 ? (float)n_pos : 1.0f;
    for (int i = 0; i < (int)R; ++i) {
      const int b = sample_of(rstart.data(), B, i);
      float lab = 0.0f, lw = 0.0f, bw = 0.0f;
      int64_t mask = 0;
      if (b < B) {
        lab = label_of(ious[i], cls_pos_thr, cls_neg_thr);
        lw = (lab >= 0.0f ? 1.0f : 0.0f) / lden;
        mask = (i - rstart[b]) < (pstart[b + 1] - pstart[b]) ? 1 : 0;
        bw = (mask ? 1.0f : 0.0f) / bden;
      }
      label[i] = lab;
      label_weights[i] = lw;
      reg_mask[i] = mask;
      bbox_weights[i] = bw;
    }
    for (int j = 0; j < (int)P; ++j) {
      float t[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (j < pstart[B]) target_row(pos_bboxes + (int64_t)j * 7, pos_gt_bboxes + (int64_t)j * 7, clockwise != 0, t);
      for (int k = 0; k < 7; ++k) bbox_targets[(int64_t)j * 7 + k] = t[k];
    }
  } catch (...) {
    return GD3D_E_HOST;
  }
  return 0;
}

int gd3d_roi_head_loss_cpu(const float* cls_score, const float* bbox_pred, const float* rois, int32_t roi_stride, int32_t first_col,
                           const float* labels, const float* bbox_targets, const float* pos_gt_bboxes, const int64_t* reg_mask,
                           const float* label_weights, const float* bbox_weights, int64_t R, int64_t P, float beta, float cls_weight,
                           float bbox_weight, int32_t with_corner_loss, int32_t clockwise, float* losses, float* grad_cls,
                           float* grad_bbox, float* grad_bbox_l1, float* grad_bbox_corner) {
  if (R < 0 || P < 0 || roi_stride < 7 || first_col < 0 || first_col + 7 > roi_stride || !(beta > 0.0f)) return GD3D_E_BADARG;
  if (P > MAX_ROWS || R > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (losses == nullptr) return GD3D_E_BADARG;
  if (R > 0 && (cls_score == nullptr || bbox_pred == nullptr || rois == nullptr || labels == nullptr || reg_mask == nullptr ||
                label_weights == nullptr || bbox_weights == nullptr))
    return GD3D_E_BADARG;
  if (P > 0 && (bbox_targets == nullptr || pos_gt_bboxes == nullptr)) return GD3D_E_BADARG;
  const int cw = clockwise != 0;
  int64_t n_pos = 0;
  for (int64_t i = 0; i < R; ++i) n_pos += reg_mask[i] > 0 ? 1 : 0;
  const int64_t pairs = n_pos < P ? n_pos : P;
  const float corner_scale = pairs > 0 ? 1.0f / (float)pairs : 0.0f;
  double s_cls = 0.0, s_l1 = 0.0, s_corner = 0.0;
  int64_t rank = 0;
  for (int64_t i = 0; i < R; ++i) {
    float gc;
    s_cls += (double)cls_row(cls_score[i], labels[i], label_weights[i], cls_weight, &gc);
    if (grad_cls != nullptr) grad_cls[i] = gc;
    float g1[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, g2[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (reg_mask[i] > 0) {
      if (rank < P) {
        const float* p = bbox_pred + i * 7;
        s_l1 += (double)smooth_l1_row(p, bbox_targets + rank * 7, bbox_weights[i], beta, bbox_weight, g1);
        if (with_corner_loss)
          s_corner += (double)corner_row(rois + i * roi_stride + first_col, p, pos_gt_bboxes + rank * 7, cw, corner_scale, g2);
      }
      ++rank;
    }
    for (int k = 0; k < 7; ++k) {
      if (grad_bbox_l1 != nullptr) grad_bbox_l1[i * 7 + k] = g1[k];
      if (grad_bbox_corner != nullptr) grad_bbox_corner[i * 7 + k] = g2[k];
      if (grad_bbox != nullptr) grad_bbox[i * 7 + k] = g1[k] + g2[k];
    }
  }
  losses[0] = (float)((double)cls_weight * s_cls);
  losses[1] = (float)((double)bbox_weight * s_l1);
  losses[2] = (float)(pairs > 0 ? s_corner / (double)pairs : 0.0);
  return 0;
}

}  // extern "C"
