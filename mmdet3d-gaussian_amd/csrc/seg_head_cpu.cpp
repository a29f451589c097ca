// seg_head_cpu.cpp — the `_cpu` twins of PV-RCNN's keypoint segmentation slice (include/gd3d.h, gd3d_seg_head_loss_cpu and
// gd3d_keypoint_reweight*_cpu): plain loops over the per-element math of csrc/seg_head_common.h, the source csrc/seg_head.hip
// compiles for the device (both units with -ffp-contract=off).  n_pos and the winner columns are bit-identical to the kernels';
// the values that pass through expf / log1pf / powf follow the host's libm.  The loss sum is fp64, taken in row order; the
// backward's row dot product replays the kernel's lane layout and butterfly (group_lanes), so it is the kernel's sum bit for bit.
// Host memory in and out, no stream, no HIP call, one thread.
#define GD3D_HOST_TWIN 1
#include "seg_head_common.h"

#include "../../include/gd3d.h"

using namespace seg_head;

extern "C" {

int gd3d_seg_head_loss_cpu(const float* seg_preds, const int64_t* seg_targets, int64_t N, int32_t K, int32_t num_classes,
                           int32_t class_agnostic, float gamma, float alpha, float loss_weight, float* out, float* grad) {
  if (N < 0 || num_classes < 1 || K != (class_agnostic ? 1 : num_classes) || K > MAX_K || !(gamma >= 0.0f) ||
      !(alpha >= 0.0f && alpha <= 1.0f) || out == nullptr)
    return GD3D_E_BADARG;
  if (N > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (N > 0 && (seg_preds == nullptr || seg_targets == nullptr)) return GD3D_E_BADARG;
  const int agnostic = class_agnostic != 0;
  const bool gamma_is_2 = gamma == 2.0f;
  int positives = 0;
  for (int64_t i = 0; i < N; ++i) positives += row_kind(seg_targets[i], num_classes) == 1 ? 1 : 0;
  const float w = 1.0f / (positives > 1 ? (float)positives : 1.0f);
  double sum = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    const int64_t c = seg_targets[i];
    const int kind = row_kind(c, num_classes);
    const int hot = hot_column(c, kind, agnostic);
    for (int k = 0; k < K; ++k) {
      float d = 0.0f;
      if (kind >= 0) {
        sum += (double)(w * focal_elem(seg_preds[i * K + k], k == hot, gamma, alpha, gamma_is_2, &d));
        d = loss_weight * (w * d);
      }
      if (grad != nullptr) grad[i * K + k] = d;
    }
  }
  out[0] = (float)((double)loss_weight * sum);
  out[1] = (float)positives;
  return 0;
}

int gd3d_keypoint_reweight_cpu(const float* feats, const float* seg_preds, int64_t N, int64_t C, int32_t K, float* out, uint8_t* win) {
  if (N < 0 || C < 1 || K < 1 || K > MAX_K) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (feats == nullptr || seg_preds == nullptr || out == nullptr) return GD3D_E_BADARG;
  for (int64_t i = 0; i < N; ++i) {
    int w;
    const float s = row_max_sigmoid(seg_preds + i * K, K, &w);
    if (win != nullptr) win[i] = (uint8_t)w;
    for (int64_t c = 0; c < C; ++c) out[i * C + c] = feats[i * C + c] * s;
  }
  return 0;
}

int gd3d_keypoint_reweight_backward_cpu(const float* grad_out, const float* feats, const float* seg_preds, const uint8_t* win, int64_t N,
                                        int64_t C, int32_t K, float* grad_feats, float* grad_seg) {
  if (N < 0 || C < 1 || K < 1 || K > MAX_K) return GD3D_E_BADARG;
  if (N == 0 || (grad_feats == nullptr && grad_seg == nullptr)) return 0;
  if (grad_out == nullptr || seg_preds == nullptr || win == nullptr || (grad_seg != nullptr && feats == nullptr)) return GD3D_E_BADARG;
  const int G = group_lanes(C);
  for (int64_t i = 0; i < N; ++i) {
    int w = win[i];
    w = w < K ? w : K - 1;
    const float s = sigmoid(seg_preds[i * K + w]);
    const float* g = grad_out + i * C;
    if (grad_feats != nullptr)
      for (int64_t c = 0; c < C; ++c) grad_feats[i * C + c] = g[c] * s;
    if (grad_seg == nullptr) continue;
    const float* f = feats + i * C;
    float lane[64];
    for (int l = 0; l < G; ++l) {      // lane l of the group: every G-th quad, its columns in order
      float dot = 0.0f;
      for (int64_t c = (int64_t)l * QUAD; c < C; c += (int64_t)G * QUAD)
        for (int j = 0; j < QUAD && c + j < C; ++j) dot += g[c + j] * f[c + j];
      lane[l] = dot;
    }
    for (int off = G >> 1; off > 0; off >>= 1)   // the butterfly as lane 0 sees it
      for (int l = 0; l < off; ++l) lane[l] = lane[l] + lane[l + off];
    const float d = lane[0] * (s * (1.0f - s));
    for (int k = 0; k < K; ++k) grad_seg[i * K + k] = k == w ? d : 0.0f;
  }
  return 0;
}

}  // extern "C"
