// seg_head_common.h — what csrc/seg_head.hip (gfx950 kernels) and csrc/seg_head_cpu.cpp (their `_cpu` twins) share: the per-element
// math of PV-RCNN's keypoint segmentation slice as ONE sequence of fp32 operations each — the reweighting's sigmoid, the sigmoid focal loss of one
// logit with its derivative (PointwiseMaskHead.loss, models/roi_heads/mask_heads/pointwise_mask_head.py:124-144, on mmdet 2.x's
// published py_sigmoid_focal_loss), the row class of a segmentation target, the winning column of a row of logits and the lane
// layout and summation order of the reweighting's backward (models/roi_heads/pvrcnn_roi_head.py:211-212).  Both units are compiled
// with -ffp-contract=off.  The decisions (row class, n_pos, the winner on equal fp32 sigmoid values) are integer tests and
// comparisons of fp32 values; expf / log1pf / powf come from each target's own math library, so the VALUES agree to a few ulp.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD inline
#endif

namespace seg_head {

constexpr int WG = 1024;                    // threads of the loss kernel's one workgroup = rows of a chunk
constexpr long long MAX_ROWS = 1LL << 24;   // the loss: n_pos and the normaliser are exact in fp32 up to here
constexpr int MAX_K = 255;                  // the winner column is a byte
constexpr int RW_BLOCK = 256;               // threads of a reweight workgroup
constexpr int QUAD = 4;                     // columns a lane takes at a time (one 16-byte access on the vector path)

// 1 / (1 + exp(-x)): exactly 0 once exp(-x) overflows, exactly 1 once 1 + exp(-x) rounds to 1, finite everywhere
SH_HD float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

SH_HD float focal_pow(float b, float gamma, bool gamma_is_2) { return gamma_is_2 ? b * b : powf(b, gamma); }

// the sigmoid focal loss of one logit x against the one-hot value t, and *grad = d loss / d x:
//   t = 1:  -alpha (1-p)^gamma log p,        d/dx = alpha (1-p)^gamma (gamma p log p - (1-p))
//   t = 0:  -(1-alpha) p^gamma log(1-p),     d/dx = (1-alpha) p^gamma (p - gamma (1-p) log(1-p))
// All four of p, 1-p, log p = -softplus(-x) and log(1-p) = -softplus(x) come from ONE e = exp(-|x|) (the kernel is one workgroup: its
// time is the length of this chain): sigmoid(|x|) = 1 / (1 + e), sigmoid(-|x|) = e / (1 + e), softplus(+-x) = max(+-x, 0) + log1p(e).
// No overflow and no cancellation: finite at |x| = 100.
SH_HD float focal_elem(float x, bool t, float gamma, float alpha, bool gamma_is_2, float* grad) {
  const bool up = x >= 0.0f;
  const float e = expf(up ? -x : x);
  const float hi = 1.0f / (1.0f + e), lo = e / (1.0f + e);
  const float p = up ? hi : lo, q = up ? lo : hi;
  const float l1p = log1pf(e);
  if (t) {
    const float lp = -((up ? 0.0f : -x) + l1p);
    const float m = alpha * focal_pow(q, gamma, gamma_is_2);
    *grad = m * (gamma * p * lp - q);
    return -(m * lp);
  }
  const float lq = -((up ? x : 0.0f) + l1p);
  const float m = (1.0f - alpha) * focal_pow(p, gamma, gamma_is_2);
  *grad = m * (p - gamma * q * lq);
  return -(m * lq);
}

// the class of a row: 1 positive (0 <= c < num_classes), 0 background (c == num_classes), -1 weightless (ignored, or past background)
SH_HD int row_kind(int64_t c, int num_classes) { return c >= 0 && c < num_classes ? 1 : (c == num_classes ? 0 : -1); }

// the column whose one-hot value is 1 for a row of weight > 0, -1 for none: class agnostic, the label is `positive` (0 or 1) and
// the single column is column 0, so it is hit by the NON-positive rows (what the reference computes); else the class itself
SH_HD int hot_column(int64_t c, int kind, int class_agnostic) { return class_agnostic ? (kind == 1 ? -1 : 0) : (kind == 1 ? (int)c : -1); }

// max_k sigmoid(x[k]) over a row of K logits; on equal fp32 sigmoid values the lowest column wins
SH_HD float row_max_sigmoid(const float* x, int K, int* win) {
  float best = sigmoid(x[0]);
  int w = 0;
  for (int k = 1; k < K; ++k) {
    const float s = sigmoid(x[k]);
    if (s > best) {
      best = s;
      w = k;
    }
  }
  *win = w;
  return best;
}

// the lanes that share a row of C columns: the power of two that covers its quads, 64 at most (a lane then takes every G-th quad)
SH_HD int group_lanes(int64_t C) {
  const int64_t quads = (C + QUAD - 1) / QUAD;
  int g = 1;
  while (g < 64 && g < quads) g <<= 1;
  return g;
}

}  // namespace seg_head
