// roi_head.hip — the training slice of PVRCNNBboxHead for gfx950 (include/gd3d.h, gd3d_roi_head_*): `get_targets` with
// `_get_target_single` (models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:213-316, the concat=True form) as ONE launch, and `loss`
// with `get_corner_loss_lidar` (:140-211, :318-351) — the three losses AND their gradients — as one more.  The reference spends
// hundreds of small torch launches and three host syncs on 10^2..10^4 rows; at that size the work is launch-bound, so both
// kernels are a SINGLE workgroup of up to 1024 threads that walks the rows in chunks of its own size:
//   * no second launch and no atomics on floats: the normalisers of the targets are COUNTS (LDS integer adds: exact in any
//     order), and the loss sums are fp64 partials per lane, folded across the wave by a butterfly of shuffles and across the
//     waves by three lanes, one per loss, each in wave order — the same bits on every run;
//   * the j-th positive row pairs with bbox_targets[j]: its rank comes from a ballot / popcount inside the wave, the waves'
//     totals through LDS, and a running offset from chunk to chunk — no nonzero(), no host read;
//   * every output element is written (zero gradients for the rows that are not positive; zero targets past the counts).
// Compiled with -ffp-contract=off: the per-row math (csrc/roi_head_common.h) is the operation sequence of csrc/roi_head_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "roi_head_common.h"

namespace roi_head {

struct TargetArgs {
  const float* roi;          // (P, 7) the positives' RoIs
  const float* gt;           // (P, 7) their gt boxes
  const float* iou;          // (R)
  const int32_t* pos_cnt;    // (B)
  const int32_t* roi_cnt;    // (B)
  int B, P, R;
  float pos_thr, neg_thr;
  int clockwise;
  float* label;              // (R)
  float* target;             // (P, 7)
  int64_t* reg_mask;         // (R)
  float* label_weights;      // (R)
  float* bbox_weights;       // (R)
};

__global__ __launch_bounds__(WG) void targets_kernel(const TargetArgs a) {
  __shared__ int rstart[MAX_SAMPLES + 1], pstart[MAX_SAMPLES + 1];
  __shared__ int n_label, n_pos;
  const int tid = threadIdx.x, T = blockDim.x;
  if (tid == 0) {   // the samples' clamped segments: B is small, the counts sit in one or two cache lines
    int rs = 0, ps = 0, np = 0;
    rstart[0] = 0;
    pstart[0] = 0;
    for (int b = 0; b < a.B; ++b) {
      const int rn = clamp_count(a.roi_cnt[b], a.R - rs), pn = clamp_count(a.pos_cnt[b], a.P - ps);
      np += pn < rn ? pn : rn;
      rs += rn;
      ps += pn;
      rstart[b + 1] = rs;
      pstart[b + 1] = ps;
    }
    n_pos = np;
    n_label = 0;
  }
  __syncthreads();
  const int covered = rstart[a.B];
  int cnt = 0;
  for (int i = tid; i < covered; i += T) cnt += label_of(a.iou[i], a.pos_thr, a.neg_thr) >= 0.0f ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((tid & 63) == 0 && cnt != 0) atomicAdd(&n_label, cnt);   // an integer sum: the same in any order
  __syncthreads();
  const float lden = n_label > 1 ? (float)n_label : 1.0f;      // torch.clamp(weights.sum(), min=1.0): sums of ones, exact
  const float bden = n_pos > 1 ? (float)n_pos : 1.0f;
  for (int i = tid; i < a.R; i += T) {
    const int b = sample_of(rstart, a.B, i);
    float label = 0.0f, lw = 0.0f, bw = 0.0f;
    int64_t mask = 0;
    if (b < a.B) {   // a row past the counts' sum belongs to no sample: weightless
      label = label_of(a.iou[i], a.pos_thr, a.neg_thr);
      lw = (label >= 0.0f ? 1.0f : 0.0f) / lden;
      mask = (i - rstart[b]) < (pstart[b + 1] - pstart[b]) ? 1 : 0;
      bw = (mask ? 1.0f : 0.0f) / bden;
    }
    a.label[i] = label;
    a.label_weights[i] = lw;
    a.reg_mask[i] = mask;
    a.bbox_weights[i] = bw;
  }
  const int paired = pstart[a.B];
  for (int j = tid; j < a.P; j += T) {
    float t[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (j < paired) target_row(a.roi + (long long)j * 7, a.gt + (long long)j * 7, a.clockwise, t);
    float* o = a.target + (long long)j * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = t[k];
  }
}

struct LossArgs {
  const float* cls;          // (R)
  const float* pred;         // (R, 7)
  const float* rois;         // R rows of `stride` floats, the box at column `first`
  int stride, first;
  const float* label;        // (R)
  const float* target;       // (P, 7)
  const float* gt;           // (P, 7)
  const int64_t* reg_mask;   // (R)
  const float* label_weights;
  const float* bbox_weights;
  int R, P;
  float beta, w_cls, w_bbox;
  int corner, clockwise;
  float* out;                // (3) loss_cls, loss_bbox, loss_corner
  float* g_cls;              // (R) nullable
  float* g_box;              // (R, 7) nullable: d(loss_bbox + loss_corner) / d bbox_pred
  float* g_l1;               // (R, 7) nullable: d loss_bbox / d bbox_pred
  float* g_corner;           // (R, 7) nullable: d loss_corner / d bbox_pred
};

__device__ __forceinline__ void store7(float* base, long long row, const float* v) {
  if (base == nullptr) return;
  float* o = base + row * 7;
#pragma unroll
  for (int k = 0; k < 7; ++k) o[k] = v[k];
}

__global__ __launch_bounds__(WG) void loss_kernel(const LossArgs a) {
  __shared__ int wave_cnt[WG / 64];
  __shared__ int n_pos;
  __shared__ double part[3][WG / 64];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  if (tid == 0) n_pos = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < a.R; i += T) cnt += a.reg_mask[i] > 0 ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0 && cnt != 0) atomicAdd(&n_pos, cnt);
  __syncthreads();
  const int pairs = n_pos < a.P ? n_pos : a.P;   // rows that have a target: the mean of the corner loss runs over these
  const float corner_scale = pairs > 0 ? 1.0f / (float)pairs : 0.0f;
  double s_cls = 0.0, s_l1 = 0.0, s_corner = 0.0;
  int run = 0;                                    // positives before this chunk
  for (int base = 0; base < a.R; base += T) {     // block-uniform trip count: the barriers below are reached by every thread
    const int i = base + tid;
    const bool valid = i < a.R;
    const bool pos = valid && a.reg_mask[i] > 0;
    const unsigned long long m = __ballot(pos);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < waves; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    __syncthreads();                              // wave_cnt is rewritten by the next chunk
    const int rank = run + before + __popcll(m & ((1ull << lane) - 1ull));
    run += total;
    if (!valid) continue;
    float gc;
    s_cls += (double)cls_row(a.cls[i], a.label[i], a.label_weights[i], a.w_cls, &gc);
    if (a.g_cls != nullptr) a.g_cls[i] = gc;
    float g1[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, g2[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (pos && rank < a.P) {
      float p[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) p[k] = a.pred[(long long)i * 7 + k];
      s_l1 += (double)smooth_l1_row(p, a.target + (long long)rank * 7, a.bbox_weights[i], a.beta, a.w_bbox, g1);
      if (a.corner)
        s_corner += (double)corner_row(a.rois + (long long)i * a.stride + a.first, p, a.gt + (long long)rank * 7, a.clockwise,
                                       corner_scale, g2);
    }
    store7(a.g_l1, i, g1);
    store7(a.g_corner, i, g2);
    if (a.g_box != nullptr) {
      float gs[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) gs[k] = g1[k] + g2[k];
      store7(a.g_box, i, gs);
    }
  }
  // fixed order: a butterfly inside the wave (every lane ends with the same sum), then one lane per loss (tid 0..2) over the waves' partials in wave order
  for (int off = 32; off > 0; off >>= 1) {
    s_cls += __shfl_xor(s_cls, off);
    s_l1 += __shfl_xor(s_l1, off);
    s_corner += __shfl_xor(s_corner, off);
  }
  if (lane == 0) {
    part[0][wave] = s_cls;
    part[1][wave] = s_l1;
    part[2][wave] = s_corner;
  }
  __syncthreads();
  if (tid < 3) {   // three lanes, one loss each: vector stores
    double s = 0.0;
    for (int w = 0; w < waves; ++w) s += part[tid][w];
    const double v = tid == 0 ? (double)a.w_cls * s : (tid == 1 ? (double)a.w_bbox * s : (pairs > 0 ? s / (double)pairs : 0.0));
    a.out[tid] = (float)v;
  }
}

static unsigned threads_for(long long rows) {
  const long long t = (rows + 63) / 64 * 64;
  return (unsigned)(t < 64 ? 64 : (t > WG ? WG : t));
}

}  // namespace roi_head

using namespace roi_head;

extern "C" {

int gd3d_roi_head_targets(const float* pos_bboxes, const float* pos_gt_bboxes, const float* ious, const int32_t* pos_batch_cnt,
                          const int32_t* roi_batch_cnt, int32_t B, int64_t P, int64_t R, float cls_pos_thr, float cls_neg_thr,
                          int32_t clockwise, float* label, float* bbox_targets, int64_t* reg_mask, float* label_weights,
                          float* bbox_weights, void* stream) {
  if (B < 0 || P < 0 || R < 0) return GD3D_E_BADARG;
  if (B > MAX_SAMPLES || P > MAX_ROWS || R > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (P == 0 && R == 0) return 0;
  if (B > 0 && (pos_batch_cnt == nullptr || roi_batch_cnt == nullptr)) return GD3D_E_BADARG;
  if (R > 0 && (ious == nullptr || label == nullptr || reg_mask == nullptr || label_weights == nullptr || bbox_weights == nullptr))
    return GD3D_E_BADARG;
  if (P > 0 && (pos_bboxes == nullptr || pos_gt_bboxes == nullptr || bbox_targets == nullptr)) return GD3D_E_BADARG;
  TargetArgs a;
  a.roi = pos_bboxes; a.gt = pos_gt_bboxes; a.iou = ious; a.pos_cnt = pos_batch_cnt; a.roi_cnt = roi_batch_cnt;
  a.B = B; a.P = (int)P; a.R = (int)R; a.pos_thr = cls_pos_thr; a.neg_thr = cls_neg_thr; a.clockwise = clockwise != 0;
  a.label = label; a.target = bbox_targets; a.reg_mask = reg_mask; a.label_weights = label_weights; a.bbox_weights = bbox_weights;
  hipLaunchKernelGGL(targets_kernel, dim3(1), dim3(threads_for(R > P ? R : P)), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_roi_head_loss(const float* cls_score, const float* bbox_pred, const float* rois, int32_t roi_stride, int32_t first_col,
                       const float* labels, const float* bbox_targets, const float* pos_gt_bboxes, const int64_t* reg_mask,
                       const float* label_weights, const float* bbox_weights, int64_t R, int64_t P, float beta, float cls_weight,
                       float bbox_weight, int32_t with_corner_loss, int32_t clockwise, float* losses, float* grad_cls,
                       float* grad_bbox, float* grad_bbox_l1, float* grad_bbox_corner, void* stream) {
  if (R < 0 || P < 0 || roi_stride < 7 || first_col < 0 || first_col + 7 > roi_stride || !(beta > 0.0f)) return GD3D_E_BADARG;
  if (P > MAX_ROWS || R > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (losses == nullptr) return GD3D_E_BADARG;
  if (R > 0 && (cls_score == nullptr || bbox_pred == nullptr || rois == nullptr || labels == nullptr || reg_mask == nullptr ||
                label_weights == nullptr || bbox_weights == nullptr))
    return GD3D_E_BADARG;
  if (P > 0 && (bbox_targets == nullptr || pos_gt_bboxes == nullptr)) return GD3D_E_BADARG;
  LossArgs a;
  a.cls = cls_score; a.pred = bbox_pred; a.rois = rois; a.stride = roi_stride; a.first = first_col; a.label = labels;
  a.target = bbox_targets; a.gt = pos_gt_bboxes; a.reg_mask = reg_mask; a.label_weights = label_weights; a.bbox_weights = bbox_weights;
  a.R = (int)R; a.P = (int)P; a.beta = beta; a.w_cls = cls_weight; a.w_bbox = bbox_weight; a.corner = with_corner_loss != 0;
  a.clockwise = clockwise != 0; a.out = losses; a.g_cls = grad_cls; a.g_box = grad_bbox; a.g_l1 = grad_bbox_l1;
  a.g_corner = grad_bbox_corner;
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(threads_for(R)), 0, (hipStream_t)stream, a);   // R == 0: the three zeros are written
  return (int)hipGetLastError();
}

}  // extern "C"
