// seg_head.hip — PV-RCNN's keypoint segmentation slice for gfx950 (include/gd3d.h, gd3d_seg_head_loss / gd3d_keypoint_reweight*):
//   * `PointwiseMaskHead.loss` (models/roi_heads/mask_heads/pointwise_mask_head.py:124-144: weights, normaliser, relabelling and
//     mmdet's sigmoid FocalLoss, reduction 'sum') — the loss AND its gradient — as ONE launch.  N is 10^3..10^4 keypoints with K = 1
//     or 3 logits: launch-bound, so the kernel is a SINGLE workgroup of up to 1024 threads that walks the rows in chunks of its
//     own size (as §3.10): the normaliser is a COUNT (LDS integer adds: exact in any order), the loss sum is an
//     fp64 partial per lane, folded by a butterfly of shuffles inside the wave and over the waves' partials in wave order by one
//     lane.  No float atomics, no second launch: the same inputs give the same bits.  Every gradient element is written (zeros on
//     the rows of weight 0).  Correct up to 2^24 rows, NOT meant to be fast beyond about 10^5 (one CU does all the work).
//   * the keypoint reweighting of `PVRCNNROIHead._bbox_forward` (models/roi_heads/pvrcnn_roi_head.py:211-212),
//     feats * max_k sigmoid(seg_preds[:, k]), forward and backward, one launch each: streaming kernels over many workgroups.  A
//     row is shared by a group of G = group_lanes(C) lanes, a lane takes every G-th quad of 4 columns — one 16-byte access when
//     C % 4 == 0 and the base pointers are 16-byte aligned (decided per launch), four 4-byte ones otherwise, the SAME columns per
//     lane either way.  The backward's row dot product is a sequential sum per lane and a butterfly of shuffles inside the group:
//     no LDS, no atomics, one order, the same bits on every run and on both access paths.
// Compiled with -ffp-contract=off: the per-element math (csrc/seg_head_common.h) is the operation sequence of csrc/seg_head_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "seg_head_common.h"

namespace seg_head {

struct LossArgs {
  const float* x;            // (N, K)
  const int64_t* target;     // (N)
  long long N;
  int K, num_classes, class_agnostic, gamma_is_2;
  float gamma, alpha, loss_weight;
  float* out;                // (2) loss, n_pos
  float* grad;               // (N, K) nullable
};

__global__ __launch_bounds__(WG) void seg_loss_kernel(const LossArgs a) {
  __shared__ int n_pos;
  __shared__ double part[WG / 64];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  if (tid == 0) n_pos = 0;
  __syncthreads();
  int cnt = 0;
  for (long long i = tid; i < a.N; i += T) cnt += row_kind(a.target[i], a.num_classes) == 1 ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0 && cnt != 0) atomicAdd(&n_pos, cnt);   // an integer sum: the same in any order
  __syncthreads();
  const int positives = n_pos;
  const float w = 1.0f / (positives > 1 ? (float)positives : 1.0f);   // (pos + neg) / clamp(pos.sum(), min=1): a division of exact counts
  double sum = 0.0;
  for (long long i = tid; i < a.N; i += T) {
    const int64_t c = a.target[i];
    const int kind = row_kind(c, a.num_classes);
    const int hot = hot_column(c, kind, a.class_agnostic);
    const float* x = a.x + i * a.K;
    float* g = a.grad != nullptr ? a.grad + i * a.K : nullptr;
    for (int k = 0; k < a.K; ++k) {
      float d = 0.0f;
      if (kind >= 0) {
        sum += (double)(w * focal_elem(x[k], k == hot, a.gamma, a.alpha, a.gamma_is_2 != 0, &d));
        d = a.loss_weight * (w * d);
      }
      if (g != nullptr) g[k] = d;
    }
  }
  // fixed order: a butterfly inside the wave (every lane ends with the same sum), then lane 0 over the waves' partials in wave order
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (tid < 2) {   // two lanes, one value each: vector stores
    double s = 0.0;
    for (int v = 0; v < waves; ++v) s += part[v];
    a.out[tid] = tid == 0 ? (float)((double)a.loss_weight * s) : (float)positives;
  }
}

static unsigned threads_for(long long rows) {
  const long long t = (rows + 63) / 64 * 64;
  return (unsigned)(t < 64 ? 64 : (t > WG ? WG : t));
}

// ---- the reweighting -----------------------------------------------------------------------------------------------------------

struct Quad {
  float v[QUAD];
};

// columns [c, c + 4) of a row, clipped to C: one 16-byte access on the vector path (C % 4 == 0 there, so a quad is never clipped)
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float* row, long long c, long long C) {
  Quad q;
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(row + c);
    q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < QUAD; ++j) q.v[j] = c + j < C ? row[c + j] : 0.0f;
  }
  return q;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* row, long long c, long long C, const Quad& q) {
  if (VEC) {
    *reinterpret_cast<float4*>(row + c) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < QUAD; ++j)
      if (c + j < C) row[c + j] = q.v[j];
  }
}

struct ReweightArgs {
  const float* feats;        // (N, C)
  const float* x;            // (N, K)
  long long N, C;
  int K, G;                  // G = group_lanes(C): lanes per row
  float* out;                // (N, C)
  uint8_t* win;              // (N) nullable
};

template <bool VEC>
__global__ __launch_bounds__(RW_BLOCK) void reweight_kernel(const ReweightArgs a) {
  const int sub = threadIdx.x & (a.G - 1), rows = RW_BLOCK / a.G;
  for (long long row0 = (long long)blockIdx.x * rows; row0 < a.N; row0 += (long long)gridDim.x * rows) {
    const long long i = row0 + threadIdx.x / a.G;
    if (i >= a.N) continue;            // no cross-lane operation in this kernel
    int w;
    const float s = row_max_sigmoid(a.x + i * a.K, a.K, &w);   // every lane of the group: the logits are one or two cache lines
    if (sub == 0 && a.win != nullptr) a.win[i] = (uint8_t)w;
    const float* f = a.feats + i * a.C;
    float* o = a.out + i * a.C;
    for (long long c = (long long)sub * QUAD; c < a.C; c += (long long)a.G * QUAD) {
      Quad q = load_quad<VEC>(f, c, a.C);
#pragma unroll
      for (int j = 0; j < QUAD; ++j) q.v[j] = q.v[j] * s;
      store_quad<VEC>(o, c, a.C, q);
    }
  }
}

struct ReweightBwdArgs {
  const float* g;            // (N, C) the upstream gradient
  const float* feats;        // (N, C)
  const float* x;            // (N, K)
  const uint8_t* win;        // (N)
  long long N, C;
  int K, G;
  float* g_feats;            // (N, C) nullable
  float* g_x;                // (N, K) nullable
};

template <bool VEC>
__global__ __launch_bounds__(RW_BLOCK) void reweight_backward_kernel(const ReweightBwdArgs a) {
  const int sub = threadIdx.x & (a.G - 1), rows = RW_BLOCK / a.G;
  // the trip count is the same for every thread of the workgroup: all 64 lanes of a wave reach the shuffles below
  for (long long row0 = (long long)blockIdx.x * rows; row0 < a.N; row0 += (long long)gridDim.x * rows) {
    const long long i = row0 + threadIdx.x / a.G;
    const bool valid = i < a.N;
    int w = 0;
    float s = 0.0f, dot = 0.0f;
    if (valid) {
      w = a.win[i];
      w = w < a.K ? w : a.K - 1;       // a winner array from elsewhere must not index past the row
      s = sigmoid(a.x[i * a.K + w]);
      const float* g = a.g + i * a.C;
      const float* f = a.feats + i * a.C;
      float* o = a.g_feats != nullptr ? a.g_feats + i * a.C : nullptr;
      for (long long c = (long long)sub * QUAD; c < a.C; c += (long long)a.G * QUAD) {
        const Quad qg = load_quad<VEC>(g, c, a.C);
        if (a.g_x != nullptr) {
          const Quad qf = load_quad<VEC>(f, c, a.C);
#pragma unroll
          for (int j = 0; j < QUAD; ++j) dot += qg.v[j] * qf.v[j];   // a clipped column adds 0 * 0
        }
        if (o != nullptr) {
          Quad q;
#pragma unroll
          for (int j = 0; j < QUAD; ++j) q.v[j] = qg.v[j] * s;
          store_quad<VEC>(o, c, a.C, q);
        }
      }
    }
    if (a.g_x == nullptr) continue;    // uniform over the launch
    for (int off = a.G >> 1; off > 0; off >>= 1) dot += __shfl_xor(dot, off);   // inside the group; every lane ends with the same sum
    if (!valid) continue;
    const float d = dot * (s * (1.0f - s));
    float* gx = a.g_x + i * a.K;
    for (int k = sub; k < a.K; k += a.G) gx[k] = k == w ? d : 0.0f;
  }
}

static unsigned reweight_grid(long long N, int G) {
  const long long rows = RW_BLOCK / G, blocks = (N + rows - 1) / rows;
  return (unsigned)(blocks < 8192 ? blocks : 8192);   // beyond that a workgroup strides over the rows
}

static bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

}  // namespace seg_head

using namespace seg_head;

extern "C" {

int gd3d_seg_head_loss(const float* seg_preds, const int64_t* seg_targets, int64_t N, int32_t K, int32_t num_classes,
                       int32_t class_agnostic, float gamma, float alpha, float loss_weight, float* out, float* grad, void* stream) {
  if (N < 0 || num_classes < 1 || K != (class_agnostic ? 1 : num_classes) || K > MAX_K || !(gamma >= 0.0f) ||
      !(alpha >= 0.0f && alpha <= 1.0f) || out == nullptr)
    return GD3D_E_BADARG;
  if (N > MAX_ROWS) return GD3D_E_TOOLARGE;
  if (N > 0 && (seg_preds == nullptr || seg_targets == nullptr)) return GD3D_E_BADARG;
  LossArgs a;
  a.x = seg_preds; a.target = seg_targets; a.N = N; a.K = K; a.num_classes = num_classes; a.class_agnostic = class_agnostic != 0;
  a.gamma_is_2 = gamma == 2.0f; a.gamma = gamma; a.alpha = alpha; a.loss_weight = loss_weight; a.out = out; a.grad = grad;
  hipLaunchKernelGGL(seg_loss_kernel, dim3(1), dim3(threads_for(N)), 0, (hipStream_t)stream, a);   // N == 0: the two zeros are written
  return (int)hipGetLastError();
}

int gd3d_keypoint_reweight(const float* feats, const float* seg_preds, int64_t N, int64_t C, int32_t K, float* out, uint8_t* win,
                           void* stream) {
  if (N < 0 || C < 1 || K < 1 || K > MAX_K) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (feats == nullptr || seg_preds == nullptr || out == nullptr) return GD3D_E_BADARG;
  ReweightArgs a;
  a.feats = feats; a.x = seg_preds; a.N = N; a.C = C; a.K = K; a.G = group_lanes(C); a.out = out; a.win = win;
  const bool vec = C % QUAD == 0 && aligned16(feats) && aligned16(out);
  const dim3 grid(reweight_grid(N, a.G)), block(RW_BLOCK);
  if (vec) hipLaunchKernelGGL(reweight_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(reweight_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_keypoint_reweight_backward(const float* grad_out, const float* feats, const float* seg_preds, const uint8_t* win, int64_t N,
                                    int64_t C, int32_t K, float* grad_feats, float* grad_seg, void* stream) {
  if (N < 0 || C < 1 || K < 1 || K > MAX_K) return GD3D_E_BADARG;
  if (N == 0 || (grad_feats == nullptr && grad_seg == nullptr)) return 0;
  if (grad_out == nullptr || seg_preds == nullptr || win == nullptr || (grad_seg != nullptr && feats == nullptr)) return GD3D_E_BADARG;
  ReweightBwdArgs a;
  a.g = grad_out; a.feats = feats; a.x = seg_preds; a.win = win; a.N = N; a.C = C; a.K = K; a.G = group_lanes(C);
  a.g_feats = grad_feats; a.g_x = grad_seg;
  const bool vec = C % QUAD == 0 && aligned16(grad_out) && aligned16(grad_seg != nullptr ? feats : nullptr) && aligned16(grad_feats);
  const dim3 grid(reweight_grid(N, a.G)), block(RW_BLOCK);
  if (vec) hipLaunchKernelGGL(reweight_backward_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(reweight_backward_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
