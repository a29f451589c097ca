// gd3d_anchor_head.hip — the anchor-head slice of the Gaussian-distance losses for gfx950: gather, decode, loss and
// gradient scatter of the positives in one kernel, and its C-ABI entry points (include/gd3d.h, gd3d_anchor_head_*).
#include "gd3d_loss_common.h"

namespace gd3d {

// Anchor-head slice with the gather fused in (gd_anchor3d_head.py:95-141): one thread per POSITIVE.
// It reads its 7 encoded predictions straight out of the NCHW head output (B, A*7, H, W) — no permute/reshape copy,
// no index kernels — its target / weight rows from the (M,7) arrays and its anchor from the per-sample anchor list,
// decodes both boxes (DeltaXYZWLHR), evaluates the loss and scatters the chained gradient back into the NCHW
// gradient (pre-zeroed by the caller).  P is O(1e2..1e4): latency-bound, so no LDS tiling.
struct HeadArgs {
  const float* bbox_pred;      // (B, A*7, H, W)
  const float* bbox_targets;   // (M,7), M = B*H*W*A, row m = ((b*H + h)*W + w)*A + a
  const float* bbox_weights;   // (M,7) nullable
  const float* anchors;        // (H*W*A, 7) anchors of one sample
  const long long* pos_inds;   // (P) positive rows, or NULL: dense mode, thread m tests labels[m] itself
  const long long* labels;     // dense mode: (M) class labels; positive iff 0 <= label < num_classes
  int num_classes;
  float* grad_bbox_pred;       // (B, A*7, H, W), zero-filled by the caller; nullable
  float* partials;
  long long P;
  int A, H, W;
  float dw[7];                 // train_cfg['decode_weight'] (all 1 when weights are given without it)
  float scale, alpha, ia2, tau, c0, c1, c2;
  // encoded-box SmoothL1 term of loss_single (gd_anchor3d_head.py:152-159), added to the same sum / gradient
  int dw_on;                   // GD term weighted by mean_k(bbox_weights * dw); else unweighted
  int sl1;                     // 0: off
  int sl1_cw;                  // element weight = bbox_weights * cw (train_cfg['code_weight']); else 1
  int sin_diff;                // diff_rad_by_sin: add_sin_difference on the yaw column
  float beta, sl1_scale;       // SmoothL1Loss.beta (0 = L1Loss), loss_weight / avg_factor
  float cw[7];
  // device-resident normaliser (ABI 4): when avg_dev != NULL the two scales are w_gd / *avg_dev and w_sl1 / *avg_dev, divided in
  // double and rounded once, as the host does with a host-side avg_factor
  const float* avg_dev;
  double w_gd, w_sl1;
};

template <int LOSS, int FUN, bool FLAG>
__global__ __launch_bounds__(HEAD_T) void head_anchor_kernel(const HeadArgs a) {
  __shared__ float swave[HEAD_T / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long i = (long long)blockIdx.x * HEAD_T + tid;
  bool valid = i < a.P;
  long long m = i;
  if (valid) {
    if (a.pos_inds != nullptr) {
      m = a.pos_inds[i];
    } else {  // dense mode: no nonzero()/compaction/host sync upstream; non-positives leave here
      const long long lab = a.labels[i];
      valid = lab >= 0 && lab < a.num_classes;
    }
  }
  float fl = 0.0f;
  if (valid) {
    const long long hwa = (long long)a.H * a.W * a.A;
    const long long b = m / hwa, r = m - b * hwa;
    const int an_i = (int)(r % a.A);
    const long long hw = r / a.A;                                  // h*W + w
    const long long plane = (long long)a.H * a.W;
    const float* pbase = a.bbox_pred + ((b * a.A + an_i) * 7) * plane + hw;   // + k*plane per channel
    float pe[7], te[7], an[7], pv[7], tv[7], wrow[7];
    float wi = 1.0f;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      pe[k] = pbase[k * plane];
      te[k] = a.bbox_targets[m * 7 + k];
      an[k] = a.anchors[r * 7 + k];
      wrow[k] = a.bbox_weights != nullptr ? a.bbox_weights[m * 7 + k] : 1.0f;
    }
    if (a.dw_on) {
      float sum = wrow[0] * a.dw[0];
#pragma unroll
      for (int k = 1; k < 7; ++k) sum += wrow[k] * a.dw[k];
      wi = sum / 7.0f;
    }
    DecodeJac Jp, Jt;
    decode_anchor(pe, an, pv, Jp);
    decode_anchor(te, an, tv, Jt);
    const float c[3] = {a.c0, a.c1, a.c2};
    float gd_scale = a.scale, sl1_scale = a.sl1_scale;
    if (a.avg_dev != nullptr) {
      const double avg = (double)*a.avg_dev;
      gd_scale = (float)(a.w_gd / avg);
      sl1_scale = (float)(a.w_sl1 / avg);
    }
    const float f = gd_scale * wi;
    float g1[7], g2[7];
    const float L = pair_loss<LOSS, FUN, FLAG, false>(pv, tv, c, a.alpha, a.ia2, a.tau, f, g1, g2);
    fl = f * L;
    float gs[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a.sl1) {  // uniform.  mmdet smooth_l1_loss on the ENCODED rows, weight (P,7), sum / avg_factor
      float d[7], j6 = 1.0f;
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = pe[k] - te[k];
      if (a.sin_diff) {  // add_sin_difference: sin(p)cos(t) vs cos(p)sin(t); both sides depend on the prediction
        float sp6, cp6, st6, ct6;
        sincos_f(pe[6], sp6, cp6);
        sincos_f(te[6], st6, ct6);
        d[6] = sp6 * ct6 - cp6 * st6;
        j6 = cp6 * ct6 + sp6 * st6;
      } else {
        d[6] = pe[6] - te[6];
      }
      float ls = 0.0f;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const float ad = fabsf(d[k]);
        const bool quad = ad < a.beta;
        const float l = quad ? 0.5f * ad * ad / a.beta : ad - 0.5f * a.beta;
        const float sg = d[k] > 0.0f ? 1.0f : (d[k] < 0.0f ? -1.0f : 0.0f);   // torch abs'(0) = 0
        const float g = quad ? d[k] / a.beta : sg;
        const float w = a.sl1_cw ? wrow[k] * a.cw[k] : 1.0f;
        ls += l * w;
        gs[k] = g * w * sl1_scale * (k == 6 ? j6 : 1.0f);
      }
      fl += sl1_scale * ls;
    }
    if (a.grad_bbox_pred != nullptr) {
      encode_grad(g1, Jp, true);
#pragma unroll
      for (int k = 0; k < 7; ++k) g1[k] += gs[k];
      float* gbase = a.grad_bbox_pred + ((b * a.A + an_i) * 7) * plane + hw;
#pragma unroll
      for (int k = 0; k < 7; ++k) gbase[k * plane] = g1[k];
    }
  }
  if (a.partials != nullptr) {
    const float ws = wave_sum(fl);
    if (lane == 0) swave[wave] = ws;
    __syncthreads();
    if (tid == 0) a.partials[blockIdx.x] = (swave[0] + swave[1]) + (swave[2] + swave[3]);
  }
}

}  // namespace gd3d

using namespace gd3d;

extern "C" {

static int anchor_head_impl(const gd3d_params* p, const gd3d_smooth_l1* sl1, const float* bbox_pred, int32_t B, int32_t A,
                            int32_t H, int32_t W, const float* bbox_targets, const float* bbox_weights,
                            const float* decode_weight,
                            const float* anchors, const int64_t* pos_inds, const int64_t* labels, int32_t num_classes,
                            int64_t P, float scale, float* loss_sum, float* grad_bbox_pred, void* workspace,
                            void* stream, const float* avg_dev = nullptr, double w_gd = 0.0, double w_sl1 = 0.0) {
  if (p == nullptr || P < 0 || B <= 0 || A <= 0 || H <= 0 || W <= 0) return GD3D_E_BADARG;
  if (check_instance(p->loss_type, p->fun) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) {
    if (loss_sum != nullptr) return fill_words(loss_sum, sizeof(float), 0u, s);
    return 0;
  }
  if (bbox_pred == nullptr || bbox_targets == nullptr || anchors == nullptr) return GD3D_E_BADARG;
  if (pos_inds == nullptr && labels == nullptr) return GD3D_E_BADARG;
  if (loss_sum != nullptr && workspace == nullptr) return GD3D_E_BADARG;
  HeadArgs a;
  a.bbox_pred = bbox_pred;
  a.bbox_targets = bbox_targets;
  a.bbox_weights = bbox_weights;
  a.anchors = anchors;
  a.pos_inds = (const long long*)pos_inds;
  a.labels = (const long long*)labels;
  a.num_classes = num_classes;
  a.grad_bbox_pred = grad_bbox_pred;
  a.partials = (float*)workspace;
  a.P = P;
  a.A = A;
  a.H = H;
  a.W = W;
  for (int k = 0; k < 7; ++k) a.dw[k] = decode_weight != nullptr ? decode_weight[k] : 1.0f;  // HOST array of 7
  a.dw_on = bbox_weights != nullptr && (decode_weight != nullptr || sl1 == nullptr);
  a.sl1 = 0;
  a.sl1_cw = a.sin_diff = 0;
  a.beta = a.sl1_scale = 0.0f;
  for (int k = 0; k < 7; ++k) a.cw[k] = 1.0f;
  if (sl1 != nullptr) {
    if (!(sl1->beta >= 0.0f)) return GD3D_E_BADARG;
    if (sl1->has_code_weight && bbox_weights == nullptr) return GD3D_E_BADARG;
    a.sl1 = 1;
    a.sl1_cw = sl1->has_code_weight != 0;
    a.sin_diff = sl1->diff_rad_by_sin != 0;
    a.beta = sl1->beta;
    a.sl1_scale = sl1->scale;
    for (int k = 0; k < 7; ++k) a.cw[k] = sl1->code_weight[k];
  }
  a.scale = scale;
  a.avg_dev = avg_dev;
  a.w_gd = w_gd;
  a.w_sl1 = w_sl1;
  a.alpha = p->alpha;
  a.ia2 = gd3d_inv_alpha2(p->alpha);
  a.tau = p->tau;
  a.c0 = p->center_offset[0];
  a.c1 = p->center_offset[1];
  a.c2 = p->center_offset[2];
  const long long nb = (P + HEAD_T - 1) / HEAD_T;
  if (nb > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  with_instance(p->loss_type, p->fun, p->flag != 0, [&](auto inst) {
    using I = decltype(inst);
    hipLaunchKernelGGL((head_anchor_kernel<I::loss, I::fun, I::flag>), dim3((unsigned)nb), dim3(HEAD_T), 0, s, a);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (loss_sum != nullptr) return reduce_partials((const float*)workspace, nb, loss_sum, s);
  return 0;
}

int gd3d_anchor_head_loss(const gd3d_params* p, const float* bbox_pred, int32_t B, int32_t A, int32_t H, int32_t W,
                          const float* bbox_targets, const float* bbox_weights, const float* decode_weight,
                          const float* anchors, const int64_t* pos_inds, int64_t P, float scale, float* loss_sum,
                          float* grad_bbox_pred, void* workspace, void* stream) {
  if (P > 0 && pos_inds == nullptr) return GD3D_E_BADARG;
  return anchor_head_impl(p, nullptr, bbox_pred, B, A, H, W, bbox_targets, bbox_weights, decode_weight, anchors, pos_inds,
                          nullptr, 0, P, scale, loss_sum, grad_bbox_pred, workspace, stream);
}

int gd3d_anchor_head_bbox_loss(const gd3d_params* p, const gd3d_smooth_l1* sl1, const float* bbox_pred, int32_t B,
                               int32_t A, int32_t H, int32_t W, const float* bbox_targets, const float* bbox_weights,
                               const float* decode_weight, const float* anchors, const int64_t* pos_inds, int64_t P,
                               const int64_t* labels, int32_t num_classes, float scale, float* loss_sum,
                               float* grad_bbox_pred, void* workspace, void* stream) {
  if (B <= 0 || A <= 0 || H <= 0 || W <= 0) return GD3D_E_BADARG;
  if ((pos_inds != nullptr) == (labels != nullptr)) return GD3D_E_BADARG;  // exactly one way to name the positives
  if (labels != nullptr) P = (int64_t)B * A * H * W;
  return anchor_head_impl(p, sl1, bbox_pred, B, A, H, W, bbox_targets, bbox_weights, decode_weight, anchors, pos_inds,
                          labels, num_classes, P, scale, loss_sum, grad_bbox_pred, workspace, stream);
}

int gd3d_anchor_head_bbox_loss_dyn(const gd3d_params* p, const gd3d_smooth_l1* sl1, const float* bbox_pred, int32_t B,
                                   int32_t A, int32_t H, int32_t W, const float* bbox_targets, const float* bbox_weights,
                                   const float* decode_weight, const float* anchors, const int64_t* labels,
                                   int32_t num_classes, double gd_weight, double sl1_weight, const float* avg_dev,
                                   float* loss_sum, float* grad_bbox_pred, void* workspace, void* stream) {
  if (B <= 0 || A <= 0 || H <= 0 || W <= 0 || labels == nullptr || avg_dev == nullptr) return GD3D_E_BADARG;
  return anchor_head_impl(p, sl1, bbox_pred, B, A, H, W, bbox_targets, bbox_weights, decode_weight, anchors, nullptr, labels,
                          num_classes, (int64_t)B * A * H * W, 0.0f, loss_sum, grad_bbox_pred, workspace, stream, avg_dev,
                          gd_weight, sl1_weight);
}

int gd3d_anchor_head_loss_dense(const gd3d_params* p, const float* bbox_pred, int32_t B, int32_t A, int32_t H, int32_t W,
                                const float* bbox_targets, const float* bbox_weights, const float* decode_weight,
                                const float* anchors, const int64_t* labels, int32_t num_classes, float scale,
                                float* loss_sum, float* grad_bbox_pred, void* workspace, void* stream) {
  if (B <= 0 || A <= 0 || H <= 0 || W <= 0 || labels == nullptr) return GD3D_E_BADARG;
  const int64_t M = (int64_t)B * A * H * W;
  return anchor_head_impl(p, nullptr, bbox_pred, B, A, H, W, bbox_targets, bbox_weights, decode_weight, anchors, nullptr,
                          labels, num_classes, M, scale, loss_sum, grad_bbox_pred, workspace, stream);
}

}  // extern "C"
