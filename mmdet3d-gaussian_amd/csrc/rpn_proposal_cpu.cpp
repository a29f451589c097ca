// rpn_proposal_cpu.cpp — the `_cpu` twin of csrc/rpn_proposal.hip (include/gd3d.h, gd3d_rpn_proposals_cpu): plain loops over the
// values and decisions of csrc/rpn_proposal_common.h, the source the kernels compile for the device (both units with
// -ffp-contract=off; exp is a fixed polynomial sequence), a stable sort where the device selects by radix and orders by counting,
// and the library's CPU NMS (csrc/rbox_cpu.cpp) for the NMS step.  Every output is BIT-IDENTICAL to the kernels'.  Host memory in
// and out, no stream, no HIP call, one thread.  Also the one text of the argument checks (check_args).
#define GD3D_HOST_TWIN 1
#include "rpn_proposal_common.h"

#include "../../include/gd3d.h"

#include <algorithm>
#include <vector>

namespace rpn_proposal {

int check_args(int32_t B, int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num, float nms_thr,
               float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset, Params& p) {
  if (B < 1 || A < 1 || C < 1 || H < 1 || W < 1 || nms_post < 1 || max_num < 1) return GD3D_E_BADARG;
  if (nms_thr != nms_thr || score_thr != score_thr || dir_offset != dir_offset || dir_limit_offset != dir_limit_offset) return GD3D_E_BADARG;
  if (C > MAX_CLASSES || B > MAX_SAMPLES) return GD3D_E_TOOLARGE;
  const int64_t HW = (int64_t)H * W, N = HW * A;
  if (N >= (1LL << 30)) return GD3D_E_TOOLARGE;
  const int64_t cap = (nms_pre > 0 && nms_pre < N) ? nms_pre : N;
  if (cap > MAX_CAND) return GD3D_E_TOOLARGE;
  p.B = B; p.A = A; p.C = C; p.H = H; p.W = W;
  p.HW = (int)HW;
  p.N = (int)N;
  p.cap = (int)cap;
  p.M = nms_post < max_num ? nms_post : max_num;
  p.rotate = use_rotate_nms != 0;
  p.nms_thr = nms_thr;
  p.score_thr = score_thr;
  p.dir_offset = dir_offset;
  p.dir_limit_offset = dir_limit_offset;
  return 0;
}

}  // namespace rpn_proposal

using namespace rpn_proposal;

extern "C" {

int gd3d_rpn_proposals_cpu(const float* cls_score, const float* bbox_pred, const float* dir_cls_pred, const float* anchors, int32_t B,
                           int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num,
                           float nms_thr, float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset,
                           float* boxes_3d, float* scores_3d, int64_t* labels_3d, float* cls_preds, float* rois, int32_t* batch_cnt,
                           int64_t* cand_inds, int32_t* cand_cnt, void* workspace, size_t workspace_bytes) {
  Params p;
  const int rc = check_args(B, A, C, H, W, nms_pre, nms_post, max_num, nms_thr, score_thr, use_rotate_nms, dir_offset, dir_limit_offset, p);
  if (rc != 0) return rc;
  (void)workspace;
  (void)workspace_bytes;
  if (cls_score == nullptr || bbox_pred == nullptr || dir_cls_pred == nullptr || anchors == nullptr || boxes_3d == nullptr ||
      scores_3d == nullptr || labels_3d == nullptr || cls_preds == nullptr || rois == nullptr || batch_cnt == nullptr)
    return GD3D_E_BADARG;
  try {
    const size_t HW = (size_t)p.HW;
    const int N = p.N, cap = p.cap, M = p.M;
    std::vector<unsigned> key((size_t)N);
    std::vector<int> idx, label((size_t)cap), dir((size_t)cap);
    std::vector<float> box7((size_t)cap * 7), bev5((size_t)cap * 5), score((size_t)cap);
    std::vector<int64_t> keep((size_t)cap);
    size_t row = 0;
    for (int b = 0; b < B; ++b) {
      const float* cls = cls_score + (size_t)b * A * C * HW;
      const float* bp = bbox_pred + (size_t)b * A * 7 * HW;
      const float* dp = dir_cls_pred + (size_t)b * A * 2 * HW;
      idx.clear();
      for (int n = 0; n < N; ++n) {
        const size_t cell = (size_t)(n / A), a = (size_t)(n % A);
        float best;
        int l;
        const bool ok = anchor_best(cls + a * C * HW + cell, HW, C, best, l);
        key[(size_t)n] = ok ? key_of(best) : 0u;
        if (ok) idx.push_back(n);
      }
      std::stable_sort(idx.begin(), idx.end(), [&](int i, int j) { return key[(size_t)i] > key[(size_t)j]; });
      const int n_sel = (int)std::min<size_t>(idx.size(), (size_t)cap);
      int cnt = 0;
      for (int s = 0; s < n_sel; ++s) {
        const int n = idx[(size_t)s];
        const size_t cell = (size_t)(n / A), a = (size_t)(n % A);
        float best, t[7];
        anchor_best(cls + a * C * HW + cell, HW, C, best, label[(size_t)s]);
        score[(size_t)s] = sigmoid(best);
        dir[(size_t)s] = dp[(a * 2 + 1) * HW + cell] > dp[(a * 2) * HW + cell] ? 1 : 0;
        for (int j = 0; j < 7; ++j) t[j] = bp[(a * 7 + (size_t)j) * HW + cell];
        decode(anchors + (size_t)n * 7, t, &box7[(size_t)s * 7], &bev5[(size_t)s * 5]);
        cnt += score[(size_t)s] > p.score_thr ? 1 : 0;
      }
      if (cand_inds != nullptr)
        for (int s = 0; s < cap; ++s) cand_inds[(size_t)b * cap + s] = s < n_sel ? idx[(size_t)s] : -1;
      if (cand_cnt != nullptr) cand_cnt[b] = cnt;
      int64_t nk = 0;
      const int nrc = p.rotate ? rnms_bev_cpu(bev5.data(), cnt, p.nms_thr, keep.data(), &nk)
                               : rnms_normal_bev_cpu(bev5.data(), cnt, p.nms_thr, keep.data(), &nk);
      if (nrc != 0) return nrc;
      const int m = rows_of(nk, M);
      batch_cnt[b] = m;
      for (int r = 0; r < m; ++r, ++row) {
        const size_t s = (size_t)keep[(size_t)r];
        const int n = idx[s];
        const size_t cell = (size_t)(n / A), a = (size_t)(n % A);
        float* o = boxes_3d + row * 7;
        for (int j = 0; j < 6; ++j) o[j] = box7[s * 7 + j];
        o[6] = dir_fix(box7[s * 7 + 6], dir[s], p.dir_offset, p.dir_limit_offset);
        scores_3d[row] = score[s];
        labels_3d[row] = label[s];
        for (int c = 0; c < C; ++c) cls_preds[row * C + c] = sigmoid(cls[(a * C + (size_t)c) * HW + cell]);
        rois[row * 8] = (float)b;
        for (int j = 0; j < 7; ++j) rois[row * 8 + 1 + j] = o[j];
      }
    }
    for (; row < (size_t)B * M; ++row) {
      for (int j = 0; j < 7; ++j) boxes_3d[row * 7 + j] = 0.0f;
      scores_3d[row] = 0.0f;
      labels_3d[row] = -1;
      for (int c = 0; c < C; ++c) cls_preds[row * C + c] = 0.0f;
      rois[row * 8] = -1.0f;
      for (int j = 0; j < 7; ++j) rois[row * 8 + 1 + j] = 0.0f;
    }
  } catch (...) {
    return GD3D_E_HOST;
  }
  return 0;
}

}  // extern "C"
