// simota_cpu.cpp — the `_cpu` twin of csrc/simota.hip (include/gd3d.h, gd3d_simota_assign_cpu): plain loops over the decisions of
// csrc/simota_common.h, the source the kernels compile for the device (both units with -ffp-contract=off; sin / cos / atan2 / log
// are fixed polynomial sequences).  Every output is BIT-IDENTICAL to the kernels'.  Host memory in and out, no stream, no HIP call,
// one thread.  Also the one text of the argument checks (check_args) and of the workspace size.
#define GD3D_HOST_TWIN 1
#include "simota_common.h"

#include "../../include/gd3d.h"

#include <algorithm>
#include <functional>
#include <vector>

namespace simota {

int check_args(int64_t P, int64_t prior_rows, int64_t prior_stride, int32_t shared_priors, int64_t G, int32_t B, int32_t C, int32_t G_cap,
               float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight, float match_init, Params& p) {
  if (P < 0 || prior_rows < 0 || G < 0 || B < 1 || C < 1 || G_cap < 0 || candidate_topk < 1 || prior_stride < 2) return GD3D_E_BADARG;
  if (shared_priors != 0 && shared_priors != 1) return GD3D_E_BADARG;
  if (!shared_priors && prior_rows != P) return GD3D_E_BADARG;
  if (center_radius != center_radius || iou_weight != iou_weight || cls_weight != cls_weight || match_init != match_init) return GD3D_E_BADARG;
  if (P > MAX_ROWS || prior_rows > MAX_ROWS || G > MAX_ROWS || B > MAX_SAMPLES || C > MAX_CLASSES || G_cap > MAX_GTS ||
      candidate_topk > MAX_TOPK || prior_stride > (1 << 20) || (int64_t)G_cap * candidate_topk > MAX_MATCHES)
    return GD3D_E_TOOLARGE;
  p.C = C;
  p.K = candidate_topk;
  p.radius = center_radius;
  p.iou_w = iou_weight;
  p.cls_w = cls_weight;
  p.match_init = match_init;
  return 0;
}

}  // namespace simota

using namespace simota;

extern "C" {

size_t gd3d_simota_workspace_bytes(int64_t P, int32_t B, int32_t G_cap, int32_t candidate_topk) {
  if (P < 0 || B < 0 || G_cap < 0 || candidate_topk < 0) return 0;
  Args a;
  return carve(a, nullptr, P, B, G_cap, candidate_topk);
}

int gd3d_simota_assign_cpu(const float* pred_scores, const float* decoded_bboxes, const float* priors, int64_t prior_rows,
                           int64_t prior_stride, int32_t shared_priors, const int32_t* prior_batch_cnt, int64_t P,
                           const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B,
                           int32_t C, int32_t G_cap, float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight,
                           float match_init, int64_t* gt_inds, int64_t* labels, float* max_overlaps, int32_t* pos_cnt,
                           int64_t* pos_inds, int64_t* pos_gt_inds, void* workspace, size_t workspace_bytes) {
  Params prm;
  const int rc = check_args(P, prior_rows, prior_stride, shared_priors, G, B, C, G_cap, center_radius, candidate_topk, iou_weight,
                            cls_weight, match_init, prm);
  if (rc != 0) return rc;
  (void)workspace;
  (void)workspace_bytes;
  if (prior_batch_cnt == nullptr || gt_batch_cnt == nullptr || pos_cnt == nullptr) return GD3D_E_BADARG;
  if (P > 0 && (pred_scores == nullptr || decoded_bboxes == nullptr || gt_inds == nullptr || labels == nullptr || max_overlaps == nullptr))
    return GD3D_E_BADARG;
  if (prior_rows > 0 && priors == nullptr) return GD3D_E_BADARG;
  if (G > 0 && (gt_bboxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  const int64_t L = (int64_t)G_cap * candidate_topk;
  if (L > 0 && (pos_inds == nullptr || pos_gt_inds == nullptr)) return GD3D_E_BADARG;
  try {
    for (int64_t i = 0; i < P; ++i) {
      gt_inds[i] = 0;
      labels[i] = -1;
      max_overlaps[i] = -1e8f;
    }
    for (int64_t i = 0; i < (int64_t)B * L; ++i) pos_inds[i] = pos_gt_inds[i] = -1;
    VertexScratch<1> vs;
    std::vector<GtC> gc;
    std::vector<OBox> gbox, pbox;
    std::vector<Lite> glite, plite;
    std::vector<int> cand;
    std::vector<float> iou;
    std::vector<unsigned long long> ent, ient;
    std::vector<std::pair<int, int>> match;   // (prior, slot)
    std::vector<float> match_iou;
    auto pair_iou = [&](const float* pr, const OBox& A, const Lite& pa, const float* gr, const OBox& Bx, const Lite& gb) {
      return may_overlap(pa, gb) ? clean_iou(iou3d<1>(pr, A, gr, Bx, vs, 0)) : 0.0f;
    };
    for (int b = 0; b < B; ++b) {
      long long p0, pn, g0, gn_all;
      segment_of(prior_batch_cnt, b, P, p0, pn);
      segment_of(gt_batch_cnt, b, G, g0, gn_all);
      const int gn = (int)(gn_all < G_cap ? gn_all : G_cap);
      pos_cnt[b] = 0;
      if (gn == 0 || pn == 0) continue;
      const float* gts = gt_bboxes + g0 * 7;
      gc.resize((size_t)gn);
      gbox.resize((size_t)gn);
      glite.resize((size_t)gn);
      for (int g = 0; g < gn; ++g) {
        gc[(size_t)g] = gt_constants(gts + g * 7);
        bev_obox(gts + g * 7, gbox[(size_t)g]);
        lite_of(gts + g * 7, glite[(size_t)g]);
      }
      // 1. candidates
      cand.clear();
      for (long long n = 0; n < pn; ++n) {
        float x, y;
        if (!prior_xy(priors, prior_stride, shared_priors, prior_rows, p0, n, x, y)) continue;
        bool any = false;
        for (int g = 0; g < gn && !any; ++g) any = in_gt(gc[(size_t)g], x, y) || in_ct(gc[(size_t)g], x, y, prm.radius);
        if (any) cand.push_back((int)n);
      }
      const int V = (int)cand.size();
      if (V == 0) continue;
      const int Kc = prm.K < V ? prm.K : V;
      pbox.resize((size_t)V);
      plite.resize((size_t)V);
      for (int v = 0; v < V; ++v) {
        const float* pr = decoded_bboxes + (p0 + cand[(size_t)v]) * 7;
        bev_obox(pr, pbox[(size_t)v]);
        lite_of(pr, plite[(size_t)v]);
      }
      auto cost_of = [&](int n, int g, float u) {
        float x = 0.0f, y = 0.0f;
        prior_xy(priors, prior_stride, shared_priors, prior_rows, p0, n, x, y);
        const bool both = in_gt(gc[(size_t)g], x, y) && in_ct(gc[(size_t)g], x, y, prm.radius);
        return pair_cost(cls_cost(pred_scores + (p0 + n) * C, C, gt_labels[g0 + g]), u, both, prm);
      };
      // 2. - 6. per gt: the dynamic k, the k cheapest candidates
      match.clear();
      match_iou.clear();
      iou.resize((size_t)V);
      for (int g = 0; g < gn; ++g) {
        ent.clear();
        ient.clear();
        for (int v = 0; v < V; ++v) {
          const int n = cand[(size_t)v];
          const float u = pair_iou(decoded_bboxes + (p0 + n) * 7, pbox[(size_t)v], plite[(size_t)v], gts + g * 7, gbox[(size_t)g], glite[(size_t)g]);
          iou[(size_t)v] = u;
          if (u > 0.0f) ient.push_back(iou_entry(u, (unsigned)n));
          ent.push_back(cost_entry(cost_of(n, g, u), (unsigned)n));
        }
        const size_t ki = std::min(ient.size(), (size_t)Kc);
        std::partial_sort(ient.begin(), ient.begin() + (long)ki, ient.end(), std::greater<unsigned long long>());
        float sum = 0.0f;
        for (size_t i = 0; i < ki; ++i) sum = sum + bits_f32((unsigned)(ient[i] >> 32));
        const int k = dynamic_k(sum, Kc);
        std::partial_sort(ent.begin(), ent.begin() + k, ent.end(), std::greater<unsigned long long>());
        for (int j = 0; j < k; ++j) {
          const int n = (int)entry_prior(ent[(size_t)j]);
          const int v = (int)(std::lower_bound(cand.begin(), cand.end(), n) - cand.begin());
          match.push_back({n, g * prm.K + j});
          match_iou.push_back(iou[(size_t)v]);
        }
      }
      // 7. - 8. ascending prior index; a prior more than one gt took goes to the cheapest gt of its whole row
      std::vector<size_t> order(match.size());
      for (size_t i = 0; i < order.size(); ++i) order[i] = i;
      std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return match[x] < match[y]; });
      int npos = 0;
      for (size_t i = 0; i < order.size();) {
        size_t j = i + 1;
        const int n = match[order[i]].first;
        while (j < order.size() && match[order[j]].first == n) ++j;
        int g = match[order[i]].second / prm.K;
        float u = match_iou[order[i]];
        if (j - i > 1) {
          const float* pr = decoded_bboxes + (p0 + n) * 7;
          OBox A;
          Lite pa;
          bev_obox(pr, A);
          lite_of(pr, pa);
          unsigned long long best = ~0ull;
          for (int h = 0; h < gn; ++h) {
            const float uh = pair_iou(pr, A, pa, gts + h * 7, gbox[(size_t)h], glite[(size_t)h]);
            const unsigned long long key = ((unsigned long long)cost_key(cost_of(n, h, uh)) << 32) | (unsigned long long)h;
            if (key < best) {
              best = key;
              g = h;
              u = uh;
            }
          }
        }
        gt_inds[p0 + n] = g + 1;
        labels[p0 + n] = gt_labels[g0 + g];
        max_overlaps[p0 + n] = u;
        pos_inds[(int64_t)b * L + npos] = p0 + n;
        pos_gt_inds[(int64_t)b * L + npos] = g0 + g;
        ++npos;
        i = j;
      }
      pos_cnt[b] = npos;
    }
  } catch (...) {
    return GD3D_E_HOST;
  }
  return 0;
}

}  // extern "C"
