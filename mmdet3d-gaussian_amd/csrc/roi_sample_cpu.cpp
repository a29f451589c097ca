// roi_sample_cpu.cpp — the `_cpu` twins of csrc/roi_sample.hip (include/gd3d.h, gd3d_roi_iou3d_cpu / gd3d_roi_assign_sample_cpu):
// plain loops over the IoU and the decisions of csrc/roi_sample_common.h, the source the kernels compile for the device (both
// units with -ffp-contract=off; sin / cos / atan2 are fixed polynomial sequences).  Every output is BIT-IDENTICAL to the kernels'.
// Host memory in and out, no stream, no HIP call, one thread.  Also the one text of the argument checks (make_rules).
#define GD3D_HOST_TWIN 1
#include "roi_sample_common.h"

#include "../../include/gd3d.h"

#include <algorithm>
#include <vector>

namespace roi_sample {

int make_rules(int64_t N, int64_t G, int32_t B, int32_t C, const float* pos_iou_thr, const float* neg_iou_thr, const float* min_pos_iou,
               const int32_t* assign_flags, int32_t num, int32_t npos, int32_t K, const double* neg_piece_fractions,
               const float* neg_iou_piece_thrs, Rules& r) {
  if (N < 0 || G < 0 || B < 0 || C < 1 || num < 1 || npos < 0 || npos > num || K < 1) return GD3D_E_BADARG;
  if (N > MAX_ROWS || G > MAX_ROWS || B > MAX_SAMPLES || C > MAX_CLASSES || num > MAX_NUM || K > MAX_PIECES) return GD3D_E_TOOLARGE;
  if (pos_iou_thr == nullptr || neg_iou_thr == nullptr || min_pos_iou == nullptr || assign_flags == nullptr ||
      neg_piece_fractions == nullptr || neg_iou_piece_thrs == nullptr)
    return GD3D_E_BADARG;
  r.C = C;
  for (int c = 0; c < C; ++c) {
    if (pos_iou_thr[c] != pos_iou_thr[c] || neg_iou_thr[c] != neg_iou_thr[c] || min_pos_iou[c] != min_pos_iou[c]) return GD3D_E_BADARG;
    r.pos[c] = pos_iou_thr[c];
    r.neg[c] = neg_iou_thr[c];
    r.min_pos[c] = min_pos_iou[c];
    r.flags[c] = assign_flags[c];
  }
  r.num = num;
  r.npos = npos;
  r.K = K;
  for (int i = 0; i < K; ++i) {   // pieces [thr[i + 1], thr[i]) must not meet: strictly descending, positive
    if (!(neg_iou_piece_thrs[i] > 0.0f) || (i > 0 && !(neg_iou_piece_thrs[i] < neg_iou_piece_thrs[i - 1]))) return GD3D_E_BADARG;
    if (!(neg_piece_fractions[i] >= 0.0 && neg_piece_fractions[i] <= 1.0)) return GD3D_E_BADARG;
    r.piece_thr[i] = neg_iou_piece_thrs[i];
    r.piece_frac[i] = neg_piece_fractions[i];
  }
  return 0;
}

}  // namespace roi_sample

using namespace roi_sample;

extern "C" {

int gd3d_roi_iou3d_cpu(const float* bboxes1, int64_t n1, const float* bboxes2, int64_t n2, float* iou) {
  if (n1 < 0 || n2 < 0) return GD3D_E_BADARG;
  if (n1 == 0 || n2 == 0) return 0;
  if (n1 > MAX_ROWS || n2 > MAX_ROWS || n1 * n2 > (1LL << 31) - NT) return GD3D_E_TOOLARGE;
  if (bboxes1 == nullptr || bboxes2 == nullptr || iou == nullptr) return GD3D_E_BADARG;
  try {
    std::vector<OBox> ob((size_t)n2);
    for (int64_t j = 0; j < n2; ++j) bev_obox(bboxes2 + j * 7, ob[(size_t)j]);
    VertexScratch<1> vs;
    for (int64_t i = 0; i < n1; ++i) {
      OBox A;
      bev_obox(bboxes1 + i * 7, A);
      for (int64_t j = 0; j < n2; ++j) iou[i * n2 + j] = iou3d<1>(bboxes1 + i * 7, A, bboxes2 + j * 7, ob[(size_t)j], vs, 0);
    }
  } catch (...) {
    return GD3D_E_HOST;
  }
  return 0;
}

int gd3d_roi_assign_sample_cpu(const float* proposals, const int64_t* proposal_labels, const int32_t* prop_batch_cnt, int64_t N,
                               const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B,
                               const float* keys, const float* fill_keys, int32_t C, const float* pos_iou_thr,
                               const float* neg_iou_thr, const float* min_pos_iou, const int32_t* assign_flags, int32_t num,
                               int32_t npos, int32_t K, const double* neg_piece_fractions, const float* neg_iou_piece_thrs,
                               float* rois, float* ious, int64_t* inds, float* pos_bboxes, float* pos_gt_bboxes,
                               int64_t* pos_assigned_gt_inds, int32_t* pos_batch_cnt, int32_t* roi_batch_cnt, int64_t* gt_inds,
                               float* max_overlaps, int64_t* labels, int32_t* stage) {
  Rules r;
  const int rc = make_rules(N, G, B, C, pos_iou_thr, neg_iou_thr, min_pos_iou, assign_flags, num, npos, K, neg_piece_fractions,
                            neg_iou_piece_thrs, r);
  if (rc != 0) return rc;
  if (B == 0) return N == 0 ? 0 : GD3D_E_BADARG;
  if (prop_batch_cnt == nullptr || gt_batch_cnt == nullptr || fill_keys == nullptr || rois == nullptr || ious == nullptr ||
      inds == nullptr || pos_batch_cnt == nullptr || roi_batch_cnt == nullptr || stage == nullptr)
    return GD3D_E_BADARG;
  if (N > 0 && (proposals == nullptr || proposal_labels == nullptr || keys == nullptr || gt_inds == nullptr ||
                max_overlaps == nullptr || labels == nullptr))
    return GD3D_E_BADARG;
  if (G > 0 && (gt_bboxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  if (npos > 0 && (pos_bboxes == nullptr || pos_gt_bboxes == nullptr || pos_assigned_gt_inds == nullptr)) return GD3D_E_BADARG;
  try {
    VertexScratch<1> vs;
    std::vector<OBox> gbox;
    std::vector<int> glab, arg_of, strat;
    std::vector<float> gmax;
    std::vector<int> gfirst;
    std::vector<unsigned long long> list;
    std::vector<int> sel((size_t)num);
    const int64_t stride = 2 + num;
    int p0 = 0, g0 = 0, r0 = 0, q0 = 0;
    for (int b = 0; b < B; ++b) {
      const int pn = clamp_count(prop_batch_cnt[b], (int)N - p0), gn = clamp_count(gt_batch_cnt[b], (int)G - g0);
      const int Np = pn < MAX_PROPS ? pn : MAX_PROPS, Ng = gn < MAX_GTS ? gn : MAX_GTS;
      const float* prop = proposals + (int64_t)p0 * 7;
      const float* gts = gt_bboxes + (int64_t)g0 * 7;
      gbox.resize((size_t)Ng);
      glab.assign((size_t)Ng, -1);
      gmax.assign((size_t)Ng, 0.0f);
      gfirst.assign((size_t)Ng, -1);
      for (int g = 0; g < Ng; ++g) {
        bev_obox(gts + g * 7, gbox[(size_t)g]);
        const int64_t l = gt_labels[g0 + g];
        glab[(size_t)g] = (l >= 0 && l < C) ? (int)l : -1;
      }
      arg_of.assign((size_t)Np, -1);
      // pass 1
      for (int n = 0; n < Np; ++n) {
        const int64_t l = proposal_labels[p0 + n];
        const int c = (l >= 0 && l < C) ? (int)l : -1;
        float best = 0.0f;
        int arg = -1;
        if (c >= 0) {
          OBox A;
          bev_obox(prop + n * 7, A);
          for (int g = 0; g < Ng; ++g) {
            if (glab[(size_t)g] != c) continue;
            const float v = clean_iou(iou3d<1>(prop + n * 7, A, gts + g * 7, gbox[(size_t)g], vs, 0));
            if (arg < 0 || v > best) {
              best = v;
              arg = g;
            }
            if (gfirst[(size_t)g] < 0 || v > gmax[(size_t)g]) {   // ascending n: the lowest index keeps a tie
              gmax[(size_t)g] = v;
              gfirst[(size_t)g] = n;
            }
          }
        }
        max_overlaps[p0 + n] = best;
        arg_of[(size_t)n] = arg;
      }
      // pass 2
      int cnt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      strat.assign((size_t)Np, -1);
      for (int n = 0; n < Np; ++n) {
        const float mo = max_overlaps[p0 + n];
        const int arg = arg_of[(size_t)n];
        int gi = 0;
        if (arg >= 0) {
          const int c = glab[(size_t)arg];
          gi = assign_first(mo, arg, r.pos[c], r.neg[c]);
          if (r.flags[c] & FLAG_LOW_QUALITY) {
            const bool all = (r.flags[c] & FLAG_ASSIGN_ALL) != 0;
            OBox A;
            bool have = false;
            for (int g = Ng - 1; g >= 0; --g) {
              if (glab[(size_t)g] != c) continue;
              const float gm = gmax[(size_t)g];
              if (!(gm >= r.min_pos[c])) continue;
              bool match;
              if (!all) {
                match = gfirst[(size_t)g] == n;
              } else if (g == arg) {
                match = mo == gm;
              } else if (!(mo >= gm)) {
                match = false;
              } else {
                if (!have) {
                  bev_obox(prop + n * 7, A);
                  have = true;
                }
                match = clean_iou(iou3d<1>(prop + n * 7, A, gts + g * 7, gbox[(size_t)g], vs, 0)) == gm;
              }
              if (match) {
                gi = g + 1;
                break;
              }
            }
          }
        }
        gt_inds[p0 + n] = gi;
        labels[p0 + n] = gi > 0 ? gt_labels[g0 + gi - 1] : -1;
        const int s = stratum_of(gi, mo, r);
        strat[(size_t)n] = s;
        if (s >= 0) ++cnt[s];
      }
      for (int n = Np; n < pn; ++n) {
        gt_inds[p0 + n] = -1;
        max_overlaps[p0 + n] = 0.0f;
        labels[p0 + n] = -1;
      }
      // the draws
      Plan plan;
      make_plan(cnt, r, plan);
      list.clear();
      for (int n = 0; n < Np; ++n)
        if (strat[(size_t)n] >= 0) list.push_back(draw_entry(strat[(size_t)n], keys[p0 + n], n));
      std::sort(list.begin(), list.end(), [](unsigned long long x, unsigned long long y) { return x > y; });
      int start[16];
      for (int s = 0, s0 = 0; s <= K; ++s) {
        start[s] = s0;
        s0 += cnt[s];
      }
      std::vector<int> drawn;
      for (int t = 0; t < plan.npos; ++t) drawn.push_back(entry_index(list[(size_t)t]));
      std::sort(drawn.begin(), drawn.end());
      for (int t = 0; t < plan.npos; ++t) sel[(size_t)t] = drawn[(size_t)t];
      for (int i = 0; i < K; ++i)
        for (int t = 0; t < plan.take[i]; ++t)
          sel[(size_t)(plan.npos + plan.off[i] + t)] = entry_index(list[(size_t)(start[1 + i] + t)]);
      std::vector<int> last;
      if (plan.fill > 0 && plan.fill_from_last)
        for (int n = 0; n < Np; ++n)
          if (strat[(size_t)n] == K) last.push_back(n);
      const int before = plan.npos + plan.chosen;
      for (int t = 0; t < plan.fill; ++t) {
        const int j = before + t;
        const int k = fill_member(fill_keys[(int64_t)b * num + j], plan.m);
        sel[(size_t)j] = plan.fill_from_last ? last[(size_t)k] : sel[(size_t)(plan.npos + k)];
      }
      const int rows = before + plan.fill;
      int32_t* st = stage + b * stride;
      st[0] = plan.npos;
      st[1] = rows;
      for (int j = 0; j < num; ++j) st[2 + j] = j < rows ? sel[(size_t)j] : -1;
      // pack
      pos_batch_cnt[b] = plan.npos;
      roi_batch_cnt[b] = rows;
      for (int j = 0; j < rows; ++j) {
        const int n = sel[(size_t)j];
        const int64_t row = r0 + j, src = (int64_t)p0 + n;
        rois[row * 8] = (float)b;
        for (int k = 0; k < 7; ++k) rois[row * 8 + 1 + k] = proposals[src * 7 + k];
        ious[row] = max_overlaps[src];
        inds[row] = n;
      }
      for (int j = 0; j < plan.npos; ++j) {
        const int n = sel[(size_t)j];
        const int64_t row = q0 + j, src = (int64_t)p0 + n, gi = gt_inds[src] - 1;
        for (int k = 0; k < 7; ++k) {
          pos_bboxes[row * 7 + k] = proposals[src * 7 + k];
          pos_gt_bboxes[row * 7 + k] = gt_bboxes[((int64_t)g0 + gi) * 7 + k];
        }
        pos_assigned_gt_inds[row] = gi;
      }
      p0 += pn;
      g0 += gn;
      r0 += rows;
      q0 += plan.npos;
    }
    for (int64_t i = p0; i < N; ++i) {
      gt_inds[i] = -1;
      max_overlaps[i] = 0.0f;
      labels[i] = -1;
    }
    for (int64_t row = r0; row < (int64_t)B * num; ++row) {
      rois[row * 8] = -1.0f;
      for (int k = 1; k < 8; ++k) rois[row * 8 + k] = 0.0f;
      ious[row] = 0.0f;
      inds[row] = 0;
    }
    for (int64_t row = q0; row < (int64_t)B * npos; ++row) {
      for (int k = 0; k < 7; ++k) pos_bboxes[row * 7 + k] = pos_gt_bboxes[row * 7 + k] = 0.0f;
      pos_assigned_gt_inds[row] = 0;
    }
  } catch (...) {
    return GD3D_E_HOST;
  }
  return 0;
}

}  // extern "C"
