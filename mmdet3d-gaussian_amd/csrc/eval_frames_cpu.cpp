// eval_frames_cpu.cpp — the `_cpu` twin of csrc/eval_frames.hip (include/gd3d.h "Flexible mAP, a batch of frames"): the same contract on
// HOST memory.  The problems are walked over `nthreads` threads; each problem runs the existing twins — riou_eval_*_cpu for the
// affinities, eval_match_coco_cpu per breakdown row, eval_tp_records_cpu for the rows — and then the alias copy, so the four columns
// carry the bits of the per-frame path by construction.
#define GD3D_HOST_TWIN 1
#include <vector>

#include "eval_frames_common.h"
#include "host_threads.h"

using namespace eval_frames;

extern "C" {

int eval_frames_records_cpu(int32_t mode, float z_offset, int32_t negate, const float* det, const float* score, const int32_t* det_seg,
                            int64_t ND, const float* gt, const int32_t* gt_seg, int64_t NG, const uint8_t* gt_crowd, const int64_t* pair_off,
                            int64_t pairs, int64_t max_gt, const uint8_t* det_flag, const uint8_t* gt_flag, const int32_t* group,
                            const float* thrs, int32_t P, int32_t R, int32_t T, int32_t alias_tp, int32_t* out_group, float* out_score,
                            uint32_t* out_tp_bits, uint32_t* out_msk_bits, int32_t nthreads) {
  const int rc = check_frames(mode, det, score, det_seg, ND, gt, gt_seg, NG, pair_off, pairs, max_gt, det_flag, gt_flag, group, thrs, P, R, T,
                              out_group, out_score, out_tp_bits, out_msk_bits);
  if (rc != 0 || ND == 0) return rc;
  // the tables are host memory here: what the device entry can only guard against is refused
  if (det_seg[0] != 0 || gt_seg[0] != 0 || pair_off[0] != 0 || det_seg[P] != ND || gt_seg[P] != NG || pair_off[P] != pairs) return GD3D_E_BADARG;
  for (int32_t p = 0; p < P; ++p) {
    const int64_t D = (int64_t)det_seg[p + 1] - det_seg[p], G = (int64_t)gt_seg[p + 1] - gt_seg[p];
    if (D < 0 || G < 0 || G > max_gt || pair_off[p + 1] - pair_off[p] != D * G) return GD3D_E_BADARG;
  }
  std::vector<float> thr((size_t)T);
  for (int t = 0; t < T; ++t) thr[(size_t)t] = negate ? -thrs[t] : thrs[t];
  std::atomic<int> err{0};
  const bool team_ok = gd3d_host::parallel_ranges(P, gd3d_host::team_size(nthreads, P, 1, 2), [&](int64_t p0, int64_t p1) {
    std::vector<float> cost;
    std::vector<int32_t> matched;
    std::vector<uint8_t> ignore, crowd;
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t ds = det_seg[p], D = det_seg[p + 1] - ds, gs = gt_seg[p], G = gt_seg[p + 1] - gs;
      if (D == 0) continue;
      int e = 0;
      if (G > 0) {
        cost.resize((size_t)(D * G));
        if (mode == 0) e = riou_eval_3d_cpu(det + ds * 7, D, gt + gs * 7, G, z_offset, cost.data(), 1);
        else if (mode == 1) e = riou_eval_bev_cpu(det + ds * 7, D, gt + gs * 7, G, cost.data(), 1);
        else e = riou_eval_trans_bev_cpu(det + ds * 7, D, 7, gt + gs * 7, G, 7, cost.data(), 1);
        if (negate)
          for (auto& v : cost) v = -v;
        matched.resize((size_t)(T * D));
        ignore.resize((size_t)G);
        crowd.assign((size_t)G, 0);
        if (gt_crowd != nullptr) crowd.assign(gt_crowd + gs, gt_crowd + gs + G);
      }
      int last = -1;      // the last row that applies to the problem
      for (int b = 0; b < R && e == 0; ++b) {
        const int64_t at = (int64_t)b * ND + ds;
        const int32_t g = group[p * R + b];
        if (g < 0) {
          for (int64_t i = 0; i < D; ++i) {
            out_group[at + i] = -1;
            out_score[at + i] = score[ds + i];
            out_tp_bits[at + i] = out_msk_bits[at + i] = 0u;
          }
          continue;
        }
        last = b;
        const uint8_t* gf = G > 0 ? gt_flag + (int64_t)b * NG + gs : nullptr;
        if (G > 0) {
          for (int64_t k = 0; k < G; ++k) ignore[(size_t)k] = gf[k] == 0;
          e = eval_match_coco_cpu(cost.data(), thr.data(), ignore.data(), crowd.data(), D, G, T, matched.data(), 1);
          if (e != 0) break;
        }
        e = eval_tp_records_cpu(G > 0 ? matched.data() : nullptr, det_flag + at, gf, score + ds, g, D, G, T, out_group + at, out_score + at,
                                out_tp_bits + at, out_msk_bits + at);
      }
      if (e == 0 && alias_tp && last > 0)
        for (int b = 0; b < last; ++b)
          if (group[p * R + b] >= 0)
            for (int64_t i = 0; i < D; ++i) out_tp_bits[(int64_t)b * ND + ds + i] = out_tp_bits[(int64_t)last * ND + ds + i];
      if (e != 0) err.store(e, std::memory_order_relaxed);
    }
  });
  if (err.load() != 0) return err.load();
  return team_ok ? 0 : GD3D_E_HOST;
}

}  // extern "C"
