// eval_ap_cpu.cpp — the `_cpu` twins of csrc/eval_ap.hip (include/gd3d.h "Flexible mAP"): the same contracts on HOST memory as plain
// loops.  The rank order is a stable sort of the keys of eval_ap_common.h; per (group, threshold) one pass forward gives the
// precisions, one pass backward the envelope, whose 2^-84 units are added in a 128-bit integer: the same exact sum, the same single
// rounding and the same divisions as the kernels, hence the same bits.
#define GD3D_HOST_TWIN 1
#include <algorithm>
#include <numeric>
#include <vector>

#include "eval_ap_common.h"
#include "host_threads.h"

using namespace eval_ap;

extern "C" {

int eval_tp_records_cpu(const int32_t* matched, const uint8_t* det_flag, const uint8_t* gt_flag, const float* score, int32_t group, int64_t D,
                        int64_t G, int32_t T, int32_t* out_group, float* out_score, uint32_t* out_tp_bits, uint32_t* out_msk_bits) {
  const int rc = check_records(det_flag, gt_flag, score, D, G, T, out_group, out_score, out_tp_bits, out_msk_bits);
  if (rc != 0) return rc;
  for (int64_t d = 0; d < D; ++d) {
    const bool df = det_flag[d] != 0;
    uint32_t tp = 0, msk = 0;
    for (int t = 0; t < T; ++t) {
      const int32_t m = matched != nullptr ? clamp_match(matched[(int64_t)t * D + d], G) : -1;
      const bool hit = m > -1;
      const bool in = hit ? gt_flag[m] != 0 : df;
      tp |= (uint32_t)hit << t;
      msk |= (uint32_t)in << t;
    }
    out_group[d] = group;
    out_score[d] = score[d];
    out_tp_bits[d] = tp;
    out_msk_bits[d] = msk;
  }
  return 0;
}

int eval_ap_accumulate_cpu(const int32_t* group, const float* score, const uint32_t* tp_bits, const uint32_t* msk_bits, const int64_t* num_gt,
                           int64_t n, int64_t K, int32_t T, int64_t* num_det, double* recall, double* ap, int32_t nthreads) {
  const int rc = check_accumulate(group, score, tp_bits, msk_bits, num_gt, n, K, T, num_det, recall, ap);
  if (rc != 0) return rc;
  try {
    std::vector<uint64_t> key((size_t)n);
    std::vector<int32_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) key[(size_t)i] = record_key(group[i], score[i], (int32_t)K);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    // first[g] .. first[g + 1]: the group's rows in rank order
    std::vector<int64_t> first((size_t)K + 1, n);
    {
      int64_t i = 0;
      for (int64_t g = 0; g <= K; ++g) {
        while (i < n && (int64_t)(key[(size_t)order[(size_t)i]] >> 32) < g) ++i;
        first[(size_t)g] = i;
      }
    }
    const int team = gd3d_host::team_size(nthreads, K * T, 1, 2);
    const bool ok = gd3d_host::parallel_ranges(K * T, team, [&](int64_t a, int64_t b) {
      std::vector<double> p;
      for (int64_t item = a; item < b; ++item) {
        const int64_t g = item / T;
        const int t = (int)(item - g * T);
        p.clear();
        uint32_t D = 0, C = 0;
        for (int64_t i = first[(size_t)g]; i < first[(size_t)g + 1]; ++i) {
          const int32_t r = order[(size_t)i];
          if (!((msk_bits[r] >> t) & 1u)) continue;
          const bool h = (tp_bits[r] >> t) & 1u;
          ++D;
          C += h;
          const double q = (double)C / (double)D;
          p.push_back(h ? q : -q);   // the sign carries h_j (a precision of 0 has h_j clear)
        }
        unsigned __int128 units = 0;
        double e = 0.0;
        for (size_t j = p.size(); j-- > 0;) {
          const double q = p[j] < 0 ? -p[j] : p[j];
          e = q > e ? q : e;
          if (p[j] > 0) {
            const Limbs l = limbs_of(e);
            units += (unsigned __int128)l.l[0] + ((unsigned __int128)l.l[1] << 21) + ((unsigned __int128)l.l[2] << 42) +
                     ((unsigned __int128)l.l[3] << 63);
          }
        }
        // the total as limb sums again: limbs_to_double is the one rounding both units share
        const uint64_t mask = (1ull << 21) - 1;
        const double esum = limbs_to_double((uint64_t)units & mask, (uint64_t)(units >> 21) & mask, (uint64_t)(units >> 42) & mask,
                                            (uint64_t)(units >> 63));
        finish(D, C, esum, num_gt[g], num_det + item, recall + item, ap + item);
      }
    });
    return ok ? 0 : GD3D_E_HOST;
  } catch (...) {
    return GD3D_E_HOST;
  }
}

}  // extern "C"
