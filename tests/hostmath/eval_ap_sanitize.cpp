// TEST INFRASTRUCTURE (tests/test_cpu_eval_ap.py): a stand-alone driver of csrc/eval_ap_cpu.cpp, compiled together with it under
// -fsanitize=address,undefined,float-cast-overflow and run as a program on the CPU.  Exactly sized heap blocks; n = 0, a NULL
// `matched`, G = 0, matches and groups outside their ranges (the ends of int32 among them), NaN and infinite scores, T = 1 and 32,
// K = 1 and a few thousand, nthreads 1, 3 and 0.  Checks num_det and recall against plain counts, the bounds of ap and that every
// thread count gives the same bits, and prints OK.
#include "../../include/gd3d.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uni() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}
static uint32_t word(int T, double p) {
  uint32_t w = 0;
  for (int t = 0; t < T; ++t) w |= (uint32_t)(uni() < p) << t;
  return w;
}

static bool records(int64_t D, int64_t G, int T, bool with_matched) {
  const int32_t wild[6] = {-7, (int32_t)G, (int32_t)G + 5, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min(), -2};
  std::vector<int32_t> matched(with_matched ? (size_t)(T * D) : 0);
  std::vector<uint8_t> det_flag((size_t)D), gt_flag((size_t)G);
  std::vector<float> score((size_t)D);
  for (auto& v : matched) v = uni() < 0.3 ? wild[(size_t)(uni() * 6)] : (int32_t)(uni() * (double)(G + 1)) - 1;
  for (auto& v : det_flag) v = uni() < 0.7;
  for (auto& v : gt_flag) v = uni() < 0.6 ? 3 : 0;          // any non-zero byte is a set flag
  for (auto& v : score) v = (float)uni();
  const int64_t pad = 3;
  std::vector<int32_t> o_group((size_t)(D + 2 * pad), -1);
  std::vector<float> o_score((size_t)(D + 2 * pad), -1.0f);
  std::vector<uint32_t> o_tp((size_t)(D + 2 * pad), 0xdeadbeefu), o_msk((size_t)(D + 2 * pad), 0xdeadbeefu);
  const int rc = eval_tp_records_cpu(with_matched ? matched.data() : nullptr, det_flag.data(), gt_flag.data(), score.data(), 5, D, G, T,
                                     o_group.data() + pad, o_score.data() + pad, o_tp.data() + pad, o_msk.data() + pad);
  if (rc != 0) return false;
  for (int64_t i = 0; i < D + 2 * pad; ++i) {
    const bool guard = i < pad || i >= pad + D;
    if (guard && (o_group[(size_t)i] != -1 || o_score[(size_t)i] != -1.0f || o_tp[(size_t)i] != 0xdeadbeefu || o_msk[(size_t)i] != 0xdeadbeefu))
      return false;
    if (guard) continue;
    const int64_t d = i - pad;
    uint32_t tp = 0, msk = 0;
    for (int t = 0; t < T; ++t) {
      int64_t m = with_matched ? matched[(size_t)(t * D + d)] : -1;
      if (m < 0 || m >= G) m = -1;
      tp |= (uint32_t)(m >= 0) << t;
      msk |= (uint32_t)(m >= 0 ? gt_flag[(size_t)m] != 0 : det_flag[(size_t)d] != 0) << t;
    }
    if (o_group[(size_t)i] != 5 || o_score[(size_t)i] != score[(size_t)d] || o_tp[(size_t)i] != tp || o_msk[(size_t)i] != msk) return false;
  }
  return true;
}

static bool accumulate(int64_t n, int64_t K, int T, bool hostile) {
  const int32_t stray[4] = {-1, (int32_t)K, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
  const float odd[6] = {std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                        -std::numeric_limits<float>::infinity(), -0.0f, 1e-40f};
  std::vector<int32_t> group((size_t)n);
  std::vector<float> score((size_t)n);
  std::vector<uint32_t> tp((size_t)n), msk((size_t)n);
  std::vector<int64_t> num_gt((size_t)K);
  for (int64_t i = 0; i < n; ++i) {
    group[(size_t)i] = hostile && uni() < 0.2 ? stray[(size_t)(uni() * 4)] : (int32_t)(uni() * (double)K);
    score[(size_t)i] = hostile && uni() < 0.2 ? odd[(size_t)(uni() * 6)] : (float)((int)(uni() * 50) / 50.0);
    tp[(size_t)i] = word(T, 0.5);
    msk[(size_t)i] = word(T, 0.8);
  }
  for (auto& v : num_gt) v = (int64_t)(uni() * 4) - 1;       // -1 and 0 among them: the 1e-7 denominator
  const size_t kt = (size_t)(K * T);
  std::vector<int64_t> want_det(kt, 0), want_tp(kt, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t g = group[(size_t)i];
    if (g < 0 || g >= K) continue;
    for (int t = 0; t < T; ++t)
      if ((msk[(size_t)i] >> t) & 1u) {
        ++want_det[(size_t)(g * T + t)];
        want_tp[(size_t)(g * T + t)] += (tp[(size_t)i] >> t) & 1u;
      }
  }
  std::vector<int64_t> first_det;
  std::vector<double> first_recall, first_ap;
  const int threads[3] = {1, 3, 0};
  for (int k = 0; k < 3; ++k) {
    std::vector<int64_t> num_det(kt, -77);
    std::vector<double> recall(kt, -77.0), ap(kt, -77.0);
    const int rc = eval_ap_accumulate_cpu(group.data(), score.data(), tp.data(), msk.data(), num_gt.data(), n, K, T, num_det.data(), recall.data(),
                                          ap.data(), threads[k]);
    if (rc != 0) {
      std::printf("rc %d\n", rc);
      return false;
    }
    for (size_t i = 0; i < kt; ++i) {
      const double den = num_gt[i / (size_t)T] > 0 ? (double)num_gt[i / (size_t)T] : 1e-7;
      if (num_det[i] != want_det[i]) return false;
      if (recall[i] != (want_det[i] ? (double)want_tp[i] / den : 0.0)) return false;
      if (!(ap[i] >= 0.0) || ap[i] > recall[i] || (want_tp[i] > 0) != (ap[i] > 0.0)) return false;   // every e_j lies in (0, 1]
    }
    if (k == 0) {
      first_det = num_det;
      first_recall = recall;
      first_ap = ap;
    } else if (first_det != num_det || std::memcmp(first_recall.data(), recall.data(), kt * 8) != 0 ||
               std::memcmp(first_ap.data(), ap.data(), kt * 8) != 0) {
      return false;
    }
  }
  return true;
}

int main() {
  bool ok = true;
  ok = ok && records(0, 5, 2, true) && records(0, 0, 1, false);
  ok = ok && records(1, 1, 1, true) && records(300, 40, 2, true) && records(257, 9, 32, true);
  ok = ok && records(64, 7, 3, false) && records(33, 0, 32, true) && records(33, 0, 2, false);
  ok = ok && accumulate(0, 1, 1, false) && accumulate(0, 3000, 32, false);
  ok = ok && accumulate(1, 1, 1, false) && accumulate(1, 1, 32, true);
  ok = ok && accumulate(5000, 1, 32, true) && accumulate(5000, 3, 2, true);
  ok = ok && accumulate(20000, 3001, 32, true) && accumulate(7000, 4096, 1, false);
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
