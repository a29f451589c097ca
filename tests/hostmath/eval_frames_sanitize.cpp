// TEST INFRASTRUCTURE (tests/test_cpu_eval_frames.py): a stand-alone driver of csrc/eval_frames_cpu.cpp, compiled together with it and the
// twins it calls (csrc/eval_ap_cpu.cpp, csrc/rbox_cpu.cpp) under -fsanitize=address,undefined and run as a program on the CPU.  Exactly
// sized heap blocks; empty problems first, last and adjacent, G = 0, D = 0, rows of group -1 (a whole problem, the last row), all three
// modes, T = 1 and 32, crowd flags given and NULL, alias on and off, nthreads 1, 3 and 0.  Checks the group and score columns, the zero
// bits of rows that do not apply, the alias rule, the guard rows and that every thread count gives the same bits, and prints OK.
#include "../../include/gd3d.h"

#include <cstdint>
#include <cstdio>
#include <vector>

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static double uni() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static void box(float* b) {
  b[0] = (float)(uni() * 20 - 10);
  b[1] = (float)(uni() * 20 - 10);
  b[2] = (float)(uni() * 2 - 1.5);
  for (int k = 3; k < 6; ++k) b[k] = (float)(1.2 + uni() * 3);
  b[6] = (float)(uni() * 6.2 - 3.1);
}

struct Size {
  int D, G;
};

static bool run(int mode, const std::vector<Size>& sizes, int R, int T, bool crowd, bool alias) {
  const int P = (int)sizes.size();
  std::vector<int32_t> det_seg((size_t)P + 1, 0), gt_seg((size_t)P + 1, 0);
  std::vector<int64_t> pair_off((size_t)P + 1, 0);
  int64_t max_gt = 0;
  for (int p = 0; p < P; ++p) {
    det_seg[(size_t)p + 1] = det_seg[(size_t)p] + sizes[(size_t)p].D;
    gt_seg[(size_t)p + 1] = gt_seg[(size_t)p] + sizes[(size_t)p].G;
    pair_off[(size_t)p + 1] = pair_off[(size_t)p] + (int64_t)sizes[(size_t)p].D * sizes[(size_t)p].G;
    max_gt = sizes[(size_t)p].G > max_gt ? sizes[(size_t)p].G : max_gt;
  }
  const int64_t ND = det_seg[(size_t)P], NG = gt_seg[(size_t)P];
  std::vector<float> det((size_t)ND * 7), gt((size_t)NG * 7), score((size_t)ND), thrs((size_t)T);
  for (int64_t i = 0; i < NG; ++i) box(&gt[(size_t)i * 7]);
  for (int p = 0; p < P; ++p)
    for (int i = det_seg[(size_t)p]; i < det_seg[(size_t)p + 1]; ++i) {
      box(&det[(size_t)i * 7]);
      if (sizes[(size_t)p].G > 0 && uni() < 0.6) {      // on a gt of its problem, a little off
        const int g = gt_seg[(size_t)p] + (int)(uni() * sizes[(size_t)p].G);
        for (int k = 0; k < 7; ++k) det[(size_t)i * 7 + k] = gt[(size_t)g * 7 + k];
        det[(size_t)i * 7] += (float)(uni() * 0.4 - 0.2);
      }
    }
  for (auto& v : score) v = (float)((int)(uni() * 50) / 50.0);
  for (int t = 0; t < T; ++t) thrs[(size_t)t] = mode == 2 ? 0.2f + 0.2f * (float)t : 0.1f + 0.8f * (float)t / (float)T;
  std::vector<uint8_t> det_flag((size_t)(R * ND)), gt_flag((size_t)(R * NG)), gt_crowd((size_t)NG);
  for (auto& v : det_flag) v = uni() < 0.7;
  for (auto& v : gt_flag) v = uni() < 0.7 ? 3 : 0;
  for (auto& v : gt_crowd) v = uni() < 0.2;
  std::vector<int32_t> group((size_t)(P * R));
  for (int p = 0; p < P; ++p)
    for (int b = 0; b < R; ++b) {
      const bool off = (p % 5 == 2) || (p % 3 == 1 && b == R - 1 && R > 1);
      group[(size_t)(p * R + b)] = off ? -1 : p * R + b;
    }
  const int64_t rows = (int64_t)R * ND, pad = 3;
  std::vector<int32_t> first_group;
  std::vector<float> first_score;
  std::vector<uint32_t> first_tp, first_msk;
  const int threads[3] = {1, 3, 0};
  for (int k = 0; k < 3; ++k) {
    std::vector<int32_t> o_group((size_t)(rows + 2 * pad), -9);
    std::vector<float> o_score((size_t)(rows + 2 * pad), -9.0f);
    std::vector<uint32_t> o_tp((size_t)(rows + 2 * pad), 0xdeadbeefu), o_msk((size_t)(rows + 2 * pad), 0xdeadbeefu);
    const int rc = eval_frames_records_cpu(mode, 0.5f, mode != 2, det.data(), score.data(), det_seg.data(), ND, gt.data(), gt_seg.data(), NG,
                                           crowd ? gt_crowd.data() : nullptr, pair_off.data(), pair_off[(size_t)P], max_gt, det_flag.data(),
                                           gt_flag.data(), group.data(), thrs.data(), P, R, T, alias, o_group.data() + pad, o_score.data() + pad,
                                           o_tp.data() + pad, o_msk.data() + pad, threads[k]);
    if (rc != 0) {
      std::printf("rc %d\n", rc);
      return false;
    }
    for (int64_t i = 0; i < rows + 2 * pad; ++i) {
      const bool guard = i < pad || i >= pad + rows;
      if (guard && (o_group[(size_t)i] != -9 || o_score[(size_t)i] != -9.0f || o_tp[(size_t)i] != 0xdeadbeefu || o_msk[(size_t)i] != 0xdeadbeefu))
        return false;
    }
    for (int p = 0; p < P; ++p) {
      int last = -1;
      for (int b = 0; b < R; ++b)
        if (group[(size_t)(p * R + b)] >= 0) last = b;
      for (int b = 0; b < R; ++b)
        for (int i = det_seg[(size_t)p]; i < det_seg[(size_t)p + 1]; ++i) {
          const size_t at = (size_t)(pad + (int64_t)b * ND + i);
          const int32_t g = group[(size_t)(p * R + b)];
          if (o_group[at] != g || o_score[at] != score[(size_t)i]) return false;
          if (g < 0 && (o_tp[at] != 0 || o_msk[at] != 0)) return false;
          if (sizes[(size_t)p].G == 0 && g >= 0 && (o_tp[at] != 0 || o_msk[at] != (det_flag[(size_t)((int64_t)b * ND + i)] ? (T == 32 ? 0xffffffffu : (1u << T) - 1) : 0u)))
            return false;
          if (alias && g >= 0 && o_tp[at] != o_tp[(size_t)(pad + (int64_t)last * ND + i)]) return false;
          if (T < 32 && ((o_tp[at] | o_msk[at]) >> T) != 0) return false;
        }
    }
    if (k == 0) {
      first_group = o_group;
      first_score = o_score;
      first_tp = o_tp;
      first_msk = o_msk;
    } else if (first_group != o_group || first_score != o_score || first_tp != o_tp || first_msk != o_msk) {
      return false;
    }
  }
  return true;
}

int main() {
  const std::vector<Size> mixed = {{0, 0}, {0, 4}, {5, 3}, {33, 9}, {7, 0}, {0, 0}, {0, 2}, {64, 65}, {65, 64}, {1, 1}, {12, 70}, {9, 0}, {0, 0}};
  bool ok = true;
  for (int mode = 0; mode < 3; ++mode) {
    ok = ok && run(mode, mixed, 4, 2, mode != 1, true);
    ok = ok && run(mode, mixed, 1, 32, mode == 1, false);
    ok = ok && run(mode, {{3, 300}}, 2, 1, true, true);
  }
  ok = ok && run(0, {}, 2, 2, false, true) && run(1, {{0, 0}}, 1, 1, false, false) && run(2, {{0, 7}, {0, 0}}, 3, 3, true, true);
  ok = ok && run(0, {{40, 0}}, 4, 32, false, true);
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
