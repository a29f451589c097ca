// TEST INFRASTRUCTURE (tests/test_cpu_simota.py): a stand-alone driver of csrc/simota_cpu.cpp.
//   simota_sanitize            : compiled together with simota_cpu.cpp under -fsanitize=address,undefined and run as a program on
//                                the CPU: exactly sized heap blocks; batches with empty samples, counts past the rows and negative,
//                                a shared grid shorter than a sample; NaN, +-inf and +-1e30 in boxes, priors and scores; labels
//                                outside [0, C).  Checks the outputs' invariants and prints OK.
//   simota_sanitize logf IN OUT: reads fp32 values from IN, writes fx_logf (csrc/fx_log.h, the host build) of each, then the host
//                                libm's logf of each, to OUT — the error measurement of the test suite.
#define GD3D_HOST_TWIN 1
#include "../../mmdet3d-gaussian_amd/csrc/fx_log.h"

#include "../../include/gd3d.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uni() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static int logf_mode(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> x((size_t)bytes / 4), y(x.size() * 2);
  if (std::fread(x.data(), 4, x.size(), f) != x.size()) return 2;
  std::fclose(f);
  for (size_t i = 0; i < x.size(); ++i) {
    y[i] = rbox::fx_logf(x[i]);
    y[x.size() + i] = std::log(x[i]);
  }
  f = std::fopen(out, "wb");
  if (!f) return 2;
  std::fwrite(y.data(), 4, y.size(), f);
  std::fclose(f);
  return 0;
}

static bool run(int B, int C, int topk, int G_cap, int shared, bool hostile, const std::vector<int>& pcnt, const std::vector<int>& gcnt, int P,
                int G, int prior_rows, int stride) {
  const float bad[5] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                        -std::numeric_limits<float>::infinity(), 1e30f, -1e30f};
  std::vector<float> scores((size_t)P * C), boxes((size_t)P * 7), priors((size_t)prior_rows * stride), gts((size_t)G * 7);
  std::vector<int64_t> glab((size_t)G);
  for (auto& v : scores) v = (float)uni();
  for (int g = 0; g < G; ++g) {
    float* r = &gts[(size_t)g * 7];
    r[0] = (float)(uni() * 8); r[1] = (float)(uni() * 8); r[2] = -1.0f; r[3] = (float)(1.5 + uni() * 3); r[4] = (float)(1 + uni() * 1.5);
    r[5] = 1.6f; r[6] = (float)(uni() * 6.4 - 3.2);
    glab[(size_t)g] = (int64_t)(uni() * (C + 2)) - 1;                      // -1 .. C: some outside [0, C)
  }
  for (int p = 0; p < prior_rows; ++p) {
    priors[(size_t)p * stride] = (float)(uni() * 8);
    priors[(size_t)p * stride + 1] = (float)(uni() * 8);
  }
  for (int p = 0; p < P; ++p) {
    float* r = &boxes[(size_t)p * 7];
    const float* pr = &priors[(size_t)(prior_rows ? p % prior_rows : 0) * stride];
    r[0] = prior_rows ? pr[0] : 0.0f; r[1] = prior_rows ? pr[1] : 0.0f; r[2] = -1.0f; r[3] = (float)(1.5 + uni() * 3);
    r[4] = (float)(1 + uni() * 1.5); r[5] = 1.6f; r[6] = (float)(uni() * 6.4 - 3.2);
  }
  if (hostile) {
    // the yaw columns stay finite here: fx_sincosf's float-to-int conversion of a non-finite quotient is what the sanitizer would stop at
    for (int i = 0; i < P / 4; ++i) boxes[(size_t)(uni() * P) * 7 + (size_t)(uni() * 6)] = bad[i % 5];
    for (int i = 0; i < prior_rows / 8; ++i) priors[(size_t)(uni() * prior_rows * stride)] = bad[i % 5];
    for (int i = 0; i < P / 4; ++i) scores[(size_t)(uni() * P * C)] = i % 3 == 0 ? bad[0] : (i % 3 == 1 ? -1.0f : 2.0f);
    for (int i = 0; i < G / 3; ++i) gts[(size_t)(uni() * G) * 7 + (size_t)(uni() * 6)] = bad[i % 5];
  }
  const size_t L = (size_t)G_cap * topk;
  std::vector<int64_t> gt_inds((size_t)P, 77), labels((size_t)P, 77), pos_inds((size_t)B * L, 77), pos_gt((size_t)B * L, 77);
  std::vector<float> mo((size_t)P, 77.0f);
  std::vector<int32_t> pos_cnt((size_t)B, 77);
  const int rc = gd3d_simota_assign_cpu(scores.data(), boxes.data(), priors.data(), prior_rows, stride, shared, pcnt.data(), P, gts.data(),
                                        glab.data(), gcnt.data(), G, B, C, G_cap, 0.5f, topk, 3.0f, 1.0f, 2.0f, gt_inds.data(), labels.data(),
                                        mo.data(), pos_cnt.data(), pos_inds.data(), pos_gt.data(), nullptr, 0);
  if (rc != 0) {
    std::printf("rc %d\n", rc);
    return false;
  }
  long long positives = 0;
  for (int p = 0; p < P; ++p) {
    if (gt_inds[(size_t)p] < 0 || gt_inds[(size_t)p] > G_cap) return false;
    positives += gt_inds[(size_t)p] > 0;
    if ((gt_inds[(size_t)p] == 0) != (mo[(size_t)p] == -1e8f)) return false;
  }
  long long listed = 0;
  for (int b = 0; b < B; ++b) {
    if (pos_cnt[(size_t)b] < 0 || (size_t)pos_cnt[(size_t)b] > L) return false;
    listed += pos_cnt[(size_t)b];
    for (size_t r = 0; r < L; ++r) {
      const int64_t n = pos_inds[(size_t)b * L + r], g = pos_gt[(size_t)b * L + r];
      if (r < (size_t)pos_cnt[(size_t)b]) {
        if (n < 0 || n >= P || g < 0 || g >= G || gt_inds[(size_t)n] <= 0) return false;
        if (r > 0 && pos_inds[(size_t)b * L + r - 1] >= n) return false;
      } else if (n != -1 || g != -1) {
        return false;
      }
    }
  }
  return listed == positives;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "logf") == 0) return logf_mode(argv[2], argv[3]);
  bool ok = true;
  ok = ok && run(1, 3, 10, 5, 0, false, {300}, {5}, 300, 5, 300, 3);
  ok = ok && run(4, 3, 10, 9, 0, true, {200, 0, 150, 50}, {9, 4, 0, 3}, 400, 16, 400, 2);
  ok = ok && run(3, 1, 1, 4, 0, true, {1000, -5, 1000}, {7, 2, 100}, 500, 10, 500, 5);       // counts past the rows, negative, gts past G_cap
  ok = ok && run(3, 32, 32, 6, 1, true, {120, 100, 120}, {6, 6, 1}, 340, 13, 110, 3);        // a shared grid shorter than two samples
  ok = ok && run(2, 2, 4, 0, 0, false, {10, 10}, {0, 0}, 20, 0, 20, 2);                      // no gts at all
  ok = ok && run(2, 2, 4, 3, 1, false, {0, 0}, {3, 3}, 0, 6, 0, 2);                          // no priors at all
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
