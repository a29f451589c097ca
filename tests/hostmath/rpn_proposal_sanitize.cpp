// TEST INFRASTRUCTURE (tests/test_cpu_rpn_proposal.py): a stand-alone driver of csrc/rpn_proposal_cpu.cpp.
//   rpn_proposal_sanitize            : compiled together with rpn_proposal_cpu.cpp (and csrc/rbox_cpu.cpp, whose CPU NMS the twin
//                                      calls) under -fsanitize=address,undefined and run as a program on the CPU: exactly sized
//                                      heap blocks; one cell, one anchor, one class and sixteen; nms_pre below, at and above the
//                                      anchor count; samples without a candidate; NaN and +-inf logits, deltas of +-100 (sizes
//                                      of +inf and 0).  Checks the outputs' invariants and prints OK.
//   rpn_proposal_sanitize expf IN OUT: reads fp32 values from IN, writes fx_expf (csrc/fx_exp.h, the host build) of each, then
//                                      the host libm's expf of each, to OUT — the error measurement of the test suite.
#define GD3D_HOST_TWIN 1
#include "../../mmdet3d-gaussian_amd/csrc/fx_exp.h"

#include "../../include/gd3d.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uni() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static int expf_mode(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> x((size_t)bytes / 4), y(x.size() * 2);
  if (std::fread(x.data(), 4, x.size(), f) != x.size()) return 2;
  std::fclose(f);
  for (size_t i = 0; i < x.size(); ++i) {
    y[i] = rbox::fx_expf(x[i]);
    y[x.size() + i] = std::exp(x[i]);
  }
  f = std::fopen(out, "wb");
  if (!f) return 2;
  std::fwrite(y.data(), 4, y.size(), f);
  std::fclose(f);
  return 0;
}

static bool run(int B, int A, int C, int H, int W, int nms_pre, int nms_post, int max_num, int rotate, bool hostile, int dead_sample) {
  const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                        -std::numeric_limits<float>::infinity()};
  const size_t HW = (size_t)H * W, N = HW * A;
  std::vector<float> cls((size_t)B * A * C * HW), bbox((size_t)B * A * 7 * HW), dir((size_t)B * A * 2 * HW), anchors(N * 7);
  for (auto& v : cls) v = (float)(uni() * 6 - 3);
  for (auto& v : bbox) v = (float)(uni() * 0.6 - 0.3);
  for (auto& v : dir) v = (float)(uni() * 2 - 1);
  for (size_t n = 0; n < N; ++n) {
    float* r = &anchors[n * 7];
    r[0] = (float)((n / A) % W) * 0.8f; r[1] = (float)((n / A) / W) * 0.8f; r[2] = -1.78f; r[3] = 1.6f; r[4] = 3.9f; r[5] = 1.56f;
    r[6] = (n % 2) ? 1.57f : 0.0f;
  }
  if (dead_sample >= 0)
    for (size_t i = 0; i < (size_t)A * C * HW; ++i) cls[(size_t)dead_sample * A * C * HW + i] = -20.0f;
  if (hostile) {
    for (size_t i = 0; i < cls.size() / 5 + 1; ++i) cls[(size_t)(uni() * cls.size())] = bad[i % 3];
    // the yaw deltas stay moderate: fx_sincosf's float-to-int conversion of a huge quotient is unspecified (include/gd3d.h)
    for (size_t i = 0; i < bbox.size() / 8 + 1; ++i) {
      const size_t at = (size_t)(uni() * bbox.size());
      if ((at / HW) % 7 != 6) bbox[at] = i % 2 ? 100.0f : -100.0f;
    }
  }
  const int64_t cap = (nms_pre > 0 && (size_t)nms_pre < N) ? nms_pre : (int64_t)N;
  const size_t M = (size_t)(nms_post < max_num ? nms_post : max_num), R = (size_t)B * M;
  std::vector<float> boxes(R * 7, 77.0f), scores(R, 77.0f), preds(R * C, 77.0f), rois(R * 8, 77.0f);
  std::vector<int64_t> labels(R, 77), cand((size_t)B * cap, 77);
  std::vector<int32_t> cnt((size_t)B, 77), ccnt((size_t)B, 77);
  const int rc = gd3d_rpn_proposals_cpu(cls.data(), bbox.data(), dir.data(), anchors.data(), B, A, C, H, W, nms_pre, nms_post, max_num, 0.7f,
                                        0.3f, rotate, 0.7854f, 0.0f, boxes.data(), scores.data(), labels.data(), preds.data(), rois.data(),
                                        cnt.data(), cand.data(), ccnt.data(), nullptr, 0);
  if (rc != 0) {
    std::printf("rc %d\n", rc);
    return false;
  }
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    if (cnt[b] < 0 || (size_t)cnt[b] > M || ccnt[b] < cnt[b] || ccnt[b] > cap) return false;
    if (b == dead_sample && !hostile && cnt[b] != 0) return false;   // a hostile +inf logit revives it
    for (int r = 0; r < cnt[b]; ++r, ++total) {
      if (rois[total * 8] != (float)b || labels[total] < 0 || labels[total] >= C || !(scores[total] > 0.3f)) return false;
      if (r > 0 && scores[total] > scores[total - 1]) return false;
    }
  }
  for (size_t r = total; r < R; ++r)
    if (rois[r * 8] != -1.0f || labels[r] != -1 || scores[r] != 0.0f || boxes[r * 7 + 3] != 0.0f || preds[r * C] != 0.0f) return false;
  for (size_t i = 0; i < cand.size(); ++i)
    if (cand[i] < -1 || cand[i] >= (int64_t)N) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "expf") return expf_mode(argv[2], argv[3]);
  bool ok = true;
  for (int hostile = 0; hostile < 2; ++hostile) {
    ok = ok && run(1, 1, 1, 1, 1, 0, 1, 1, 1, hostile != 0, -1);
    ok = ok && run(2, 6, 3, 5, 7, 209, 30, 20, 1, hostile != 0, -1);
    ok = ok && run(2, 6, 3, 5, 7, 210, 20, 30, 0, hostile != 0, -1);
    ok = ok && run(3, 6, 3, 5, 7, 211, 500, 400, 1, hostile != 0, 1);
    ok = ok && run(2, 2, 16, 8, 11, 50, 10, 10, 0, hostile != 0, 0);
    ok = ok && run(2, 1, 3, 8, 11, -1, 88, 88, 1, hostile != 0, -1);
  }
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
