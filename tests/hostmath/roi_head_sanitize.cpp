// TEST INFRASTRUCTURE: a stand-alone program that calls the `_cpu` twins of the RoI-head training slice (csrc/roi_head_cpu.cpp) on
// the edge shapes of tests/pvrcnn_train_ref.py with exactly sized heap buffers, to be compiled TOGETHER with that unit under
// -fsanitize=address,undefined and run on the CPU (tests/test_cpu_pvrcnn_train.py does):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tests/hostmath/roi_head_sanitize.cpp mmdet3d-gaussian_amd/csrc/roi_head_cpu.cpp -o roi_head_sanitize
// Prints one line per shape and "OK"; a sanitizer report or a failed check ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gd3d.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
float uniform() {   // [0, 1)
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((state >> 40) & 0xFFFFFF) / 16777216.0f;
}

void box(float* b) {
  b[0] = uniform() * 60 - 30; b[1] = uniform() * 60 - 30; b[2] = uniform() * 2 - 2;
  b[3] = uniform() * 3 + 0.6f; b[4] = uniform() * 1.2f + 0.6f; b[5] = uniform() + 0.6f;
  b[6] = (uniform() * 2 - 1) * 3.14159265f * 3;   // several periods either side
}

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);                 \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// one step on B samples of (n[b] RoIs, p[b] positives); `pad` extra rows past the counts; `cnt_scale` multiplies the counts handed
// to the twin (> 1: counts that overrun the rows and must be clamped); grads nullable
void run(const std::vector<int>& n, const std::vector<int>& p, int pad, int cnt_scale, bool with_grads, int clockwise) {
  const int B = (int)n.size();
  int64_t R = pad, P = pad;
  for (int b = 0; b < B; ++b) { R += n[b]; P += p[b]; }
  std::vector<float> roi((size_t)P * 7), gt((size_t)P * 7), iou((size_t)R), rois((size_t)R * 8), cls((size_t)R), pred((size_t)R * 7);
  for (int64_t j = 0; j < P; ++j) {
    box(&roi[j * 7]);
    box(&gt[j * 7]);
  }
  for (int64_t i = 0; i < R; ++i) {
    iou[i] = uniform();
    rois[i * 8] = 0.0f;
    box(&rois[i * 8 + 1]);
    cls[i] = uniform() * 8 - 4;
    for (int k = 0; k < 7; ++k) pred[i * 7 + k] = uniform() * 0.4f - 0.2f;
  }
  std::vector<int32_t> pc((size_t)B), rc((size_t)B);
  for (int b = 0; b < B; ++b) {
    pc[b] = p[b] * cnt_scale;
    rc[b] = n[b] * cnt_scale;
  }
  std::vector<float> label((size_t)R), lw((size_t)R), bw((size_t)R), tgt((size_t)P * 7);
  std::vector<int64_t> mask((size_t)R);
  int rc1 = gd3d_roi_head_targets_cpu(roi.data(), gt.data(), iou.data(), pc.data(), rc.data(), B, P, R, 0.75f, 0.25f, clockwise, label.data(),
                                      tgt.data(), mask.data(), lw.data(), bw.data());
  CHECK(rc1 == 0);
  int64_t positives = 0;
  double lsum = 0.0, bsum = 0.0;
  for (int64_t i = 0; i < R; ++i) {
    positives += mask[i];
    lsum += lw[i];
    bsum += bw[i];
  }
  if (cnt_scale == 1) {
    int64_t want = 0;
    for (int b = 0; b < B; ++b) want += p[b] < n[b] ? p[b] : n[b];
    CHECK(positives == want);
    CHECK(std::fabs(lsum - (R - pad > 0 ? 1.0 : 0.0)) < 1e-4 && std::fabs(bsum - (positives > 0 ? 1.0 : 0.0)) < 1e-4);
  }
  for (float v : tgt) CHECK(std::isfinite(v));
  float losses[3] = {-1.0f, -1.0f, -1.0f};
  std::vector<float> gc((size_t)R), gb((size_t)R * 7), g1((size_t)R * 7), g2((size_t)R * 7);
  int rc2 = gd3d_roi_head_loss_cpu(cls.data(), pred.data(), rois.data(), 8, 1, label.data(), tgt.data(), gt.data(), mask.data(), lw.data(), bw.data(),
                                   R, P, 1.0f / 9.0f, 1.0f, 1.0f, 1, clockwise, losses, with_grads ? gc.data() : nullptr,
                                   with_grads ? gb.data() : nullptr, with_grads ? g1.data() : nullptr, with_grads ? g2.data() : nullptr);
  CHECK(rc2 == 0);
  CHECK(std::isfinite(losses[0]) && std::isfinite(losses[1]) && std::isfinite(losses[2]));
  if (positives == 0) CHECK(losses[1] == 0.0f && losses[2] == 0.0f);
  if (with_grads)
    for (float v : gb) CHECK(std::isfinite(v));
  std::printf("B=%d R=%lld P=%lld pad=%d counts x%d clockwise=%d: positives %lld, losses %.6g %.6g %.6g\n", B, (long long)R, (long long)P, pad,
              cnt_scale, clockwise, (long long)positives, losses[0], losses[1], losses[2]);
}

}  // namespace

int main() {
  for (int cw = 0; cw < 2; ++cw) {
    run({1}, {1}, 0, 1, true, cw);
    run({63}, {20}, 0, 1, true, cw);
    run({64}, {64}, 0, 1, true, cw);
    run({65}, {33}, 0, 1, false, cw);
    run({128, 0, 37}, {64, 0, 0}, 0, 1, true, cw);
    run({40, 30}, {0, 0}, 0, 1, true, cw);
    run({512, 512}, {256, 200}, 0, 1, true, cw);
    run({1025}, {512}, 0, 1, true, cw);
    run({1024, 1000, 25}, {512, 64, 25}, 0, 1, true, cw);
    run({128, 0, 37}, {64, 0, 5}, 11, 1, true, cw);    // rows past the counts' sum
    run({128, 0, 37}, {64, 0, 5}, 0, 1000, true, cw);  // counts that overrun the rows: clamped
    run({}, {}, 0, 1, true, cw);                       // nothing at all
    run({}, {}, 5, 1, true, cw);                       // rows but no sample
  }
  // argument checks never touch memory
  CHECK(gd3d_roi_head_targets_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, -1, 0, 0, 0.75f, 0.25f, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
        GD3D_E_BADARG);
  CHECK(gd3d_roi_head_targets_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, 2000, 0, 4, 0.75f, 0.25f, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
        GD3D_E_TOOLARGE);
  CHECK(gd3d_roi_head_loss_cpu(nullptr, nullptr, nullptr, 8, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 4, 0, 0.0f, 1.0f, 1.0f, 1, 0, nullptr,
                               nullptr, nullptr, nullptr, nullptr) == GD3D_E_BADARG);
  std::printf("OK\n");
  return 0;
}
