// TEST INFRASTRUCTURE: a stand-alone program that calls the `_cpu` twins of the keypoint segmentation slice
// (csrc/seg_head_cpu.cpp) on the edge shapes of tests/pvrcnn_seg_ref.py with exactly sized heap buffers, to be compiled TOGETHER
// with that unit under -fsanitize=address,undefined and run on the CPU (tests/test_cpu_pvrcnn_seg.py does):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tests/hostmath/seg_head_sanitize.cpp mmdet3d-gaussian_amd/csrc/seg_head_cpu.cpp -o seg_head_sanitize
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

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);                 \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// the loss on N rows: targets over -1 .. num_classes + 2 (ignored rows and rows past background included), logits up to |x| = 100
void run_loss(int64_t N, int num_classes, int agnostic, float gamma, bool with_grad) {
  const int K = agnostic ? 1 : num_classes;
  std::vector<float> x((size_t)(N * K)), grad((size_t)(N * K), -77.0f);
  std::vector<int64_t> t((size_t)N);
  int64_t want_pos = 0;
  for (int64_t i = 0; i < N; ++i) {
    t[i] = (int64_t)(uniform() * (num_classes + 4)) - 1;
    want_pos += t[i] >= 0 && t[i] < num_classes ? 1 : 0;
    for (int k = 0; k < K; ++k) x[i * K + k] = uniform() < 0.1f ? (uniform() < 0.5f ? 100.0f : -100.0f) : uniform() * 12 - 6;
  }
  float out[2] = {-1.0f, -1.0f};
  const int rc = gd3d_seg_head_loss_cpu(N > 0 ? x.data() : nullptr, N > 0 ? t.data() : nullptr, N, K, num_classes, agnostic, gamma, 0.25f, 1.0f, out,
                                        with_grad && N > 0 ? grad.data() : nullptr);
  CHECK(rc == 0);
  CHECK(std::isfinite(out[0]) && out[0] >= 0.0f && out[1] == (float)want_pos);
  if (N == 0) CHECK(out[0] == 0.0f);
  if (with_grad)
    for (int64_t i = 0; i < N; ++i)
      for (int k = 0; k < K; ++k) {
        const float g = grad[i * K + k];
        CHECK(std::isfinite(g) && g != -77.0f);
        if (t[i] < 0 || t[i] > num_classes) CHECK(g == 0.0f);
      }
  std::printf("loss N=%lld K=%d agnostic=%d gamma=%g grad=%d: loss %.6g, n_pos %g\n", (long long)N, K, agnostic, gamma, (int)with_grad, out[0], out[1]);
}

void run_reweight(int64_t N, int64_t C, int K, bool with_win, bool with_gf, bool with_gx) {
  std::vector<float> f((size_t)(N * C)), g((size_t)(N * C)), x((size_t)(N * K)), out((size_t)(N * C), -77.0f);
  for (float& v : f) v = uniform() * 2 - 1;
  for (float& v : g) v = uniform() * 2 - 1;
  for (float& v : x) v = uniform() < 0.1f ? (uniform() < 0.5f ? 100.0f : -100.0f) : uniform() * 12 - 6;
  std::vector<uint8_t> win((size_t)N, 255);
  int rc = gd3d_keypoint_reweight_cpu(f.data(), x.data(), N, C, K, out.data(), with_win ? win.data() : nullptr);
  CHECK(rc == 0);
  for (float v : out) CHECK(std::isfinite(v) && v != -77.0f);
  if (!with_win) {   // the backward needs one: a second forward call fills it
    rc = gd3d_keypoint_reweight_cpu(f.data(), x.data(), N, C, K, out.data(), win.data());
    CHECK(rc == 0);
  }
  for (int64_t i = 0; i < N; ++i) CHECK(win[i] < K);
  std::vector<float> gf((size_t)(N * C), -77.0f), gx((size_t)(N * K), -77.0f);
  rc = gd3d_keypoint_reweight_backward_cpu(g.data(), with_gx ? f.data() : nullptr, x.data(), win.data(), N, C, K, with_gf ? gf.data() : nullptr,
                                           with_gx ? gx.data() : nullptr);
  CHECK(rc == 0);
  if (with_gf)
    for (float v : gf) CHECK(std::isfinite(v) && v != -77.0f);
  if (with_gx)
    for (int64_t i = 0; i < N; ++i)
      for (int k = 0; k < K; ++k) {
        const float v = gx[i * K + k];
        CHECK(std::isfinite(v) && v != -77.0f);
        if (k != win[i]) CHECK(v == 0.0f);
      }
  std::printf("reweight N=%lld C=%lld K=%d win=%d grad_feats=%d grad_seg=%d\n", (long long)N, (long long)C, K, (int)with_win, (int)with_gf, (int)with_gx);
}

}  // namespace

int main() {
  for (int agnostic = 0; agnostic < 2; ++agnostic) {
    run_loss(0, 3, agnostic, 2.0f, true);
    run_loss(1, 3, agnostic, 2.0f, true);
    run_loss(1, 3, agnostic, 2.0f, false);      // a null gradient pointer
    run_loss(65, 3, agnostic, 2.0f, true);
    run_loss(2049, 3, agnostic, 1.5f, true);
    run_loss(130, 3, agnostic, 0.0f, false);
  }
  run_loss(7, 255, 0, 2.0f, true);               // K = 255
  const int64_t shapes[][3] = {{1, 1, 1}, {65, 3, 3}, {65, 4, 1}, {33, 128, 1}, {17, 260, 3}, {9, 132, 2}, {3, 5, 255}, {2, 1024, 255}};
  for (const auto& s : shapes) {
    run_reweight(s[0], s[1], (int)s[2], true, true, true);
    run_reweight(s[0], s[1], (int)s[2], false, true, false);   // a null winner array in the forward; no grad_seg
    run_reweight(s[0], s[1], (int)s[2], true, false, true);    // no grad_feats
  }
  // N = 0 touches nothing; nothing asked for writes nothing; argument checks never touch memory
  CHECK(gd3d_keypoint_reweight_cpu(nullptr, nullptr, 0, 8, 1, nullptr, nullptr) == 0);
  CHECK(gd3d_keypoint_reweight_backward_cpu(nullptr, nullptr, nullptr, nullptr, 0, 8, 1, nullptr, nullptr) == 0);
  CHECK(gd3d_keypoint_reweight_backward_cpu(nullptr, nullptr, nullptr, nullptr, 4, 8, 1, nullptr, nullptr) == 0);
  CHECK(gd3d_keypoint_reweight_cpu(nullptr, nullptr, 4, 8, 256, nullptr, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_keypoint_reweight_cpu(nullptr, nullptr, 4, 0, 1, nullptr, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_keypoint_reweight_cpu(nullptr, nullptr, 4, 8, 1, nullptr, nullptr) == GD3D_E_BADARG);
  float out[2];
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, 4, 3, 3, 1, 2.0f, 0.25f, 1.0f, out, nullptr) == GD3D_E_BADARG);    // K = 3 with class_agnostic
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, 4, 1, 3, 0, 2.0f, 0.25f, 1.0f, out, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, 4, 1, 3, 1, -1.0f, 0.25f, 1.0f, out, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, 4, 1, 3, 1, 2.0f, 1.5f, 1.0f, out, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, 4, 1, 3, 1, 2.0f, 0.25f, 1.0f, nullptr, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_seg_head_loss_cpu(nullptr, nullptr, (int64_t)1 << 25, 1, 3, 1, 2.0f, 0.25f, 1.0f, out, nullptr) == GD3D_E_TOOLARGE);
  std::printf("OK\n");
  return 0;
}
