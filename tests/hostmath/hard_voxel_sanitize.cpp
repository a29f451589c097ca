// TEST INFRASTRUCTURE: a stand-alone program that calls the `_cpu` twins of hard voxelization, dynamic voxelization and the mean voxel
// encoder (csrc/hard_voxel_cpu.cpp) with exactly sized heap buffers on the face and the cut inputs — coordinates on and one ulp either
// side of every face of the range, NaN, +-inf and +-1e30 in every column, more cells than max_voxels, more points than max_num_points,
// empty samples, counts that overrun the stack — to be compiled TOGETHER with that unit under
// -fsanitize=address,undefined,float-cast-overflow and run on the CPU (tests/test_cpu_hard_voxel.py does):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -ffp-contract=off \
//       tests/hostmath/hard_voxel_sanitize.cpp mmdet3d-gaussian_amd/csrc/hard_voxel_cpu.cpp -o hard_voxel_sanitize
// The device kernels compile the same cell code (csrc/hard_voxel_common.h).  Every result is checked against a walk with a linear search
// written here.  Prints one line per shape and "OK"; a sanitizer report or a failed check ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

const float INF = std::numeric_limits<float>::infinity();
const float QNAN = std::numeric_limits<float>::quiet_NaN();
const float VS[3] = {0.5f, 0.5f, 1.0f}, LO[3] = {0.0f, -4.0f, -2.0f}, HI[3] = {8.0f, 4.0f, 2.0f};
const int32_t GRID[3] = {16, 16, 4};

// a coordinate on axis j: every kind of trouble, and ordinary ones (confined to `cells` cells so that voxels fill up)
float coordinate(int kind, int j, int cells) {
  switch (kind % 12) {
    case 0: return QNAN;
    case 1: return INF;
    case 2: return -INF;
    case 3: return 1e30f;
    case 4: return -1e30f;
    case 5: return LO[j];
    case 6: return HI[j];
    case 7: return std::nextafterf(HI[j], -INF);
    case 8: return std::nextafterf(LO[j], -INF);
    default: return LO[j] + VS[j] * (float)cells * uniform();
  }
}

bool cell(const float* p, int32_t* c) {   // x y z, the stated sequence
  bool in = true;
  for (int j = 0; j < 3; ++j) {
    const float f = std::floor((p[j] - LO[j]) / VS[j]);
    const bool ok = f >= 0.0f && f < (float)GRID[j];
    c[j] = ok ? (int32_t)f : -1;
    in = in && ok;
  }
  return in;
}

void run(const std::vector<int32_t>& cnt, int64_t N, int64_t stride, int32_t C, int32_t F, int32_t P, int32_t MV, int cells, bool with_voxels) {
  const int32_t B = (int32_t)cnt.size();
  std::vector<float> pts((size_t)(N * stride));
  for (int64_t i = 0; i < N; ++i) {
    const int trouble = (int)(uniform() * 4.0f) == 0 ? (int)(uniform() * 9.0f) : 11, axis = (int)(uniform() * 3.0f);
    for (int j = 0; j < 3; ++j) pts[i * stride + j] = coordinate(j == axis ? trouble : 11, j, cells);
    for (int64_t d = 3; d < stride; ++d) pts[i * stride + d] = uniform() * 2 - 1;
  }
  int64_t cap = (int64_t)B * MV;
  const int64_t R = N < cap ? N : cap;
  std::vector<float> voxels(with_voxels ? (size_t)(R * P * C) : 0, -77.0f), mean((size_t)(R * F), -77.0f), mean2((size_t)(R * F), -77.0f);
  std::vector<int32_t> coors((size_t)(R * 4), 7), num_points((size_t)R, 7), vbc((size_t)B, 7), dyn((size_t)(N * 4), 7);
  int64_t num[2] = {-5, -5};
  CHECK(gd3d_hard_voxelize_cpu(N > 0 ? pts.data() : nullptr, N, stride, C, B > 0 ? cnt.data() : nullptr, B, VS, LO, GRID, P, MV, F, nullptr,
                               with_voxels && R > 0 ? voxels.data() : nullptr, R > 0 ? mean.data() : nullptr, R > 0 ? coors.data() : nullptr,
                               R > 0 ? num_points.data() : nullptr, B > 0 ? vbc.data() : nullptr, num) == 0);
  CHECK(gd3d_dynamic_voxelize_cpu(N > 0 ? pts.data() : nullptr, N, stride, B > 0 ? cnt.data() : nullptr, B, VS, LO, GRID, N > 0 ? dyn.data() : nullptr) == 0);
  // the walk, with a linear search over the sample's voxels
  std::vector<int32_t> wc((size_t)(R * 4), -1), wn((size_t)R, 0);
  std::vector<float> wv((size_t)(R * P * C), 0.0f);
  int64_t start = 0, total = 0, dropped = 0;
  for (int32_t b = 0; b < B; ++b) {
    int64_t end = start + (cnt[(size_t)b] > 0 ? cnt[(size_t)b] : 0);
    end = end < N ? end : N;
    const int64_t base = total;
    int64_t voxel_num = 0;
    for (int64_t i = start; i < end; ++i) {
      int32_t c[3];
      const bool in = cell(&pts[i * stride], c);
      CHECK(dyn[i * 4] == (in ? b : -1) && dyn[i * 4 + 1] == (in ? c[2] : -1) && dyn[i * 4 + 2] == (in ? c[1] : -1) && dyn[i * 4 + 3] == (in ? c[0] : -1));
      if (!in) {
        ++dropped;
        continue;
      }
      int64_t v = -1;
      for (int64_t u = base; u < base + voxel_num; ++u)
        if (wc[u * 4 + 1] == c[2] && wc[u * 4 + 2] == c[1] && wc[u * 4 + 3] == c[0]) v = u;
      if (v < 0) {
        if (voxel_num >= MV) continue;
        v = base + voxel_num++;
        wc[v * 4] = b; wc[v * 4 + 1] = c[2]; wc[v * 4 + 2] = c[1]; wc[v * 4 + 3] = c[0];
      }
      if (wn[(size_t)v] >= P) continue;
      for (int32_t d = 0; d < C; ++d) wv[(v * P + wn[(size_t)v]) * C + d] = pts[i * stride + d];
      wn[(size_t)v] += 1;
    }
    CHECK(vbc[(size_t)b] == voxel_num);
    total += voxel_num;
    start = end;
  }
  for (int64_t i = start; i < N; ++i) CHECK(dyn[i * 4] == -1 && dyn[i * 4 + 3] == -1);   // rows of no sample
  dropped += N - start;
  CHECK(num[0] == total && num[1] == dropped);
  for (int64_t v = 0; v < R; ++v) {
    CHECK(num_points[(size_t)v] == wn[(size_t)v]);
    for (int d = 0; d < 4; ++d) CHECK(coors[v * 4 + d] == wc[v * 4 + d]);
    if (with_voxels)
      for (int64_t e = 0; e < (int64_t)P * C; ++e) CHECK(voxels[v * P * C + e] == wv[v * P * C + e]);
    for (int32_t f = 0; f < F; ++f) {
      float acc = 0.0f;
      for (int k = 0; k < wn[(size_t)v]; ++k) acc += wv[(v * P + k) * C + f];
      const float want = wn[(size_t)v] > 0 ? acc / (float)wn[(size_t)v] : 0.0f;
      CHECK(mean[v * F + f] == want);
    }
  }
  if (R > 0) {
    CHECK(gd3d_voxel_mean_cpu(wv.data(), wn.data(), R, P, C, F, mean2.data()) == 0);
    for (size_t e = 0; e < mean.size(); ++e) CHECK(mean2[e] == mean[e]);
  }
  std::printf("N=%lld stride=%lld C=%d F=%d P=%d MV=%d B=%d voxels=%d: V=%lld dropped=%lld\n", (long long)N, (long long)stride, C, F, P, MV, B,
              (int)with_voxels, (long long)total, (long long)dropped);
}

}  // namespace

int main() {
  for (int with_voxels = 0; with_voxels < 2; ++with_voxels) {
    run({0}, 0, 4, 4, 4, 5, 10, 16, with_voxels);
    run({1}, 1, 4, 4, 4, 5, 10, 16, with_voxels);
    run({63, 0, 65}, 128, 4, 4, 4, 5, 1000, 16, with_voxels);          // nothing is cut but the slots
    run({257, 64}, 321, 4, 4, 3, 1, 16, 6, with_voxels);               // P = 1, 216 cells for 16 voxels
    run({300, 300}, 600, 7, 5, 5, 32, 1, 2, with_voxels);              // one voxel per sample, 32 slots, a stride beyond C
    run({200, 50}, 250, 3, 3, 3, 5, 40, 4, with_voxels);               // rows of exactly three floats
    run({100, 100, 100}, 250, 4, 4, 4, 5, 16, 6, with_voxels);         // the counts overrun the stack
    run({100, -3, 100}, 250, 6, 4, 2, 5, 16, 6, with_voxels);          // a negative count, rows of no sample
  }
  // argument checks never touch memory
  int64_t num[2];
  CHECK(gd3d_hard_voxelize_cpu(nullptr, (int64_t)1 << 31, 4, 4, nullptr, 1, VS, LO, GRID, 5, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_TOOLARGE);
  const int32_t huge[3] = {1 << 24, 1 << 24, 1 << 24};
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 4, 4, nullptr, 4, VS, LO, huge, 5, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_TOOLARGE);
  const int32_t wide[3] = {(1 << 24) + 1, 4, 4};
  CHECK(gd3d_dynamic_voxelize_cpu(nullptr, 8, 4, nullptr, 1, VS, LO, wide, nullptr) == GD3D_E_TOOLARGE);
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 4, 4, nullptr, 1, VS, LO, GRID, 0, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_BADARG);
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 4, 4, nullptr, 1, VS, LO, GRID, 5, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_BADARG);
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 4, 4, nullptr, 1, VS, LO, GRID, 5, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 3, 4, nullptr, 1, VS, LO, GRID, 5, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_BADARG);
  CHECK(gd3d_hard_voxelize_cpu(nullptr, 8, 4, 4, nullptr, 1, VS, LO, GRID, 5, 10, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, num) == GD3D_E_BADARG);   // null operands
  const float bad_vs[3] = {0.5f, 0.0f, 1.0f};
  CHECK(gd3d_dynamic_voxelize_cpu(nullptr, 8, 4, nullptr, 1, bad_vs, LO, GRID, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_voxel_mean_cpu(nullptr, nullptr, 4, 0, 4, 4, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_voxel_mean_cpu(nullptr, nullptr, 4, 5, 4, 5, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_voxel_mean_cpu(nullptr, nullptr, 0, 5, 4, 4, nullptr) == 0);
  std::printf("OK\n");
  return 0;
}
