// TEST INFRASTRUCTURE: a stand-alone program that calls the `_cpu` twins of the voxel query ops (csrc/voxel_query_cpu.cpp) with exactly
// sized heap buffers on the robustness inputs — `coors` with -1 rows, rows past the grid and the extremes of their type, a caller's
// dense table full of garbage, query cells anywhere in int32, NaN / +-inf / 1e30 points — to be compiled TOGETHER with that unit under
// -fsanitize=address,undefined,float-cast-overflow and run on the CPU (tests/test_cpu_voxel_query.py does):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -ffp-contract=off -pthread \
//       tests/hostmath/voxel_query_sanitize.cpp mmdet3d-gaussian_amd/csrc/voxel_query_cpu.cpp -o voxel_query_sanitize
// The device kernels compile the same window, key and cell code (csrc/voxel_query_common.h).  Prints one line per shape and "OK"; a
// sanitizer report or a failed check ends it with a non-zero status.
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

float trouble(int kind, float lo, float hi) {
  switch (kind % 8) {
    case 0: return QNAN;
    case 1: return INF;
    case 2: return -INF;
    case 3: return 1e30f;
    case 4: return -1e30f;
    case 5: return hi;
    default: return lo + (hi - lo) * uniform();
  }
}

template <typename T>
void run(int64_t N, int64_t M, int32_t B, int32_t Z, int32_t Y, int32_t X, int32_t rz, int32_t ry, int32_t rx, int32_t nsample, int32_t C) {
  std::vector<T> coors((size_t)(N * 4));
  for (int64_t i = 0; i < N; ++i) {
    const int kind = (int)(uniform() * 10);
    const int32_t dims[4] = {B, Z, Y, X};
    for (int a = 0; a < 4; ++a) {
      T v = (T)(uniform() * (float)(dims[a] + 1));   // the extent itself included
      if (kind == 0) v = (T)-1;
      if (kind == 1 && a == (int)(i % 4)) v = std::numeric_limits<T>::max();
      if (kind == 2 && a == (int)(i % 4)) v = std::numeric_limits<T>::min();
      coors[(size_t)(i * 4 + a)] = v;
    }
  }
  std::vector<float> xyz((size_t)(N * 3)), q((size_t)(M * 3)), feats((size_t)(N * C));
  for (int64_t i = 0; i < N * 3; ++i) xyz[(size_t)i] = trouble((int)(uniform() * 40), -2.0f, (float)X + 2.0f);
  for (int64_t i = 0; i < M * 3; ++i) q[(size_t)i] = trouble((int)(uniform() * 40), -2.0f, (float)X + 2.0f);
  for (float& v : feats) v = uniform();
  const int64_t cells = (int64_t)B * Z * Y * X;
  std::vector<int64_t> skey((size_t)N, -7);
  std::vector<int32_t> srow((size_t)N, -7), table((size_t)cells, 12345), cnts((size_t)B), nc((size_t)(M * 4), -7);
  CHECK(gd3d_vsa_voxel_index_cpu(N > 0 ? coors.data() : nullptr, sizeof(T) == 8, N, B, Z, Y, X, nullptr, N > 0 ? skey.data() : nullptr,
                                 N > 0 ? srow.data() : nullptr) == 0);
  for (int64_t i = 0; i < N; ++i) {
    CHECK(skey[(size_t)i] >= 0 && skey[(size_t)i] <= cells && srow[(size_t)i] >= 0 && srow[(size_t)i] < N);
    CHECK(i == 0 || skey[(size_t)i - 1] < skey[(size_t)i] || (skey[(size_t)i - 1] == skey[(size_t)i] && srow[(size_t)i - 1] < srow[(size_t)i]));
  }
  CHECK(gd3d_vsa_voxel_table_cpu(N > 0 ? coors.data() : nullptr, sizeof(T) == 8, N, B, Z, Y, X, cells > 0 ? table.data() : nullptr) == 0);
  for (int32_t v : table) CHECK(v >= -1 && v < N);
  for (int32_t b = 0; b < B; ++b) cnts[(size_t)b] = (int32_t)(uniform() * (float)(2 * M / (B > 0 ? B : 1) + 2)) - 1;   // negative and too large included
  const float cell[3] = {1.0f, 0.5f, 0.25f}, lo[3] = {0.0f, -1.0f, 0.5f};
  CHECK(gd3d_vsa_voxel_coords_cpu(M > 0 ? q.data() : nullptr, B > 0 ? cnts.data() : nullptr, B, M, cell, lo, M > 0 ? nc.data() : nullptr) == 0);
  for (int64_t m = 0; m < M; ++m) CHECK(nc[(size_t)(m * 4)] >= -1 && nc[(size_t)(m * 4)] < B);
  for (int64_t m = 0; m < M; ++m) {   // query cells anywhere: in the grid, around it, at the ends of int32
    const int kind = (int)(uniform() * 8);
    const int32_t dims[4] = {B, Z, Y, X};
    for (int a = 0; a < 4; ++a) {
      int32_t v = (int32_t)(uniform() * (float)(dims[a] + 2 * 17)) - 17;
      if (kind == 0 && a == (int)(m % 4)) v = std::numeric_limits<int32_t>::max();
      if (kind == 1 && a == (int)(m % 4)) v = std::numeric_limits<int32_t>::min();
      if (a == 0 && kind > 2) v = (int32_t)(uniform() * (float)B);
      nc[(size_t)(m * 4 + a)] = v;
    }
  }
  std::vector<int32_t> garbage((size_t)cells);
  for (int32_t& v : garbage) v = (int32_t)((uniform() * 2.0f - 1.0f) * 2147483000.0f);
  const int32_t rng[3] = {rz, ry, rx};
  const int ct = 3 + C;
  for (int form = 0; form < 3; ++form) {   // the sorted keys, the table, a table of garbage
    std::vector<int32_t> idx((size_t)(M * nsample), -7), cnt((size_t)M, -7);
    std::vector<uint8_t> mask((size_t)M, 7);
    std::vector<float> out((size_t)(M * ct * nsample), -77.0f);
    const int32_t* tab = form == 0 ? nullptr : (form == 1 ? table.data() : garbage.data());
    CHECK(gd3d_vsa_voxel_query_and_group_cpu(N > 0 ? xyz.data() : nullptr, M > 0 ? q.data() : nullptr, M > 0 ? nc.data() : nullptr,
                                             form == 0 && N > 0 ? skey.data() : nullptr, form == 0 && N > 0 ? srow.data() : nullptr,
                                             cells > 0 ? tab : nullptr, N > 0 && C > 0 ? feats.data() : nullptr, B, Z, Y, X, N, M, C, rng, 1.5f,
                                             nsample, 1, M > 0 ? out.data() : nullptr, M > 0 ? idx.data() : nullptr, M > 0 ? cnt.data() : nullptr,
                                             M > 0 ? mask.data() : nullptr, 3) == 0);
    for (int64_t m = 0; m < M; ++m) {
      CHECK(cnt[(size_t)m] >= 0 && cnt[(size_t)m] <= nsample && mask[(size_t)m] == (cnt[(size_t)m] == 0 ? 1 : 0));
      for (int s = 0; s < nsample; ++s) CHECK(idx[(size_t)(m * nsample + s)] >= 0 && (idx[(size_t)(m * nsample + s)] < N || N == 0));
    }
    for (float v : out) CHECK(!(v == -77.0f));
  }
  std::printf("N=%lld M=%lld grid=(%d,%d,%d,%d) range=(%d,%d,%d) nsample=%d C=%d int%d\n", (long long)N, (long long)M, B, Z, Y, X, rz, ry, rx,
              nsample, C, (int)(8 * sizeof(T)));
}

}  // namespace

int main() {
  run<int32_t>(400, 131, 3, 5, 12, 14, 1, 1, 3, 16, 5);
  run<int64_t>(400, 131, 3, 5, 12, 14, 2, 6, 1, 5, 0);
  run<int32_t>(900, 37, 2, 4, 9, 11, 16, 16, 16, 1024, 2);   // the largest window and idx row
  run<int64_t>(50, 9, 1, 1, 1, 1, 0, 0, 0, 1, 1);
  run<int32_t>(0, 21, 2, 3, 3, 3, 1, 1, 1, 4, 3);             // no voxels
  run<int32_t>(30, 0, 2, 3, 3, 3, 1, 1, 1, 4, 3);             // no queries
  run<int32_t>(30, 11, 0, 3, 3, 3, 1, 1, 1, 4, 3);            // no samples: every query empty
  // argument checks never touch memory
  const int32_t ok[3] = {1, 1, 1}, wide[3] = {1, 17, 1}, neg[3] = {-1, 1, 1};
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 4, wide, 1.0f, 4, nullptr, nullptr, nullptr, 1) == GD3D_E_TOOLARGE);
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 4, neg, 1.0f, 4, nullptr, nullptr, nullptr, 1) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 4, ok, 1.0f, 1025, nullptr, nullptr, nullptr, 1) == GD3D_E_TOOLARGE);
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 4, ok, 1.0f, 0, nullptr, nullptr, nullptr, 1) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 0, 3, 5, 4, ok, 1.0f, 4, nullptr, nullptr, nullptr, 1) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 4, ok, 1.0f, 4, nullptr, nullptr, nullptr, 1) == GD3D_E_BADARG);   // null operands
  CHECK(gd3d_vsa_voxel_query_cpu(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 3, 3, 3, 5, 0, ok, 1.0f, 4, nullptr, nullptr, nullptr, 1) == 0);              // M == 0
  CHECK(gd3d_vsa_voxel_index_cpu(nullptr, 0, 5, 2, 3, 3, 3, nullptr, nullptr, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_index_cpu(nullptr, 0, 5, 2, 3, 3, (1 << 24) + 1, nullptr, nullptr, nullptr) == GD3D_E_TOOLARGE);
  CHECK(gd3d_vsa_voxel_table_cpu(nullptr, 0, 5, 2, 3, 3, 3, nullptr) == GD3D_E_BADARG);
  const float one[3] = {1.0f, 1.0f, 1.0f}, zero[3] = {1.0f, 0.0f, 1.0f};
  CHECK(gd3d_vsa_voxel_coords_cpu(nullptr, nullptr, 2, 5, zero, one, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_coords_cpu(nullptr, nullptr, 2, 5, one, one, nullptr) == GD3D_E_BADARG);
  CHECK(gd3d_vsa_voxel_coords_cpu(nullptr, nullptr, 2, 0, one, one, nullptr) == 0);
  std::printf("OK\n");
  return 0;
}
