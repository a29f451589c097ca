// pillar_feat_sanitize.cpp — a stand-alone driver (its own main) for the `_cpu` twins of the pillar encoders' point decoration
// (csrc/pillar_feat_cpu.cpp), compiled together with them under -fsanitize=address,undefined by tests/test_cpu_pillar_feat.py and
// run as a program on the CPU.  Every buffer is an exactly sized heap block, so a read or write one element past any operand is
// reported: all 128 flag sets of gd3d_point_voxel_stats_cpu over int32 and int64 rows, strided points and a strided, offset output,
// dropped and partly negative rows, N == 0, V == 0; all 8 flag sets of gd3d_pillar_decorate_cpu over the shapes of the tests with
// num_points 0, P and above P and NaN in the padded slots.  Prints OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gd3d.h"

namespace {

int fails = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++fails;
  }
}

template <class T>
T* block(size_t n) {   // exactly n elements (at least one byte, so that the pointer is a real block)
  return static_cast<T*>(std::malloc(n * sizeof(T) > 0 ? n * sizeof(T) : 1));
}

float rnd(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return (float)(s >> 8) / 16777216.0f;
}

int width_of(int flags, int C) {
  return 3 + ((flags & 1) ? 3 : 0) + ((flags & 2) ? 3 : 0) + ((flags & 4) ? 9 : 0) + ((flags & 8) ? 3 : 0) + ((flags & 16) ? 3 : 0) +
         ((flags & 32) ? 1 : 0) + ((flags & 64) ? C - 3 : 0);
}

template <class I>
void run_stats(int64_t N, int64_t V, int ndim, int C, int64_t stride, bool wide) {
  uint32_t seed = 12345u + (uint32_t)N * 7u + (uint32_t)V;
  float* points = block<float>(N > 0 ? (size_t)((N - 1) * stride + C) : 0);   // the last row ends where its C columns end
  I* coors = block<I>((size_t)(N * ndim));
  int32_t* map = block<int32_t>((size_t)N);
  int32_t* counts = block<int32_t>((size_t)V);
  int32_t* order = block<int32_t>((size_t)N);
  int32_t* seg = block<int32_t>((size_t)(V + 1));
  for (int64_t v = 0; v < V; ++v) counts[v] = 0;
  for (int64_t i = 0; i < N; ++i) {
    for (int c = 0; c < C; ++c) points[i * stride + c] = rnd(seed) * 10.0f - 5.0f;
    const bool drop = V == 0 || i % 7 == 3;
    map[i] = drop ? -1 : (int32_t)((i * 5) % V);
    for (int c = 0; c < ndim; ++c) coors[i * ndim + c] = drop ? (I)(c == 1 && i % 2 ? 4 : -1) : (I)((map[i] + c) % 50);
    if (!drop) ++counts[map[i]];
  }
  int64_t at = 0;
  for (int64_t i = 0; i < N; ++i)
    if (map[i] < 0) order[at++] = (int32_t)i;
  for (int64_t v = 0; v < V; ++v) {
    seg[v] = (int32_t)at;
    for (int64_t i = 0; i < N; ++i)
      if (map[i] == v) order[at++] = (int32_t)i;
  }
  seg[V] = (int32_t)at;
  const float vs[3] = {0.2f, 0.25f, 4.0f}, off[3] = {0.1f, -39.875f, -1.0f};
  for (int flags = 0; flags < 128; ++flags) {
    const int W = width_of(flags, C);
    const int64_t ostride = wide ? W + 5 : W;
    const int col = wide ? 2 : 0;
    float* out = block<float>(N > 0 ? (size_t)((N - 1) * ostride + col + W) : 0);
    float* table = block<float>((size_t)(V * ((flags & 4) ? 12 : 3)));
    const int rc = gd3d_point_voxel_stats_cpu(points, N, stride, C, coors, sizeof(I) == 8, ndim, map, counts, order, seg, V, vs, off,
                                              flags, (flags & 7) ? table : nullptr, out + col, ostride);
    expect(rc == 0, "gd3d_point_voxel_stats_cpu returned an error");
    if (rc == 0 && N > 0) {
      expect(out[col] == points[0], "column 0 is x");
      if (flags & 32) expect(out[col + W - 1 - ((flags & 64) ? C - 3 : 0)] == (map[0] < 0 ? 0.0f : (float)counts[map[0]]), "the count column");
    }
    std::free(out);
    std::free(table);
  }
  std::free(points); std::free(coors); std::free(map); std::free(counts); std::free(order); std::free(seg);
}

void run_deco(int64_t V, int P, int C) {
  uint32_t seed = 99u + (uint32_t)V + (uint32_t)P * 31u;
  float* feats = block<float>((size_t)(V * P * C));
  int32_t* num = block<int32_t>((size_t)V);
  int32_t* coors = block<int32_t>((size_t)(V * 4));
  for (int64_t v = 0; v < V; ++v) {
    num[v] = v == 0 ? P : (v == 1 ? 0 : (v == 2 ? P + 2 : (int32_t)(rnd(seed) * (float)(P + 1))));
    for (int c = 0; c < 4; ++c) coors[v * 4 + c] = (int32_t)(rnd(seed) * 400.0f);
    for (int p = 0; p < P; ++p)
      for (int c = 0; c < C; ++c) feats[(v * P + p) * C + c] = p < num[v] ? rnd(seed) * 70.0f : NAN;
  }
  const float vs[3] = {0.16f, 0.16f, 4.0f}, off[3] = {0.08f, -39.6f, -1.0f};
  for (int flags = 0; flags < 8; ++flags) {
    const int W = C + ((flags & 1) ? 3 : 0) + ((flags & 2) ? 3 : 0) + ((flags & 4) ? 1 : 0);
    float* out = block<float>((size_t)(V * P * W));
    const int rc = gd3d_pillar_decorate_cpu(feats, num, coors, V, P, C, vs, off, flags, out);
    expect(rc == 0, "gd3d_pillar_decorate_cpu returned an error");
    for (int64_t i = 0; rc == 0 && i < V * P * W; ++i)
      if (std::isnan(out[i])) {
        expect(false, "a NaN of a padded slot leaked into the output");
        break;
      }
    std::free(out);
  }
  std::free(feats); std::free(num); std::free(coors);
}

}  // namespace

int main() {
  run_stats<int32_t>(0, 0, 4, 3, 3, false);
  run_stats<int32_t>(1, 1, 3, 3, 3, false);
  run_stats<int32_t>(37, 0, 4, 4, 4, false);          // every point dropped
  run_stats<int32_t>(131, 23, 4, 5, 5, false);
  run_stats<int64_t>(131, 23, 3, 5, 8, true);         // int64 rows, strided points, a strided output at a column offset
  run_stats<int64_t>(300, 1, 4, 3, 4, true);          // one voxel
  const int shapes[][3] = {{0, 5, 4}, {1, 1, 3}, {3, 20, 4}, {40, 32, 4}, {17, 33, 5}, {5, 100, 5}};
  for (const auto& s : shapes) run_deco(s[0], s[1], s[2]);
  float dummy = 0.0f;
  const float g[3] = {1.0f, 1.0f, 1.0f};
  expect(gd3d_point_voxel_stats_cpu(&dummy, 1, 2, 3, nullptr, 0, 4, nullptr, nullptr, nullptr, nullptr, 0, g, g, 0, nullptr, &dummy, 3) ==
             GD3D_E_BADARG, "row_stride < C must be refused");
  expect(gd3d_pillar_decorate_cpu(&dummy, nullptr, nullptr, 1, 0, 4, g, g, 0, &dummy) == GD3D_E_BADARG, "P < 1 must be refused");
  expect(gd3d_pillar_decorate_cpu(&dummy, nullptr, nullptr, 1, 4, 4, g, g, 8, &dummy) == GD3D_E_BADARG, "an unknown flag must be refused");
  if (fails == 0) std::printf("OK\n");
  return fails == 0 ? 0 : 1;
}
