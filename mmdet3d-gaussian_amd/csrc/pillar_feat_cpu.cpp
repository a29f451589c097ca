// pillar_feat_cpu.cpp — the `_cpu` twins of the pillar encoders' point decoration (include/gd3d.h, gd3d_point_voxel_stats_cpu /
// gd3d_pillar_decorate_cpu).  Plain loops: voxel by voxel for the table (the voxel's points in ascending point index, added in
// sequence to +0, one division; then the covariance over d = xyz - the rounded mean), then point by point, column by column through
// the per-element source of csrc/pillar_feat_common.h, which csrc/pillar_feat.hip compiles for the device (both units with
// -ffp-contract=off): every output is the kernels' bits.  Host memory in and out, no stream, no HIP call, one thread.
#define GD3D_HOST_TWIN 1
#include "pillar_feat_common.h"

#include "../../include/gd3d.h"

using namespace pillar_feat;

namespace {

// column k of the run's points added in sequence to +0
float sum_column(const StatsArgs& a, int b, int e, int k) {
  float acc = 0.0f;
  for (int j = b; j < e; ++j) {
    const int pid = a.order[j];
    if (pid < 0 || pid >= a.n) continue;
    acc += a.points[(long long)pid * a.stride + k];
  }
  return acc;
}

// (x_ka - ca) * (x_kb - cb) of the run's points added in sequence to +0
float sum_product(const StatsArgs& a, int b, int e, int ka, float ca, int kb, float cb) {
  float acc = 0.0f;
  for (int j = b; j < e; ++j) {
    const int pid = a.order[j];
    if (pid < 0 || pid >= a.n) continue;
    const float* p = a.points + (long long)pid * a.stride;
    const float da = p[ka] - ca, db = p[kb] - cb;
    const float prod = da * db;
    acc += prod;
  }
  return acc;
}

}  // namespace

extern "C" {

int gd3d_point_voxel_stats_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const void* coors,
                               int32_t coors_is_int64, int32_t ndim, const int32_t* map, const int32_t* counts, const int32_t* order,
                               const int32_t* seg, int64_t V, const float* voxel_size, const float* offset, int32_t flags,
                               float* table, float* out, int64_t out_stride) {
  StatsArgs a;
  const int rc = stats_make(points, N, row_stride, C, coors, coors_is_int64, ndim, map, counts, order, seg, V, voxel_size, offset,
                            flags, table, out, out_stride, &a);
  if (rc != 0 || N == 0) return rc;
  if (stats_needs_table(flags)) {
    for (int64_t v = 0; v < V; ++v) {
      int b, e;
      stats_run(a, v, &b, &e);
      const float cnt = (float)(e - b);
      float* row = table + v * a.ts;
      for (int k = 0; k < 3; ++k) row[k] = sum_column(a, b, e, k) / cnt;
      if (a.ts == 12)
        for (int ka = 0; ka < 3; ++ka)
          for (int kb = 0; kb < 3; ++kb) row[3 + ka * 3 + kb] = sum_product(a, b, e, ka, row[ka], kb, row[kb]) / cnt;
    }
  }
  const int W = a.start[8];
  for (int64_t i = 0; i < N; ++i)
    for (int col = 0; col < W; ++col) out[i * out_stride + col] = stats_element(a, i, col);
  return 0;
}

int gd3d_pillar_decorate_cpu(const float* features, const int32_t* num_points, const int32_t* coors, int64_t V, int32_t P, int32_t C,
                             const float* voxel_size, const float* offset, int32_t flags, float* out) {
  DecoArgs a;
  const int rc = deco_make(features, num_points, coors, V, P, C, voxel_size, offset, flags, out, &a);
  if (rc != 0 || V == 0) return rc;
  for (int64_t v = 0; v < V; ++v) {
    const int n = deco_slots(a, v);
    float mean[3] = {0.0f, 0.0f, 0.0f};
    if ((flags & GD3D_PD_CLUSTER_CENTER) != 0 && n > 0)
      for (int k = 0; k < 3; ++k) mean[k] = deco_mean(a, v, n, k);
    for (int p = 0; p < P; ++p) {
      float* row = out + (v * P + p) * a.width;
      for (int col = 0; col < a.width; ++col) row[col] = p < n ? deco_element(a, v, p, col, mean) : 0.0f;
    }
  }
  return 0;
}

}  // extern "C"
