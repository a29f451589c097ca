// hard_voxel_cpu.cpp — the `_cpu` twins of hard voxelization, dynamic voxelization and the mean voxel encoder (include/gd3d.h,
// gd3d_hard_voxelize_cpu / gd3d_dynamic_voxelize_cpu / gd3d_voxel_mean_cpu).  The hard twin is the sequential walk of mmdet3d's
// published `hard_voxelize`, sample by sample, point by point, over a hash map from cell to voxel — an independent statement of the
// algorithm, not a copy of the kernels' sort path, and without mmdet3d's dense grid of cell -> voxel indices (360 MB at KITTI's grid).
// The cell of a point is the per-element source of csrc/hard_voxel_common.h, which csrc/hard_voxel.hip compiles for the device (both
// units with -ffp-contract=off): every output is the kernels' bits.  Host memory in and out, no stream, no HIP call, one thread.
#define GD3D_HOST_TWIN 1
#include "hard_voxel_common.h"

#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/gd3d.h"

using namespace hard_voxel;

namespace {

// slots 0, 1, 2, .. of one voxel added in sequence to +0, then one division; n == 0 gives zeros
void mean_row(const float* const* rows, int n, int F, float* out) {
  for (int f = 0; f < F; ++f) {
    float acc = 0.0f;
    for (int k = 0; k < n; ++k) acc += rows[k][f];
    out[f] = n > 0 ? acc / (float)n : 0.0f;
  }
}

}  // namespace

extern "C" {

int gd3d_hard_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                           const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t max_num_points,
                           int32_t max_voxels, int32_t num_features, void* workspace, float* voxels, float* mean, int32_t* coors,
                           int32_t* num_points, int32_t* voxel_batch_cnt, int64_t* num) {
  (void)workspace;
  Geometry g;
  const int rc = make_geometry(voxel_size, range_min, grid_size, N, B, &g);
  if (rc != 0) return rc;
  if (max_num_points < 1 || max_voxels < 1 || C < 3 || row_stride < C || num == nullptr) return GD3D_E_BADARG;
  if (mean != nullptr && (num_features < 1 || num_features > C)) return GD3D_E_BADARG;
  if (B > MAX_B || C > MAX_C) return GD3D_E_TOOLARGE;
  if (B > 0 && (points_batch_cnt == nullptr || voxel_batch_cnt == nullptr)) return GD3D_E_BADARG;
  num[0] = num[1] = 0;
  for (int32_t b = 0; b < B; ++b) voxel_batch_cnt[b] = 0;
  const int64_t rows = row_bound(N, B, max_voxels);
  if (rows == 0) return 0;
  if (points == nullptr || coors == nullptr || num_points == nullptr) return GD3D_E_BADARG;
  const int64_t P = max_num_points;
  if (voxels != nullptr)
    for (int64_t i = 0; i < rows * P * C; ++i) voxels[i] = 0.0f;
  if (mean != nullptr)
    for (int64_t i = 0; i < rows * num_features; ++i) mean[i] = 0.0f;
  for (int64_t v = 0; v < rows; ++v) {
    coors[v * 4] = coors[v * 4 + 1] = coors[v * 4 + 2] = coors[v * 4 + 3] = -1;
    num_points[v] = 0;
  }
  try {
    std::unordered_map<int64_t, int64_t> voxel_of;              // cell key -> row, one sample at a time
    std::vector<const float*> slots(mean != nullptr ? (size_t)(rows * P) : 0);   // the rows the mean adds, in slot order
    int64_t start = 0, total = 0, dropped = 0;
    for (int32_t b = 0; b < B; ++b) {
      int64_t end = start + (points_batch_cnt[b] > 0 ? points_batch_cnt[b] : 0);
      end = end < N ? end : N;
      voxel_of.clear();
      const int64_t base = total;
      int64_t voxel_num = 0;
      for (int64_t i = start; i < end; ++i) {
        const float* p = points + i * row_stride;
        int32_t x, y, z;
        if (!cell_of(p, g, &x, &y, &z)) {
          ++dropped;
          continue;
        }
        const int64_t key = cell_key(g, x, y, z);
        auto it = voxel_of.find(key);
        int64_t v;
        if (it == voxel_of.end()) {
          if (voxel_num >= max_voxels) continue;                // a `continue`: later points of numbered voxels still join them
          v = base + voxel_num++;
          voxel_of.emplace(key, v);
          coors[v * 4] = b; coors[v * 4 + 1] = z; coors[v * 4 + 2] = y; coors[v * 4 + 3] = x;
        } else {
          v = it->second;
        }
        const int64_t slot = num_points[v];
        if (slot >= P) continue;
        if (voxels != nullptr)
          for (int32_t c = 0; c < C; ++c) voxels[(v * P + slot) * C + c] = p[c];
        if (mean != nullptr) slots[(size_t)(v * P + slot)] = p;
        num_points[v] = (int32_t)(slot + 1);
      }
      voxel_batch_cnt[b] = (int32_t)voxel_num;
      total += voxel_num;
      start = end;
    }
    dropped += N - start;                                       // rows of no sample
    if (mean != nullptr)
      for (int64_t v = 0; v < total; ++v) mean_row(slots.data() + v * P, num_points[v], num_features, mean + v * num_features);
    num[0] = total;
    num[1] = dropped;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
  return 0;
}

int gd3d_dynamic_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, const int32_t* points_batch_cnt, int32_t B,
                              const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t* coors) {
  Geometry g;
  const int rc = make_geometry(voxel_size, range_min, grid_size, N, B, &g);
  if (rc != 0) return rc;
  if (row_stride < 3) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || coors == nullptr || (B > 0 && points_batch_cnt == nullptr)) return GD3D_E_BADARG;
  for (int64_t i = 0; i < N; ++i) {
    int32_t x, y, z;
    const int32_t b = sample_of(i, points_batch_cnt, B);
    const bool in = cell_of(points + i * row_stride, g, &x, &y, &z) && b >= 0;
    int32_t* c = coors + i * 4;
    c[0] = in ? b : -1; c[1] = in ? z : -1; c[2] = in ? y : -1; c[3] = in ? x : -1;
  }
  return 0;
}

int gd3d_voxel_mean_cpu(const float* voxels, const int32_t* num_points, int64_t V, int32_t P, int32_t C, int32_t num_features,
                        float* mean) {
  if (V < 0 || P < 1 || C < 1 || num_features < 1 || num_features > C) return GD3D_E_BADARG;
  if (V > 0x7fffffffLL || C > MAX_C) return GD3D_E_TOOLARGE;
  if (V == 0) return 0;
  if (voxels == nullptr || num_points == nullptr || mean == nullptr) return GD3D_E_BADARG;
  for (int64_t v = 0; v < V; ++v) {
    int n = num_points[v];
    n = n < 0 ? 0 : (n > P ? P : n);
    for (int32_t f = 0; f < num_features; ++f) {
      float acc = 0.0f;
      for (int k = 0; k < n; ++k) acc += voxels[(v * P + k) * C + f];
      mean[v * num_features + f] = n > 0 ? acc / (float)n : 0.0f;
    }
  }
  return 0;
}

}  // extern "C"
