// pillar_feat_common.h — what csrc/pillar_feat.hip (gfx950 kernels) and csrc/pillar_feat_cpu.cpp (their `_cpu` twins) share: the
// column layout of the two outputs, the argument checks, and the PER-ELEMENT code — one output element of gd3d_point_voxel_stats
// from the (voxel, 3 | 12) table, one output element of gd3d_pillar_decorate from its voxel's mean — plus the fixed-order walks
// that fill the table and the mean.  Both units are compiled with -ffp-contract=off and correctly rounded division and square root:
// every multiply, add, subtract, divide and root below rounds on its own, on both targets, so every output is the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gd3d.h"

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define PF_HD __host__ __device__ __forceinline__
#else
#define PF_HD inline
#endif

namespace pillar_feat {

constexpr int BLOCK = 256;               // threads of a workgroup, every kernel
constexpr int MAX_C = 256;               // columns of a point / slot row
constexpr int STATS_ROWS = 64;           // point rows a workgroup of the point-ordered launch writes (a multiple of 4)
constexpr int DECO_MAX_GV = 64;          // voxels a workgroup of the decoration launch owns, at most
constexpr int DECO_ELEMS = 4096;         // output elements a workgroup of the decoration launch aims at

// ---- gd3d_point_voxel_stats ------------------------------------------------------------------------------------------------------

struct StatsArgs {
  const float* points;      // (N, >= C) rows, `stride` floats apart; columns 0, 1, 2 = x, y, z
  long long n, stride;
  const void* coors;        // (N, ndim) int32 or int64; the last three columns are z, y, x
  int coors64, ndim;
  const int32_t *map, *counts, *order, *seg;
  long long v;
  float vs[3], off[3];      // x, y, z
  const float* table;       // (V, ts): the voxel's mean xyz, then (ts == 12) its covariance
  int ts;
  int start[9];             // first output column of: xyz, c, d, cov, ctr, xyz - ctr, count, features; start[8] = the width
  float* out;
  long long out_stride;
};

// the layout from the flags and C; returns the width
inline int stats_layout(int32_t flags, int32_t C, int* start) {
  const int len[8] = {3,
                      (flags & GD3D_PVS_CLUSTER_CENTER) ? 3 : 0,
                      (flags & GD3D_PVS_CLUSTER_OFFSET) ? 3 : 0,
                      (flags & GD3D_PVS_COVARIANCE) ? 9 : 0,
                      (flags & GD3D_PVS_VOXEL_CENTER) ? 3 : 0,
                      (flags & GD3D_PVS_VOXEL_OFFSET) ? 3 : 0,
                      (flags & GD3D_PVS_POINT_COUNT) ? 1 : 0,
                      (flags & GD3D_PVS_APPEND) ? C - 3 : 0};
  start[0] = 0;
  for (int k = 0; k < 8; ++k) start[k + 1] = start[k] + len[k];
  return start[8];
}

inline bool stats_needs_table(int32_t flags) {
  return (flags & (GD3D_PVS_CLUSTER_CENTER | GD3D_PVS_CLUSTER_OFFSET | GD3D_PVS_COVARIANCE)) != 0;
}

// the checks both entry points make before they touch anything; fills everything of `a` but the pointers' targets
inline int stats_make(const float* points, int64_t N, int64_t row_stride, int32_t C, const void* coors, int32_t coors_is_int64,
                      int32_t ndim, const int32_t* map, const int32_t* counts, const int32_t* order, const int32_t* seg, int64_t V,
                      const float* voxel_size, const float* offset, int32_t flags, float* table, float* out, int64_t out_stride,
                      StatsArgs* a) {
  if (N < 0 || V < 0 || V > N || C < 3 || row_stride < C || ndim < 3 || voxel_size == nullptr || offset == nullptr) return GD3D_E_BADARG;
  if ((flags & ~GD3D_PVS_ALL) != 0) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || C > MAX_C || ndim > 8) return GD3D_E_TOOLARGE;
  const int width = stats_layout(flags, C, a->start);
  if (out_stride < width) return GD3D_E_BADARG;
  a->points = points; a->n = N; a->stride = row_stride;
  a->coors = coors; a->coors64 = coors_is_int64 != 0; a->ndim = ndim;
  a->map = map; a->counts = counts; a->order = order; a->seg = seg; a->v = V;
  for (int k = 0; k < 3; ++k) {
    a->vs[k] = voxel_size[k];
    a->off[k] = offset[k];
  }
  a->table = table; a->ts = (flags & GD3D_PVS_COVARIANCE) ? 12 : 3;
  a->out = out; a->out_stride = out_stride;
  if (N == 0) return 0;
  if (points == nullptr || out == nullptr) return GD3D_E_BADARG;
  if ((flags & (GD3D_PVS_VOXEL_CENTER | GD3D_PVS_VOXEL_OFFSET)) != 0 && coors == nullptr) return GD3D_E_BADARG;
  if ((stats_needs_table(flags) || (flags & GD3D_PVS_POINT_COUNT) != 0) && map == nullptr) return GD3D_E_BADARG;
  if ((flags & GD3D_PVS_POINT_COUNT) != 0 && V > 0 && counts == nullptr) return GD3D_E_BADARG;
  if (stats_needs_table(flags) && V > 0 && (order == nullptr || seg == nullptr || table == nullptr)) return GD3D_E_BADARG;
  return 0;
}

// the voxel of point i, or -1 for a dropped point (a map entry outside [0, V) counts as dropped)
PF_HD long long stats_voxel(const StatsArgs& a, long long i) {
  const long long m = a.map[i];
  return (m >= 0 && m < a.v) ? m : -1;
}

// centre of the point's own cell on axis k (0 = x: the LAST coors column): one conversion, one multiply, one add
PF_HD float stats_centre(const StatsArgs& a, long long i, int k) {
  const long long at = i * a.ndim + (a.ndim - 1 - k);
  const float c = a.coors64 ? (float)((const int64_t*)a.coors)[at] : (float)((const int32_t*)a.coors)[at];
  const float scaled = c * a.vs[k];
  return scaled + a.off[k];
}

// output element (point i, column col): the torch statements of PointVoxelStatsCalculator.forward, one element at a time
PF_HD float stats_element(const StatsArgs& a, long long i, int col) {
  const float* p = a.points + i * a.stride;
  if (col < a.start[1]) return p[col];
  if (col < a.start[2]) {                                       // c
    const long long m = stats_voxel(a, i);
    return m >= 0 ? a.table[m * a.ts + (col - a.start[1])] : 0.0f;
  }
  if (col < a.start[3]) {                                       // d = xyz - c
    const int k = col - a.start[2];
    const long long m = stats_voxel(a, i);
    const float c = m >= 0 ? a.table[m * a.ts + k] : 0.0f;
    return p[k] - c;
  }
  if (col < a.start[4]) {                                       // covariance
    const long long m = stats_voxel(a, i);
    return m >= 0 ? a.table[m * a.ts + 3 + (col - a.start[3])] : 0.0f;
  }
  if (col < a.start[5]) return stats_centre(a, i, col - a.start[4]);
  if (col < a.start[6]) {
    const int k = col - a.start[5];
    return p[k] - stats_centre(a, i, k);
  }
  if (col < a.start[7]) {
    const long long m = stats_voxel(a, i);
    return m >= 0 ? (float)a.counts[m] : 0.0f;
  }
  return p[3 + (col - a.start[7])];
}

// The run of `order` that voxel v owns, cut to [0, n]; a point id outside [0, n) adds nothing (never read).
PF_HD void stats_run(const StatsArgs& a, long long v, int* b, int* e) {
  int lo = a.seg[v], hi = a.seg[v + 1];
  lo = lo < 0 ? 0 : lo;
  hi = (long long)hi > a.n ? (int)a.n : hi;
  *b = lo;
  *e = hi > lo ? hi : lo;
}

// ---- gd3d_pillar_decorate --------------------------------------------------------------------------------------------------------

struct DecoArgs {
  const float* features;    // (V, P, C)
  const int32_t *num_points, *coors;   // (V), (V, 4) = (b, z, y, x)
  long long v;
  int P, C;
  float vs[3], off[3];
  int flags, width;
  float* out;               // (V, P, width)
};

inline int deco_width(int32_t flags, int32_t C) {
  return C + ((flags & GD3D_PD_CLUSTER_CENTER) ? 3 : 0) + ((flags & GD3D_PD_VOXEL_CENTER) ? 3 : 0) + ((flags & GD3D_PD_DISTANCE) ? 1 : 0);
}

inline int deco_make(const float* features, const int32_t* num_points, const int32_t* coors, int64_t V, int32_t P, int32_t C,
                     const float* voxel_size, const float* offset, int32_t flags, float* out, DecoArgs* a) {
  if (V < 0 || P < 1 || C < 3 || voxel_size == nullptr || offset == nullptr || (flags & ~GD3D_PD_ALL) != 0) return GD3D_E_BADARG;
  if (V > 0x7fffffffLL || C > MAX_C || (long long)P * (C + 7) > (1LL << 30)) return GD3D_E_TOOLARGE;
  a->features = features; a->num_points = num_points; a->coors = coors; a->v = V; a->P = P; a->C = C;
  for (int k = 0; k < 3; ++k) {
    a->vs[k] = voxel_size[k];
    a->off[k] = offset[k];
  }
  a->flags = flags; a->width = deco_width(flags, C); a->out = out;
  if (V == 0) return 0;
  if (features == nullptr || num_points == nullptr || out == nullptr) return GD3D_E_BADARG;
  if ((flags & GD3D_PD_VOXEL_CENTER) != 0 && coors == nullptr) return GD3D_E_BADARG;
  return 0;
}

// the slots of voxel v that hold points: min(max(num_points, 0), P)
PF_HD int deco_slots(const DecoArgs& a, long long v) {
  const int n = a.num_points[v];
  return n < 0 ? 0 : (n > a.P ? a.P : n);
}

// mean of column k over the voxel's n filled slots: slots 0, 1, 2, .. added in sequence to +0, then one division (n >= 1)
PF_HD float deco_mean(const DecoArgs& a, long long v, int n, int k) {
  const float* f = a.features + v * a.P * a.C + k;
  float acc = 0.0f;
  int s = 0;
  for (; s + 4 <= n; s += 4) {                                  // four independent loads in flight, added in slot order
    const float x0 = f[(long long)s * a.C], x1 = f[(long long)(s + 1) * a.C], x2 = f[(long long)(s + 2) * a.C],
                x3 = f[(long long)(s + 3) * a.C];
    acc += x0; acc += x1; acc += x2; acc += x3;
  }
  for (; s < n; ++s) acc += f[(long long)s * a.C];
  return acc / (float)n;
}

// output element (voxel v, slot p < n, column col); `mean` = the voxel's three means (read for the f_cluster columns only)
PF_HD float deco_element(const DecoArgs& a, long long v, int p, int col, const float* mean) {
  const float* f = a.features + (v * a.P + p) * a.C;
  if (col < a.C) return f[col];
  col -= a.C;
  if ((a.flags & GD3D_PD_CLUSTER_CENTER) != 0) {
    if (col < 3) return f[col] - mean[col];
    col -= 3;
  }
  if ((a.flags & GD3D_PD_VOXEL_CENTER) != 0) {
    if (col < 3) {
      const float c = (float)a.coors[v * 4 + 3 - col];
      const float scaled = c * a.vs[col];
      const float centre = scaled + a.off[col];
      return f[col] - centre;
    }
    col -= 3;
  }
  const float xx = f[0] * f[0], yy = f[1] * f[1], zz = f[2] * f[2];
  const float xy = xx + yy;
  return sqrtf(xy + zz);
}

}  // namespace pillar_feat
