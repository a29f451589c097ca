// hard_voxel_common.h — what csrc/hard_voxel.hip (gfx950 kernels) and csrc/hard_voxel_cpu.cpp (their `_cpu` twins) share: the cell of
// a point (mmdet3d's `hard_voxelize` / `dynamic_voxelize`, restated in include/gd3d.h), the argument checks, the row bound and the
// sample of a stacked point.  Both units are compiled with -ffp-contract=off and with correctly rounded division, so a point falls in
// the same cell on both targets.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gd3d.h"

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define HV_HD __host__ __device__ __forceinline__
#else
#define HV_HD inline
#endif

namespace hard_voxel {

constexpr int BLOCK = 256;                   // threads of a workgroup, every kernel
constexpr int64_t MAX_SIDE = 1LL << 24;      // cells per axis: (float)grid and the comparison against it are exact up to here
constexpr int MAX_B = 1024;                  // samples per call (the kernels keep a word per sample in LDS)
constexpr int MAX_C = 256;                   // columns of a point row that are copied
constexpr int64_t MAX_KEY = 1LL << 62;       // B * G, the dropped points' key, must stay below this

struct Geometry {
  float vs[3], lo[3];      // x, y, z
  float gf[3];             // the grid as fp32 (exact: grid <= 2^24)
  int64_t gx, gy, gz, G;   // cells per axis and per sample
};

// the checks every entry point makes before it touches anything; fills `g`
inline int make_geometry(const float* voxel_size, const float* range_min, const int32_t* grid_size, int64_t N, int32_t B, Geometry* g) {
  if (N < 0 || B < 0 || voxel_size == nullptr || range_min == nullptr || grid_size == nullptr) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  for (int j = 0; j < 3; ++j) {
    if (!(voxel_size[j] > 0.0f) || !(range_min[j] == range_min[j]) || grid_size[j] < 1) return GD3D_E_BADARG;
    if (grid_size[j] > MAX_SIDE) return GD3D_E_TOOLARGE;
    g->vs[j] = voxel_size[j];
    g->lo[j] = range_min[j];
    g->gf[j] = (float)grid_size[j];
  }
  g->gx = grid_size[0]; g->gy = grid_size[1]; g->gz = grid_size[2];
  g->G = g->gx * g->gy;                                           // < 2^48
  long long all = 0;
  if (__builtin_mul_overflow((long long)g->G, (long long)g->gz, &all)) return GD3D_E_TOOLARGE;
  g->G = all;
  if (__builtin_mul_overflow(all, (long long)(B > 0 ? B : 1), &all) || all >= MAX_KEY) return GD3D_E_TOOLARGE;
  return 0;
}

// rows of every per-voxel output: min(N, B * max_voxels)
inline int64_t row_bound(int64_t N, int32_t B, int32_t max_voxels) {
  const int64_t cap = (int64_t)B * (int64_t)max_voxels;
  return N < cap ? N : cap;
}

// The cell of point p on one axis: one subtraction, one correctly rounded division, one floor, in fp32.  Compared as a FLOAT before
// any conversion: NaN fails the comparison, +-inf and 1e30 fail it, so the conversion that follows sees [0, grid) only.
HV_HD bool axis_cell(float p, float lo, float vs, float gf, int32_t* c) {
  const float f = floorf((p - lo) / vs);
  const bool in = f >= 0.0f && f < gf;
  *c = in ? (int32_t)f : -1;
  return in;
}

// (x, y, z) cell of a point; false: the point is dropped
HV_HD bool cell_of(const float* p, const Geometry& g, int32_t* x, int32_t* y, int32_t* z) {
  const bool a = axis_cell(p[0], g.lo[0], g.vs[0], g.gf[0], x);
  const bool b = axis_cell(p[1], g.lo[1], g.vs[1], g.gf[1], y);
  const bool c = axis_cell(p[2], g.lo[2], g.vs[2], g.gf[2], z);
  return a && b && c;
}

// the key of cell (z, y, x) inside its sample: (z * Gy + y) * Gx + x
HV_HD int64_t cell_key(const Geometry& g, int32_t x, int32_t y, int32_t z) { return ((int64_t)z * g.gy + y) * g.gx + x; }

// The sample of stacked row i: the first b with i < cnt[0] + .. + cnt[b] (negative counts count as 0); -1 past the last sample.
// B is a batch size: a short loop over values every lane reads alike.
HV_HD int32_t sample_of(int64_t i, const int32_t* cnt, int32_t B) {
  int64_t end = 0;
  for (int32_t b = 0; b < B; ++b) {
    end += cnt[b] > 0 ? cnt[b] : 0;
    if (i < end) return b;
  }
  return -1;
}

}  // namespace hard_voxel
