// view_net_common.h — what csrc/view_net.hip (gfx950 kernels) and csrc/view_net_cpu.cpp (their `_cpu` twins) share: the per-element
// source of the multi-view pillar encoder's view ops (include/gd3d.h, gd3d_multi_view_voxelize / gd3d_pillar_scatter* /
// gd3d_view_sample*) —
//   * the `to_cylindrical` / `to_spherical` transforms of models/detectors/pillar_od.py:24-70 as ONE sequence of fp32 operations
//     each (correctly rounded sqrt, the fixed-sequence fx_atan2f of csrc/rbox_device.h), followed by the cell of the transformed point
//     (csrc/hard_voxel_common.h's cell_of, unchanged) in the reference's coors layout: the sample id in every row of a sample;
//   * the cell of a voxel row on the dense pillar canvas (mmdet3d's PointPillarsScatter, restated);
//   * the grid normalisation of SingleViewNet.forward (models/voxel_encoders/pillar_mvf_encoder.py:88-91) and ATen's
//     F.grid_sample(align_corners=False, padding_mode='zeros') unnormalisation, neighbours and weights, in their order.
// Both units are compiled with -ffp-contract=off and with correctly rounded division and sqrt, so every decision and every forward
// value is the same bits on both targets.  csrc/vsa_bev_common.h lends the neighbour record, the bilinear sum's order, the lanes of a
// row and the strides of a dense map.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rbox_device.h"   // fx_atan2f; under GD3D_HOST_TWIN: the same source for the host
#include "hard_voxel_common.h"
#include "vsa_bev_common.h"

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define VN_HD __device__ __forceinline__
#else
#define VN_HD inline
#endif

namespace view_net {

constexpr int BLOCK = 256;                  // threads of a workgroup, every kernel
constexpr int QUAD = 4;                     // channels a lane takes at a time on the 16-byte path
constexpr int TILE = 64;                    // voxels and channels of the LDS tile of the NCHW canvas kernels
constexpr int MAX_VIEWS = 4;
constexpr int MAX_C = 256;                  // columns of a point row that are copied
constexpr int64_t MAX_SIDE = 1LL << 24;     // H, W, ny, nx: (float)n and the comparisons against it are exact up to here
constexpr int64_t MAX_ROWS = 0x7fffffffLL;  // points / voxels per call

// ---- the view transforms -----------------------------------------------------------------------------------------------------------

struct View {
  int kind;                 // GD3D_VIEW_*
  hard_voxel::Geometry g;   // of this view's voxelizer; unused when coors is null
  float* pts;               // (N, C) transformed rows, nullable
  int32_t* coors;           // (N, 4) [b, z, y, x], nullable
};

struct VoxArgs {
  const float* points;      // row i at points + i * stride
  long long n, stride;
  int C;
  const int32_t* cnt;       // (B) rows per sample
  int B, nviews;
  View v[MAX_VIEWS];
};

// the checks of gd3d_multi_view_voxelize and of its twin: nothing is touched before they pass; fills `a`
inline int make_vox_args(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* cnt, int32_t B, int32_t num_views,
                         const int32_t* kinds, const float* voxel_sizes, const float* range_mins, const int32_t* grid_sizes,
                         float* const* view_points, int32_t* const* view_coors, VoxArgs* a) {
  if (N < 0 || B < 0 || C < 3 || row_stride < C || num_views < 1 || num_views > MAX_VIEWS || kinds == nullptr || view_points == nullptr ||
      view_coors == nullptr)
    return GD3D_E_BADARG;
  if (N > MAX_ROWS || C > MAX_C || B > hard_voxel::MAX_B) return GD3D_E_TOOLARGE;
  for (int k = 0; k < num_views; ++k) {
    View& v = a->v[k];
    v.kind = kinds[k];
    v.pts = view_points[k];
    v.coors = view_coors[k];
    if (v.kind != GD3D_VIEW_CARTESIAN && v.kind != GD3D_VIEW_CYLINDRICAL && v.kind != GD3D_VIEW_SPHERICAL) return GD3D_E_BADARG;
    if (v.coors != nullptr) {
      if (voxel_sizes == nullptr || range_mins == nullptr || grid_sizes == nullptr) return GD3D_E_BADARG;
      const int rc = hard_voxel::make_geometry(voxel_sizes + 3 * k, range_mins + 3 * k, grid_sizes + 3 * k, N, B, &v.g);
      if (rc != 0) return rc;
    } else {
      v.g = hard_voxel::Geometry();
    }
  }
  if (N > 0 && (points == nullptr || (B > 0 && cnt == nullptr))) return GD3D_E_BADARG;
  a->points = points; a->n = N; a->stride = row_stride; a->C = C; a->cnt = cnt; a->B = B; a->nviews = num_views;
  return 0;
}

// (x, y, z) in the view's coordinates, each step ONE fp32 operation:
//   cylindrical: s = x*x + y*y, rho = sqrt(s), phi = fx_atan2f(y, x)                          -> (phi, z, rho)
//   spherical  : s2 = x*x + y*y, r2 = sqrt(s2), rho = sqrt(s2 + z*z), yaw = fx_atan2f(y, x),
//                pitch = fx_atan2f(z, r2)  (the reference's asin(z / rho), NaN at the origin, restated)  -> (yaw, pitch, rho)
VN_HD void transform(int kind, float x, float y, float z, float* t) {
  if (kind == GD3D_VIEW_CARTESIAN) {
    t[0] = x; t[1] = y; t[2] = z;
    return;
  }
  const float xx = x * x, yy = y * y;
  const float s = xx + yy;
  const float ang = rbox::fx_atan2f(y, x);
  if (kind == GD3D_VIEW_CYLINDRICAL) {
    t[0] = ang; t[1] = z; t[2] = sqrtf(s);
    return;
  }
  const float r2 = sqrtf(s), zz = z * z;
  t[0] = ang; t[1] = rbox::fx_atan2f(z, r2); t[2] = sqrtf(s + zz);
}

// everything the launch writes for stacked row i
VN_HD void voxelize_point(const VoxArgs& a, long long i) {
  const float* p = a.points + i * a.stride;
  const float x = p[0], y = p[1], z = p[2];
  const int32_t b = hard_voxel::sample_of(i, a.cnt, a.B);
  for (int k = 0; k < a.nviews; ++k) {
    const View& v = a.v[k];
    float t[3];
    transform(v.kind, x, y, z, t);
    if (v.pts != nullptr) {
      float* row = v.pts + i * a.C;
      row[0] = t[0]; row[1] = t[1]; row[2] = t[2];
      for (int c = 3; c < a.C; ++c) row[c] = p[c];
    }
    if (v.coors != nullptr) {
      int32_t cx, cy, cz;
      const bool in = hard_voxel::cell_of(t, v.g, &cx, &cy, &cz);    // false for a non-finite transformed coordinate too
      int32_t* c = v.coors + i * 4;
      c[0] = b;                                                       // -1: a row of no sample
      c[1] = (in && b >= 0) ? cz : -1;
      c[2] = (in && b >= 0) ? cy : -1;
      c[3] = (in && b >= 0) ? cx : -1;
    }
  }
}

// ---- the pillar canvas -------------------------------------------------------------------------------------------------------------

struct CanvasArgs {
  const float* src;          // forward: voxel_features (V, C); backward: grad_canvas
  float* dst;                // forward: the canvas; backward: grad_features (V, C)
  const void* coors;         // (V, ncol) int32 or int64
  int is64, ncol;            // ncol 4: [b, z, y, x]; 3: [z, y, x], b = 0
  long long V, C, B, ny, nx;
  long long sB, sC, sH, sW;  // element strides of the canvas
};

inline int check_canvas(int32_t ncol, int32_t layout, int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx) {
  if (V < 0 || C < 1 || B < 0 || ny < 1 || nx < 1 || (ncol != 3 && ncol != 4) || (layout != 0 && layout != 1)) return GD3D_E_BADARG;
  if (ncol == 3 && B > 1) return GD3D_E_BADARG;
  if (V > MAX_ROWS || ny > MAX_SIDE || nx > MAX_SIDE) return GD3D_E_TOOLARGE;
  long long all = 0;
  if (__builtin_mul_overflow((long long)ny, (long long)nx, &all) || __builtin_mul_overflow(all, (long long)C, &all) ||
      __builtin_mul_overflow(all, (long long)(B > 0 ? B : 1), &all) || all >= (1LL << 60))
    return GD3D_E_TOOLARGE;
  return 0;
}

VN_HD long long coor_at(const void* coors, int is64, long long i) {
  return is64 ? (long long)static_cast<const int64_t*>(coors)[i] : (long long)static_cast<const int32_t*>(coors)[i];
}

// the element offset of channel 0 of voxel row v's cell, -1 for a row outside the canvas (b, y or x out of range): compared as
// 64-bit integers, the z column is not read
VN_HD long long canvas_cell(const CanvasArgs& a, long long v) {
  const long long base = v * a.ncol;
  const long long b = a.ncol == 4 ? coor_at(a.coors, a.is64, base) : 0;
  const long long y = coor_at(a.coors, a.is64, base + a.ncol - 2), x = coor_at(a.coors, a.is64, base + a.ncol - 1);
  const bool in = b >= 0 && b < a.B && y >= 0 && y < a.ny && x >= 0 && x < a.nx;
  return in ? b * a.sB + y * a.sH + x * a.sW : -1;
}

// ---- the view-map sampling ---------------------------------------------------------------------------------------------------------

struct SampleArgs {
  const float* xyz;          // row n at xyz + n * xyz_stride: columns 0 (x) and 1 (y)
  long long xyz_stride;
  const void* ids;           // sample id of row n at ids[n * id_stride], int32 or int64
  int is64;
  long long id_stride;
  const float* map;          // forward: the view map
  const float* gout;         // backward: (N, C) upstream gradient
  long long sB, sC, sH, sW;  // element strides of the map / of its gradient
  long long N, B, C, H, W;
  float lo_x, half_x, lo_y, half_y;
  int L;                     // lanes per point
  float* out;                // forward: (N, C); backward: the map's gradient (or its channels-last workspace)
};

inline int check_sample(int64_t xyz_stride, int64_t id_stride, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W,
                        float lo_x, float half_x, float lo_y, float half_y) {
  if (N < 0 || B < 0 || C < 1 || H < 1 || W < 1 || xyz_stride < 0 || id_stride < 0 || (layout != 0 && layout != 1) ||
      !(half_x > 0.0f) || !(half_y > 0.0f) || !(half_x < INFINITY) || !(half_y < INFINITY) || !(lo_x == lo_x) || !(lo_y == lo_y))
    return GD3D_E_BADARG;
  if (N > MAX_ROWS || H > MAX_SIDE || W > MAX_SIDE) return GD3D_E_TOOLARGE;
  long long all = 0;
  if (__builtin_mul_overflow((long long)H, (long long)W, &all) || __builtin_mul_overflow(all, (long long)C, &all) ||
      __builtin_mul_overflow(all, (long long)(B > 0 ? B : 1), &all) || all >= (1LL << 60))
    return GD3D_E_TOOLARGE;
  return 0;
}

// the pixel coordinate of v on an axis of n cells over [lo, lo + 2 * half): the reference's grid statement, then ATen's unnormalize
// for align_corners=False, each step ONE fp32 operation:  g = (v - lo) / half - 1;  pix = ((g + 1) * (float)n - 1) / 2
VN_HD float pixel_coord(float v, float lo, float half, int64_t n) {
  const float d = v - lo;
  const float q = d / half;
  const float g = q - 1.0f;
  const float u = g + 1.0f;
  const float m = u * (float)n;
  const float e = m - 1.0f;
  return e / 2.0f;
}

// The four neighbours of point (x, y) of sample b, in the fixed order nw, ne, sw, se, with ATen's weights
//   nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy), sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0),  x1 = x0 + 1.
// The float-to-int conversions happen only after the comparisons have confined both coordinates to (-1, n): NaN fails every
// comparison, +-inf and anything a cell or more outside fail one; a sample id outside [0, B) fails too.  Such a point gets four
// unused neighbours (a zero row, no gradient).  No index leaves the map for any input.
VN_HD vsa_bev::Taps make_taps(const SampleArgs& a, float x, float y, long long b) {
  vsa_bev::Taps t;
  const float ix = pixel_coord(x, a.lo_x, a.half_x, a.W), iy = pixel_coord(y, a.lo_y, a.half_y, a.H);
  const bool reach = ix > -1.0f && ix < (float)a.W && iy > -1.0f && iy < (float)a.H && b >= 0 && b < a.B;
  const float fx0 = reach ? floorf(ix) : 0.0f, fy0 = reach ? floorf(iy) : 0.0f;
  const float px = reach ? ix : 0.0f, py = reach ? iy : 0.0f;
  const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
  const float bx = fx1 - px, ax = px - fx0, by = fy1 - py, ay = py - fy0;
  const int64_t x0 = (int64_t)fx0, y0 = (int64_t)fy0;                        // in [-1, n - 1]
  t.w[0] = bx * by;
  t.w[1] = ax * by;
  t.w[2] = bx * ay;
  t.w[3] = ax * ay;
  for (int j = 0; j < 4; ++j) {
    const int64_t xj = x0 + (j & 1), yj = y0 + (j >> 1);
    t.use[j] = reach && xj >= 0 && xj < a.W && yj >= 0 && yj < a.H;
    t.off[j] = t.use[j] ? b * a.sB + yj * a.sH + xj * a.sW : 0;
  }
  return t;
}

VN_HD vsa_bev::Taps taps_of(const SampleArgs& a, long long n) {
  const float* p = a.xyz + n * a.xyz_stride;
  return make_taps(a, p[0], p[1], coor_at(a.ids, a.is64, n * a.id_stride));
}

}  // namespace view_net
