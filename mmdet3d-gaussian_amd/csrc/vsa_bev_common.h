// vsa_bev_common.h — what csrc/vsa_bev.hip (gfx950 kernels) and csrc/vsa_bev_cpu.cpp (their `_cpu` twins) share: the per-element
// source of VoxelSetAbstraction's keypoint BEV interpolation (models/middle_encoders/voxel_set_abstraction.py:153-177: the grid
// normalisation and F.grid_sample(align_corners=True, padding_mode='zeros'), bilinear) and of its voxel centres (:179-193), as ONE
// sequence of fp32 operations each.  Both units are compiled with -ffp-contract=off and with correctly rounded division, so the
// pixel coordinates, the four weights, the interpolated values and the voxel centres are the same bits on both targets.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gd3d.h"

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define VB_HD __host__ __device__ __forceinline__
#else
#define VB_HD inline
#endif

namespace vsa_bev {

constexpr int BLOCK = 256;                  // threads of a workgroup, every kernel
constexpr int QUAD = 4;                     // channels a lane takes at a time on the 16-byte path
constexpr int64_t MAX_SIDE = 1LL << 24;     // H, W: (float)(n - 1) and the comparisons against (float)n are exact up to here

// the argument checks of both interpolation entry points and of their twins: nothing is touched before they pass
inline int check_interp(int64_t kp_stride_b, int64_t kp_stride_m, int32_t layout, int64_t B, int64_t M, int64_t C, int64_t H, int64_t W,
                        float tl_x, float tl_y, float br_x, float br_y) {
  if (B < 0 || M < 0 || C < 1 || H < 2 || W < 2 || kp_stride_b < 0 || kp_stride_m < 0 || (layout != 0 && layout != 1) ||
      !(br_x > tl_x) || !(br_y > tl_y))   // false for a NaN corner too
    return GD3D_E_BADARG;
  if (H > MAX_SIDE || W > MAX_SIDE) return GD3D_E_TOOLARGE;
  return 0;
}

// the pixel coordinate of v on an axis of n cells whose first and last cell centres lie at tl and br (align_corners=True):
// a difference, a product and ONE correctly rounded division, left to right — dividing last keeps a keypoint that sits on a cell
// centre of a grid of exactly representable centres on the integer
VB_HD float pixel_coord(float v, float tl, float br, int64_t n) { return ((v - tl) * (float)(n - 1)) / (br - tl); }

// the four neighbours of one keypoint, in the fixed order nw, ne, sw, se
struct Taps {
  int64_t off[4];      // element offset of channel 0 of the neighbour inside bev_features; 0 where `use` is false
  float w[4];          // its bilinear weight
  bool use[4];         // false: out of the map (padding_mode='zeros'), or the whole keypoint is out of reach: the neighbour contributes 0
};

// Keypoint (x, y) of sample b on a (H, W) map with element strides (sB, sH, sW).  The float-to-int conversions happen only after
// the comparisons below have confined both coordinates to (-1, n): NaN fails every comparison, +-inf and anything a cell or more
// outside the map fail one, and such a keypoint gets four unused neighbours (a zero row, no gradient).  Inside, floor is in
// [-1, n - 1] and every neighbour that is used lies in [0, n - 1]: no index leaves the map for any input.
VB_HD Taps make_taps(float x, float y, int64_t b, float tl_x, float tl_y, float br_x, float br_y, int64_t H, int64_t W, int64_t sB,
                     int64_t sH, int64_t sW) {
  Taps t;
  const float ix = pixel_coord(x, tl_x, br_x, W), iy = pixel_coord(y, tl_y, br_y, H);
  const bool reach = ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H;
  const float fx0 = reach ? floorf(ix) : 0.0f, fy0 = reach ? floorf(iy) : 0.0f;
  const float ax = reach ? ix - fx0 : 0.0f, ay = reach ? iy - fy0 : 0.0f;   // the weights of the +1 neighbours
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const int64_t x0 = (int64_t)fx0, y0 = (int64_t)fy0;                        // in [-1, n - 1]
  t.w[0] = bx * by;
  t.w[1] = ax * by;
  t.w[2] = bx * ay;
  t.w[3] = ax * ay;
  for (int j = 0; j < 4; ++j) {
    const int64_t xj = x0 + (j & 1), yj = y0 + (j >> 1);
    t.use[j] = reach && xj >= 0 && xj < W && yj >= 0 && yj < H;
    t.off[j] = t.use[j] ? b * sB + yj * sH + xj * sW : 0;
  }
  return t;
}

// the bilinear sum in its one order: ((nw + ne) + sw) + se, each term value * weight, an unused neighbour's value being 0
VB_HD float blend(float nw, float ne, float sw, float se, const float* w) {
  float acc = nw * w[0];
  acc = acc + ne * w[1];
  acc = acc + sw * w[2];
  acc = acc + se * w[3];
  return acc;
}

// the lanes that share a keypoint's row of `items` items (channels, or quads of channels): the power of two covering them, 64 at most
VB_HD int row_lanes(int64_t items) {
  int g = 1;
  while (g < 64 && g < items) g <<= 1;
  return g;
}

// element strides (sB, sC, sH, sW) of a dense (B, C, H, W) map: layout 0 = contiguous NCHW, 1 = channels last (NHWC in memory)
VB_HD void map_strides(int layout, int64_t C, int64_t H, int64_t W, int64_t* sB, int64_t* sC, int64_t* sH, int64_t* sW) {
  *sB = C * H * W;
  if (layout == 0) {
    *sC = H * W;
    *sH = W;
    *sW = 1;
  } else {
    *sC = 1;
    *sH = W * C;
    *sW = C;
  }
}

// one axis of a voxel centre: ((c * vs) * scale + min) + add, left to right; c is the integer coordinate converted to fp32
VB_HD float centre_axis(float c, float vs, float scale, float mn, float add) { return ((c * vs) * scale + mn) + add; }

}  // namespace vsa_bev
