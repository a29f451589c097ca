// pib_common.h — what csrc/pib.hip (gfx950 kernels) and csrc/pib_cpu.cpp (their `_cpu` twins) share: the point-in-rotated-box
// test of mmdet3d 1.0's roiaware_pool3d (`check_pt_in_box3d`) and the RoI grid point as ONE fixed sequence of fp32 operations
// each, and the resolution of a stacked batch into clamped segments.  Both units are compiled with -ffp-contract=off and
// take the sine and cosine from rbox_device.h's fixed-sequence fx_sincosf (no libm), so every membership decision and every
// grid point is the same bits on the device and on the host.
#pragma once
#include <stdint.h>

#include "rbox_device.h"   // under GD3D_HOST_TWIN: the same source for the host

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define PIB_HD __device__ __forceinline__
#else
#define PIB_HD inline
#endif

namespace pib {

constexpr int WG = 256;          // threads of a workgroup = points a workgroup owns (all of ONE sample)
constexpr int BOX_TILE = 256;    // boxes whose constants a workgroup holds in LDS at a time
constexpr int MAX_GRID = 16;     // RoI grid size G

// The constants of a box [x, y, z, dx, dy, dz, rz] ((x, y, z) the BOTTOM centre) the pair test consumes.
struct BoxC {
  float x, y, czm, hx, hy, hz, c, s;
};

PIB_HD BoxC box_constants(float x, float y, float z, float dx, float dy, float dz, float rz) {
  BoxC k;
  k.x = x;
  k.y = y;
  k.hz = dz * 0.5f;
  k.czm = z + k.hz;
  k.hx = dx * 0.5f;
  k.hy = dy * 0.5f;
  rbox::fx_sincosf(-rz, k.s, k.c);
  return k;
}

// mmdet3d's `enlarged_box`: z - w, every dim + 2 w (2 w is exact), each ONE fp32 operation
PIB_HD BoxC box_constants_enlarged(float x, float y, float z, float dx, float dy, float dz, float rz, float w) {
  const float w2 = w * 2.0f;
  return box_constants(x, y, z - w, dx + w2, dy + w2, dz + w2, rz);
}

// z faces INCLUSIVE, x / y faces STRICT.  The z test is written as `|pz - czm| <= hz` (for ordered operands the complement of
// check_pt_in_box3d's `> hz -> outside`), so that a NaN pz fails it as a NaN px or py fails the strict tests: a point with a
// NaN coordinate is in no box.  hz < 0 (negative dz) and hx <= 0 or hy <= 0 (zero or negative dx, dy) contain nothing.
PIB_HD bool contains(float cx, float cy, float czm, float hx, float hy, float hz, float c, float s, float px, float py, float pz) {
  const float az = pz - czm;
  const bool in_z = (az < 0.0f ? -az : az) <= hz;
  const float sx = px - cx, sy = py - cy;
  const float ns = -s;
  const float a0 = sx * c, a1 = sy * ns;
  const float b0 = sx * s, b1 = sy * c;
  const float lx = a0 + a1, ly = b0 + b1;
  return in_z && lx > -hx && lx < hx && ly > -hy && ly < hy;
}
PIB_HD bool contains(const BoxC& k, float px, float py, float pz) {
  return contains(k.x, k.y, k.czm, k.hx, k.hy, k.hz, k.c, k.s, px, py, pz);
}

// The RoI [x, y, z, dx, dy, dz, rz]'s frame for its grid points: point (i, j, k) of a G^3 grid is
//   u = (i + 0.5f) / G - 0.5f, v = (j + 0.5f) / G - 0.5f, w = (k + 0.5f) / G;  local = (u dx, v dy, w dz);
//   counter-clockwise: x' = lx c - ly s, y' = lx s + ly c;  clockwise: x' = lx c + ly s, y' = ly c - lx s   (fx_sincosf(rz));
//   out = (x' + x, y' + y, lz + z)      — one fp32 operation per step, the division correctly rounded.
struct RoiC {
  float x, y, z, dx, dy, dz, c, s;
};

PIB_HD RoiC roi_constants(const float* r) {
  RoiC k;
  k.x = r[0]; k.y = r[1]; k.z = r[2]; k.dx = r[3]; k.dy = r[4]; k.dz = r[5];
  rbox::fx_sincosf(r[6], k.s, k.c);
  return k;
}

PIB_HD float grid_frac(int i, float g) { return ((float)i + 0.5f) / g; }

// comp 0 / 1 / 2 of grid point (i, j, k)
PIB_HD float grid_coord(const RoiC& r, int i, int j, int k, float g, int clockwise, int comp) {
  if (comp == 2) {
    const float lz = grid_frac(k, g) * r.dz;
    return lz + r.z;
  }
  const float lx = (grid_frac(i, g) - 0.5f) * r.dx;
  const float ly = (grid_frac(j, g) - 0.5f) * r.dy;
  if (comp == 0) {
    const float a = lx * r.c, b = ly * r.s;
    return (clockwise ? a + b : a - b) + r.x;
  }
  const float a = lx * r.s, b = ly * r.c;
  return (clockwise ? b - a : a + b) + r.y;
}

PIB_HD long long clamp_count(int c, long long room) {
  const long long v = c < 0 ? 0 : (long long)c;
  return v < room ? v : room;
}

// boxes of sample b that are tested: box_cnt[b] clamped to [0, T]; all T without a count array
PIB_HD int boxes_of(const int32_t* box_cnt, int b, int T) { return box_cnt != nullptr ? (int)clamp_count(box_cnt[b], T) : T; }

// Work item j of a launch that gives every sample ceil(points / WG) consecutive items -> the sample b, the item's first point
// row p0 and its np <= WG points.  Rows of the point array beyond the counts' sum form one more segment, b == B, that has no
// boxes.  False: j is past the last item.
PIB_HD bool point_block(const int32_t* pcnt, int B, long long N, long long j, int& b, long long& p0, int& np) {
  long long ps = 0;
  for (int s = 0; s <= B; ++s) {
    const long long pn = s < B ? clamp_count(pcnt[s], N - ps) : N - ps;
    const long long items = (pn + WG - 1) / WG;
    if (j < items) {
      b = s;
      p0 = ps + j * WG;
      const long long left = pn - j * WG;
      np = (int)(left < WG ? left : WG);
      return true;
    }
    j -= items;
    ps += pn;
  }
  return false;
}

}  // namespace pib
