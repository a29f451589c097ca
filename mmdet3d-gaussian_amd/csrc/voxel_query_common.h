// voxel_query_common.h — what csrc/voxel_query.hip (gfx950 kernels) and csrc/voxel_query_cpu.cpp (their `_cpu` twins) share: the cell
// window of a query and its enumeration, the row and key arithmetic of both look-up forms, the fp32 cell sequence of
// gd3d_vsa_voxel_coords and the argument checks.  The key is sparse_conv::in_key's, the look-up sparse_conv::lower_bound, the distance
// vsa::dist2: one definition each.  Both units are compiled with -ffp-contract=off and correctly rounded division.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "sparse_conv_common.h"
#include "vsa_common.h"

namespace voxel_query {

using sparse_conv::Geo;

constexpr int MAX_RANGE = 16;            // cells either side of the query's cell, per axis
constexpr int QW = 4;                    // waves = queries per workgroup (query kernels)
constexpr int BLOCK = 256;               // threads of a workgroup, every kernel
constexpr float CELL_LIMIT = 1073741824.0f;   // 2^30: a query cell outside [-2^30, 2^30) makes the query empty (b = -1)

struct Window {
  int rz, ry, rx;      // max_range
  int ny, nx;          // 2 * ry + 1, 2 * rx + 1
  int rows, cells;     // (2 rz + 1) * ny and rows * nx
};

// the grid of the look-up (B, Z, Y, X) as a sparse_conv::Geo (a 1x1x1 layer: its checks bound every side by 2^24, the key by 2^62
// and N by 2^31 - 1) and the window; GD3D_E_* or 0
inline int make_grid(int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X, Geo* g) {
  const int32_t shape[3] = {Z, Y, X}, one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
  return sparse_conv::make_geo(N, B, shape, one, one, zero, 0, g);
}

inline int make_window(const int32_t* max_range, Window* w) {
  if (max_range == nullptr) return GD3D_E_BADARG;
  for (int a = 0; a < 3; ++a) {
    if (max_range[a] < 0) return GD3D_E_BADARG;
    if (max_range[a] > MAX_RANGE) return GD3D_E_TOOLARGE;
  }
  w->rz = max_range[0]; w->ry = max_range[1]; w->rx = max_range[2];
  w->ny = 2 * w->ry + 1;
  w->nx = 2 * w->rx + 1;
  w->rows = (2 * w->rz + 1) * w->ny;
  w->cells = w->rows * w->nx;
  return 0;
}

// row i of coors (N, 4) [b, z, y, x], int32 or int64: its key, or the sentinel g.in_sent (which sorts last) when any coordinate
// is outside the grid.  Compared in 64 bits BEFORE anything is narrowed or linearised.
SC_HD long long row_key(const void* coors, int is64, long long i, const Geo& g) {
  long long c[4];
  for (int a = 0; a < 4; ++a)
    c[a] = is64 ? (long long)static_cast<const int64_t*>(coors)[i * 4 + a] : (long long)static_cast<const int32_t*>(coors)[i * 4 + a];
  const bool in = c[0] >= 0 && c[0] < g.B && c[1] >= 0 && c[1] < g.n[0] && c[2] >= 0 && c[2] < g.n[1] && c[3] >= 0 && c[3] < g.n[2];
  return in ? sparse_conv::in_key(g, (int)c[0], (int)c[1], (int)c[2], (int)c[3]) : g.in_sent;
}

// window row j (dz slowest, then dy, each ascending from -r) of the query at cell (b, cz, cy, cx), b in [0, B): the keys
// [*k0, *k1] of its cells x - rx .. x + rx clipped to [0, X); false: the row lies outside the grid or the clipped run is empty.
// The clipping keeps a run inside its y row: the keys of (b, Z-1, Y-1, X-1) and (b+1, 0, 0, 0) are neighbours.
SC_HD bool window_row(const Geo& g, const Window& w, int b, int cz, int cy, int cx, int j, long long* k0, long long* k1) {
  const int jz = j / w.ny;
  const long long z = (long long)cz + (jz - w.rz), y = (long long)cy + ((j - jz * w.ny) - w.ry);
  if (z < 0 || z >= g.n[0] || y < 0 || y >= g.n[1]) return false;
  long long x0 = (long long)cx - w.rx, x1 = (long long)cx + w.rx;
  x0 = x0 < 0 ? 0 : x0;
  x1 = x1 >= g.n[2] ? (long long)g.n[2] - 1 : x1;
  if (x0 > x1) return false;
  *k0 = sparse_conv::in_key(g, b, (int)z, (int)y, (int)x0);
  *k1 = *k0 + (x1 - x0);
  return true;
}

// window cell j (dz slowest, dx fastest): its key; false: outside the grid
SC_HD bool window_cell(const Geo& g, const Window& w, int b, int cz, int cy, int cx, int j, long long* key) {
  const int jr = j / w.nx;
  const int jz = jr / w.ny;
  const long long z = (long long)cz + (jz - w.rz), y = (long long)cy + ((jr - jz * w.ny) - w.ry), x = (long long)cx + ((j - jr * w.nx) - w.rx);
  if (z < 0 || z >= g.n[0] || y < 0 || y >= g.n[1] || x < 0 || x >= g.n[2]) return false;
  *key = sparse_conv::in_key(g, b, (int)z, (int)y, (int)x);
  return true;
}

// inclusive, and false for a NaN distance
SC_HD bool is_member(const float* q, const float* p, float radius2) {
  return vsa::dist2(q[0], q[1], q[2], p[0], p[1], p[2]) <= radius2;
}

// gd3d_vsa_voxel_coords, one axis: one subtraction, one correctly rounded division, one floor (hard_voxelize's sequence).  Compared
// as a FLOAT before the conversion: NaN, +-inf and 1e30 fail it.
SC_HD bool axis_cell(float p, float lo, float vsl, int32_t* c) {
  const float f = floorf((p - lo) / vsl);
  const bool ok = f >= -CELL_LIMIT && f < CELL_LIMIT;
  *c = ok ? (int32_t)f : 0;
  return ok;
}

// the sample of stacked query row m, as vsa::row_segment resolves rows (counts clamped to the rows left); -1 past the counts' sum
SC_HD int32_t sample_of_row(const int32_t* qcnt, int B, long long M, long long m) {
  long long qs = 0;
  for (int b = 0; b < B; ++b) {
    qs += vsa::clamp_count(qcnt[b], M - qs);
    if (m < qs) return b;
  }
  return -1;
}

// row m of new_coords [b, z, y, x]; vsl, lo: (x, y, z)
SC_HD void query_coords(const float* p, int32_t b, const float* vsl, const float* lo, int32_t* out) {
  const bool x = axis_cell(p[0], lo[0], vsl[0], out + 3);
  const bool y = axis_cell(p[1], lo[1], vsl[1], out + 2);
  const bool z = axis_cell(p[2], lo[2], vsl[2], out + 1);
  out[0] = (x && y && z) ? b : -1;
}

// the checks of the two query entries, device and `_cpu` alike; *run = false with 0: nothing to compute
inline int check_query(const void* xyz, const void* new_xyz, const void* new_coords, const void* skey, const void* srow, const void* table,
                       const void* features, int32_t B, int32_t Z, int32_t Y, int32_t X, int64_t N, int64_t M, int32_t C,
                       const int32_t* max_range, int32_t nsample, int32_t use_xyz, const void* out, const void* idx, Geo* g, Window* w,
                       bool* run) {
  *run = false;
  if (M < 0 || C < 0 || nsample <= 0) return GD3D_E_BADARG;
  if (nsample > vsa::MAX_NSAMPLE) return GD3D_E_TOOLARGE;
  int rc = make_window(max_range, w);
  if (rc != 0) return rc;
  rc = make_grid(N, B, Z, Y, X, g);
  if (rc != 0) return rc;
  const bool group = out != nullptr;
  if (group && !use_xyz && C == 0) return GD3D_E_BADARG;   // nothing to write
  if ((long long)((use_xyz ? 3 : 0) + C) * nsample > 0x7fffffffLL || (M + QW - 1) / QW > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (M == 0) return 0;
  if (new_xyz == nullptr || new_coords == nullptr || idx == nullptr) return GD3D_E_BADARG;
  if (table != nullptr && (skey != nullptr || srow != nullptr)) return GD3D_E_BADARG;   // one look-up form: the table, else the sorted keys
  if (table == nullptr && N > 0 && B > 0 && (skey == nullptr || srow == nullptr)) return GD3D_E_BADARG;
  if (N > 0 && (xyz == nullptr || (group && C > 0 && features == nullptr))) return GD3D_E_BADARG;
  *run = true;
  return 0;
}

}  // namespace voxel_query
