// sparse_bn_common.h — what csrc/sparse_bn.hip and csrc/sparse_bn_cpu.cpp share of the live-row batch normalisation (include/gd3d.h,
// gd3d_sparse_bn_*): which rows are live (csrc/sparse_conv_common.h's rule), how R rows are cut into tiles, how the
// lanes of a workgroup are laid over rows and channels (csrc/sparse_elem.h), the workspace layout and the argument checks.  The cut and the lane layout
// depend on (R, C) and the element size alone: nothing a row holds can change the order of a sum.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sparse_conv_common.h"

namespace sparse_bn {

constexpr int MAX_C = sparse_conv::MAX_C;   // channels
constexpr int BLOCK = 256;                  // threads of a workgroup, every kernel
constexpr int TILE_ROWS = 64;               // T: a tile is a multiple of this many rows (tests name their row counts from it)
constexpr int MAX_TILES = 256;              // P: the cap on the per-tile partials

// `tiles` tiles of `chunk` rows: a tile per TILE_ROWS rows until MAX_TILES of them exist, longer tiles from there on
inline void cut_rows(int64_t R, int64_t* tiles, int64_t* chunk) {
  int64_t t = (R + TILE_ROWS - 1) / TILE_ROWS;
  t = t < 1 ? 1 : (t > MAX_TILES ? MAX_TILES : t);
  int64_t c = (R + t - 1) / t;
  c = (c + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS;
  if (c < TILE_ROWS) c = TILE_ROWS;
  *chunk = c;
  *tiles = R > 0 ? (R + c - 1) / c : 0;
}

// the lane layout of every kernel here: sparse_elem::lanes_of(C, dtype, BLOCK)

// the workspace, in 4-byte words: the tiles' live-row counts, three (tiles, C) planes of partials, the merged (2, C) plane, the count
struct Space {
  size_t cnt, plane[3], merged, total, words;
};

SC_HD Space space_of(int32_t C) {
  Space s;
  s.cnt = 0;
  s.plane[0] = MAX_TILES;
  s.plane[1] = s.plane[0] + (size_t)MAX_TILES * (size_t)C;
  s.plane[2] = s.plane[1] + (size_t)MAX_TILES * (size_t)C;
  s.merged = s.plane[2] + (size_t)MAX_TILES * (size_t)C;
  s.total = s.merged + 2 * (size_t)C;
  s.words = s.total + 4;
  return s;
}

// GD3D_E_* or 0: the scalar arguments of every entry
inline int check_dims(int64_t R, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W, int32_t act, int32_t dtype) {
  if (R < 0 || C < 1 || B < 0 || D < 1 || H < 1 || W < 1) return GD3D_E_BADARG;
  if (!sparse_conv::act_ok(act) || !sparse_elem::dtype_ok(dtype)) return GD3D_E_BADARG;
  if (C > MAX_C || R > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  return 0;
}

}  // namespace sparse_bn
