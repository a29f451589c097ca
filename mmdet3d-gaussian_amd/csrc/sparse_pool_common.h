// sparse_pool_common.h — what csrc/sparse_pool.hip and csrc/sparse_pool_cpu.cpp share of the sparse max pooling (include/gd3d.h,
// gd3d_sparse_max_pool_*): the limits, how the lanes of a workgroup are laid over rows and channels, the row limit and
// the argument checks.  The layout depends on C and the element size alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sparse_conv_common.h"

namespace sparse_pool {

constexpr int MAX_C = sparse_conv::MAX_C;   // channels
constexpr int MAX_K = sparse_conv::MAX_K;   // offsets of one window
constexpr int BLOCK = 256;                  // threads of a workgroup
constexpr int MAX_BLOCKS = 2048;            // workgroups of a launch: the rows beyond are reached by striding over the grid

// the lane layout: a lane owns `vec` adjacent channels of one row (16 bytes where the row pitch allows it, else one element), `groups`
// lanes cover a row, one workgroup covers `rows` rows at a time (tests name their row counts from it)
struct Lanes {
  int vec, groups, rows;
};

inline Lanes lanes_of(int32_t C, int32_t dtype) {
  const int wide = dtype == 0 ? 4 : 8;
  Lanes l;
  l.vec = C % wide == 0 ? wide : 1;
  l.groups = C / l.vec;
  l.rows = BLOCK / l.groups;
  return l;
}

inline size_t elem_size(int32_t dtype) { return dtype == 0 ? 4 : 2; }

inline bool misaligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

using sparse_conv::row_limit;               // rows at and past num[0] are zeros; num nullable: every row counts

// GD3D_E_* or 0: the scalar arguments of every entry, as the sparse-conv entries order their checks
inline int check_dims(int64_t N, int64_t R, int32_t K, int32_t C, int32_t dtype) {
  if (K < 1 || C < 1 || N < 0 || R < 0) return GD3D_E_BADARG;
  if (dtype != 0 && dtype != GD3D_DTYPE_F16 && dtype != GD3D_DTYPE_BF16) return GD3D_E_BADARG;
  if (K > MAX_K || C > MAX_C || N > 0x7fffffffLL || R > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  return 0;
}

}  // namespace sparse_pool
