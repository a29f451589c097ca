// sparse_pool_common.h — what csrc/sparse_pool.hip and csrc/sparse_pool_cpu.cpp share of the sparse max pooling (include/gd3d.h,
// gd3d_sparse_max_pool_*): the limits, how the lanes of a workgroup are laid over rows and channels (csrc/sparse_elem.h), the row limit and
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

// the lane layout of both kernels: sparse_elem::lanes_of(C, dtype, BLOCK)

using sparse_conv::row_limit;               // rows at and past num[0] are zeros; num nullable: every row counts

// GD3D_E_* or 0: the scalar arguments of every entry, as the sparse-conv entries order their checks
inline int check_dims(int64_t N, int64_t R, int32_t K, int32_t C, int32_t dtype) {
  if (K < 1 || C < 1 || N < 0 || R < 0) return GD3D_E_BADARG;
  if (!sparse_elem::dtype_ok(dtype)) return GD3D_E_BADARG;
  if (K > MAX_K || C > MAX_C || N > 0x7fffffffLL || R > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  return 0;
}

}  // namespace sparse_pool
