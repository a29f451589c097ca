// sparse_pool.hip — max pooling over the neighbour tables of a sparse tensor, forward and backward, fp32 / fp16 / bf16, for gfx950
// (include/gd3d.h, gd3d_sparse_max_pool_*).
//
//   pool_kernel      a lane owns one 16-byte piece of one output row (4 fp32 or 8 16-bit channels; one element where the row pitch is no
//                    multiple of 16 bytes): it walks the K table entries of its row — the lanes of a row read the same entries, one
//                    request — loads each valid neighbour's piece with one 16-byte load and keeps the maximum AS THE ELEMENT IT READ.
//                    The comparison is written out: a candidate wins when it is greater or a NaN.  A row without a valid neighbour, or
//                    at or past num[0], is zero.
//   unpool_kernel    the same walk over the transposed table for one input row: grad_out of every window whose maximum EQUALS this
//                    input element, added in ascending offset order in fp32 and rounded once.
// Both are gathers bound by bytes: no LDS, no atomics, one launch each; BLOCK / groups rows per workgroup, at most MAX_BLOCKS workgroups
// that stride over the rows (csrc/sparse_pool_common.h).  Nothing depends on the order in which workgroups run: the same bits every run.
#include <hip/hip_runtime.h>

#include "sparse_pool_common.h"

using namespace sparse_pool;
using namespace sparse_elem;

namespace {

struct Args {
  const void *x, *y, *gy;      // features (N, C); the pooled output (R, C) and its gradient (the backward only)
  void* dst;                   // out (R, C) or grad_features (N, C)
  const int32_t* table;        // (rows, K): nbr forward, nbr_t backward
  const long long* num;        // forward only, nullable
  long long n_src, rows;       // rows of the operand the table points into; rows written
  int K, C, groups, lane_rows;
  unsigned wide;               // bit per operand: its base is 16-byte aligned
};

enum { W_X = 1, W_Y = 2, W_GY = 4, W_DST = 8 };

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void pool_kernel(Args a) {
  typedef typename E::T T;
  const int tid = threadIdx.x, rr = tid / a.groups, g = tid % a.groups;
  if (rr >= a.lane_rows) return;
  const T* x = (const T*)a.x;
  T* out = (T*)a.dst;
  const long long limit = row_limit(a.num, a.rows);
  const bool wx = a.wide & W_X, wd = a.wide & W_DST;
  for (long long row = (long long)blockIdx.x * a.lane_rows + rr; row < a.rows; row += (long long)gridDim.x * a.lane_rows) {
    T best[V], cur[V];
    float top[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { best[v] = (T)0; top[v] = 0.0f; }      // all bits clear: +0 in every type
    bool any = false;
    if (row < limit) {
      const int32_t* t = a.table + row * a.K;
      for (int j = 0; j < a.K; ++j) {
        const int i = t[j];
        if (i < 0 || i >= a.n_src) continue;
        load<T, V>(x, (long long)i * a.C + g * V, wx, cur);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float c = E::widen(cur[v]);
          if (!any || c > top[v] || c != c) { best[v] = cur[v]; top[v] = c; }      // a NaN wins and is never displaced
        }
        any = true;
      }
    }
    store<T, V>(out, row * a.C + g * V, wd, best);
  }
}

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void unpool_kernel(Args a) {
  typedef typename E::T T;
  const int tid = threadIdx.x, rr = tid / a.groups, g = tid % a.groups;
  if (rr >= a.lane_rows) return;
  const T *x = (const T*)a.x, *y = (const T*)a.y, *gy = (const T*)a.gy;
  T* gx = (T*)a.dst;
  const bool wx = a.wide & W_X, wy = a.wide & W_Y, wg = a.wide & W_GY, wd = a.wide & W_DST;
  for (long long row = (long long)blockIdx.x * a.lane_rows + rr; row < a.rows; row += (long long)gridDim.x * a.lane_rows) {
    const long long at = row * a.C + g * V;
    T xv[V], yv[V], gv[V], ov[V];
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    bool have = false;
    const int32_t* t = a.table + row * a.K;
    for (int j = 0; j < a.K; ++j) {
      const int o = t[j];
      if (o < 0 || o >= a.n_src) continue;
      if (!have) { load<T, V>(x, at, wx, xv); have = true; }
      const long long src = (long long)o * a.C + g * V;
      load<T, V>(y, src, wy, yv);
      load<T, V>(gy, src, wg, gv);
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (E::widen(xv[v]) == E::widen(yv[v])) acc[v] = acc[v] + E::widen(gv[v]);      // a NaN compares unequal: no gradient
    }
#pragma unroll
    for (int v = 0; v < V; ++v) ov[v] = E::narrow(acc[v]);
    store<T, V>(gx, at, wd, ov);
  }
}

template <typename E>
int launch(const Args& a, bool vec, bool forward, hipStream_t s) {
  constexpr int V = E::WIDE;
  const long long b = (a.rows + a.lane_rows - 1) / a.lane_rows;
  const dim3 grid((unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS)), block(BLOCK);
  if (forward) {
    if (vec) hipLaunchKernelGGL((pool_kernel<E, V>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((pool_kernel<E, 1>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((unpool_kernel<E, V>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((unpool_kernel<E, 1>), grid, block, 0, s, a);
  }
  return (int)hipGetLastError();
}

int dispatch(Args& a, int32_t C, int32_t dtype, bool forward, void* stream) {
  const Lanes l = lanes_of(C, dtype, BLOCK);
  a.C = C; a.groups = l.groups; a.lane_rows = l.rows;
  hipStream_t s = (hipStream_t)stream;
  return with_elem(dtype, [&](auto e) { return launch<decltype(e)>(a, l.vec > 1, forward, s); });
}

}  // namespace

extern "C" {

int gd3d_sparse_max_pool_forward(const void* features, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t C,
                                 int32_t dtype, void* out, void* stream) {
  const int rc = check_dims(N, R, K, C, dtype);
  if (rc != 0) return rc;
  if (R == 0) return 0;
  if (nbr == nullptr || out == nullptr || (N > 0 && features == nullptr)) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(features, es) || misaligned(out, es) || misaligned(nbr, 4) || misaligned(num, 8)) return GD3D_E_BADARG;
  Args a = {};
  a.x = features; a.dst = out; a.table = nbr; a.num = (const long long*)num; a.n_src = N; a.rows = R; a.K = K;
  a.wide = wide_bit(features, W_X) | wide_bit(out, W_DST);
  return dispatch(a, C, dtype, true, stream);
}

int gd3d_sparse_max_pool_backward(const void* grad_out, const void* features, const void* out, const int32_t* nbr_t, int64_t N, int64_t R,
                                  int32_t K, int32_t C, int32_t dtype, void* grad_features, void* stream) {
  const int rc = check_dims(N, R, K, C, dtype);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (nbr_t == nullptr || grad_features == nullptr || features == nullptr || (R > 0 && (grad_out == nullptr || out == nullptr))) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(grad_out, es) || misaligned(features, es) || misaligned(out, es) || misaligned(grad_features, es) || misaligned(nbr_t, 4))
    return GD3D_E_BADARG;
  Args a = {};
  a.x = features; a.y = out; a.gy = grad_out; a.dst = grad_features; a.table = nbr_t; a.num = nullptr; a.n_src = R; a.rows = N; a.K = K;
  a.wide = wide_bit(features, W_X) | wide_bit(out, W_Y) | wide_bit(grad_out, W_GY) | wide_bit(grad_features, W_DST);
  return dispatch(a, C, dtype, false, stream);
}

}  // extern "C"
