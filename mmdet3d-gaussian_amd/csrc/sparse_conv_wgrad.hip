// sparse_conv_wgrad.hip — the weight and bias gradient of the sparse 3D convolution (include/gd3d.h, gd3d_sparse_conv_backward_weight,
// gd3d_sparse_conv_backward_weight_16) for gfx950, ONE source for fp32, fp16 and bf16 operands: an element policy
// E gives the storage type and `widen`, the identity for fp32 and exact for the 16-bit types (csrc/sparse_elem.h), so the three
// forms run the same fp32 sequence and the 16-bit entries equal the fp32 entry on the widened operands bit for bit.  fp32 out.
//   wgrad_kernel  per (row chunk, offset, tile of W[j] of 16, 32 or 64 channels a side): the rows of the chunk in steps of WG_ROWS,
//                 the gathered X rows and the gY rows staged in LDS as fp32, partial sums into the workspace.  No atomics.
//   bias_kernel   column sums of gY over the chunk's rows that have a neighbour.
//   wfinish_kernel  adds the chunks' partial sums of both in ascending chunk order.
// The tables are those of csrc/sparse_conv.hip's index build; weight_parts (csrc/sparse_conv_common.h) cuts the rows into chunks.
// Compiled with -ffp-contract=off; the multiply-adds are explicit fmaf.  The matrix-core stage one for fp16 / bf16
// (gd3d_sparse_conv_backward_weight_16_mfma) is csrc/sparse_conv_wgrad_16.hip: it shares the arguments and the workspace
// (csrc/sparse_conv_wgrad.h) and runs bias_kernel and wfinish_kernel of this unit through finish_wgrad.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "sparse_conv_wgrad.h"

namespace sparse_conv {

constexpr int BLOCK = 256;

// grid (parts, K, tiles of TI x TO of W[j]): the partial sum of chunk p.  TI, TO in {16, 32, 64}: the smallest tiles that hold Cin and
// Cout; a thread owns TI / 16 x TO / 16 elements.
template <class E, int TI, int TO>
__global__ __launch_bounds__(BLOCK) void wgrad_kernel(const WgradArgs a) {
  constexpr int MI = TI / 16, MO = TO / 16;
  __shared__ int nb[WG_ROWS];
  __shared__ float Xg[WG_ROWS][TI];
  __shared__ float Gy[WG_ROWS][TO];
  const typename E::T* X = (const typename E::T*)a.X;
  const typename E::T* gY = (const typename E::T*)a.gY;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int j = blockIdx.y;
  const int ci0 = (blockIdx.z / a.tiles_co) * TI, co0 = (blockIdx.z % a.tiles_co) * TO;
  const long long limit = row_limit(a.num, a.rows);
  const long long begin = (long long)blockIdx.x * a.chunk;
  long long end = begin + a.chunk;
  end = end < limit ? end : limit;
  float acc[MI][MO];
  for (int i = 0; i < MI; ++i)
    for (int q = 0; q < MO; ++q) acc[i][q] = 0.0f;
  for (long long r0 = begin; r0 < end; r0 += WG_ROWS) {          // begin, end, r0: the same for the whole workgroup
    int v = -1;
    if (t < WG_ROWS && r0 + t < end) {
      v = a.nbr[(r0 + t) * a.K + j];
      if (v < 0 || v >= a.n_src) v = -1;
    }
    if (t < WG_ROWS) nb[t] = v;
    if (!__syncthreads_or(v >= 0)) continue;
    for (int idx = t; idx < WG_ROWS * TI; idx += BLOCK) {
      const int r = idx / TI, c = idx % TI;
      const int row = nb[r];
      Xg[r][c] = (row >= 0 && ci0 + c < a.Cin) ? E::widen(X[(long long)row * a.Cin + ci0 + c]) : 0.0f;
    }
    for (int idx = t; idx < WG_ROWS * TO; idx += BLOCK) {
      const int r = idx / TO, c = idx % TO;
      Gy[r][c] = (nb[r] >= 0 && co0 + c < a.Cout) ? E::widen(gY[(r0 + r) * a.Cout + co0 + c]) : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < WG_ROWS; ++r) {
      float x[MI], g[MO];
#pragma unroll
      for (int i = 0; i < MI; ++i) x[i] = Xg[r][ty * MI + i];
#pragma unroll
      for (int q = 0; q < MO; ++q) g[q] = Gy[r][tx * MO + q];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < MO; ++q) acc[i][q] = __builtin_fmaf(x[i], g[q], acc[i][q]);
    }
    __syncthreads();
  }
  float* dst = a.part_w + ((long long)blockIdx.x * a.K + j) * a.Cin * a.Cout;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int ci = ci0 + ty * MI + i;
    if (ci >= a.Cin) continue;
#pragma unroll
    for (int q = 0; q < MO; ++q) {
      const int co = co0 + tx * MO + q;
      if (co < a.Cout) dst[(long long)ci * a.Cout + co] = acc[i][q];
    }
  }
}

template <class E, int TI>
static void launch_wgrad_in(WgradArgs& a, int to, hipStream_t s) {
  a.tiles_co = (a.Cout + to - 1) / to;
  const dim3 grid((unsigned)a.parts, (unsigned)a.K, (unsigned)(((a.Cin + TI - 1) / TI) * a.tiles_co));
  switch (to) {
    case 16: hipLaunchKernelGGL((wgrad_kernel<E, TI, 16>), grid, dim3(BLOCK), 0, s, a); break;
    case 32: hipLaunchKernelGGL((wgrad_kernel<E, TI, 32>), grid, dim3(BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL((wgrad_kernel<E, TI, 64>), grid, dim3(BLOCK), 0, s, a); break;
  }
}

// grid (parts): column sums of gY over the chunk's rows that have a neighbour.  The workgroup's threads form 256 / CP groups of CP >= Cout
// columns (CP a power of two); group g adds the rows g, g + groups, ... of every 256-row step, then the groups are added in ascending order.
template <class E>
__global__ __launch_bounds__(BLOCK) void bias_kernel(const WgradArgs a, const int CP) {
  __shared__ int live[BLOCK];
  __shared__ float red[BLOCK];
  const typename E::T* gY = (const typename E::T*)a.gY;
  const int t = threadIdx.x, col = t % CP, grp = t / CP, groups = BLOCK / CP;
  const long long limit = row_limit(a.num, a.rows);
  const long long begin = (long long)blockIdx.x * a.chunk;
  long long end = begin + a.chunk;
  end = end < limit ? end : limit;
  float acc = 0.0f;
  for (long long r0 = begin; r0 < end; r0 += BLOCK) {
    int any = 0;
    if (r0 + t < end) {
      for (int j = 0; j < a.K; ++j) {
        const int v = a.nbr[(r0 + t) * a.K + j];
        any |= v >= 0 && v < a.n_src;
      }
    }
    live[t] = any;
    __syncthreads();
    const int rn = end - r0 < BLOCK ? (int)(end - r0) : BLOCK;
    if (col < a.Cout)
      for (int r = grp; r < rn; r += groups)
        if (live[r]) acc += E::widen(gY[(r0 + r) * a.Cout + col]);
    __syncthreads();
  }
  red[t] = acc;
  __syncthreads();
  if (grp == 0 && col < a.Cout) {
    float s = 0.0f;
    for (int g = 0; g < groups; ++g) s += red[g * CP + col];
    a.part_b[(long long)blockIdx.x * a.Cout + col] = s;
  }
}

// the chunks' partial sums added in ascending chunk order
__global__ __launch_bounds__(BLOCK) void wfinish_kernel(const WgradArgs a) {
  const long long kcc = (long long)a.K * a.Cin * a.Cout;
  const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (idx < kcc) {
    float s = 0.0f;
    for (long long p = 0; p < a.parts; ++p) s += a.part_w[p * kcc + idx];
    a.gW[idx] = s;
  } else if (a.gb != nullptr && idx - kcc < a.Cout) {
    const long long c = idx - kcc;
    float s = 0.0f;
    for (long long p = 0; p < a.parts; ++p) s += a.part_b[p * a.Cout + c];
    a.gb[c] = s;
  }
}

template <class E>
static int run_finish(const WgradArgs& a, hipStream_t s) {
  if (a.gb != nullptr) {
    int cp = 1;
    while (cp < a.Cout) cp <<= 1;                                // <= 256 = BLOCK
    hipLaunchKernelGGL(bias_kernel<E>, dim3((unsigned)a.parts), dim3(BLOCK), 0, s, a, cp);
  }
  const long long threads = (long long)a.K * a.Cin * a.Cout + a.Cout;
  hipLaunchKernelGGL(wfinish_kernel, dim3((unsigned)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

int finish_wgrad(const WgradArgs& a, int32_t dtype, hipStream_t s) {
  return sparse_elem::with_elem(dtype, [&](auto e) { return run_finish<decltype(e)>(a, s); });
}

template <class E>
static int run_wgrad(WgradArgs& a, hipStream_t s) {
  const int to = tile_of(a.Cout);
  switch (tile_of(a.Cin)) {
    case 16: launch_wgrad_in<E, 16>(a, to, s); break;
    case 32: launch_wgrad_in<E, 32>(a, to, s); break;
    default: launch_wgrad_in<E, 64>(a, to, s); break;
  }
  return run_finish<E>(a, s);
}

// elem 4: fp32 operands, dtype 0; elem 2: dtype GD3D_DTYPE_F16 / GD3D_DTYPE_BF16
static int backward_weight(size_t elem, int32_t dtype, const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num,
                           int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight, float* grad_bias,
                           hipStream_t s) {
  bool run;
  const int rc = check_wgrad_call(elem, dtype, N, R, K, Cin, Cout, features, grad_out, nbr, workspace, true, grad_weight, &run);
  if (rc != 0) return rc;
  if (!run) return zero_wgrad(K, Cin, Cout, grad_weight, grad_bias, s);
  WgradArgs a;
  fill_args(a, features, grad_out, nbr, num, N, R, K, Cin, Cout, workspace, grad_weight, grad_bias);
  return sparse_elem::with_elem(dtype, [&](auto e) { return run_wgrad<decltype(e)>(a, s); });
}

}  // namespace sparse_conv

using namespace sparse_conv;

extern "C" {

size_t gd3d_sparse_conv_backward_weight_workspace_bytes(int64_t R, int32_t K, int32_t Cin, int32_t Cout) {
  if (R <= 0 || check_channels(K, Cin, Cout) != 0) return 256;
  const int64_t kcc = (int64_t)K * Cin * Cout;
  WgradArgs a;
  a.Cout = Cout;
  weight_parts(R, kcc, (int64_t*)&a.parts, (int64_t*)&a.chunk);
  return carve(a, nullptr, kcc);
}

int gd3d_sparse_conv_backward_weight(const float* features, const float* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                     int64_t R, int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight,
                                     float* grad_bias, void* stream) {
  return backward_weight(4, 0, features, grad_out, nbr, num, N, R, K, Cin, Cout, workspace, grad_weight, grad_bias, (hipStream_t)stream);
}

int gd3d_sparse_conv_backward_weight_16(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                        int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                        float* grad_weight, float* grad_bias, void* stream) {
  return backward_weight(2, dtype, features, grad_out, nbr, num, N, R, K, Cin, Cout, workspace, grad_weight, grad_bias, (hipStream_t)stream);
}

}  // extern "C"
