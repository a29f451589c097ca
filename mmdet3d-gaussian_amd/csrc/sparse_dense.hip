// sparse_dense.hip — SparseConvTensor.dense() and its backward (include/gd3d.h, gd3d_sparse_to_dense*) for gfx950,
// one source for 4-byte and 2-byte elements: the values are copied as they are, so fp16 and bf16 share the uint16_t instance.
//   forward    zeros (the library's word fill; edge_kernel for an odd 2-byte element at either end), then dense_kernel scatters every
//              active row.  Active rows are unique: no two threads write one cell.
//   backward   dense_kernel<T, true> gathers; an inactive row gets zeros.
// Compiled with -ffp-contract=off as the rest of the sparse convolution; no arithmetic on values here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "sparse_conv_common.h"

namespace sparse_conv {

constexpr int BLOCK = 256;

static unsigned blocks_of(long long threads) { return (unsigned)((threads + BLOCK - 1) / BLOCK); }

// a thread per (row, channel); BACKWARD: the gather
template <class T, bool BACKWARD>
__global__ __launch_bounds__(BLOCK) void dense_kernel(const T* __restrict__ src, const int32_t* __restrict__ coors, long long n, int C,
                                                      const Geo g, T* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * C) return;
  const long long i = t / C;
  const int ch = (int)(t - i * C);
  const int32_t* c = coors + i * 4;
  const bool in = row_active(c, g);
  const long long plane = (long long)g.n[0] * g.n[1] * g.n[2];
  const long long at = in ? ((long long)c[0] * C + ch) * plane + ((long long)c[1] * g.n[1] + c[2]) * g.n[2] + c[3] : 0;
  if (BACKWARD) dst[t] = in ? src[at] : (T)0;
  else if (in) dst[at] = src[t];
}

// the element before the first and after the last whole word of a 2-byte buffer
__global__ void edge_kernel(uint16_t* head, uint16_t* tail) {
  if (head != nullptr) *head = 0;
  if (tail != nullptr) *tail = 0;
}

// n zeros of 2 bytes: whole words through the library's fill, an odd element at either end on its own
static int fill_zero16(uint16_t* p, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  uint16_t* head = ((uintptr_t)p & 2u) ? p : nullptr;
  uint16_t* body = head != nullptr ? p + 1 : p;
  const size_t rest = head != nullptr ? n - 1 : n;
  uint16_t* tail = (rest & 1) ? body + rest - 1 : nullptr;
  int e = 0;
  if (rest / 2 > 0) e = gd3d::fill_words(body, (rest / 2) * 4, 0u, s);
  if (e == 0 && (head != nullptr || tail != nullptr)) {
    hipLaunchKernelGGL(edge_kernel, dim3(1), dim3(1), 0, s, head, tail);
    e = (int)hipGetLastError();
  }
  return e;
}

// a 2-byte element at an odd address; 4-byte elements are taken as they come
template <class T>
static bool misplaced(const void* p) { return sizeof(T) == 2 && misaligned(p, 2); }

template <class T>
static int to_dense(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W, void* dense,
                    hipStream_t s) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (dense == nullptr || misplaced<T>(dense)) return GD3D_E_BADARG;
  const size_t cells = (size_t)g.in_sent * (size_t)C;
  int e;
  if constexpr (sizeof(T) == 2) e = fill_zero16((uint16_t*)dense, cells, s);
  else e = gd3d::fill_words(dense, sizeof(T) * cells, 0u, s);
  if (e != 0 || N == 0) return e;
  if (features == nullptr || coors == nullptr || misplaced<T>(features)) return GD3D_E_BADARG;
  hipLaunchKernelGGL((dense_kernel<T, false>), dim3(blocks_of(N * C)), dim3(BLOCK), 0, s, (const T*)features, coors, (long long)N, (int)C, g,
                     (T*)dense);
  return (int)hipGetLastError();
}

template <class T>
static int to_dense_backward(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                             void* grad_features, hipStream_t s) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || grad_features == nullptr || (B > 0 && grad_dense == nullptr)) return GD3D_E_BADARG;
  if (misplaced<T>(grad_dense) || misplaced<T>(grad_features)) return GD3D_E_BADARG;
  hipLaunchKernelGGL((dense_kernel<T, true>), dim3(blocks_of(N * C)), dim3(BLOCK), 0, s, (const T*)grad_dense, coors, (long long)N, (int)C, g,
                     (T*)grad_features);
  return (int)hipGetLastError();
}

}  // namespace sparse_conv

using namespace sparse_conv;

extern "C" {

int gd3d_sparse_to_dense(const float* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                         float* dense, void* stream) {
  return to_dense<float>(features, coors, N, C, B, D, H, W, dense, (hipStream_t)stream);
}

int gd3d_sparse_to_dense_backward(const float* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                  int32_t W, float* grad_features, void* stream) {
  return to_dense_backward<float>(grad_dense, coors, N, C, B, D, H, W, grad_features, (hipStream_t)stream);
}

int gd3d_sparse_to_dense_16(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                            void* dense, void* stream) {
  return to_dense<uint16_t>(features, coors, N, C, B, D, H, W, dense, (hipStream_t)stream);
}

int gd3d_sparse_to_dense_backward_16(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                     int32_t W, void* grad_features, void* stream) {
  return to_dense_backward<uint16_t>(grad_dense, coors, N, C, B, D, H, W, grad_features, (hipStream_t)stream);
}

}  // extern "C"
