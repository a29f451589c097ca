// sparse_conv_elem16.h — the two 16-bit element types of the sparse 3D convolution, shared by csrc/sparse_conv_16.hip
// (the matrix-core GEMM) and csrc/sparse_conv_wgrad.hip (the weight gradient on widened operands): 16-bit storage as uint16_t, an exact
// widening to fp32, ONE rounding to nearest even on the way out, and the type's v_mfma_f32_16x16x32.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sparse_conv16 {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct F16 {
  typedef uint16_t T;
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
  static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
struct BF16 {
  typedef uint16_t T;
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
  static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
};

}  // namespace sparse_conv16
