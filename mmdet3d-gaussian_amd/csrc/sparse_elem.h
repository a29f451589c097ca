// sparse_elem.h — the element types of the sparse stack, ONE definition for the device units (csrc/sparse_conv_16.hip,
// sparse_conv_wgrad.hip, sparse_bn.hip, sparse_pool.hip) and their `_cpu` twins: fp32, and fp16 / bf16 stored as uint16_t with an exact
// widening to fp32 and ONE rounding to nearest even on the way out.  With them what every unit derives from the element size: the
// 16-byte pack and its load / store, the dtype and alignment tests of the entries, the lane layout of the row-sweeping kernels, and the
// step from a runtime `dtype` to a policy type.
// A policy's body is the device's expression in device code and the host's in host code, as they have always differed: the device casts
// ((_Float16)x, (__bf16)x, __builtin_bit_cast), the host goes through memcpy and rounds bf16 by explicit bit operations (fp16 through
// _Float16: F16C at x86-64-v3).  Both round to nearest even; the tests hold the two to each other.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gd3d.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SC_HD __host__ __device__ __forceinline__
#else
#define SC_HD inline
#endif

namespace sparse_elem {

#if defined(__HIPCC__)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#endif

// T: the stored element; WIDE: elements of a 16-byte piece; widen: exact; narrow: one rounding to nearest even; mfma (16-bit types,
// device only): the type's v_mfma_f32_16x16x32
struct F32 {
  typedef float T;
  static constexpr int WIDE = 4;
  static SC_HD float widen(float x) { return x; }
  static SC_HD float narrow(float x) { return x; }
};
struct F16 {
  typedef uint16_t T;
  static constexpr int WIDE = 8;
#if defined(__HIPCC__)
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
#endif
  static SC_HD float widen(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, h);
#else
    _Float16 v;
    memcpy(&v, &h, 2);
    return (float)v;
#endif
  }
  static SC_HD uint16_t narrow(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint16_t, (_Float16)x);
#else
    const _Float16 v = (_Float16)x;
    uint16_t h;
    memcpy(&h, &v, 2);
    return h;
#endif
  }
};
struct BF16 {
  typedef uint16_t T;
  static constexpr int WIDE = 8;
#if defined(__HIPCC__)
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
#endif
  static SC_HD float widen(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, (uint32_t)h << 16);
#else
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
  }
  static SC_HD uint16_t narrow(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint16_t, (__bf16)x);
#else
    uint32_t u;                            // round to nearest even; inf stays inf, a NaN stays a (quiet) NaN
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
#endif
  }
};

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// V adjacent elements at p[at] as they are stored: one 16-byte load where `wide`, V element loads otherwise (V == 1: the element)
template <typename T, int V>
SC_HD void load(const T* p, long long at, bool wide, T* out) {
  if (V > 1 && wide) {
    const Pack<T, V> k = *reinterpret_cast<const Pack<T, V>*>(p + at);
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = k.v[v];
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = p[at + v];
  }
}

template <typename T, int V>
SC_HD void store(T* p, long long at, bool wide, const T* in) {
  if (V > 1 && wide) {
    Pack<T, V> k;
#pragma unroll
    for (int v = 0; v < V; ++v) k.v[v] = in[v];
    *reinterpret_cast<Pack<T, V>*>(p + at) = k;
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) p[at + v] = in[v];
  }
}

// the same pair through fp32, named by the policy E instead of the stored type: widened after the load, narrowed before the store.
// Written out, not layered on the pair above: through a temporary of E::T the 16-byte instances of BatchNorm's kernels come out with
// other register numbers.
template <typename E, int V>
SC_HD void load(const typename E::T* p, long long at, bool wide, float* out) {
  if (V > 1 && wide) {
    const Pack<typename E::T, V> k = *reinterpret_cast<const Pack<typename E::T, V>*>(p + at);
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = E::widen(k.v[v]);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = E::widen(p[at + v]);
  }
}

template <typename E, int V>
SC_HD void store(typename E::T* p, long long at, bool wide, const float* in) {
  if (V > 1 && wide) {
    Pack<typename E::T, V> k;
#pragma unroll
    for (int v = 0; v < V; ++v) k.v[v] = E::narrow(in[v]);
    *reinterpret_cast<Pack<typename E::T, V>*>(p + at) = k;
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) p[at + v] = E::narrow(in[v]);
  }
}

// ---- what an entry asks of a dtype code and of a pointer (host) ----------------------------------------------------------------------

inline bool is_16bit(int32_t dtype) { return dtype == GD3D_DTYPE_F16 || dtype == GD3D_DTYPE_BF16; }
inline bool dtype_ok(int32_t dtype) { return dtype == 0 || is_16bit(dtype); }
inline size_t elem_size(int32_t dtype) { return dtype == 0 ? 4 : 2; }
inline bool misaligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) != 0; }   // to: a power of two; a null pointer is aligned
inline unsigned wide_bit(const void* p, unsigned bit) { return p != nullptr && !misaligned(p, 16) ? bit : 0u; }   // `bit` where p's base takes 16-byte accesses

// the lane layout of a row-sweeping workgroup of `block` threads: a lane owns `vec` adjacent channels of one row (16 bytes where the
// row pitch allows it, else one element), `groups` lanes cover a row, the workgroup covers `rows` rows at a time (tests name their row
// counts from it).  It depends on C and the element size alone.
struct Lanes {
  int vec, groups, rows;
};

inline Lanes lanes_of(int32_t C, int32_t dtype, int block) {
  const int wide = 16 / (int)elem_size(dtype);
  Lanes l;
  l.vec = C % wide == 0 ? wide : 1;
  l.groups = C / l.vec;
  l.rows = block / l.groups;
  return l;
}

// f(E()) with E the policy of a dtype code that passed dtype_ok: `with_elem(dtype, [&](auto e) { return run<decltype(e)>(...); })`
template <typename F>
inline auto with_elem(int32_t dtype, F&& f) {
  switch (dtype) {
    case 0: return f(F32());
    case GD3D_DTYPE_F16: return f(F16());
    default: return f(BF16());
  }
}

}  // namespace sparse_elem
