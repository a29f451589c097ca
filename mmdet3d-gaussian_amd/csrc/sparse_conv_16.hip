// sparse_conv_16.hip — the fp16 / bf16 forms of the sparse 3D convolution (include/gd3d.h, gd3d_sparse_conv_*_16)
// for gfx950: the forward and input-gradient implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}, the two-stage weight gradient on 16-bit
// operands, and dense() with its backward for 2-byte elements.  The tables are those of csrc/sparse_conv.hip's index build.
//   gemm_kernel   output stationary.  A workgroup of 4 waves owns ROWS = 128 rows x TN = 16, 32 or 64 output channels (the smallest tile
//                 that holds Cout); a wave owns RT = 2 tiles of 16 rows.  The reduction axis is the concatenation (offset j, channel c),
//                 K * Cr long, walked 32 at a time.  A operand: lane l loads the 16-byte piece src[table[row l&15][j]][c .. c+7] of its
//                 gathered row straight from global memory (k = 8 (l >> 4) .. + 7 of the step: the instruction's own A map), zeros for
//                 a missing neighbour and past the end of the axis; a step in which none of the wave's rows has a neighbour is skipped
//                 wave-uniformly.  B operand: the weight slab of a chunk of the axis (the whole weight where it fits 32 KB, else 128
//                 elements = 4 steps) is staged in LDS TRANSPOSED — Wt[column][k] — so that a lane's 8 consecutive k of column l&15
//                 are one 16-byte LDS read (staged 16 bytes a load where the weight's alignment and shape allow, else element by
//                 element); a chunk no row of the workgroup uses is not staged.  C/D: col = lane & 15,
//                 row = (lane >> 4) * 4 + reg; the epilogue adds the fp32 bias to live rows, rounds once to the 16-bit type, turns
//                 the tile through LDS and writes every element of every row once, 16 bytes a lane.  The input gradient is the same
//                 kernel over the transposed table and weight.  No atomics: the bits replay.
//                 Cr % 8 != 0 or a misaligned base: the gather loads element by element; Co % 8 != 0 or a misaligned output: the
//                 stores are element by element.  Same arithmetic on either path.
//                 FUSED (gd3d_sparse_conv_forward_fused_16): the forward form with a per-channel scale, a residual row
//                 and a ReLU in the epilogue, the tile staged unrounded in fp32 — a compile-time variant, the plain instances keep their code.
//   wgrad_kernel  csrc/sparse_conv.hip's scheme and summation order on operands widened from 16 bits (the products of two 16-bit
//                 values are exact in fp32): partial sums per chunk of rows, wfinish_kernel adds them in ascending order.  fp32 out.
//   dense_kernel  the copy kernels for 2-byte elements.
// Compiled with -ffp-contract=off; the multiply-adds of the weight gradient are explicit fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "sparse_conv_common.h"

namespace sparse_conv16 {

using namespace sparse_conv;

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int RT = 2;                       // 16-row tiles of one wave
constexpr int ROWS = TILE_M16;              // output rows of one workgroup
constexpr int CHUNK = 128;                  // reduction elements of one staged weight slab where the whole weight does not fit
constexpr int PAD = 8;                      // elements between the rows of an LDS image: 16 bytes, keeps every piece 16-byte aligned
constexpr int WHOLE_BYTES = 32 << 10;       // a weight slab up to this size stays in LDS for the whole workgroup
static_assert(ROWS == WAVES * RT * 16, "TILE_M16 is the row tile of this kernel");
static_assert(ROWS <= BLOCK, "one thread per row in the prologue");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the two element types: 16-bit storage as uint16_t, one rounding to nearest even on the way out
struct F16 {
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
  static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
struct BF16 {
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
  static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
};

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static unsigned blocks_of(long long threads) { return (unsigned)((threads + BLOCK - 1) / BLOCK); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static int tile_of(int channels) { return channels <= 16 ? 16 : (channels <= 32 ? 32 : 64); }

__device__ __forceinline__ long long row_limit(const long long* num, long long rows) {
  if (num == nullptr) return rows;
  const long long k = num[0];
  return k < rows ? (k < 0 ? 0 : k) : rows;
}

// ---- the implicit GEMM ---------------------------------------------------------------------------------------------------------------

struct GemmArgs {
  const uint16_t* src;     // (n_src, Cr): the rows gathered
  const uint16_t* W;       // (K, Cin, Cout)
  const float* bias;       // (Co) fp32 or null
  const int32_t* table;    // (rows, K)
  const long long* num;    // nullable: rows at and past num[0] are zeros
  long long n_src, rows;
  int K, Cr, Co, flip;     // flip: the table's column of offset j is K - 1 - j (the submanifold transpose)
  int chunk;               // reduction elements of one staged slab, a multiple of 32
  int vec_in, vec_out;     // Cr % 8 == 0 and src 16-byte aligned; Co % 8 == 0 and out 16-byte aligned
  int vec_w;               // W 16-byte aligned and 8 | its contiguous axis as the kernel reads it (Co forward, Cr transposed)
  uint16_t* out;           // (rows, Co)
  // the FUSED epilogue only: t = fmaf(acc, scale, bias) (+ residual), ReLU, one rounding; `bias` is the folded shift
  const float* scale;      // (Co) fp32 or null
  const uint16_t* residual;   // (rows, Co) or null; read at live rows only
  int act;                 // GD3D_ACT_*
  int vec_res;             // Co % 8 == 0 and `residual` 16-byte aligned: independent of vec_out
};

constexpr int FPAD = 4;                     // floats between the rows of the fused epilogue's fp32 tile: rows stay 16-byte aligned, and the 4 rows
                                            // between two lane groups are 16 banks apart (TN + 4 = 4 mod 8): a half-wave's ds_write_b32 do not conflict

// TRANS: the weight is read transposed (the input gradient: Cr = Cout, Co = Cin).
// FUSED (gd3d_sparse_conv_forward_fused_16): a lane applies scale and shift to its accumulators and stages them
// UNROUNDED, in fp32, in the per-wave tile; the row-major read-back adds the residual (16 bytes a load), applies the ReLU, rounds ONCE
// and stores 16 bytes a lane.  A compile-time variant: the plain instances keep their code.
template <class E, bool TRANS, int TN, bool FUSED = false>
__global__ __launch_bounds__(BLOCK) void gemm_kernel(const GemmArgs a) {
  constexpr int NT = TN / 16, OP = TN + PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int nb[ROWS * MAX_K];                               // the workgroup's rows of the table, -1 for everything invalid
  __shared__ int live[ROWS];
  uint16_t* Wt = reinterpret_cast<uint16_t*>(smem);              // [TN][chunk + PAD]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r16 = lane & 15, g = lane >> 4;
  const long long row0 = (long long)blockIdx.x * ROWS;
  const int col0 = blockIdx.y * TN;
  const int KT = a.K * a.Cr, KTP = (KT + 31) & ~31, CH = a.chunk, CHP = CH + PAD;
  const long long limit = row_limit(a.num, a.rows);
  if (t < ROWS) live[t] = 0;
  __syncthreads();
  for (int idx = t; idx < ROWS * a.K; idx += BLOCK) {
    const int r = idx / a.K, j = idx - r * a.K;
    int v = -1;
    if (row0 + r < limit) {
      v = a.table[(row0 + r) * a.K + (a.flip ? a.K - 1 - j : j)];
      if (v < 0 || v >= a.n_src) v = -1;
    }
    nb[r * MAX_K + j] = v;
    if (v >= 0) live[r] = 1;
  }
  __syncthreads();
  f32x4 acc[RT][NT];
  for (int rt = 0; rt < RT; ++rt)
    for (int n = 0; n < NT; ++n) acc[rt][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = 0; k0 < KTP; k0 += CH) {                         // k0, kn: the same for the whole workgroup
    const int kn = KTP - k0 < CH ? KTP - k0 : CH;
    int need = 0;
    if (t < ROWS) {
      const int j_lo = k0 / a.Cr;
      int j_hi = (k0 + kn - 1) / a.Cr;
      j_hi = j_hi < a.K - 1 ? j_hi : a.K - 1;
      for (int j = j_lo; j <= j_hi; ++j) need |= nb[t * MAX_K + j] >= 0;
    }
    if (!__syncthreads_or(need)) continue;                       // the barrier also ends every read of the previous slab
    if (a.vec_w) {                                               // 8 elements a load; the same image as the element-wise staging below
      for (int idx = t; idx < kn * TN / 8; idx += BLOCK) {
        u32x4 w = u32x4{0u, 0u, 0u, 0u};
        if (TRANS) {                                             // 8 | Cr: 8 consecutive k of one column lie in one offset, contiguous in memory
          const int c = idx / (kn / 8), kk = (idx - c * (kn / 8)) * 8, k = k0 + kk;
          if (k < KT && col0 + c < a.Co) {
            const int j = k / a.Cr, cr = k - j * a.Cr;
            w = *reinterpret_cast<const u32x4*>(a.W + ((long long)j * a.Co + col0 + c) * a.Cr + cr);
          }
          *reinterpret_cast<u32x4*>(Wt + c * CHP + kk) = w;
        } else {                                                 // 8 | Co: 8 consecutive columns of one k
          const int kk = idx / (TN / 8), c = (idx - kk * (TN / 8)) * 8, k = k0 + kk;
          if (k < KT && col0 + c < a.Co) {
            const int j = k / a.Cr, cr = k - j * a.Cr;
            w = *reinterpret_cast<const u32x4*>(a.W + ((long long)j * a.Cr + cr) * a.Co + col0 + c);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            Wt[(c + 2 * q) * CHP + kk] = (uint16_t)(w[q] & 0xffffu);
            Wt[(c + 2 * q + 1) * CHP + kk] = (uint16_t)(w[q] >> 16);
          }
        }
      }
    } else {
      for (int idx = t; idx < kn * TN; idx += BLOCK) {
        int kk, c;
        if (TRANS) { c = idx / kn; kk = idx - c * kn; } else { kk = idx / TN; c = idx - kk * TN; }
        const int k = k0 + kk;
        uint16_t w = 0;                                          // zeros past the axis and past Co: 0 * 0, never 0 * garbage
        if (k < KT && col0 + c < a.Co) {
          const int j = k / a.Cr, cr = k - j * a.Cr;
          w = TRANS ? a.W[((long long)j * a.Co + col0 + c) * a.Cr + cr] : a.W[((long long)j * a.Cr + cr) * a.Co + col0 + c];
        }
        Wt[c * CHP + kk] = w;
      }
    }
    __syncthreads();
    for (int kk = 0; kk < kn; kk += 32) {
      const int k = k0 + kk + 8 * g;                             // this lane's 8 elements of the step
      u32x4 af[RT];
      bool any = false;
      if (a.vec_in) {                                            // 8 | Cr: the 8 elements lie in one offset
        const int j = k / a.Cr, cr = k - j * a.Cr;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          af[rt] = u32x4{0u, 0u, 0u, 0u};
          const int v = k < KT ? nb[((wave * RT + rt) * 16 + r16) * MAX_K + j] : -1;
          if (v >= 0) {
            af[rt] = *reinterpret_cast<const u32x4*>(a.src + (long long)v * a.Cr + cr);
            any = true;
          }
        }
      } else {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          uint32_t e[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            e[q] = 0u;
            const int kq = k + q;
            if (kq < KT) {
              const int j = kq / a.Cr, cr = kq - j * a.Cr;
              const int v = nb[((wave * RT + rt) * 16 + r16) * MAX_K + j];
              if (v >= 0) {
                e[q] = a.src[(long long)v * a.Cr + cr];
                any = true;
              }
            }
          }
          af[rt] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
        }
      }
      if (__builtin_amdgcn_ballot_w64(any) == 0) continue;       // wave-uniform: none of the wave's rows has a neighbour here
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(Wt + (n * 16 + r16) * CHP + kk + 8 * g);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][n] = E::mfma(af[rt], b, acc[rt][n]);
      }
    }
  }
  __syncthreads();                                               // the slab is free: a wave turns its tiles through it
  if constexpr (FUSED) {
    constexpr int OPF = TN + FPAD;
    float* otf = reinterpret_cast<float*>(smem) + wave * 16 * OPF;   // [16][TN + FPAD] fp32
    const bool relu = a.act == GD3D_ACT_RELU;
    for (int rt = 0; rt < RT; ++rt) {
      const int rbase = (wave * RT + rt) * 16;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int c = n * 16 + r16;
        const bool in = col0 + c < a.Co;
        const float b = (a.bias != nullptr && in) ? a.bias[col0 + c] : 0.0f;
        const float sc = (a.scale != nullptr && in) ? a.scale[col0 + c] : 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = g * 4 + q;
          const float v = a.scale != nullptr ? __builtin_fmaf(acc[rt][n][q], sc, b) : acc[rt][n][q] + b;
          otf[r * OPF + c] = live[rbase + r] ? v : 0.0f;           // a row without neighbours stays zero: its residual is not read below
        }
      }
      __syncthreads();
      if (a.vec_out) {
        constexpr int PIECES = TN / 8;
        for (int idx = lane; idx < 16 * PIECES; idx += 64) {
          const int r = idx / PIECES, p = idx - r * PIECES;
          const long long row = row0 + rbase + r;
          const int c = col0 + p * 8;
          if (row < a.rows && c < a.Co) {                          // 8 | Co: a piece that starts inside the row ends inside it
            const f32x4 lo = *reinterpret_cast<const f32x4*>(otf + r * OPF + p * 8);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(otf + r * OPF + p * 8 + 4);
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if (a.residual != nullptr && live[rbase + r]) {
              const uint16_t* src = a.residual + row * a.Co + c;
              if (a.vec_res) {
                const u32x4 w = *reinterpret_cast<const u32x4*>(src);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  v[2 * i] = v[2 * i] + E::widen((uint16_t)(w[i] & 0xffffu));
                  v[2 * i + 1] = v[2 * i + 1] + E::widen((uint16_t)(w[i] >> 16));
                }
              } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = v[i] + E::widen(src[i]);
              }
            }
            uint32_t h[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = E::narrow(relu && v[i] < 0.0f ? 0.0f : v[i]);
            *reinterpret_cast<u32x4*>(a.out + row * a.Co + c) = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
          }
        }
      } else {
        for (int idx = lane; idx < 16 * TN; idx += 64) {
          const int r = idx / TN, c = idx - r * TN;
          const long long row = row0 + rbase + r;
          if (row < a.rows && col0 + c < a.Co) {
            float v = otf[r * OPF + c];
            if (a.residual != nullptr && live[rbase + r]) v = v + E::widen(a.residual[row * a.Co + col0 + c]);
            a.out[row * a.Co + col0 + c] = E::narrow(relu && v < 0.0f ? 0.0f : v);
          }
        }
      }
      __syncthreads();
    }
    return;
  }
  uint16_t* ot =reinterpret_cast<uint16_t*>(smem) + wave * 16 * OP;   // [16][TN + PAD]
  for (int rt = 0; rt < RT; ++rt) {
    const int rbase = (wave * RT + rt) * 16;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int c = n * 16 + r16;
      const float b = (a.bias != nullptr && col0 + c < a.Co) ? a.bias[col0 + c] : 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = g * 4 + q;                                 // a row without neighbours (inactive, or past the count) is zero, bias or not
        ot[r * OP + c] = live[rbase + r] ? E::narrow(acc[rt][n][q] + b) : (uint16_t)0;
      }
    }
    __syncthreads();
    if (a.vec_out) {
      constexpr int PIECES = TN / 8;
      for (int idx = lane; idx < 16 * PIECES; idx += 64) {
        const int r = idx / PIECES, p = idx - r * PIECES;
        const long long row = row0 + rbase + r;
        const int c = col0 + p * 8;
        if (row < a.rows && c < a.Co)
          *reinterpret_cast<u32x4*>(a.out + row * a.Co + c) = *reinterpret_cast<const u32x4*>(ot + r * OP + p * 8);
      }
    } else {
      for (int idx = lane; idx < 16 * TN; idx += 64) {
        const int r = idx / TN, c = idx - r * TN;
        const long long row = row0 + rbase + r;
        if (row < a.rows && col0 + c < a.Co) a.out[row * a.Co + col0 + c] = ot[r * OP + c];
      }
    }
    __syncthreads();
  }
}

// fused: the forward form with the FUSED epilogue (never transposed)
template <class E, int TN>
static int launch_gemm_tile(GemmArgs& a, bool trans, bool fused, hipStream_t s) {
  const int ktp = (a.K * a.Cr + 31) & ~31;
  a.chunk = (size_t)TN * (ktp + PAD) * 2 <= (size_t)WHOLE_BYTES ? ktp : CHUNK;
  size_t lds = (size_t)TN * (a.chunk + PAD) * 2;
  const size_t turn = fused ? (size_t)WAVES * 16 * (TN + FPAD) * 4     // the epilogue's tiles lie in the same bytes: fp32 in the fused form
                            : (size_t)WAVES * 16 * (TN + PAD) * 2;
  lds = lds > turn ? lds : turn;
  const dim3 grid((unsigned)((a.rows + ROWS - 1) / ROWS), (unsigned)((a.Co + TN - 1) / TN));
  if (fused) hipLaunchKernelGGL((gemm_kernel<E, false, TN, true>), grid, dim3(BLOCK), lds, s, a);
  else if (trans) hipLaunchKernelGGL((gemm_kernel<E, true, TN>), grid, dim3(BLOCK), lds, s, a);
  else hipLaunchKernelGGL((gemm_kernel<E, false, TN>), grid, dim3(BLOCK), lds, s, a);
  return (int)hipGetLastError();
}

template <class E>
static int launch_gemm(GemmArgs& a, bool trans, hipStream_t s, bool fused = false) {
  a.vec_in = a.Cr % 8 == 0 && aligned16(a.src);
  a.vec_out = a.Co % 8 == 0 && aligned16(a.out);
  a.vec_w = (trans ? a.Cr : a.Co) % 8 == 0 && aligned16(a.W);
  a.vec_res = fused && a.residual != nullptr && a.Co % 8 == 0 && aligned16(a.residual);
  switch (tile_of(a.Co)) {
    case 16: return launch_gemm_tile<E, 16>(a, trans, fused, s);
    case 32: return launch_gemm_tile<E, 32>(a, trans, fused, s);
    default: return launch_gemm_tile<E, 64>(a, trans, fused, s);
  }
}

// ---- the weight gradient ---------------------------------------------------------------------------------------------------------------

struct WgradArgs {
  const uint16_t *X, *gY;
  const int32_t* nbr;
  const long long* num;
  long long n_src, rows, chunk, parts;
  int K, Cin, Cout, tiles_co;
  float *part_w, *part_b;   // (parts, K, Cin, Cout) and (parts, Cout)
  float *gW, *gb;           // gb nullable
};

// csrc/sparse_conv.hip's wgrad_kernel on operands widened from 16 bits: the same tiles, the same order of the fmaf
template <class E, int TI, int TO>
__global__ __launch_bounds__(BLOCK) void wgrad_kernel(const WgradArgs a) {
  constexpr int MI = TI / 16, MO = TO / 16;
  __shared__ int nb[WG_ROWS];
  __shared__ float Xg[WG_ROWS][TI];
  __shared__ float Gy[WG_ROWS][TO];
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
      Xg[r][c] = (row >= 0 && ci0 + c < a.Cin) ? E::widen(a.X[(long long)row * a.Cin + ci0 + c]) : 0.0f;
    }
    for (int idx = t; idx < WG_ROWS * TO; idx += BLOCK) {
      const int r = idx / TO, c = idx % TO;
      Gy[r][c] = (nb[r] >= 0 && co0 + c < a.Cout) ? E::widen(a.gY[(r0 + r) * a.Cout + co0 + c]) : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < WG_ROWS; ++r) {
      float x[MI], gy[MO];
#pragma unroll
      for (int i = 0; i < MI; ++i) x[i] = Xg[r][ty * MI + i];
#pragma unroll
      for (int q = 0; q < MO; ++q) gy[q] = Gy[r][tx * MO + q];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < MO; ++q) acc[i][q] = __builtin_fmaf(x[i], gy[q], acc[i][q]);
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

template <class E>
static void launch_wgrad(WgradArgs& a, hipStream_t s) {
  const int to = tile_of(a.Cout);
  switch (tile_of(a.Cin)) {
    case 16: launch_wgrad_in<E, 16>(a, to, s); break;
    case 32: launch_wgrad_in<E, 32>(a, to, s); break;
    default: launch_wgrad_in<E, 64>(a, to, s); break;
  }
}

// csrc/sparse_conv.hip's bias_kernel on a widened grad_out
template <class E>
__global__ __launch_bounds__(BLOCK) void bias_kernel(const WgradArgs a, const int CP) {
  __shared__ int live[BLOCK];
  __shared__ float red[BLOCK];
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
        if (live[r]) acc += E::widen(a.gY[(r0 + r) * a.Cout + col]);
    __syncthreads();
  }
  red[t] = acc;
  __syncthreads();
  if (grp == 0 && col < a.Cout) {
    float s = 0.0f;
    for (int gi = 0; gi < groups; ++gi) s += red[gi * CP + col];
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
static int run_wgrad(WgradArgs& a, hipStream_t s) {
  launch_wgrad<E>(a, s);
  if (a.gb != nullptr) {
    int cp = 1;
    while (cp < a.Cout) cp <<= 1;                                // <= 256 = BLOCK
    hipLaunchKernelGGL(bias_kernel<E>, dim3((unsigned)a.parts), dim3(BLOCK), 0, s, a, cp);
  }
  hipLaunchKernelGGL(wfinish_kernel, dim3(blocks_of((long long)a.K * a.Cin * a.Cout + a.Cout)), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

// ---- dense() ---------------------------------------------------------------------------------------------------------------------------

// a thread per (row, channel); BACKWARD: the gather
template <bool BACKWARD>
__global__ __launch_bounds__(BLOCK) void dense_kernel(const uint16_t* __restrict__ src, const int32_t* __restrict__ coors, long long n, int C,
                                                      const Geo g, uint16_t* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * C) return;
  const long long i = t / C;
  const int ch = (int)(t - i * C);
  const int32_t* c = coors + i * 4;
  const bool in = row_active(c, g);
  const long long plane = (long long)g.n[0] * g.n[1] * g.n[2];
  const long long at = in ? ((long long)c[0] * C + ch) * plane + ((long long)c[1] * g.n[1] + c[2]) * g.n[2] + c[3] : 0;
  if (BACKWARD) dst[t] = in ? src[at] : (uint16_t)0;
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

static int dense_geo(int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W, Geo* g) {
  const int32_t shape[3] = {D, H, W}, one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
  if (C < 1) return GD3D_E_BADARG;
  if (C > MAX_C) return GD3D_E_TOOLARGE;
  const int rc = make_geo(N, B, shape, one, one, zero, 0, g);
  if (rc != 0) return rc;
  if (g->in_sent > (1LL << 62) / C || N * C > (1LL << 40)) return GD3D_E_TOOLARGE;
  return 0;
}

static bool dtype_ok(int32_t dtype) { return dtype == GD3D_DTYPE_F16 || dtype == GD3D_DTYPE_BF16; }

}  // namespace sparse_conv16

using namespace sparse_conv16;

extern "C" {

int gd3d_sparse_conv_forward_16(const void* features, const void* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* out, void* stream) {
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!dtype_ok(dtype) || N < 0 || R < 0) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || R * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (R == 0) return 0;
  if (weight == nullptr || nbr == nullptr || out == nullptr || (N > 0 && features == nullptr)) return GD3D_E_BADARG;
  if ((((uintptr_t)features | (uintptr_t)weight | (uintptr_t)out) & 1u) != 0) return GD3D_E_BADARG;
  GemmArgs a;
  a.src = (const uint16_t*)features; a.W = (const uint16_t*)weight; a.bias = bias; a.table = nbr; a.num = (const long long*)num;
  a.n_src = N; a.rows = R; a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = (uint16_t*)out;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, false, (hipStream_t)stream) : launch_gemm<BF16>(a, false, (hipStream_t)stream);
}

int gd3d_sparse_conv_forward_fused_16(const void* features, const void* weight, const float* scale, const float* shift, const void* residual,
                                      const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout,
                                      int32_t act, int32_t dtype, void* out, void* stream) {
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!dtype_ok(dtype) || N < 0 || R < 0 || (act != GD3D_ACT_NONE && act != GD3D_ACT_RELU)) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || R * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (R == 0) return 0;
  if (weight == nullptr || nbr == nullptr || out == nullptr || (N > 0 && features == nullptr)) return GD3D_E_BADARG;
  if ((((uintptr_t)features | (uintptr_t)weight | (uintptr_t)residual | (uintptr_t)out) & 1u) != 0) return GD3D_E_BADARG;
  if (residual != nullptr && ranges_overlap(residual, out, sizeof(uint16_t) * (size_t)R * (size_t)Cout)) return GD3D_E_BADARG;
  GemmArgs a;
  a.src = (const uint16_t*)features; a.W = (const uint16_t*)weight; a.bias = shift; a.table = nbr; a.num = (const long long*)num;
  a.n_src = N; a.rows = R; a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = (uint16_t*)out;
  a.scale = scale; a.residual = (const uint16_t*)residual; a.act = act;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, false, (hipStream_t)stream, true) : launch_gemm<BF16>(a, false, (hipStream_t)stream, true);
}

int gd3d_sparse_conv_backward_input_16(const void* grad_out, const void* weight, const int32_t* table, int32_t flip, int64_t N,
                                       int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* grad_features,
                                       void* stream) {
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!dtype_ok(dtype) || N < 0 || R < 0 || (flip && N != R)) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || N * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (N == 0) return 0;
  if (weight == nullptr || table == nullptr || grad_features == nullptr || (R > 0 && grad_out == nullptr)) return GD3D_E_BADARG;
  if ((((uintptr_t)grad_out | (uintptr_t)weight | (uintptr_t)grad_features) & 1u) != 0) return GD3D_E_BADARG;
  GemmArgs a;
  a.src = (const uint16_t*)grad_out; a.W = (const uint16_t*)weight; a.bias = nullptr; a.table = table; a.num = nullptr;
  a.n_src = R; a.rows = N; a.K = K; a.Cr = Cout; a.Co = Cin; a.flip = flip ? 1 : 0; a.out = (uint16_t*)grad_features;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, true, (hipStream_t)stream) : launch_gemm<BF16>(a, true, (hipStream_t)stream);
}

int gd3d_sparse_conv_backward_weight_16(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                        int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                        float* grad_weight, float* grad_bias, void* stream) {
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!dtype_ok(dtype) || N < 0 || R < 0 || grad_weight == nullptr) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || R * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t kcc = (int64_t)K * Cin * Cout;
  if (R == 0 || N == 0) {                                        // no pair: the gradients are zeros
    int e = gd3d::fill_words(grad_weight, sizeof(float) * (size_t)kcc, 0u, s);
    if (e == 0 && grad_bias != nullptr) e = gd3d::fill_words(grad_bias, sizeof(float) * (size_t)Cout, 0u, s);
    return e;
  }
  if (features == nullptr || grad_out == nullptr || nbr == nullptr || workspace == nullptr || ((uintptr_t)workspace & 255) != 0)
    return GD3D_E_BADARG;
  if ((((uintptr_t)features | (uintptr_t)grad_out) & 1u) != 0) return GD3D_E_BADARG;
  WgradArgs a;
  a.X = (const uint16_t*)features; a.gY = (const uint16_t*)grad_out; a.nbr = nbr; a.num = (const long long*)num; a.n_src = N; a.rows = R;
  weight_parts(R, kcc, (int64_t*)&a.parts, (int64_t*)&a.chunk);
  a.K = K; a.Cin = Cin; a.Cout = Cout; a.tiles_co = 1;
  a.part_w = (float*)workspace;
  a.part_b = (float*)((char*)workspace + up256(sizeof(float) * (size_t)a.parts * (size_t)kcc));
  a.gW = grad_weight; a.gb = grad_bias;
  return dtype == GD3D_DTYPE_F16 ? run_wgrad<F16>(a, s) : run_wgrad<BF16>(a, s);
}

int gd3d_sparse_to_dense_16(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                            void* dense, void* stream) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (dense == nullptr || ((uintptr_t)dense & 1u) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int e = fill_zero16((uint16_t*)dense, (size_t)g.in_sent * (size_t)C, s);
  if (e != 0 || N == 0) return e;
  if (features == nullptr || coors == nullptr || ((uintptr_t)features & 1u) != 0) return GD3D_E_BADARG;
  hipLaunchKernelGGL(dense_kernel<false>, dim3(blocks_of(N * C)), dim3(BLOCK), 0, s, (const uint16_t*)features, coors, (long long)N, (int)C,
                     g, (uint16_t*)dense);
  return (int)hipGetLastError();
}

int gd3d_sparse_to_dense_backward_16(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                     int32_t W, void* grad_features, void* stream) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || grad_features == nullptr || (B > 0 && grad_dense == nullptr)) return GD3D_E_BADARG;
  if ((((uintptr_t)grad_dense | (uintptr_t)grad_features) & 1u) != 0) return GD3D_E_BADARG;
  hipLaunchKernelGGL(dense_kernel<true>, dim3(blocks_of(N * C)), dim3(BLOCK), 0, (hipStream_t)stream, (const uint16_t*)grad_dense, coors,
                     (long long)N, (int)C, g, (uint16_t*)grad_features);
  return (int)hipGetLastError();
}

}  // extern "C"
