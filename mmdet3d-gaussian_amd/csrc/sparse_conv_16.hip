// sparse_conv_16.hip — the fp16 / bf16 forms of the sparse 3D convolution (include/gd3d.h, gd3d_sparse_conv_*_16)
// for gfx950: the forward and input-gradient implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}.  The tables are those of
// csrc/sparse_conv.hip's index build, the element types those of csrc/sparse_elem.h; the weight gradient on 16-bit operands is
// csrc/sparse_conv_wgrad.hip's, dense() for 2-byte elements csrc/sparse_dense.hip's.
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
// Compiled with -ffp-contract=off: the epilogues' fp32 sequences are written out, the fused one's multiply-add as an explicit fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "sparse_conv_common.h"

namespace sparse_conv16 {

using namespace sparse_conv;
using namespace sparse_elem;

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int RT = 2;                       // 16-row tiles of one wave
constexpr int ROWS = TILE_M16;              // output rows of one workgroup
constexpr int CHUNK = 128;                  // reduction elements of one staged weight slab where the whole weight does not fit
constexpr int PAD = 8;                      // elements between the rows of an LDS image: 16 bytes, keeps every piece 16-byte aligned
constexpr int WHOLE_BYTES = 32 << 10;       // a weight slab up to this size stays in LDS for the whole workgroup
static_assert(ROWS == WAVES * RT * 16, "TILE_M16 is the row tile of this kernel");
static_assert(ROWS <= BLOCK, "one thread per row in the prologue");

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

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

}  // namespace sparse_conv16

using namespace sparse_conv16;

extern "C" {

int gd3d_sparse_conv_forward_16(const void* features, const void* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* out, void* stream) {
  bool run;
  const int rc = check_gemm_call(2, dtype, R, N, K, Cin, Cout, true, features, weight, nbr, nullptr, out, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = (const uint16_t*)features; a.W = (const uint16_t*)weight; a.bias = bias; a.table = nbr; a.num = (const long long*)num;
  a.n_src = N; a.rows = R; a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = (uint16_t*)out;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, false, (hipStream_t)stream) : launch_gemm<BF16>(a, false, (hipStream_t)stream);
}

int gd3d_sparse_conv_forward_fused_16(const void* features, const void* weight, const float* scale, const float* shift, const void* residual,
                                      const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout,
                                      int32_t act, int32_t dtype, void* out, void* stream) {
  bool run;
  const int rc = check_gemm_call(2, dtype, R, N, K, Cin, Cout, act_ok(act), features, weight, nbr, residual, out, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = (const uint16_t*)features; a.W = (const uint16_t*)weight; a.bias = shift; a.table = nbr; a.num = (const long long*)num;
  a.n_src = N; a.rows = R; a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = (uint16_t*)out;
  a.scale = scale; a.residual = (const uint16_t*)residual; a.act = act;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, false, (hipStream_t)stream, true) : launch_gemm<BF16>(a, false, (hipStream_t)stream, true);
}

int gd3d_sparse_conv_backward_input_16(const void* grad_out, const void* weight, const int32_t* table, int32_t flip, int64_t N,
                                       int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* grad_features,
                                       void* stream) {
  bool run;
  const int rc = check_gemm_call(2, dtype, N, R, K, Cin, Cout, !flip || N == R, grad_out, weight, table, nullptr, grad_features, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = (const uint16_t*)grad_out; a.W = (const uint16_t*)weight; a.bias = nullptr; a.table = table; a.num = nullptr;
  a.n_src = R; a.rows = N; a.K = K; a.Cr = Cout; a.Co = Cin; a.flip = flip ? 1 : 0; a.out = (uint16_t*)grad_features;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE;
  return dtype == GD3D_DTYPE_F16 ? launch_gemm<F16>(a, true, (hipStream_t)stream) : launch_gemm<BF16>(a, true, (hipStream_t)stream);
}

}  // extern "C"
