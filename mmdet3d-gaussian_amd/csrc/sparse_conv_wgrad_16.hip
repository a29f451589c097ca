// sparse_conv_wgrad_16.hip — stage one of the sparse 3D convolution's weight gradient on the matrix cores, for fp16 / bf16 operands
// (include/gd3d.h, gd3d_sparse_conv_backward_weight_16_mfma) for gfx950.  The arguments, the chunks, the workspace,
// the bias gradient and the second stage are csrc/sparse_conv_wgrad.hip's (csrc/sparse_conv_wgrad.h): only the partial X^T gY of a
// (row chunk, offset j, channel tile) is computed here, on v_mfma_f32_16x16x32_{f16,bf16}, into the same part_w.
//   wgrad16_kernel  D[ci][co] += A[ci][k] B[k][co] with k the ROW axis, 32 rows a step.  Both operands are the transpose of how rows lie
//                 in memory: a wave gathers the step's X rows and gY rows row-major into ITS OWN LDS image as 16-bit elements (16 bytes a
//                 lane where the channel count and the base allow, else element by element; zeros for a row without the neighbour, past
//                 the count, past the chunk, and for channels past Cin / Cout — zeros on BOTH operands), and reads each fragment back with
//                 two ds_read_b64_tr_b16: a 16-lane group g takes the 4 x 16 blocks of rows 8g .. 8g+3 and 8g+4 .. 8g+7 of the tile's 16
//                 columns, lane i of the group receiving column i — its 8 consecutive k.  Wave w of the four walks the steps w, w+4, ...
//                 of the chunk; a step none of whose rows has the neighbour is skipped by a ballot; no workgroup barrier inside the loop.
//                 The four waves' accumulators are then added through LDS in ascending wave order and wave 0 stores the tile.
//                 The order of every addition is fixed by (R, K, Cin, Cout) alone: no atomics, the bits replay.
// Compiled with -ffp-contract=off, like its siblings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "sparse_conv_wgrad.h"

namespace sparse_conv_wgrad16 {

using namespace sparse_conv;
using namespace sparse_elem;

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int STEP = WG_ROWS;               // rows of one MFMA step: the instruction's k
static_assert(STEP == 32, "a step is the k extent of v_mfma_f32_16x16x32");

typedef short s16x4 __attribute__((ext_vector_type(4)));

// The LDS image of a step: STEP rows of T 16-bit elements, row-major in 32-byte pieces of 16 columns, the pieces placed so that the
// transposed read of one 32-lane half — rows r .. r+3 and r+8 .. r+11 of one piece, 8 bytes a lane — touches each of the 64 banks once:
//   T = 16 (32-byte rows, 8 banks): rows 8 .. 15 of every 16 swap their halves, so that rows r and r + 8 lie 4 rows + 8 rows apart;
//   T = 32 (16 banks a row): the row's two pieces swap where bit 3 of the row is set;
//   T = 64 (32 banks a row): piece ^ (bit 1 of the row | bit 3 of the row << 1).
// -> the element offset of (row, column); a multiple of 8 for a column that is one, so 16-byte pieces stay whole and aligned.
// (The other route — the image stored transposed, [column][STEP + 8], and one 16-byte read a fragment — was measured and is slower at
// every shape, by 1.6x at 64 -> 64: DESIGN.md §3.29.)
template <int T>
__device__ __forceinline__ int img_off(int r, int c) {
  if (T == 16) return ((r ^ (((r >> 3) & 1) << 2)) << 4) + c;
  if (T == 32) return r * 32 + ((((c >> 4) ^ ((r >> 3) & 1)) << 4) | (c & 15));
  return r * 64 + ((((c >> 4) ^ (((r >> 1) & 1) | (((r >> 3) & 1) << 1))) << 4) | (c & 15));
}

// the MFMA operand of columns c0 .. c0+15 of an image: lane l receives column c0 + (l & 15), rows 8 (l >> 4) .. + 7.  Every lane of the
// wave supplies an address inside the image, 8-byte aligned; EXEC is all ones at every call (the callers' loops are wave-uniform).
template <int T>
__device__ __forceinline__ u32x4 fragment(const uint16_t* img, int lane, int c0) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  lds_s16x4* lo = (lds_s16x4*)(img + img_off<T>(8 * g + q, c0 + 4 * p));
  lds_s16x4* hi = (lds_s16x4*)(img + img_off<T>(8 * g + 4 + q, c0 + 4 * p));
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(hi);
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 x = __builtin_bit_cast(u32x2, a), y = __builtin_bit_cast(u32x2, b);
  return u32x4{x[0], x[1], y[0], y[1]};
}

// One wave gathers STEP rows of `src` (row pitch C, columns c0 .. c0+T-1), 16 bytes a lane and STEP * T / 512 pieces a lane, into
// registers.  row_of(r): the source row of step row r, or -1 (zeros).  For 8 | C and a 16-byte aligned base.
template <int T, class RowOf>
__device__ __forceinline__ void gather(u32x4* v, const uint16_t* src, int C, int c0, int lane, RowOf row_of) {
  constexpr int PIECES = T / 8;
#pragma unroll
  for (int n = 0; n < STEP * PIECES / 64; ++n) {                 // STEP * PIECES: a multiple of 64
    const int idx = n * 64 + lane, r = idx / PIECES, c = (idx - r * PIECES) * 8;
    const long long row = row_of(r);
    v[n] = u32x4{0u, 0u, 0u, 0u};
    if (row >= 0 && c0 + c < C) v[n] = *reinterpret_cast<const u32x4*>(src + row * C + c0 + c);   // 8 | C: a piece that starts inside ends inside
  }
}

// ... and writes them into the image, every element of it
template <int T>
__device__ __forceinline__ void put(uint16_t* img, const u32x4* v, int lane) {
  constexpr int PIECES = T / 8;
#pragma unroll
  for (int n = 0; n < STEP * PIECES / 64; ++n) {
    const int idx = n * 64 + lane, r = idx / PIECES, c = (idx - r * PIECES) * 8;
    *reinterpret_cast<u32x4*>(img + img_off<T>(r, c)) = v[n];
  }
}

// the same image element by element: any C, any base
template <int T, class RowOf>
__device__ __forceinline__ void stage_elements(uint16_t* img, const uint16_t* src, int C, int c0, int lane, RowOf row_of) {
#pragma unroll 4
  for (int idx0 = 0; idx0 < STEP * T; idx0 += 64) {
    const int idx = idx0 + lane, r = idx / T, c = idx - r * T;
    const long long row = row_of(r);
    img[img_off<T>(r, c)] = (row >= 0 && c0 + c < C) ? src[row * C + c0 + c] : (uint16_t)0;
  }
}

// grid (parts, K, tiles of TI x TO of W[j]), as wgrad_kernel's.  vec_x, vec_g: 16-byte staging of X / gY.
// Dynamic LDS only (no static in front of it: the transposed reads need the 16-byte aligned base): per wave an X image of STEP x TI and a
// gY image of STEP x TO elements; after the loop the same bytes carry one wave's accumulators at a time.
template <class E, int TI, int TO>
__global__ __launch_bounds__(BLOCK) void wgrad16_kernel(const WgradArgs a, const int vec_x, const int vec_g) {
  constexpr int MI = TI / 16, MO = TO / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint16_t* X = (const uint16_t*)a.X;
  const uint16_t* gY = (const uint16_t*)a.gY;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint16_t* Xs = reinterpret_cast<uint16_t*>(smem) + wave * STEP * (TI + TO);
  uint16_t* Gs = Xs + STEP * TI;
  const int j = blockIdx.y;
  const int ci0 = (blockIdx.z / a.tiles_co) * TI, co0 = (blockIdx.z % a.tiles_co) * TO;
  const long long limit = row_limit(a.num, a.rows);
  const long long begin = (long long)blockIdx.x * a.chunk;
  long long end = begin + a.chunk;
  end = end < limit ? end : limit;
  f32x4 acc[MI][MO];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int q = 0; q < MO; ++q) acc[i][q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // lane r < STEP: the neighbour of row r0 + r at offset j, -1 for none, for a row past the chunk or the count, for a lane past the step
  auto neighbour = [&](long long r0) {
    int v = -1;
    if (lane < STEP && r0 + lane < end) {
      v = a.nbr[(r0 + lane) * a.K + j];
      if (v < 0 || v >= a.n_src) v = -1;
    }
    return v;
  };
  long long r0 = begin + (long long)wave * STEP;                 // r0: the same for the whole wave
  int v = neighbour(r0);
  for (; r0 < end; r0 += WAVES * STEP) {
    const int v_next = neighbour(r0 + WAVES * STEP);             // the next step's column read is in flight during this step
    if (__builtin_amdgcn_ballot_w64(v >= 0) != 0) {              // wave-uniform: a step none of whose rows has the neighbour is skipped
      auto x_row = [&](int r) { return (long long)__shfl(v, r); };
      auto g_row = [&](int r) { return __shfl(v, r) >= 0 ? r0 + r : -1LL; };
      u32x4 xv[STEP * TI / 512], gv[STEP * TO / 512];
      if (vec_x) gather<TI>(xv, X, a.Cin, ci0, lane, x_row);
      if (vec_g) gather<TO>(gv, gY, a.Cout, co0, lane, g_row);
      if (vec_x) put<TI>(Xs, xv, lane); else stage_elements<TI>(Xs, X, a.Cin, ci0, lane, x_row);
      if (vec_g) put<TO>(Gs, gv, lane); else stage_elements<TO>(Gs, gY, a.Cout, co0, lane, g_row);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the wave's own stores before its reads of other lanes' elements
      __builtin_amdgcn_wave_barrier();
      u32x4 bf[MO];
#pragma unroll
      for (int q = 0; q < MO; ++q) bf[q] = fragment<TO>(Gs, lane, q * 16);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const u32x4 af = fragment<TI>(Xs, lane, i * 16);
#pragma unroll
        for (int q = 0; q < MO; ++q) acc[i][q] = E::mfma(af, bf[q], acc[i][q]);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");     // ... and the reads before the next step's stores
      __builtin_amdgcn_wave_barrier();
    }
    v = v_next;
  }
  // wave 0 += wave 1, 2, 3 in this order, one wave's accumulators in LDS at a time; lane-for-lane, so the C/D map does not enter
  float* red = reinterpret_cast<float*>(smem);                   // [MI * MO][4][64]
  for (int w = 1; w < WAVES; ++w) {
    __syncthreads();                                             // the images, and the previous wave's accumulators, are free
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < MO; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) red[((i * MO + q) * 4 + e) * 64 + lane] = acc[i][q][e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < MO; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][q][e] = acc[i][q][e] + red[((i * MO + q) * 4 + e) * 64 + lane];
    }
  }
  if (wave != 0) return;
  // C/D: column = lane & 15 (co), row = 4 (lane >> 4) + register (ci)
  float* dst = a.part_w + ((long long)blockIdx.x * a.K + j) * a.Cin * a.Cout;
  const int c16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int q = 0; q < MO; ++q) {
      const int co = co0 + q * 16 + c16;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ci = ci0 + i * 16 + 4 * g + e;
        if (ci < a.Cin && co < a.Cout) dst[(long long)ci * a.Cout + co] = acc[i][q][e];
      }
    }
}

template <class E, int TI, int TO>
static void launch_tile(const WgradArgs& a, const dim3 grid, int vec_x, int vec_g, hipStream_t s) {
  constexpr size_t images = (size_t)WAVES * STEP * (TI + TO) * 2, turn = (size_t)(TI / 16) * (TO / 16) * 4 * 64 * 4;
  hipLaunchKernelGGL((wgrad16_kernel<E, TI, TO>), grid, dim3(BLOCK), images > turn ? images : turn, s, a, vec_x, vec_g);
}

template <class E, int TI>
static void launch_in(const WgradArgs& a, int to, const dim3 grid, int vec_x, int vec_g, hipStream_t s) {
  switch (to) {
    case 16: launch_tile<E, TI, 16>(a, grid, vec_x, vec_g, s); break;
    case 32: launch_tile<E, TI, 32>(a, grid, vec_x, vec_g, s); break;
    default: launch_tile<E, TI, 64>(a, grid, vec_x, vec_g, s); break;
  }
}

template <class E>
static void launch_stage_one(WgradArgs& a, hipStream_t s) {
  const int ti = tile_of(a.Cin), to = tile_of(a.Cout);
  a.tiles_co = (a.Cout + to - 1) / to;
  const dim3 grid((unsigned)a.parts, (unsigned)a.K, (unsigned)(((a.Cin + ti - 1) / ti) * a.tiles_co));
  const int vec_x = a.Cin % 8 == 0 && !misaligned(a.X, 16), vec_g = a.Cout % 8 == 0 && !misaligned(a.gY, 16);
  switch (ti) {
    case 16: launch_in<E, 16>(a, to, grid, vec_x, vec_g, s); break;
    case 32: launch_in<E, 32>(a, to, grid, vec_x, vec_g, s); break;
    default: launch_in<E, 64>(a, to, grid, vec_x, vec_g, s); break;
  }
}

}  // namespace sparse_conv_wgrad16

using namespace sparse_conv_wgrad16;

extern "C" {

int gd3d_sparse_conv_backward_weight_16_mfma(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                             int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                             float* grad_weight, float* grad_bias, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  bool run;
  const int rc = check_wgrad_call(2, dtype, N, R, K, Cin, Cout, features, grad_out, nbr, workspace, true, grad_weight, &run);
  if (rc != 0) return rc;
  if (!run) return zero_wgrad(K, Cin, Cout, grad_weight, grad_bias, s);
  WgradArgs a;
  fill_args(a, features, grad_out, nbr, num, N, R, K, Cin, Cout, workspace, grad_weight, grad_bias);
  if (dtype == GD3D_DTYPE_F16) launch_stage_one<F16>(a, s); else launch_stage_one<BF16>(a, s);
  return finish_wgrad(a, dtype, s);
}

}  // extern "C"
