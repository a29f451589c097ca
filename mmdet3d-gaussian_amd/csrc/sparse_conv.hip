// sparse_conv.hip — sparse 3D convolution (spconv 1.x's SubMConv3d / SparseConv3d, restated: include/gd3d.h, gd3d_sparse_conv_*;
// DESIGN.md §3.18) for gfx950: the index build and the fp32 forward and input-gradient implicit GEMM.  The weight gradient of every
// element type is csrc/sparse_conv_wgrad.hip's, SparseConvTensor.dense() csrc/sparse_dense.hip's, the 16-bit GEMM csrc/sparse_conv_16.hip's.
// Every call is one stream-ordered run of launches that reads nothing back.
//   index build   key_kernel     one int64 key per input row, ((b * D + z) * H + y) * W + x, or the sentinel B*D*H*W for an inactive row
//                 radix sort     (key, row) pairs, stable: a look-up by lower bound finds the LOWEST row of a duplicated cell.  rocPRIM's
//                                device radix sort and scan, through csrc/device_sort.h.
//                 submanifold    subm_kernel: a thread per (row, offset) looks its neighbour's coordinate up
//                 regular        cand_kernel (the output cell of every (row, offset) pair, or the sentinel), a radix sort of those
//                                keys, head flags, a plus-scan and a compaction give the unique output keys in ascending order;
//                                finish_kernel the counts; out_kernel decodes the kept keys and looks the inputs up; nbrt_kernel
//                                looks every input row's outputs up in the kept keys
//   gemm_kernel   output stationary: a workgroup owns TILE_M rows x 16, 32 or 64 channels (the smallest tile that holds Cout), walks the offsets, skips (workgroup-uniformly)
//                 an offset no row of the tile uses, stages the gathered rows and the weight slice in LDS, accumulates with fmaf in
//                 registers and writes every element once.  The input gradient is the same kernel over the transposed table and
//                 weight.  No atomics: the bits replay.  FUSED (gd3d_sparse_conv_forward_fused): the epilogue of the
//                 forward form with a per-channel scale, a residual row and a ReLU — a compile-time variant: the plain instances
//                 keep their code.
// Compiled with -ffp-contract=off (the tables replay bit for bit in csrc/sparse_conv_cpu.cpp); the multiply-adds are explicit fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "device_sort.h"
#include "gd3d_fill.h"
#include "gd3d_workspace.h"
#include "sparse_conv_common.h"

namespace sparse_conv {

constexpr int BLOCK = 256;

static unsigned blocks_of(long long threads) { return (unsigned)((threads + BLOCK - 1) / BLOCK); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The caller's workspace (256-byte aligned) of the index build, carved: every buffer once.  At address 0 it is the size function.
struct Work {
  long long *key_in, *skey;
  int *val_in, *srow;
  long long *cand, *scand, *ukey;   // the regular form's, m = n * K entries each (none in the submanifold form)
  int *flag, *pos;
  char* sort_tmp;                   // of both sorts and the scan, one after the other
  size_t sort_bytes = 0, bytes = 0;
  hipError_t err;
  Work(void* workspace, int64_t n, int64_t m, bool subm) {
    size_t keys = 0, scan = 0;
    err = gd3d::sort_pairs_temp_bytes((size_t)n, sort_bytes);
    if (err == hipSuccess && !subm) err = gd3d::sort_keys_temp_bytes((size_t)m, keys);
    if (err == hipSuccess && !subm) err = gd3d::exclusive_sum_temp_bytes((size_t)m, scan);
    if (err != hipSuccess) return;
    sort_bytes = sort_bytes > keys ? sort_bytes : keys;
    sort_bytes = sort_bytes > scan ? sort_bytes : scan;
    const size_t mm = subm ? 0 : (size_t)m;
    gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
    key_in = c.take<long long>((size_t)n);
    skey = c.take<long long>((size_t)n);
    val_in = c.take<int>((size_t)n);
    srow = c.take<int>((size_t)n);
    ukey = cand = c.take<long long>(mm);   // the candidates are sorted out of `cand`: it is free again when the unique keys are written
    scand = c.take<long long>(mm);
    flag = c.take<int>(mm);
    pos = c.take<int>(mm);
    sort_tmp = c.take<char>(sort_bytes);
    bytes = c.bytes();
  }
};

__global__ __launch_bounds__(BLOCK) void key_kernel(const int32_t* __restrict__ coors, long long n, const Geo g,
                                                    long long* __restrict__ keys, int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t* c = coors + i * 4;
  keys[i] = row_active(c, g) ? in_key(g, c[0], c[1], c[2], c[3]) : g.in_sent;
  vals[i] = (int)i;
}

// a thread per (row, offset): out_coors = coors, nbr[o, j] = the row at the neighbour's coordinate
__global__ __launch_bounds__(BLOCK) void subm_kernel(const int32_t* __restrict__ coors, long long n, const Geo g,
                                                     const long long* __restrict__ skey, const int* __restrict__ srow,
                                                     int32_t* __restrict__ out_coors, int32_t* __restrict__ nbr) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * g.K) return;
  const long long o = t / g.K;
  const int j = (int)(t - o * g.K);
  const int32_t* c = coors + o * 4;
  if (j == 0) {
    for (int a = 0; a < 4; ++a) out_coors[o * 4 + a] = c[a];
  }
  int32_t v = -1;
  if (row_active(c, g)) {
    int off[3], in[3];
    const int oc[3] = {c[1], c[2], c[3]};
    split_offset(g, j, off);
    if (input_of(g, oc, off, in)) v = find_row(skey, srow, n, in_key(g, c[0], in[0], in[1], in[2]));
  }
  nbr[t] = v;
}

__global__ __launch_bounds__(BLOCK) void cand_kernel(const int32_t* __restrict__ coors, long long n, const Geo g,
                                                     long long* __restrict__ cand) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * g.K) return;
  const long long i = t / g.K;
  const int j = (int)(t - i * g.K);
  const int32_t* c = coors + i * 4;
  long long key = g.out_sent;
  if (row_active(c, g)) {
    int off[3], o[3];
    const int in[3] = {c[1], c[2], c[3]};
    split_offset(g, j, off);
    if (output_of(g, in, off, o)) key = out_key(g, c[0], o[0], o[1], o[2]);
  }
  cand[t] = key;
}

__global__ __launch_bounds__(BLOCK) void head_kernel(const long long* __restrict__ scand, long long m, long long sentinel,
                                                     int* __restrict__ flag) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= m) return;
  const long long key = scand[t];
  flag[t] = (key != sentinel && (t == 0 || key != scand[t - 1])) ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void compact_kernel(const long long* __restrict__ scand, const int* __restrict__ flag,
                                                        const int* __restrict__ pos, long long m, long long* __restrict__ ukey) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= m) return;
  if (flag[t]) ukey[pos[t]] = scand[t];                         // pos[t] <= t: inside the m entries of ukey
}

// One workgroup.  keys: the sorted input keys (subm) or the unique output keys (regular); `cells`: keys of one sample.
__global__ __launch_bounds__(BLOCK) void finish_kernel(const long long* __restrict__ keys, long long n_keys, const int* __restrict__ flag,
                                                       const int* __restrict__ pos, long long m, long long max_out, long long sentinel,
                                                       int B, int subm, long long* __restrict__ num, int32_t* __restrict__ out_batch_cnt) {
  long long total, kept;
  if (subm) {
    total = kept = n_keys;                                      // every row is an output row
  } else {
    total = m > 0 ? (long long)pos[m - 1] + flag[m - 1] : 0;
    kept = total < max_out ? total : max_out;
    n_keys = kept;
  }
  if (threadIdx.x == 0) { num[0] = kept; num[1] = total; }
  const long long cells = B > 0 ? sentinel / B : 0;
  for (int b = threadIdx.x; b < B; b += BLOCK)
    out_batch_cnt[b] = (int32_t)(lower_bound(keys, n_keys, (long long)(b + 1) * cells) - lower_bound(keys, n_keys, (long long)b * cells));
}

// a thread per (output row, offset) of the R = max_out rows
__global__ __launch_bounds__(BLOCK) void out_kernel(const long long* __restrict__ ukey, const long long* __restrict__ num, long long rows,
                                                    long long n, const Geo g, const long long* __restrict__ skey,
                                                    const int* __restrict__ srow, int32_t* __restrict__ out_coors,
                                                    int32_t* __restrict__ nbr) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= rows * g.K) return;
  const long long r = t / g.K;
  const int j = (int)(t - r * g.K);
  int32_t c[4] = {-1, -1, -1, -1};
  int32_t v = -1;
  if (r < num[0]) {
    decode_out(g, ukey[r], c);
    int off[3], in[3];
    const int oc[3] = {c[1], c[2], c[3]};
    split_offset(g, j, off);
    if (input_of(g, oc, off, in)) v = find_row(skey, srow, n, in_key(g, c[0], in[0], in[1], in[2]));
  }
  if (j == 0) {
    for (int a = 0; a < 4; ++a) out_coors[r * 4 + a] = c[a];
  }
  nbr[t] = v;
}

// a thread per (input row, offset): the kept output row that reads this row through this offset
__global__ __launch_bounds__(BLOCK) void nbrt_kernel(const int32_t* __restrict__ coors, long long n, const Geo g,
                                                     const long long* __restrict__ skey, const int* __restrict__ srow,
                                                     const long long* __restrict__ ukey, const long long* __restrict__ num,
                                                     int32_t* __restrict__ nbr_t) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * g.K) return;
  const long long i = t / g.K;
  const int j = (int)(t - i * g.K);
  const int32_t* c = coors + i * 4;
  int32_t v = -1;
  // of the rows of a duplicated cell only the one the look-up finds is anybody's neighbour
  if (row_active(c, g) && find_row(skey, srow, n, in_key(g, c[0], c[1], c[2], c[3])) == (int32_t)i) {
    int off[3], o[3];
    const int in[3] = {c[1], c[2], c[3]};
    split_offset(g, j, off);
    if (output_of(g, in, off, o)) {
      const long long kept = num[0], key = out_key(g, c[0], o[0], o[1], o[2]);
      const long long at = lower_bound(ukey, kept, key);
      if (at < kept && ukey[at] == key) v = (int32_t)at;
    }
  }
  nbr_t[t] = v;
}

// ---- the implicit GEMM ---------------------------------------------------------------------------------------------------------------

struct GemmArgs {
  const float* src;        // (n_src, Cr): the rows gathered
  const float* W;          // (K, Cin, Cout)
  const float* bias;       // (Co) or null
  const int32_t* table;    // (rows, K)
  const long long* num;    // nullable: rows at and past num[0] are zeros
  long long n_src, rows;
  int K, Cr, Co, flip;     // flip: the table's column of offset j is K - 1 - j (the submanifold transpose)
  float* out;              // (rows, Co)
  // the FUSED epilogue only: t = fmaf(acc, scale, bias) (+ residual), ReLU; `bias` is the folded shift
  const float* scale;      // (Co) or null
  const float* residual;   // (rows, Co) or null; read at live rows only
  int act;                 // GD3D_ACT_*
  int vec_res;             // Co % 4 == 0 and `residual` 16-byte aligned
};

// TRANS: the weight slice is read transposed (the input gradient: Cr = Cout, Co = Cin).  VEC: Co % 4 == 0 and `out` 16-byte aligned.
// FUSED: the epilogue is one fixed fp32 sequence per element of a live row — fmaf(acc, scale, shift) or acc + shift, + residual, ReLU
// (a NaN passes) — and zero for every other row, whose residual is not read.
// TN: the output channels of one workgroup, 16, 32 or 64 — the smallest that holds Co, so that a 16-channel layer keeps every thread
// busy: TN / 4 threads lie along the channels (4 each), the other BLOCK / (TN / 4) along the TILE_M rows (TN / 16 rows each).
template <bool TRANS, bool VEC, int TN, bool FUSED = false>
__global__ __launch_bounds__(BLOCK) void gemm_kernel(const GemmArgs a) {
  constexpr int CT = TN / 4, RPT = TILE_M * CT / BLOCK;
  __shared__ int nb[TILE_M];
  __shared__ int used[TILE_M];
  __shared__ float Xs[TILE_M][TILE_K + 1];
  __shared__ __attribute__((aligned(16))) float Ws[TILE_K][TN];
  const int t = threadIdx.x, tx = t % CT, ty = t / CT;
  const long long row0 = (long long)blockIdx.x * TILE_M;
  const int col0 = blockIdx.y * TN;
  long long limit = a.rows;
  if (a.num != nullptr) { const long long k = a.num[0]; limit = k < limit ? (k < 0 ? 0 : k) : limit; }
  float acc[RPT][4];
  for (int i = 0; i < RPT; ++i)
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.0f;
  int mine = 0;                                                  // thread t < TILE_M: whether row t has any neighbour
  for (int j = 0; j < a.K; ++j) {
    int v = -1;
    if (t < TILE_M && row0 + t < limit) {
      v = a.table[(row0 + t) * a.K + (a.flip ? a.K - 1 - j : j)];
      if (v < 0 || v >= a.n_src) v = -1;
    }
    if (t < TILE_M) { nb[t] = v; mine |= v >= 0; }
    if (!__syncthreads_or(v >= 0)) continue;                     // nobody reads nb[] of a skipped offset
    const float* Wj = a.W + (long long)j * a.Cr * a.Co;
    for (int kc = 0; kc < a.Cr; kc += TILE_K) {
      for (int idx = t; idx < TILE_M * TILE_K; idx += BLOCK) {
        const int r = idx / TILE_K, kk = idx % TILE_K;
        const int row = nb[r];
        Xs[r][kk] = (row >= 0 && kc + kk < a.Cr) ? a.src[(long long)row * a.Cr + kc + kk] : 0.0f;
      }
      for (int idx = t; idx < TILE_K * TN; idx += BLOCK) {
        const int kk = idx / TN, c = idx % TN;
        float w = 0.0f;
        if (kc + kk < a.Cr && col0 + c < a.Co)
          w = TRANS ? Wj[(long long)(col0 + c) * a.Cr + kc + kk] : Wj[(long long)(kc + kk) * a.Co + col0 + c];
        Ws[kk][c] = w;
      }
      __syncthreads();
      const int kn = a.Cr - kc < TILE_K ? a.Cr - kc : TILE_K;
      for (int kk = 0; kk < kn; ++kk) {
        const float4 w = *reinterpret_cast<const float4*>(&Ws[kk][tx * 4]);
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          const float x = Xs[ty * RPT + i][kk];
          acc[i][0] = __builtin_fmaf(x, w.x, acc[i][0]);
          acc[i][1] = __builtin_fmaf(x, w.y, acc[i][1]);
          acc[i][2] = __builtin_fmaf(x, w.z, acc[i][2]);
          acc[i][3] = __builtin_fmaf(x, w.w, acc[i][3]);
        }
      }
      __syncthreads();
    }
  }
  if (t < TILE_M) used[t] = mine;
  __syncthreads();
  const int c = col0 + tx * 4;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const long long row = row0 + ty * RPT + i;
    if (row >= a.rows) continue;
    const bool live = used[ty * RPT + i] != 0;                   // a row without neighbours (inactive, or past the count) is zero, bias or not
    float o[4];
    if constexpr (FUSED) {
      float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (live && a.residual != nullptr) {
        const float* src = a.residual + row * a.Co + c;
        if (a.vec_res) {                                           // 4 | Co: a piece that starts inside the row ends inside it
          if (c < a.Co) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            res[0] = v.x; res[1] = v.y; res[2] = v.z; res[3] = v.w;
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (c + q < a.Co) res[q] = src[q];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool in = c + q < a.Co;
        const float sh = (a.bias != nullptr && in) ? a.bias[c + q] : 0.0f;
        float v = a.scale != nullptr ? __builtin_fmaf(acc[i][q], in ? a.scale[c + q] : 0.0f, sh) : acc[i][q] + sh;
        if (a.residual != nullptr) v = v + res[q];
        if (a.act == GD3D_ACT_RELU) v = v < 0.0f ? 0.0f : v;
        o[q] = live ? v : 0.0f;
      }
    } else {
      for (int q = 0; q < 4; ++q) o[q] = live ? acc[i][q] + ((a.bias != nullptr && c + q < a.Co) ? a.bias[c + q] : 0.0f) : 0.0f;
    }
    float* dst = a.out + row * a.Co + c;
    if (VEC) {
      if (c < a.Co) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int q = 0; q < 4; ++q)
        if (c + q < a.Co) dst[q] = o[q];
    }
  }
}

template <int TN>
static int launch_gemm_tile(const GemmArgs& a, bool trans, hipStream_t s) {
  const dim3 grid((unsigned)((a.rows + TILE_M - 1) / TILE_M), (unsigned)((a.Co + TN - 1) / TN));
  const bool vec = a.Co % 4 == 0 && aligned16(a.out);
  if (trans) {
    if (vec) hipLaunchKernelGGL((gemm_kernel<true, true, TN>), grid, dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((gemm_kernel<true, false, TN>), grid, dim3(BLOCK), 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((gemm_kernel<false, true, TN>), grid, dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((gemm_kernel<false, false, TN>), grid, dim3(BLOCK), 0, s, a);
  }
  return (int)hipGetLastError();
}

template <int TN>
static int launch_fused_tile(const GemmArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.rows + TILE_M - 1) / TILE_M), (unsigned)((a.Co + TN - 1) / TN));
  if (a.Co % 4 == 0 && aligned16(a.out)) hipLaunchKernelGGL((gemm_kernel<false, true, TN, true>), grid, dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL((gemm_kernel<false, false, TN, true>), grid, dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

static int launch_fused(GemmArgs& a, hipStream_t s) {
  a.vec_res = a.residual != nullptr && a.Co % 4 == 0 && aligned16(a.residual);
  switch (tile_of(a.Co)) {
    case 16: return launch_fused_tile<16>(a, s);
    case 32: return launch_fused_tile<32>(a, s);
    default: return launch_fused_tile<TILE_N>(a, s);
  }
}

static int launch_gemm(const GemmArgs& a, bool trans, hipStream_t s) {
  switch (tile_of(a.Co)) {
    case 16: return launch_gemm_tile<16>(a, trans, s);
    case 32: return launch_gemm_tile<32>(a, trans, s);
    default: return launch_gemm_tile<TILE_N>(a, trans, s);
  }
}

}  // namespace sparse_conv

using namespace sparse_conv;

extern "C" {

size_t gd3d_sparse_conv_index_workspace_bytes(int64_t N, int32_t K, int32_t subm) {
  if (N <= 0 || K < 1 || K > MAX_K || N * K > 0x7fffffffLL) return 256;
  const Work w(nullptr, N, N * K, subm != 0);
  return w.err == hipSuccess ? w.bytes : 0;
}

int gd3d_sparse_conv_index(const int32_t* coors, int64_t N, int32_t B, const int32_t* spatial_shape, const int32_t* kernel_size,
                           const int32_t* stride, const int32_t* padding, int32_t subm, int64_t max_out, void* workspace,
                           int32_t* out_coors, int32_t* nbr, int32_t* nbr_t, int64_t* num, int32_t* out_batch_cnt, void* stream) {
  Geo g;
  const int rc = make_geo(N, B, spatial_shape, kernel_size, stride, padding, subm, &g);
  if (rc != 0) return rc;
  if (num == nullptr || (B > 0 && out_batch_cnt == nullptr) || max_out < 0) return GD3D_E_BADARG;
  const int64_t R = subm ? N : max_out;
  if (R > 0x7fffffffLL || R * g.K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipStream_t s = (hipStream_t)stream;
  int e = 0;
  if (R > 0) {
    if (out_coors == nullptr || nbr == nullptr) return GD3D_E_BADARG;
  }
  if (N == 0) {                                                  // no input row: the counts are zeros, every output row a tail row
    e = gd3d::fill_words(num, 2 * sizeof(int64_t), 0u, s);
    if (e == 0 && B > 0) e = gd3d::fill_words(out_batch_cnt, sizeof(int32_t) * (size_t)B, 0u, s);
    if (e == 0 && R > 0) e = gd3d::fill_words(out_coors, sizeof(int32_t) * 4 * (size_t)R, 0xffffffffu, s);
    if (e == 0 && R > 0) e = gd3d::fill_words(nbr, sizeof(int32_t) * (size_t)R * g.K, 0xffffffffu, s);
    return e;
  }
  if (coors == nullptr || workspace == nullptr || ((uintptr_t)workspace & 255) != 0) return GD3D_E_BADARG;
  if (!subm && nbr_t == nullptr) return GD3D_E_BADARG;
  const long long M = (long long)N * g.K;
  const Work w(workspace, N, M, subm != 0);
  if (w.err != hipSuccess) return (int)w.err;
  hipLaunchKernelGGL(key_kernel, dim3(blocks_of(N)), dim3(BLOCK), 0, s, coors, (long long)N, g, w.key_in, w.val_in);
  hipError_t he = gd3d::sort_pairs(w.sort_tmp, w.sort_bytes, w.key_in, w.skey, w.val_in, w.srow, (size_t)N, (unsigned)gd3d::key_bits(g.in_sent), s);
  if (he != hipSuccess) return (int)he;
  if (subm) {
    hipLaunchKernelGGL(subm_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, s, coors, (long long)N, g, (const long long*)w.skey,
                       (const int*)w.srow, out_coors, nbr);
    // the sorted keys below the sentinel are the active rows: a sample's count is a difference of two lower bounds
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(BLOCK), 0, s, (const long long*)w.skey, (long long)N, (const int*)nullptr,
                       (const int*)nullptr, 0LL, 0LL, g.in_sent, (int)B, 1, (long long*)num, out_batch_cnt);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(cand_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, s, coors, (long long)N, g, w.cand);
  he = gd3d::sort_keys(w.sort_tmp, w.sort_bytes, w.cand, w.scand, (size_t)M, (unsigned)gd3d::key_bits(g.out_sent), s);
  if (he != hipSuccess) return (int)he;
  hipLaunchKernelGGL(head_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, s, (const long long*)w.scand, M, g.out_sent, w.flag);
  he = gd3d::exclusive_sum(w.sort_tmp, w.sort_bytes, w.flag, w.pos, (size_t)M, s);
  if (he != hipSuccess) return (int)he;
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, s, (const long long*)w.scand, (const int*)w.flag, (const int*)w.pos, M,
                     w.ukey);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(BLOCK), 0, s, (const long long*)w.ukey, 0LL, (const int*)w.flag, (const int*)w.pos, M,
                     (long long)max_out, g.out_sent, (int)B, 0, (long long*)num, out_batch_cnt);
  if (R > 0)
    hipLaunchKernelGGL(out_kernel, dim3(blocks_of(R * g.K)), dim3(BLOCK), 0, s, (const long long*)w.ukey, (const long long*)num, (long long)R,
                       (long long)N, g, (const long long*)w.skey, (const int*)w.srow, out_coors, nbr);
  hipLaunchKernelGGL(nbrt_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, s, coors, (long long)N, g, (const long long*)w.skey, (const int*)w.srow,
                     (const long long*)w.ukey, (const long long*)num, nbr_t);
  return (int)hipGetLastError();
}

int gd3d_sparse_conv_forward(const float* features, const float* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                             int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* out, void* stream) {
  bool run;
  const int rc = check_gemm_call(4, 0, R, N, K, Cin, Cout, true, features, weight, nbr, nullptr, out, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = features; a.W = weight; a.bias = bias; a.table = nbr; a.num = (const long long*)num; a.n_src = N; a.rows = R;
  a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = out;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE; a.vec_res = 0;
  return launch_gemm(a, false, (hipStream_t)stream);
}

int gd3d_sparse_conv_forward_fused(const float* features, const float* weight, const float* scale, const float* shift, const float* residual,
                                   const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout,
                                   int32_t act, float* out, void* stream) {
  bool run;
  const int rc = check_gemm_call(4, 0, R, N, K, Cin, Cout, act_ok(act), features, weight, nbr, residual, out, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = features; a.W = weight; a.bias = shift; a.table = nbr; a.num = (const long long*)num; a.n_src = N; a.rows = R;
  a.K = K; a.Cr = Cin; a.Co = Cout; a.flip = 0; a.out = out;
  a.scale = scale; a.residual = residual; a.act = act; a.vec_res = 0;
  return launch_fused(a, (hipStream_t)stream);
}

int gd3d_sparse_conv_backward_input(const float* grad_out, const float* weight, const int32_t* table, int32_t flip, int64_t N,
                                    int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* grad_features, void* stream) {
  bool run;
  const int rc = check_gemm_call(4, 0, N, R, K, Cin, Cout, !flip || N == R, grad_out, weight, table, nullptr, grad_features, &run);
  if (rc != 0 || !run) return rc;
  GemmArgs a;
  a.src = grad_out; a.W = weight; a.bias = nullptr; a.table = table; a.num = nullptr; a.n_src = R; a.rows = N;
  a.K = K; a.Cr = Cout; a.Co = Cin; a.flip = flip ? 1 : 0; a.out = grad_features;
  a.scale = nullptr; a.residual = nullptr; a.act = GD3D_ACT_NONE; a.vec_res = 0;
  return launch_gemm(a, true, (hipStream_t)stream);
}

}  // extern "C"
