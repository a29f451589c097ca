// sparse_conv_common.h — the integer rules of the sparse 3D convolution (include/gd3d.h, gd3d_sparse_conv_*),
// shared by the device units (csrc/sparse_conv.hip, sparse_conv_16.hip, sparse_conv_wgrad.hip, sparse_dense.hip) and their `_cpu` twins:
// which rows are active, the 64-bit keys, the offsets, the per-axis range checks made BEFORE anything is linearised, the look-up in a
// sorted key list, the tiles and chunks of the value kernels, and the argument checks of every value entry.  Integers only: both
// targets give the same tables and the same return codes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "sparse_elem.h"

namespace sparse_conv {

using sparse_elem::misaligned;

constexpr int MAX_K = 27;     // offsets of one kernel
constexpr int MAX_C = 256;    // channels, either side
constexpr int TILE_M = 64;    // output rows of one workgroup of the forward / input-gradient kernel (tests name their row counts from it)
constexpr int TILE_N = 64;    // output channels of one workgroup
constexpr int TILE_K = 32;    // reduction chunk staged in LDS
constexpr int TILE_M16 = 128; // output rows of one workgroup of the 16-bit forward / input-gradient kernel (csrc/sparse_conv_16.hip): 4 waves x 2 tiles of 16
constexpr int WG_ROWS = 32;   // rows of one staged step of the weight gradient
constexpr int MAX_PARTS = 64; // row chunks (partial sums per offset) of the weight gradient

struct Geo {
  int32_t B, n[3], k[3], s[3], p[3], o[3], K, subm;
  long long in_sent, out_sent;   // B * D * H * W and B * oD * oH * oW: above every valid key
};

// GD3D_E_* or 0.  shape, kernel, stride, padding: 3 host values each, (z, y, x).
inline int make_geo(int64_t N, int32_t B, const int32_t* shape, const int32_t* kernel, const int32_t* stride, const int32_t* padding,
                    int32_t subm, Geo* g) {
  if (N < 0 || B < 0 || shape == nullptr || kernel == nullptr || stride == nullptr || padding == nullptr) return GD3D_E_BADARG;
  long long K = 1, cells = B > 0 ? B : 1, ocells = B > 0 ? B : 1;
  for (int a = 0; a < 3; ++a) {
    g->n[a] = shape[a]; g->k[a] = kernel[a]; g->s[a] = stride[a]; g->p[a] = padding[a];
    if (shape[a] < 1 || kernel[a] < 1 || stride[a] < 1 || padding[a] < 0) return GD3D_E_BADARG;
    if (shape[a] > (1 << 24) || kernel[a] > MAX_K || padding[a] > (1 << 24) || stride[a] > (1 << 24)) return GD3D_E_TOOLARGE;
    if (subm && (kernel[a] % 2 == 0 || stride[a] != 1 || padding[a] != kernel[a] / 2)) return GD3D_E_BADARG;
    const long long span = (long long)shape[a] + 2LL * padding[a] - kernel[a];
    g->o[a] = span < 0 ? 0 : (int32_t)(span / stride[a] + 1);              // the kernel does not fit: no output cell, every count zero
    K *= kernel[a];
    if (K > MAX_K) return GD3D_E_TOOLARGE;
    if (cells > (1LL << 62) / shape[a] || (g->o[a] > 0 && ocells > (1LL << 62) / g->o[a])) return GD3D_E_TOOLARGE;
    cells *= shape[a];
    ocells *= g->o[a];
  }
  if (N > 0x7fffffffLL || N * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  g->B = B; g->K = (int32_t)K; g->subm = subm ? 1 : 0;
  g->in_sent = B > 0 ? cells : 0;
  g->out_sent = B > 0 ? ocells : 0;
  return 0;
}

SC_HD bool row_active(const int32_t* c, const Geo& g) {
  return c[0] >= 0 && c[0] < g.B && c[1] >= 0 && c[1] < g.n[0] && c[2] >= 0 && c[2] < g.n[1] && c[3] >= 0 && c[3] < g.n[2];
}

SC_HD long long in_key(const Geo& g, int b, int z, int y, int x) {
  return (((long long)b * g.n[0] + z) * g.n[1] + y) * g.n[2] + x;
}

SC_HD long long out_key(const Geo& g, int b, int z, int y, int x) {
  return (((long long)b * g.o[0] + z) * g.o[1] + y) * g.o[2] + x;
}

SC_HD void split_offset(const Geo& g, int j, int* off) {   // j = (a * ky + b) * kx + c: kz slowest
  off[2] = j % g.k[2];
  const int ab = j / g.k[2];
  off[1] = ab % g.k[1];
  off[0] = ab / g.k[1];
}

// the input cell that output cell `o` reads through offset `off`; false when it leaves the grid on any axis
SC_HD bool input_of(const Geo& g, const int* o, const int* off, int* in) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const long long v = (long long)o[a] * g.s[a] - g.p[a] + off[a];
    ok = ok && v >= 0 && v < g.n[a];
    in[a] = (int)v;
  }
  return ok;
}

// the output cell that reads input cell `in` through offset `off`; false when there is none (not on the stride, outside out_shape)
SC_HD bool output_of(const Geo& g, const int* in, const int* off, int* o) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const long long v = (long long)in[a] + g.p[a] - off[a];
    ok = ok && v >= 0 && v % g.s[a] == 0 && v / g.s[a] < g.o[a];
    o[a] = (int)(v / g.s[a]);
  }
  return ok;
}

// first position of `keys` (ascending, n entries) that is not below `key`
SC_HD long long lower_bound(const long long* keys, long long n, long long key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the (lowest) input row at a key, or -1
SC_HD int32_t find_row(const long long* skey, const int32_t* srow, long long n, long long key) {
  const long long at = lower_bound(skey, n, key);
  return at < n && skey[at] == key ? srow[at] : -1;
}

SC_HD void decode_out(const Geo& g, long long key, int32_t* c) {   // -> [b, z, y, x]
  c[3] = (int32_t)(key % g.o[2]); key /= g.o[2];
  c[2] = (int32_t)(key % g.o[1]); key /= g.o[1];
  c[1] = (int32_t)(key % g.o[0]);
  c[0] = (int32_t)(key / g.o[0]);
}

// how the weight gradient cuts R rows: `parts` chunks of `chunk` rows (a multiple of WG_ROWS), the partials held to 64 MiB
inline void weight_parts(int64_t R, int64_t kcc, int64_t* parts, int64_t* chunk) {
  int64_t cap = ((int64_t)64 << 20) / (kcc * 4);
  cap = cap < 1 ? 1 : (cap > MAX_PARTS ? MAX_PARTS : cap);
  int64_t c = (R + cap - 1) / cap;
  c = (c + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
  if (c < WG_ROWS) c = WG_ROWS;
  *chunk = c;
  *parts = R > 0 ? (R + c - 1) / c : 0;
}

// whether two buffers of `bytes` bytes share a byte (the fused forward: the residual must not overlap the output)
inline bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

inline int check_channels(int32_t K, int32_t Cin, int32_t Cout) {
  if (K < 1 || Cin < 1 || Cout < 1) return GD3D_E_BADARG;
  if (K > MAX_K || Cin > MAX_C || Cout > MAX_C) return GD3D_E_TOOLARGE;
  return 0;
}

// rows at and past num[0] are zeros; num nullable: every row counts
SC_HD long long row_limit(const long long* num, long long rows) {
  if (num == nullptr) return rows;
  const long long k = num[0];
  return k < rows ? (k < 0 ? 0 : k) : rows;
}

inline int tile_of(int channels) { return channels <= 16 ? 16 : (channels <= 32 ? 32 : 64); }   // the smallest channel tile that holds them, at most 64

// the geometry of dense(): a 1x1x1 layer over (B, D, H, W) with C channels
inline int dense_geo(int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W, Geo* g) {
  const int32_t shape[3] = {D, H, W}, one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
  if (C < 1) return GD3D_E_BADARG;
  if (C > MAX_C) return GD3D_E_TOOLARGE;
  const int rc = make_geo(N, B, shape, one, one, zero, 0, g);
  if (rc != 0) return rc;
  if (g->in_sent > (1LL << 62) / C || N * C > (1LL << 40)) return GD3D_E_TOOLARGE;
  return 0;
}

// ---- the argument checks of the value entries, device and `_cpu` alike -----------------------------------------------------------------
// One order everywhere, so that every entry returns the same code for the same arguments: the channels, GD3D_E_BADARG for the scalars,
// GD3D_E_TOOLARGE, the empty call (0 with *run = false: nothing to compute), null pointers, odd pointers (16-bit forms), the overlap.
// elem: the operands' element size, 4 (the fp32 entries, which hand in dtype 0) or 2 (dtype one of GD3D_DTYPE_F16 / BF16, operands
// 2-byte aligned).

inline bool elem_ok(size_t elem, int32_t dtype) { return sparse_elem::dtype_ok(dtype) && sparse_elem::elem_size(dtype) == elem; }
inline bool act_ok(int32_t act) { return act == GD3D_ACT_NONE || act == GD3D_ACT_RELU; }

// The GEMM-shaped calls: `rows` output rows of Cout channels gather from `n_src` source rows through `table` — (R, N) in the forward
// forms, (N, R) in the input gradient.  scalars_ok: what the entry checks of its own scalars (act; flip).  residual: the fused forward's.
inline int check_gemm_call(size_t elem, int32_t dtype, int64_t rows, int64_t n_src, int32_t K, int32_t Cin, int32_t Cout, bool scalars_ok,
                           const void* src, const void* weight, const void* table, const void* residual, const void* out, bool* run) {
  *run = false;
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!elem_ok(elem, dtype) || rows < 0 || n_src < 0 || !scalars_ok) return GD3D_E_BADARG;
  if (rows > 0x7fffffffLL || n_src > 0x7fffffffLL || rows * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (rows == 0) return 0;
  if (weight == nullptr || table == nullptr || out == nullptr || (n_src > 0 && src == nullptr)) return GD3D_E_BADARG;
  if (elem == 2 && (misaligned(src, 2) || misaligned(weight, 2) || misaligned(residual, 2) || misaligned(out, 2))) return GD3D_E_BADARG;
  if (residual != nullptr && ranges_overlap(residual, out, elem * (size_t)rows * (size_t)Cout)) return GD3D_E_BADARG;
  *run = true;
  return 0;
}

// The weight gradient.  *run = false: no pair, the caller writes zeros.  need_work: the device form's 256-byte aligned workspace.
inline int check_wgrad_call(size_t elem, int32_t dtype, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, const void* features,
                            const void* grad_out, const void* nbr, const void* workspace, bool need_work, const void* grad_weight, bool* run) {
  *run = false;
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!elem_ok(elem, dtype) || N < 0 || R < 0 || grad_weight == nullptr) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || R * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (R == 0 || N == 0) return 0;
  if (features == nullptr || grad_out == nullptr || nbr == nullptr) return GD3D_E_BADARG;
  if (need_work && (workspace == nullptr || ((uintptr_t)workspace & 255) != 0)) return GD3D_E_BADARG;
  if (elem == 2 && (misaligned(features, 2) || misaligned(grad_out, 2))) return GD3D_E_BADARG;
  *run = true;
  return 0;
}

}  // namespace sparse_conv
