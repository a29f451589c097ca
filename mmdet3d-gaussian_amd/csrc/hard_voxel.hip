// hard_voxel.hip — hard voxelization and the mean voxel encoder for a whole stacked batch, for gfx950 (include/gd3d.h,
// gd3d_hard_voxelize / gd3d_dynamic_voxelize / gd3d_voxel_mean): PVRCNN.voxelize plus HardSimpleVFE
// (models/detectors/pv_rcnn.py:43-49, 66-86), which the reference runs as a Python loop over samples around mmdet3d's
// Voxelization op, a cat, an F.pad per sample and a host read of coors[-1, 0].  Here, in one stream-ordered call that reads
// nothing back:
//   key_kernel      one int64 key per point, b * G + (z * Gy + y) * Gx + x, or B * G for a dropped point
//   radix sort      (key, point id) pairs, stable, over the key bits in use only: ascending point id inside a cell is the slot
//                   order.  rocPRIM's device radix sort and scans, through csrc/device_sort.h.
//   head_kernel     run heads of the sorted keys; marks, in POINT order, the first point of every cell
//   two scans       max-scan of the head positions (every sorted point learns where its cell starts, hence its slot and its
//                   cell's first point) and plus-scan, in point order, of the first-point marks (a cell's rank of appearance)
//   sample_kernel   per sample: the cells seen, the voxels kept = min(cells, max_voxels), the base of its rows (so the rows lie as
//                   torch.cat would lay them), the total and the dropped points
//   scatter_kernel  one thread per sorted point: copies the point's row into its slot; heads write coors (b, z, y, x); the last
//                   point of a cell writes num_points = min(points, max_num_points)
//   mean_kernel     a thread per voxel (16-byte path) or per element: slots 0, 1, 2, .. added in sequence, one division; reads the
//                   points through the sorted order, so it does not need `voxels`
// Padding and tail rows come from the library's fill kernel (gd3d_fill.h) before the scatter.  Compiled with -ffp-contract=off:
// the cell of a point (csrc/hard_voxel_common.h) and the mean are the operation sequence of csrc/hard_voxel_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "device_sort.h"
#include "gd3d_fill.h"
#include "gd3d_workspace.h"
#include "hard_voxel_common.h"

namespace hard_voxel {

// The caller's workspace (256-byte aligned), carved: every buffer once.  At address 0 it is the size function.
struct Work {
  long long *key_in, *key_out;
  int *val_in, *order, *head_pos, *seg, *first, *cum, *cum_base, *row_base, *vstart;
  char *sort_tmp, *scan_tmp;
  size_t sort_bytes = 0, scan_bytes = 0, bytes = 0;   // scan_bytes: the larger of the two scans'
  hipError_t err;
  Work(void* workspace, int64_t n, int64_t rows) {
    size_t plus = 0;
    err = gd3d::sort_pairs_temp_bytes((size_t)n, sort_bytes);
    if (err == hipSuccess) err = gd3d::inclusive_max_temp_bytes((size_t)n, scan_bytes);
    if (err == hipSuccess) err = gd3d::inclusive_sum_temp_bytes((size_t)n, plus);
    if (err != hipSuccess) return;
    scan_bytes = scan_bytes > plus ? scan_bytes : plus;
    gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
    key_in = c.take<long long>((size_t)n);
    key_out = c.take<long long>((size_t)n);
    val_in = c.take<int>((size_t)n);
    order = c.take<int>((size_t)n);
    head_pos = c.take<int>((size_t)n);
    seg = c.take<int>((size_t)n);
    first = c.take<int>((size_t)n);
    cum = c.take<int>((size_t)n);
    cum_base = c.take<int>(MAX_B);
    row_base = c.take<int>(MAX_B);
    vstart = c.take<int>((size_t)rows);
    sort_tmp = c.take<char>(sort_bytes);
    scan_tmp = c.take<char>(scan_bytes);
    bytes = c.bytes();
  }
};

__global__ __launch_bounds__(BLOCK) void key_kernel(const float* __restrict__ points, long long n, long long stride,
                                                    const int32_t* __restrict__ cnt, int B, const Geometry g,
                                                    long long* __restrict__ keys, int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  int32_t x, y, z;
  const int32_t b = sample_of(i, cnt, B);
  const bool in = cell_of(points + i * stride, g, &x, &y, &z) && b >= 0;
  keys[i] = in ? (long long)b * g.G + cell_key(g, x, y, z) : (long long)B * g.G;
  vals[i] = (int)i;
}

__global__ __launch_bounds__(BLOCK) void head_kernel(const long long* __restrict__ skey, const int* __restrict__ order, long long n,
                                                     long long sentinel, int* __restrict__ head_pos, int* __restrict__ first) {
  const long long j = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const long long key = skey[j];
  const bool head = j == 0 || key != skey[j - 1];
  head_pos[j] = head ? (int)j : 0;
  first[order[j]] = (head && key != sentinel) ? 1 : 0;   // every point is some j's order[j]: all of `first` is written
}

// One workgroup.  Sample b owns the rows [start, end) of the stack; cum[] is the inclusive count, in point order, of first points.
__global__ __launch_bounds__(BLOCK) void sample_kernel(const int32_t* __restrict__ cnt, int B, long long n, const int* __restrict__ cum,
                                                       const long long* __restrict__ skey, long long sentinel, int max_voxels,
                                                       int* __restrict__ cum_base, int* __restrict__ row_base,
                                                       int32_t* __restrict__ voxel_batch_cnt, long long* __restrict__ num) {
  __shared__ int kept[MAX_B];
  for (int b = threadIdx.x; b < B; b += BLOCK) {
    long long start = 0;
    for (int a = 0; a < b; ++a) start += cnt[a] > 0 ? cnt[a] : 0;
    long long end = start + (cnt[b] > 0 ? cnt[b] : 0);
    start = start < n ? start : n;                              // counts that overrun the stack own nothing beyond it
    end = end < n ? end : n;
    const int before = start > 0 ? cum[start - 1] : 0, after = end > 0 ? cum[end - 1] : 0;
    const int cells = after - before;
    cum_base[b] = before;
    kept[b] = cells < max_voxels ? cells : max_voxels;
    voxel_batch_cnt[b] = kept[b];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int b = 0; b < B; ++b) {
      row_base[b] = (int)total;
      total += kept[b];
    }
    num[0] = total;
  }
  if (threadIdx.x == 64) {                                      // dropped points: the sorted keys from the first sentinel on
    long long lo = 0, hi = n;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (skey[mid] < sentinel) lo = mid + 1; else hi = mid;
    }
    num[1] = n - lo;
  }
}

struct ScatterArgs {
  const float* points;
  long long n, stride;
  int C, P, max_voxels;
  long long G, gx, gy, sentinel;
  const long long* skey;
  const int *order, *seg, *cum, *cum_base, *row_base;
  float* voxels;          // nullable
  int32_t *coors, *num_points;
  int* vstart;
};

// VEC: C == 4, a row stride that is a multiple of 4 and 16-byte aligned bases: the row moves as one float4
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void scatter_kernel(const ScatterArgs a) {
  const long long j = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= a.n) return;
  const long long key = a.skey[j];
  if (key == a.sentinel) return;
  const int s = a.seg[j];                                       // where this cell starts in the sorted order
  const int b = (int)(key / a.G);
  const int rank = a.cum[a.order[s]] - 1 - a.cum_base[b];       // the cell's rank of appearance in its sample
  if (rank >= a.max_voxels) return;                             // a cell past the limit: its points are skipped
  const long long v = (long long)a.row_base[b] + rank;          // < min(n, B * max_voxels)
  const int slot = (int)(j - s);
  if (slot == 0) {
    const long long cell = key - (long long)b * a.G;
    const long long zy = cell / a.gx;
    int32_t* c = a.coors + v * 4;
    c[0] = b; c[1] = (int32_t)(zy / a.gy); c[2] = (int32_t)(zy % a.gy); c[3] = (int32_t)(cell % a.gx);
    a.vstart[v] = s;
  }
  if (j == a.n - 1 || a.skey[j + 1] != key) a.num_points[v] = slot + 1 < a.P ? slot + 1 : a.P;
  if (slot >= a.P || a.voxels == nullptr) return;
  const float* src = a.points + (long long)a.order[j] * a.stride;
  float* dst = a.voxels + (v * a.P + slot) * a.C;
  if (VEC) {
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
  } else {
    for (int c = 0; c < a.C; ++c) dst[c] = src[c];
  }
}

struct MeanArgs {
  const float* src;        // the points (through `order`) or caller-held voxels (order == nullptr)
  long long stride;        // floats between two rows of src
  const int *order, *vstart;
  const int32_t* num_points;
  const long long* num;    // nullable: rows at or past num[0] are written as zeros
  long long rows;
  int P, F;
  float* mean;
};

// the row of slot k of voxel v
__device__ __forceinline__ const float* slot_row(const MeanArgs& a, long long v, int k) {
  return a.order != nullptr ? a.src + (long long)a.order[a.vstart[v] + k] * a.stride : a.src + (v * a.P + k) * a.stride;
}

// slots 0, 1, 2, .. added in sequence to +0, then one division.  VEC: F == 4, a thread per voxel; else a thread per element.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void mean_kernel(const MeanArgs a) {
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const long long v = VEC ? t : t / a.F;
  if (v >= a.rows) return;
  int n = 0;
  if (a.num == nullptr || v < a.num[0]) {
    n = a.num_points[v];
    n = n < 0 ? 0 : (n > a.P ? a.P : n);
  }
  if (VEC) {
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < n; ++k) {
      const float4 p = *reinterpret_cast<const float4*>(slot_row(a, v, k));
      acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
    }
    if (n > 0) {
      const float d = (float)n;
      acc.x /= d; acc.y /= d; acc.z /= d; acc.w /= d;
    }
    *reinterpret_cast<float4*>(a.mean + v * 4) = acc;
  } else {
    const int f = (int)(t - v * a.F);
    float acc = 0.0f;
    for (int k = 0; k < n; ++k) acc += slot_row(a, v, k)[f];
    a.mean[t] = n > 0 ? acc / (float)n : 0.0f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void dynamic_kernel(const float* __restrict__ points, long long n, long long stride,
                                                        const int32_t* __restrict__ cnt, int B, const Geometry g,
                                                        int32_t* __restrict__ coors) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  int32_t x, y, z;
  const int32_t b = sample_of(i, cnt, B);
  const bool in = cell_of(points + i * stride, g, &x, &y, &z) && b >= 0;
  const int4 c = in ? make_int4(b, z, y, x) : make_int4(-1, -1, -1, -1);
  if (VEC) {
    *reinterpret_cast<int4*>(coors + i * 4) = c;
  } else {
    coors[i * 4] = c.x; coors[i * 4 + 1] = c.y; coors[i * 4 + 2] = c.z; coors[i * 4 + 3] = c.w;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static unsigned blocks_of(long long threads) { return (unsigned)((threads + BLOCK - 1) / BLOCK); }   // threads <= 2^31 * 2^6

static int launch_mean(const MeanArgs& a, hipStream_t s) {
  const bool vec = a.F == 4 && a.stride % 4 == 0 && aligned16(a.src) && aligned16(a.mean);
  if (vec) hipLaunchKernelGGL(mean_kernel<true>, dim3(blocks_of(a.rows)), dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL(mean_kernel<false>, dim3(blocks_of(a.rows * a.F)), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace hard_voxel

using namespace hard_voxel;

extern "C" {

size_t gd3d_hard_voxelize_workspace_bytes(int64_t N, int32_t B, int32_t max_voxels) {
  if (N <= 0 || N > 0x7fffffffLL || B <= 0 || max_voxels < 1) return 256;
  const Work w(nullptr, N, row_bound(N, B, max_voxels));
  return w.err == hipSuccess ? w.bytes : 0;
}

int gd3d_hard_voxelize(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                       const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t max_num_points,
                       int32_t max_voxels, int32_t num_features, void* workspace, float* voxels, float* mean, int32_t* coors,
                       int32_t* num_points, int32_t* voxel_batch_cnt, int64_t* num, void* stream) {
  Geometry g;
  const int rc = make_geometry(voxel_size, range_min, grid_size, N, B, &g);
  if (rc != 0) return rc;
  if (max_num_points < 1 || max_voxels < 1 || C < 3 || row_stride < C || num == nullptr) return GD3D_E_BADARG;
  if (mean != nullptr && (num_features < 1 || num_features > C)) return GD3D_E_BADARG;
  if (B > MAX_B || C > MAX_C) return GD3D_E_TOOLARGE;
  if (B > 0 && (points_batch_cnt == nullptr || voxel_batch_cnt == nullptr)) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  int e = 0;
  const int64_t rows = row_bound(N, B, max_voxels);
  if (rows == 0) {                                              // N == 0 or B == 0: no row of any output exists; the counts are zeros
    e = gd3d::fill_words(num, 2 * sizeof(int64_t), 0u, s);
    if (e == 0 && B > 0) e = gd3d::fill_words(voxel_batch_cnt, sizeof(int32_t) * (size_t)B, 0u, s);
    return e;                                                   // (otherwise sample_kernel writes both in full)
  }
  if (points == nullptr || workspace == nullptr || coors == nullptr || num_points == nullptr) return GD3D_E_BADARG;
  if (((uintptr_t)workspace & 255) != 0) return GD3D_E_BADARG;
  const Work w(workspace, N, rows);
  if (w.err != hipSuccess) return (int)w.err;
  // padding slots, and the rows past the total: coors -1, num_points 0, zero features (the mean kernel writes its own zeros)
  if (voxels != nullptr) {
    e = gd3d::fill_words(voxels, sizeof(float) * (size_t)rows * (size_t)max_num_points * (size_t)C, 0u, s);
    if (e != 0) return e;
  }
  e = gd3d::fill_words(coors, sizeof(int32_t) * 4 * (size_t)rows, 0xffffffffu, s);
  if (e != 0) return e;
  e = gd3d::fill_words(num_points, sizeof(int32_t) * (size_t)rows, 0u, s);
  if (e != 0) return e;
  const long long sentinel = (long long)B * g.G;
  const unsigned blocks = blocks_of(N);
  hipLaunchKernelGGL(key_kernel, dim3(blocks), dim3(BLOCK), 0, s, points, (long long)N, (long long)row_stride, points_batch_cnt, (int)B,
                     g, w.key_in, w.val_in);
  hipError_t he = gd3d::sort_pairs(w.sort_tmp, w.sort_bytes, w.key_in, w.key_out, w.val_in, w.order, (size_t)N,
                                   (unsigned)gd3d::key_bits(sentinel), s);
  if (he != hipSuccess) return (int)he;
  hipLaunchKernelGGL(head_kernel, dim3(blocks), dim3(BLOCK), 0, s, (const long long*)w.key_out, (const int*)w.order, (long long)N, sentinel,
                     w.head_pos, w.first);
  he = gd3d::inclusive_max(w.scan_tmp, w.scan_bytes, w.head_pos, w.seg, (size_t)N, s);
  if (he != hipSuccess) return (int)he;
  he = gd3d::inclusive_sum(w.scan_tmp, w.scan_bytes, w.first, w.cum, (size_t)N, s);
  if (he != hipSuccess) return (int)he;
  hipLaunchKernelGGL(sample_kernel, dim3(1), dim3(BLOCK), 0, s, points_batch_cnt, (int)B, (long long)N, (const int*)w.cum,
                     (const long long*)w.key_out, sentinel, (int)max_voxels, w.cum_base, w.row_base, voxel_batch_cnt, (long long*)num);
  ScatterArgs a;
  a.points = points; a.n = N; a.stride = row_stride; a.C = C; a.P = max_num_points; a.max_voxels = max_voxels;
  a.G = g.G; a.gx = g.gx; a.gy = g.gy; a.sentinel = sentinel;
  a.skey = w.key_out; a.order = w.order; a.seg = w.seg; a.cum = w.cum; a.cum_base = w.cum_base; a.row_base = w.row_base;
  a.voxels = voxels; a.coors = coors; a.num_points = num_points; a.vstart = w.vstart;
  const bool vec = C == 4 && row_stride % 4 == 0 && aligned16(points) && aligned16(voxels);
  if (vec) hipLaunchKernelGGL(scatter_kernel<true>, dim3(blocks), dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL(scatter_kernel<false>, dim3(blocks), dim3(BLOCK), 0, s, a);
  if (mean != nullptr) {
    MeanArgs m;
    m.src = points; m.stride = row_stride; m.order = w.order; m.vstart = w.vstart; m.num_points = num_points; m.num = (const long long*)num;
    m.rows = rows; m.P = max_num_points; m.F = num_features; m.mean = mean;
    return launch_mean(m, s);
  }
  return (int)hipGetLastError();
}

int gd3d_dynamic_voxelize(const float* points, int64_t N, int64_t row_stride, const int32_t* points_batch_cnt, int32_t B,
                          const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t* coors, void* stream) {
  Geometry g;
  const int rc = make_geometry(voxel_size, range_min, grid_size, N, B, &g);
  if (rc != 0) return rc;
  if (row_stride < 3) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || coors == nullptr || (B > 0 && points_batch_cnt == nullptr)) return GD3D_E_BADARG;
  if (aligned16(coors))
    hipLaunchKernelGGL(dynamic_kernel<true>, dim3(blocks_of(N)), dim3(BLOCK), 0, (hipStream_t)stream, points, (long long)N,
                       (long long)row_stride, points_batch_cnt, (int)B, g, coors);
  else
    hipLaunchKernelGGL(dynamic_kernel<false>, dim3(blocks_of(N)), dim3(BLOCK), 0, (hipStream_t)stream, points, (long long)N,
                       (long long)row_stride, points_batch_cnt, (int)B, g, coors);
  return (int)hipGetLastError();
}

int gd3d_voxel_mean(const float* voxels, const int32_t* num_points, int64_t V, int32_t P, int32_t C, int32_t num_features, float* mean,
                    void* stream) {
  if (V < 0 || P < 1 || C < 1 || num_features < 1 || num_features > C) return GD3D_E_BADARG;
  if (V > 0x7fffffffLL || C > MAX_C) return GD3D_E_TOOLARGE;
  if (V == 0) return 0;
  if (voxels == nullptr || num_points == nullptr || mean == nullptr) return GD3D_E_BADARG;
  MeanArgs m;
  m.src = voxels; m.stride = C; m.order = nullptr; m.vstart = nullptr; m.num_points = num_points; m.num = nullptr;
  m.rows = V; m.P = P; m.F = num_features; m.mean = mean;
  return launch_mean(m, (hipStream_t)stream);
}

}  // extern "C"
