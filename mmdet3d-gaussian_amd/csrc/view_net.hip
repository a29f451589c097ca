// view_net.hip — the multi-view pillar encoder's view ops for gfx950 (include/gd3d.h, gd3d_multi_view_voxelize /
// gd3d_pillar_scatter* / gd3d_view_sample*): what PillarODCenterPoint.voxelize and SingleViewNet.forward run outside
// their networks as chains of small torch ops per view and per sample.
//   voxelize_kernel   a thread per stacked point: the point is read ONCE, every view's transformed row and [b, z, y, x] cell written.
//   scatter_rows      channels-last canvas, both directions: a voxel's row of C floats shared by L lanes along C (16-byte accesses
//                     when C % 4 == 0 and the bases are aligned); forward writes canvas[cell] = features[v], backward gathers.
//   scatter_tile      contiguous NCHW canvas, both directions: a workgroup stages 64 voxels x 64 channels through LDS, so the side
//                     that touches the (V, C) rows has its lanes along C and the side that touches a channel plane has consecutive
//                     lanes on consecutive voxels — neighbouring cells when the voxels come sorted by (b, y, x), as a Scatter's do.
//   sample_kernel     lines :88-105 of SingleViewNet.forward for the whole batch: lanes along C, the map read where it lies.
//   sample_backward   grad_map[neighbour, c] += gout[n, c] * w with float atomics, lanes along C, after a fill; for a contiguous NCHW
//                     gradient with a workspace: the same launch into a channels-last workspace, then transpose_kernel writes every
//                     element of the NCHW gradient (64 x 64 tiles through LDS).
// No host read, no memset node; every output element is written.  Grids are not capped: a workgroup owns its rows, there is no
// grid-stride loop.  Compiled with -ffp-contract=off: the per-element math (csrc/view_net_common.h) is the operation sequence of
// csrc/view_net_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "view_net_common.h"

namespace view_net {

using vsa_bev::Taps;
using vsa_bev::blend;

__global__ __launch_bounds__(BLOCK) void voxelize_kernel(const VoxArgs a) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i < a.n) voxelize_point(a, i);
}

// FWD: dst = canvas, src = features.  !FWD: dst = grad_features (zeros for a row outside the canvas), src = grad_canvas.
template <bool FWD, bool VEC>
__global__ __launch_bounds__(BLOCK) void scatter_rows(const CanvasArgs a, int L) {
  const int sub = threadIdx.x & (L - 1);
  const long long v = (long long)blockIdx.x * (BLOCK / L) + threadIdx.x / L;
  if (v >= a.V) return;
  const long long cell = canvas_cell(a, v);
  if (FWD && cell < 0) return;
  if (VEC) {
    for (long long c = (long long)sub * QUAD; c < a.C; c += (long long)L * QUAD) {
      if (FWD) {
        *reinterpret_cast<float4*>(a.dst + cell + c) = *reinterpret_cast<const float4*>(a.src + v * a.C + c);
      } else {
        *reinterpret_cast<float4*>(a.dst + v * a.C + c) =
            cell >= 0 ? *reinterpret_cast<const float4*>(a.src + cell + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
  } else {
    for (long long c = sub; c < a.C; c += L) {
      if (FWD) a.dst[cell + c * a.sC] = a.src[v * a.C + c];
      else a.dst[v * a.C + c] = cell >= 0 ? a.src[cell + c * a.sC] : 0.0f;
    }
  }
}

template <bool FWD>
__global__ __launch_bounds__(BLOCK) void scatter_tile(const CanvasArgs a) {
  __shared__ float tile[TILE][TILE + 1];
  __shared__ long long cells[TILE];
  const long long v0 = (long long)blockIdx.x * TILE;
  const int lo = threadIdx.x & (TILE - 1), hi = threadIdx.x / TILE;      // hi in [0, BLOCK / TILE)
  if (threadIdx.x < TILE) cells[threadIdx.x] = v0 + threadIdx.x < a.V ? canvas_cell(a, v0 + threadIdx.x) : -1;
  __syncthreads();
  for (long long c0 = 0; c0 < a.C; c0 += TILE) {
    if (FWD) {
      for (int r = hi; r < TILE; r += BLOCK / TILE)                       // lanes along C: the rows of (V, C)
        if (v0 + r < a.V && c0 + lo < a.C) tile[r][lo] = a.src[(v0 + r) * a.C + c0 + lo];
      __syncthreads();
      const long long cell = cells[lo];                                   // lanes along the voxels: one channel plane
      if (cell >= 0)
        for (int c = hi; c < TILE && c0 + c < a.C; c += BLOCK / TILE) a.dst[cell + (c0 + c) * a.sC] = tile[lo][c];
    } else {
      const long long cell = cells[lo];
      for (int c = hi; c < TILE && c0 + c < a.C; c += BLOCK / TILE) tile[lo][c] = cell >= 0 ? a.src[cell + (c0 + c) * a.sC] : 0.0f;
      __syncthreads();
      for (int r = hi; r < TILE; r += BLOCK / TILE)
        if (v0 + r < a.V && c0 + lo < a.C) a.dst[(v0 + r) * a.C + c0 + lo] = tile[r][lo];
    }
    __syncthreads();
  }
}

// VEC: channels last, C % 4 == 0, 16-byte aligned bases: a lane takes every L-th quad of channels.  Otherwise a lane takes every
// L-th channel through sC.  No cross-lane operation.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void sample_kernel(const SampleArgs a) {
  const int sub = threadIdx.x & (a.L - 1);
  const long long n = (long long)blockIdx.x * (BLOCK / a.L) + threadIdx.x / a.L;
  if (n >= a.N) return;
  const Taps t = taps_of(a, n);
  float* o = a.out + n * a.C;
  if (VEC) {
    for (long long c = (long long)sub * QUAD; c < a.C; c += (long long)a.L * QUAD) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = t.use[j] ? *reinterpret_cast<const float4*>(a.map + t.off[j] + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      float4 q;
      q.x = blend(v[0].x, v[1].x, v[2].x, v[3].x, t.w);
      q.y = blend(v[0].y, v[1].y, v[2].y, v[3].y, t.w);
      q.z = blend(v[0].z, v[1].z, v[2].z, v[3].z, t.w);
      q.w = blend(v[0].w, v[1].w, v[2].w, v[3].w, t.w);
      *reinterpret_cast<float4*>(o + c) = q;
    }
  } else {
    for (long long c = sub; c < a.C; c += a.L) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = t.use[j] ? a.map[t.off[j] + c * a.sC] : 0.0f;
      o[c] = blend(v[0], v[1], v[2], v[3], t.w);
    }
  }
}

// a weight of exactly 0 adds nothing and is skipped
__global__ __launch_bounds__(BLOCK) void sample_backward_kernel(const SampleArgs a) {
  const int sub = threadIdx.x & (a.L - 1);
  const long long n = (long long)blockIdx.x * (BLOCK / a.L) + threadIdx.x / a.L;
  if (n >= a.N) return;
  const Taps t = taps_of(a, n);
  if (!(t.use[0] || t.use[1] || t.use[2] || t.use[3])) return;
  const float* g = a.gout + n * a.C;
  for (long long c = sub; c < a.C; c += a.L) {
    const float gv = g[c];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t.use[j] && t.w[j] != 0.0f) unsafeAtomicAdd(a.out + t.off[j] + c * a.sC, gv * t.w[j]);   // the hardware's no-return fp32 add
  }
}

// dst (B, C, P) = src (B, P, C) transposed per sample, P = H * W: 64 x 64 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(BLOCK) void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, long long C, long long P,
                                                           long long tiles_p, long long tiles_c) {
  __shared__ float tile[TILE][TILE + 1];
  long long id = blockIdx.x;
  const long long tp = id % tiles_p;
  id /= tiles_p;
  const long long tc = id % tiles_c, b = id / tiles_c;
  const int lo = threadIdx.x & (TILE - 1), hi = threadIdx.x / TILE;
  const long long p0 = tp * TILE, c0 = tc * TILE;
  for (int r = hi; r < TILE; r += BLOCK / TILE)
    if (p0 + r < P && c0 + lo < C) tile[r][lo] = src[(b * P + p0 + r) * C + c0 + lo];
  __syncthreads();
  for (int r = hi; r < TILE; r += BLOCK / TILE)
    if (c0 + r < C && p0 + lo < P) dst[(b * C + c0 + r) * P + p0 + lo] = tile[lo][r];
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static unsigned blocks_of(long long rows, long long per) { return (unsigned)((rows + per - 1) / per); }   // rows <= 2^31 - 1

static int launch_canvas(bool fwd, const float* src, float* dst, const void* coors, int32_t is64, int32_t ncol, int32_t layout, int64_t V,
                         int64_t C, int64_t B, int64_t ny, int64_t nx, hipStream_t s) {
  CanvasArgs a;
  a.src = src; a.dst = dst; a.coors = coors; a.is64 = is64 != 0; a.ncol = ncol;
  a.V = V; a.C = C; a.B = B; a.ny = ny; a.nx = nx;
  int64_t sB, sC, sH, sW;
  vsa_bev::map_strides(layout, C, ny, nx, &sB, &sC, &sH, &sW);
  a.sB = sB; a.sC = sC; a.sH = sH; a.sW = sW;
  if (layout == 0) {
    if (fwd) hipLaunchKernelGGL(scatter_tile<true>, dim3(blocks_of(V, TILE)), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL(scatter_tile<false>, dim3(blocks_of(V, TILE)), dim3(BLOCK), 0, s, a);
  } else {
    const bool vec = C % QUAD == 0 && aligned16(src) && aligned16(dst);
    const int L = vsa_bev::row_lanes(vec ? C / QUAD : C);
    const dim3 grid(blocks_of(V, BLOCK / L));
    if (fwd && vec) hipLaunchKernelGGL((scatter_rows<true, true>), grid, dim3(BLOCK), 0, s, a, L);
    else if (fwd) hipLaunchKernelGGL((scatter_rows<true, false>), grid, dim3(BLOCK), 0, s, a, L);
    else if (vec) hipLaunchKernelGGL((scatter_rows<false, true>), grid, dim3(BLOCK), 0, s, a, L);
    else hipLaunchKernelGGL((scatter_rows<false, false>), grid, dim3(BLOCK), 0, s, a, L);
  }
  return (int)hipGetLastError();
}

static void fill_sample(SampleArgs* a, const float* xyz, int64_t xyz_stride, const void* ids, int32_t is64, int64_t id_stride, int32_t layout,
                        int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x, float half_x, float lo_y, float half_y) {
  a->xyz = xyz; a->xyz_stride = xyz_stride; a->ids = ids; a->is64 = is64 != 0; a->id_stride = id_stride;
  int64_t sB, sC, sH, sW;
  vsa_bev::map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  a->sB = sB; a->sC = sC; a->sH = sH; a->sW = sW;
  a->N = N; a->B = B; a->C = C; a->H = H; a->W = W;
  a->lo_x = lo_x; a->half_x = half_x; a->lo_y = lo_y; a->half_y = half_y;
  a->map = nullptr; a->gout = nullptr; a->out = nullptr; a->L = 1;
}

}  // namespace view_net

using namespace view_net;

extern "C" {

int gd3d_multi_view_voxelize(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                             int32_t num_views, const int32_t* view_kinds, const float* voxel_sizes, const float* range_mins,
                             const int32_t* grid_sizes, float* const* view_points, int32_t* const* view_coors, void* stream) {
  VoxArgs a;
  const int rc = make_vox_args(points, N, row_stride, C, points_batch_cnt, B, num_views, view_kinds, voxel_sizes, range_mins, grid_sizes,
                               view_points, view_coors, &a);
  if (rc != 0 || N == 0) return rc;
  hipLaunchKernelGGL(voxelize_kernel, dim3(blocks_of(N, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_pillar_scatter(const float* voxel_features, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                        int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* canvas, void* stream) {
  const int rc = check_canvas(coors_cols, layout, V, C, B, ny, nx);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (canvas == nullptr) return GD3D_E_BADARG;
  const int e = gd3d::fill_words(canvas, sizeof(float) * (size_t)(B * C * ny * nx), 0u, (hipStream_t)stream);
  if (e != 0 || V == 0) return e;
  if (voxel_features == nullptr || coors == nullptr) return GD3D_E_BADARG;
  return launch_canvas(true, voxel_features, canvas, coors, coors_is_int64, coors_cols, layout, V, C, B, ny, nx, (hipStream_t)stream);
}

int gd3d_pillar_scatter_backward(const float* grad_canvas, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                                 int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* grad_features, void* stream) {
  const int rc = check_canvas(coors_cols, layout, V, C, B, ny, nx);
  if (rc != 0 || V == 0) return rc;
  if (grad_features == nullptr || coors == nullptr || (B > 0 && grad_canvas == nullptr)) return GD3D_E_BADARG;
  return launch_canvas(false, grad_canvas, grad_features, coors, coors_is_int64, coors_cols, layout, V, C, B, ny, nx, (hipStream_t)stream);
}

int gd3d_view_sample(const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64, int64_t id_stride, const float* view_map,
                     int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x, float half_x, float lo_y, float half_y,
                     float* out, void* stream) {
  const int rc = check_sample(xyz_stride, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  if (rc != 0 || N == 0) return rc;
  if (pts_xyz == nullptr || ids == nullptr || out == nullptr || (B > 0 && view_map == nullptr)) return GD3D_E_BADARG;
  SampleArgs a;
  fill_sample(&a, pts_xyz, xyz_stride, ids, ids_is_int64, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  a.map = view_map; a.out = out;
  const bool vec = layout == 1 && C % QUAD == 0 && aligned16(view_map) && aligned16(out);
  a.L = vsa_bev::row_lanes(vec ? C / QUAD : C);
  const dim3 grid(blocks_of(N, BLOCK / a.L));
  if (vec) hipLaunchKernelGGL(sample_kernel<true>, grid, dim3(BLOCK), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(sample_kernel<false>, grid, dim3(BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_view_sample_backward(const float* grad_out, const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64,
                              int64_t id_stride, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                              float half_x, float lo_y, float half_y, float* workspace, float* grad_map, void* stream) {
  const int rc = check_sample(xyz_stride, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  if (rc != 0 || B == 0) return rc;
  if (grad_map == nullptr) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = sizeof(float) * (size_t)(B * C * H * W);
  const bool via = layout == 0 && workspace != nullptr && N > 0;       // sum in channels last, then one transpose
  const long long P = H * W, tiles_p = (P + TILE - 1) / TILE, tiles_c = (C + TILE - 1) / TILE;
  if (via && tiles_p * tiles_c * B > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  const int e = gd3d::fill_words(via ? workspace : grad_map, bytes, 0u, s);
  if (e != 0 || N == 0) return e;
  if (grad_out == nullptr || pts_xyz == nullptr || ids == nullptr) return GD3D_E_BADARG;
  SampleArgs a;
  fill_sample(&a, pts_xyz, xyz_stride, ids, ids_is_int64, id_stride, via ? 1 : layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  a.gout = grad_out; a.out = via ? workspace : grad_map;
  a.L = vsa_bev::row_lanes(C);
  hipLaunchKernelGGL(sample_backward_kernel, dim3(blocks_of(N, BLOCK / a.L)), dim3(BLOCK), 0, s, a);
  if (via)
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(tiles_p * tiles_c * B)), dim3(BLOCK), 0, s, workspace, grad_map, (long long)C, P,
                       tiles_p, tiles_c);
  return (int)hipGetLastError();
}

}  // extern "C"
