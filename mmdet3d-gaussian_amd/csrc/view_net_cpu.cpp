// view_net_cpu.cpp — the `_cpu` twins of the multi-view pillar encoder's view ops (include/gd3d.h, gd3d_multi_view_voxelize_cpu,
// gd3d_pillar_scatter*_cpu, gd3d_view_sample*_cpu): plain loops over the per-element source of csrc/view_net_common.h, the source
// csrc/view_net.hip compiles for the device (both units with -ffp-contract=off).  The transformed points, the coors, the canvas, its
// gathered gradient and the sampled features are the kernels' bits.  The sampling backward is sequential — points in row order,
// neighbours nw, ne, sw, se, channels ascending — so it is deterministic; the kernel's atomically summed gradient may differ from it
// in the last bits where several points share a cell.  Rows are scattered onto the canvas in ascending order: at a duplicated cell
// the LAST row stays (the kernels leave one of the rows).  Host memory in and out, no stream, no HIP call, one thread.
#define GD3D_HOST_TWIN 1
#include "view_net_common.h"

#include "../../include/gd3d.h"

using namespace view_net;
using vsa_bev::Taps;

namespace {

void canvas_args(CanvasArgs* a, const float* src, float* dst, const void* coors, int32_t is64, int32_t ncol, int32_t layout, int64_t V,
                 int64_t C, int64_t B, int64_t ny, int64_t nx) {
  a->src = src; a->dst = dst; a->coors = coors; a->is64 = is64 != 0; a->ncol = ncol;
  a->V = V; a->C = C; a->B = B; a->ny = ny; a->nx = nx;
  int64_t sB, sC, sH, sW;
  vsa_bev::map_strides(layout, C, ny, nx, &sB, &sC, &sH, &sW);
  a->sB = sB; a->sC = sC; a->sH = sH; a->sW = sW;
}

void sample_args(SampleArgs* a, const float* xyz, int64_t xyz_stride, const void* ids, int32_t is64, int64_t id_stride, int32_t layout,
                 int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x, float half_x, float lo_y, float half_y) {
  a->xyz = xyz; a->xyz_stride = xyz_stride; a->ids = ids; a->is64 = is64 != 0; a->id_stride = id_stride;
  int64_t sB, sC, sH, sW;
  vsa_bev::map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  a->sB = sB; a->sC = sC; a->sH = sH; a->sW = sW;
  a->N = N; a->B = B; a->C = C; a->H = H; a->W = W;
  a->lo_x = lo_x; a->half_x = half_x; a->lo_y = lo_y; a->half_y = half_y;
  a->map = nullptr; a->gout = nullptr; a->out = nullptr; a->L = 1;
}

}  // namespace

extern "C" {

int gd3d_multi_view_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                                 int32_t num_views, const int32_t* view_kinds, const float* voxel_sizes, const float* range_mins,
                                 const int32_t* grid_sizes, float* const* view_points, int32_t* const* view_coors) {
  VoxArgs a;
  const int rc = make_vox_args(points, N, row_stride, C, points_batch_cnt, B, num_views, view_kinds, voxel_sizes, range_mins, grid_sizes,
                               view_points, view_coors, &a);
  if (rc != 0) return rc;
  for (int64_t i = 0; i < N; ++i) voxelize_point(a, i);
  return 0;
}

int gd3d_pillar_scatter_cpu(const float* voxel_features, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                            int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* canvas) {
  const int rc = check_canvas(coors_cols, layout, V, C, B, ny, nx);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (canvas == nullptr) return GD3D_E_BADARG;
  const int64_t total = B * C * ny * nx;
  for (int64_t i = 0; i < total; ++i) canvas[i] = 0.0f;
  if (V == 0) return 0;
  if (voxel_features == nullptr || coors == nullptr) return GD3D_E_BADARG;
  CanvasArgs a;
  canvas_args(&a, voxel_features, canvas, coors, coors_is_int64, coors_cols, layout, V, C, B, ny, nx);
  for (int64_t v = 0; v < V; ++v) {
    const long long cell = canvas_cell(a, v);
    if (cell < 0) continue;
    for (int64_t c = 0; c < C; ++c) canvas[cell + c * a.sC] = voxel_features[v * C + c];
  }
  return 0;
}

int gd3d_pillar_scatter_backward_cpu(const float* grad_canvas, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                                     int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* grad_features) {
  const int rc = check_canvas(coors_cols, layout, V, C, B, ny, nx);
  if (rc != 0 || V == 0) return rc;
  if (grad_features == nullptr || coors == nullptr || (B > 0 && grad_canvas == nullptr)) return GD3D_E_BADARG;
  CanvasArgs a;
  canvas_args(&a, grad_canvas, grad_features, coors, coors_is_int64, coors_cols, layout, V, C, B, ny, nx);
  for (int64_t v = 0; v < V; ++v) {
    const long long cell = canvas_cell(a, v);
    for (int64_t c = 0; c < C; ++c) grad_features[v * C + c] = cell >= 0 ? grad_canvas[cell + c * a.sC] : 0.0f;
  }
  return 0;
}

int gd3d_view_sample_cpu(const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64, int64_t id_stride,
                         const float* view_map, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                         float half_x, float lo_y, float half_y, float* out) {
  const int rc = check_sample(xyz_stride, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  if (rc != 0 || N == 0) return rc;
  if (pts_xyz == nullptr || ids == nullptr || out == nullptr || (B > 0 && view_map == nullptr)) return GD3D_E_BADARG;
  SampleArgs a;
  sample_args(&a, pts_xyz, xyz_stride, ids, ids_is_int64, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  for (int64_t n = 0; n < N; ++n) {
    const Taps t = taps_of(a, n);
    float* o = out + n * C;
    for (int64_t c = 0; c < C; ++c) {
      float v[4];
      for (int j = 0; j < 4; ++j) v[j] = t.use[j] ? view_map[t.off[j] + c * a.sC] : 0.0f;
      o[c] = vsa_bev::blend(v[0], v[1], v[2], v[3], t.w);
    }
  }
  return 0;
}

int gd3d_view_sample_backward_cpu(const float* grad_out, const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64,
                                  int64_t id_stride, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                                  float half_x, float lo_y, float half_y, float* workspace, float* grad_map) {
  (void)workspace;
  const int rc = check_sample(xyz_stride, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  if (rc != 0 || B == 0) return rc;
  if (grad_map == nullptr) return GD3D_E_BADARG;
  const int64_t total = B * C * H * W;
  for (int64_t i = 0; i < total; ++i) grad_map[i] = 0.0f;
  if (N == 0) return 0;
  if (grad_out == nullptr || pts_xyz == nullptr || ids == nullptr) return GD3D_E_BADARG;
  SampleArgs a;
  sample_args(&a, pts_xyz, xyz_stride, ids, ids_is_int64, id_stride, layout, N, B, C, H, W, lo_x, half_x, lo_y, half_y);
  for (int64_t n = 0; n < N; ++n) {
    const Taps t = taps_of(a, n);
    const float* g = grad_out + n * C;
    for (int j = 0; j < 4; ++j) {
      if (!t.use[j] || t.w[j] == 0.0f) continue;
      float* cell = grad_map + t.off[j];
      for (int64_t c = 0; c < C; ++c) cell[c * a.sC] += g[c] * t.w[j];
    }
  }
  return 0;
}

}  // extern "C"
