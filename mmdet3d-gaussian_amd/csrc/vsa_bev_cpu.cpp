// vsa_bev_cpu.cpp — the `_cpu` twins of the keypoint BEV interpolation and the voxel centres (include/gd3d.h,
// gd3d_vsa_bev_interp*_cpu, gd3d_vsa_voxel_centers_cpu): plain loops over the per-element source of csrc/vsa_bev_common.h, the source
// csrc/vsa_bev.hip compiles for the device (both units with -ffp-contract=off).  The forward, the centres and the counts are the
// kernels' bits.  The backward is sequential — keypoints in row order, neighbours nw, ne, sw, se, channels ascending — so it is
// deterministic; the kernel's atomically summed gradient may differ from it in the last bits where several keypoints share a cell.
// Host memory in and out, no stream, no HIP call, one thread.
#define GD3D_HOST_TWIN 1
#include "vsa_bev_common.h"

#include "../../include/gd3d.h"

using namespace vsa_bev;

extern "C" {

int gd3d_vsa_bev_interp_cpu(const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, const float* bev, int32_t layout, int64_t B,
                            int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x, float br_y, float* out) {
  const int rc = check_interp(kp_stride_b, kp_stride_m, layout, B, M, C, H, W, tl_x, tl_y, br_x, br_y);
  if (rc != 0) return rc;
  if (B == 0 || M == 0) return 0;
  if (keypoints == nullptr || bev == nullptr || out == nullptr) return GD3D_E_BADARG;
  int64_t sB, sC, sH, sW;
  map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  for (int64_t b = 0; b < B; ++b)
    for (int64_t m = 0; m < M; ++m) {
      const float* k = keypoints + b * kp_stride_b + m * kp_stride_m;
      const Taps t = make_taps(k[0], k[1], b, tl_x, tl_y, br_x, br_y, H, W, sB, sH, sW);
      float* o = out + (b * M + m) * C;
      for (int64_t c = 0; c < C; ++c) {
        float v[4];
        for (int j = 0; j < 4; ++j) v[j] = t.use[j] ? bev[t.off[j] + c * sC] : 0.0f;
        o[c] = blend(v[0], v[1], v[2], v[3], t.w);
      }
    }
  return 0;
}

int gd3d_vsa_bev_interp_backward_cpu(const float* grad_out, const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, int32_t layout,
                                     int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x, float br_y,
                                     float* grad_bev) {
  const int rc = check_interp(kp_stride_b, kp_stride_m, layout, B, M, C, H, W, tl_x, tl_y, br_x, br_y);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (grad_bev == nullptr) return GD3D_E_BADARG;
  const int64_t total = B * C * H * W;
  for (int64_t i = 0; i < total; ++i) grad_bev[i] = 0.0f;
  if (M == 0) return 0;
  if (grad_out == nullptr || keypoints == nullptr) return GD3D_E_BADARG;
  int64_t sB, sC, sH, sW;
  map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  for (int64_t b = 0; b < B; ++b)
    for (int64_t m = 0; m < M; ++m) {
      const float* k = keypoints + b * kp_stride_b + m * kp_stride_m;
      const Taps t = make_taps(k[0], k[1], b, tl_x, tl_y, br_x, br_y, H, W, sB, sH, sW);
      const float* g = grad_out + (b * M + m) * C;
      for (int j = 0; j < 4; ++j) {
        if (!t.use[j] || t.w[j] == 0.0f) continue;
        float* cell = grad_bev + t.off[j];
        for (int64_t c = 0; c < C; ++c) cell[c * sC] += g[c] * t.w[j];
      }
    }
  return 0;
}

int gd3d_vsa_voxel_centers_cpu(const void* coors, int32_t coors_is_int64, int64_t N, const float* voxel_size, float scale,
                               const float* range_min, const float* add, int32_t batch_size, float* xyz, int32_t* xyz_batch_cnt) {
  if (N < 0 || batch_size < 0 || voxel_size == nullptr || range_min == nullptr || add == nullptr) return GD3D_E_BADARG;
  if (batch_size > 0 && xyz_batch_cnt == nullptr) return GD3D_E_BADARG;
  for (int32_t b = 0; b < batch_size; ++b) xyz_batch_cnt[b] = 0;
  if (N == 0) return 0;
  if (coors == nullptr || xyz == nullptr) return GD3D_E_BADARG;
  for (int64_t i = 0; i < N; ++i) {
    int64_t c[4];
    for (int j = 0; j < 4; ++j)
      c[j] = coors_is_int64 ? static_cast<const int64_t*>(coors)[i * 4 + j] : (int64_t)static_cast<const int32_t*>(coors)[i * 4 + j];
    for (int j = 0; j < 3; ++j) xyz[i * 3 + j] = centre_axis((float)c[3 - j], voxel_size[j], scale, range_min[j], add[j]);
    if (c[0] >= 0 && c[0] < batch_size) xyz_batch_cnt[c[0]] += 1;
  }
  return 0;
}

}  // extern "C"
