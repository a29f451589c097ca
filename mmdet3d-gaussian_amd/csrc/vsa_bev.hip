// vsa_bev.hip — the statements of PV-RCNN's VoxelSetAbstraction.forward that feed its grouping ops, for gfx950 (include/gd3d.h,
// gd3d_vsa_bev_interp* / gd3d_vsa_voxel_centers):
//   * `interpolate_from_bev_features` (models/middle_encoders/voxel_set_abstraction.py:153-177): the grid normalisation, the
//     bilinear F.grid_sample(align_corners=True, zero padding) and the squeeze / permute / contiguous, as ONE launch that writes
//     (B, M, C) directly.  A keypoint's row of C channels is shared by L lanes along C, so the output stores are coalesced; the map
//     is read where it lies through element strides — contiguous NCHW (a channel per lane: four gathers of 4 bytes) or channels
//     last (each neighbour is C contiguous floats: 16-byte accesses when C % 4 == 0 and the bases are 16-byte aligned, 4-byte ones
//     otherwise; the same bits either way, the arithmetic per element being the same).
//   * its backward with respect to the map: a fill kernel zeroes grad_bev (every element is written; no memset node, as everywhere
//     in this library), then one launch adds value * weight into the four neighbours with float atomics, lanes along C — 256
//     contiguous bytes per wave-instruction in channels last, 64 different rows in NCHW.  No gradient for the keypoints.
//   * `get_voxel_centers` (:179-193) and the per-sample count loop of forward (:303-305) as one launch after a fill of the B counts:
//     the centres elementwise, the counts as integer adds reduced per wave (one add per distinct batch id in a wave).
// Compiled with -ffp-contract=off: the per-element math (csrc/vsa_bev_common.h) is the operation sequence of csrc/vsa_bev_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "vsa_bev_common.h"

namespace vsa_bev {

struct InterpArgs {
  const float* kp;           // (B, M, >= 2): columns 0 and 1 through the strides below
  long long kp_sb, kp_sm;
  const float* bev;          // forward: the map
  const float* gout;         // backward: (B, M, C) upstream gradient
  long long sB, sC, sH, sW;  // element strides of the map / of grad_bev
  long long B, M, C, H, W;
  float tl_x, tl_y, br_x, br_y;
  int L;                     // lanes per keypoint
  float* out;                // forward: (B, M, C); backward: grad_bev
};

__device__ __forceinline__ Taps taps_of(const InterpArgs& a, long long r) {
  const long long b = r / a.M, m = r - b * a.M;
  const float* k = a.kp + b * a.kp_sb + m * a.kp_sm;
  return make_taps(k[0], k[1], b, a.tl_x, a.tl_y, a.br_x, a.br_y, a.H, a.W, a.sB, a.sH, a.sW);
}

// VEC: channels last, C % 4 == 0, 16-byte aligned bases: a lane takes every L-th quad of channels.  Otherwise a lane takes every
// L-th channel through sC.  No cross-lane operation: a lane past the last keypoint just skips.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void interp_kernel(const InterpArgs a) {
  const int sub = threadIdx.x & (a.L - 1), rows = BLOCK / a.L;
  const long long R = a.B * a.M;
  for (long long r0 = (long long)blockIdx.x * rows; r0 < R; r0 += (long long)gridDim.x * rows) {
    const long long r = r0 + threadIdx.x / a.L;
    if (r >= R) continue;
    const Taps t = taps_of(a, r);
    float* o = a.out + r * a.C;
    if (VEC) {
      for (long long c = (long long)sub * QUAD; c < a.C; c += (long long)a.L * QUAD) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = t.use[j] ? *reinterpret_cast<const float4*>(a.bev + t.off[j] + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
        for (int j = 0; j < 4; ++j) v[j] = t.use[j] ? a.bev[t.off[j] + c * a.sC] : 0.0f;
        o[c] = blend(v[0], v[1], v[2], v[3], t.w);
      }
    }
  }
}

// grad_bev[neighbour j, c] += gout[r, c] * w_j for the neighbours in use; a weight of exactly 0 adds nothing and is skipped.
// Lanes along C: consecutive lanes add into consecutive channels (contiguous in channels last, sC apart in NCHW).
__global__ __launch_bounds__(BLOCK) void interp_backward_kernel(const InterpArgs a) {
  const int sub = threadIdx.x & (a.L - 1), rows = BLOCK / a.L;
  const long long R = a.B * a.M;
  for (long long r0 = (long long)blockIdx.x * rows; r0 < R; r0 += (long long)gridDim.x * rows) {
    const long long r = r0 + threadIdx.x / a.L;
    if (r >= R) continue;
    const Taps t = taps_of(a, r);
    if (!(t.use[0] || t.use[1] || t.use[2] || t.use[3])) continue;
    const float* g = a.gout + r * a.C;
    for (long long c = sub; c < a.C; c += a.L) {
      const float gv = g[c];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t.use[j] && t.w[j] != 0.0f) unsafeAtomicAdd(a.out + t.off[j] + c * a.sC, gv * t.w[j]);   // the hardware's no-return fp32 add
    }
  }
}

static unsigned row_grid(long long R, int L) {
  const long long rows = BLOCK / L, blocks = (R + rows - 1) / rows;
  return (unsigned)(blocks < 16384 ? blocks : 16384);   // beyond that a workgroup strides over the keypoints
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

struct CentreArgs {
  const void* coors;         // (N, 4) int32 or int64: b, z, y, x
  int is64;
  long long N;
  float vs[3], scale, mn[3], add[3];   // x, y, z
  int B;
  float* xyz;                // (N, 3)
  int* cnt;                  // (B), zeroed before the launch
};

__global__ __launch_bounds__(BLOCK) void voxel_centers_kernel(const CentreArgs a) {
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every thread of the workgroup: all 64 lanes of a wave reach the ballots below
  for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < a.N; i0 += (long long)gridDim.x * BLOCK) {
    const long long i = i0 + threadIdx.x;
    long long b = -1;
    if (i < a.N) {
      long long c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        c[j] = a.is64 ? (long long)static_cast<const int64_t*>(a.coors)[i * 4 + j] : (long long)static_cast<const int32_t*>(a.coors)[i * 4 + j];
      b = c[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) a.xyz[i * 3 + j] = centre_axis((float)c[3 - j], a.vs[j], a.scale, a.mn[j], a.add[j]);
    }
    const bool counted = b >= 0 && b < a.B;             // a row of no sample is counted nowhere; its centre is written above
    const int mine = counted ? (int)b : -1;
    unsigned long long todo = __ballot(counted);
    while (todo != 0ull) {                                // one integer add per distinct batch id in the wave: order-free, exact
      const int leader = __ffsll((long long)todo) - 1;
      const int id = __shfl(mine, leader);
      const unsigned long long same = __ballot(counted && mine == id);
      if (lane == leader) atomicAdd(a.cnt + id, __popcll(same));
      todo &= ~same;
    }
  }
}

}  // namespace vsa_bev

using namespace vsa_bev;

extern "C" {

int gd3d_vsa_bev_interp(const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, const float* bev, int32_t layout, int64_t B,
                        int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x, float br_y, float* out,
                        void* stream) {
  const int rc = check_interp(kp_stride_b, kp_stride_m, layout, B, M, C, H, W, tl_x, tl_y, br_x, br_y);
  if (rc != 0) return rc;
  if (B == 0 || M == 0) return 0;
  if (keypoints == nullptr || bev == nullptr || out == nullptr) return GD3D_E_BADARG;
  InterpArgs a;
  a.kp = keypoints; a.kp_sb = kp_stride_b; a.kp_sm = kp_stride_m; a.bev = bev; a.gout = nullptr;
  int64_t sB, sC, sH, sW;
  map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  a.sB = sB; a.sC = sC; a.sH = sH; a.sW = sW;
  a.B = B; a.M = M; a.C = C; a.H = H; a.W = W; a.tl_x = tl_x; a.tl_y = tl_y; a.br_x = br_x; a.br_y = br_y; a.out = out;
  const bool vec = layout == 1 && C % QUAD == 0 && aligned16(bev) && aligned16(out);
  a.L = row_lanes(vec ? C / QUAD : C);
  const dim3 grid(row_grid(B * M, a.L)), block(BLOCK);
  if (vec) hipLaunchKernelGGL(interp_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(interp_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_vsa_bev_interp_backward(const float* grad_out, const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, int32_t layout,
                                 int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x, float br_y,
                                 float* grad_bev, void* stream) {
  const int rc = check_interp(kp_stride_b, kp_stride_m, layout, B, M, C, H, W, tl_x, tl_y, br_x, br_y);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (grad_bev == nullptr) return GD3D_E_BADARG;
  const int e = gd3d::fill_words(grad_bev, sizeof(float) * (size_t)(B * C * H * W), 0u, (hipStream_t)stream);
  if (e != 0 || M == 0) return e;
  if (grad_out == nullptr || keypoints == nullptr) return GD3D_E_BADARG;
  InterpArgs a;
  a.kp = keypoints; a.kp_sb = kp_stride_b; a.kp_sm = kp_stride_m; a.bev = nullptr; a.gout = grad_out;
  int64_t sB, sC, sH, sW;
  map_strides(layout, C, H, W, &sB, &sC, &sH, &sW);
  a.sB = sB; a.sC = sC; a.sH = sH; a.sW = sW;
  a.B = B; a.M = M; a.C = C; a.H = H; a.W = W; a.tl_x = tl_x; a.tl_y = tl_y; a.br_x = br_x; a.br_y = br_y; a.out = grad_bev;
  a.L = row_lanes(C);
  hipLaunchKernelGGL(interp_backward_kernel, dim3(row_grid(B * M, a.L)), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_vsa_voxel_centers(const void* coors, int32_t coors_is_int64, int64_t N, const float* voxel_size, float scale,
                           const float* range_min, const float* add, int32_t batch_size, float* xyz, int32_t* xyz_batch_cnt,
                           void* stream) {
  if (N < 0 || batch_size < 0 || voxel_size == nullptr || range_min == nullptr || add == nullptr) return GD3D_E_BADARG;
  if (batch_size > 0) {
    if (xyz_batch_cnt == nullptr) return GD3D_E_BADARG;
    const int e = gd3d::fill_words(xyz_batch_cnt, sizeof(int32_t) * (size_t)batch_size, 0u, (hipStream_t)stream);
    if (e != 0) return e;
  }
  if (N == 0) return 0;
  if (coors == nullptr || xyz == nullptr) return GD3D_E_BADARG;
  CentreArgs a;
  a.coors = coors; a.is64 = coors_is_int64 != 0; a.N = N; a.scale = scale; a.B = batch_size; a.xyz = xyz; a.cnt = xyz_batch_cnt;
  for (int j = 0; j < 3; ++j) {
    a.vs[j] = voxel_size[j]; a.mn[j] = range_min[j]; a.add[j] = add[j];
  }
  const long long blocks = (N + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(voxel_centers_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(BLOCK), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
