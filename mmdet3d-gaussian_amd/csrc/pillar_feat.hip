// pillar_feat.hip — the pillar encoders' point decoration for gfx950 (include/gd3d.h, gd3d_point_voxel_stats / gd3d_pillar_decorate;
// DESIGN.md §3.15): what the pillar detectors run between voxelization and their first nn.Linear as chains of small torch ops.
//
// gd3d_point_voxel_stats — PointVoxelStatsCalculator.forward (models/voxel_encoders/utils.py:48-89) plus the cat of
// DynamicPillarFeatureNet.forward (pillar_encoder.py:215-216), two launches:
//   table_kernel   voxel-ordered, as vox::reduce_kernel walks: a sub-wave per voxel (4 lanes, or 16 with the covariance), a lane per
//                  table column; the voxel's points in ascending point index, four independent row loads in flight, added in sequence
//                  to +0, one division.  The covariance is a second walk in the same kernel over d = xyz - (the ROUNDED mean).  A lane
//                  of the covariance needs the means of two columns and sums both itself: no cross-lane traffic, the same bits.
//                  Writes (V, 3 | 12) floats, which stay in L2 / the Infinity Cache for the next launch.  Skipped when no flag needs it.
//   point_kernel   point-ordered over the FLAT output: a workgroup owns 64 consecutive point rows, a thread four consecutive output
//                  elements (element -> (point, column) -> csrc/pillar_feat_common.h's stats_element), stored as 16 bytes where the
//                  output is contiguous or its rows are whole 16-byte vectors, as 4-byte stores otherwise: the same bits.
// gd3d_pillar_decorate — the decoration of PillarFeatureNet.forward (pillar_encoder.py:105-153, legacy=False), one launch: a
//   workgroup owns up to 64 consecutive voxels; 3 threads per voxel add its filled slots in slot order (the sequence of
//   gd3d_voxel_mean) into LDS, then the workgroup writes its voxels' rows as one flat run, padded slots as +0 without reading them.
// No float atomics, no host read, every output element written exactly once.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "pillar_feat_common.h"

namespace pillar_feat {

// One walk over the run's points, four independent row loads in flight, everything added in sequence to +0.
// MODE 0: *s0 = the sum of column k.   MODE 1: *s0, *s1 = the sums of columns k and k2.   MODE 2: *s0 = the sum of (x_k - c) * (x_k2 - c2).
template <int MODE>
__device__ __forceinline__ void walk(const StatsArgs& a, int b, int e, int k, float c, int k2, float c2, float* s0, float* s1) {
  float acc = 0.0f, acc2 = 0.0f;
  int j = b;
  int next[4] = {0, 0, 0, 0};                                    // the ids of the NEXT four points: their loads overlap this group's rows,
  if (j + 4 <= e) {                                             // so a long voxel pays one memory round trip per group, not two
#pragma unroll
    for (int u = 0; u < 4; ++u) next[u] = a.order[j + u];
  }
  for (; j + 4 <= e; j += 4) {
    int pid[4];
    float x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pid[u] = next[u];
    if (j + 8 <= e) {
#pragma unroll
      for (int u = 0; u < 4; ++u) next[u] = a.order[j + 4 + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = (unsigned)pid[u] < (unsigned)a.n;
      const float* p = a.points + (long long)(ok ? pid[u] : 0) * a.stride;
      x[u] = ok ? p[k] : 0.0f;
      y[u] = (MODE != 0 && ok) ? p[k2] : 0.0f;
      if (!ok) pid[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (pid[u] < 0) continue;
      if (MODE == 2) {
        const float da = x[u] - c, db = y[u] - c2;
        const float prod = da * db;
        acc += prod;
      } else {
        acc += x[u];
        if (MODE == 1) acc2 += y[u];
      }
    }
  }
  for (; j < e; ++j) {
    const int pid = a.order[j];
    if ((unsigned)pid >= (unsigned)a.n) continue;
    const float* p = a.points + (long long)pid * a.stride;
    if (MODE == 2) {
      const float da = p[k] - c, db = p[k2] - c2;
      const float prod = da * db;
      acc += prod;
    } else {
      acc += p[k];
      if (MODE == 1) acc2 += p[k2];
    }
  }
  *s0 = acc;
  *s1 = acc2;
}

template <bool COV>
__global__ __launch_bounds__(BLOCK) void table_kernel(const StatsArgs a, float* __restrict__ table) {
  constexpr int CP = COV ? 16 : 4;                               // lanes of a sub-wave
  constexpr int USED = COV ? 9 : 3;
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int sub = lane / CP, ch = lane - sub * CP;
  const long long vox = wave * (64 / CP) + sub;
  if (vox >= a.v || ch >= USED) return;
  int b, e;
  stats_run(a, vox, &b, &e);
  const float cnt = (float)(e - b);
  const int ka = COV ? ch / 3 : ch, kb = COV ? ch - ka * 3 : ch;
  float sa, sb, prod, unused;
  if (COV) walk<1>(a, b, e, ka, 0.0f, kb, 0.0f, &sa, &sb);        // each column's sum is its own sequence: the bits of a walk alone
  else walk<0>(a, b, e, kb, 0.0f, 0, 0.0f, &sb, &unused);
  const float mb = sb / cnt;
  if (ch < 3) table[vox * a.ts + ch] = mb;                        // ch < 3: ka == 0 or !COV, kb == ch
  if (COV) {
    const float ma = sa / cnt;
    walk<2>(a, b, e, ka, ma, kb, mb, &prod, &unused);
    table[vox * a.ts + 3 + ch] = prod / cnt;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void point_kernel(const StatsArgs a) {
  const unsigned W = (unsigned)a.start[8];
  const long long r0 = (long long)blockIdx.x * STATS_ROWS;
  const long long left = a.n - r0;
  const unsigned rows = left < STATS_ROWS ? (unsigned)left : (unsigned)STATS_ROWS;
  const unsigned total = rows * W;
  if (VEC) {
    for (unsigned e = threadIdx.x * 4u; e < total; e += BLOCK * 4u) {
      unsigned i = e / W, col = e - i * W;
      float* dst = a.out + (r0 + i) * a.out_stride + col;        // the four lie one after the other (see launch_points)
      const unsigned cnt = total - e < 4u ? total - e : 4u;
      float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (unsigned u = 0; u < 4; ++u) {
        if (u < cnt) {
          val[u] = stats_element(a, r0 + i, (int)col);
          if (++col == W) {
            col = 0;
            ++i;
          }
        }
      }
      if (cnt == 4u) {
        *reinterpret_cast<float4*>(dst) = make_float4(val[0], val[1], val[2], val[3]);
      } else {
        for (unsigned u = 0; u < cnt; ++u) dst[u] = val[u];
      }
    }
  } else {
    for (unsigned e = threadIdx.x; e < total; e += BLOCK) {
      const unsigned i = e / W, col = e - i * W;
      a.out[(r0 + i) * a.out_stride + col] = stats_element(a, r0 + i, (int)col);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void decorate_kernel(const DecoArgs a, int gv) {
  __shared__ float mean[DECO_MAX_GV * 3];
  __shared__ int slots[DECO_MAX_GV];
  const long long v0 = (long long)blockIdx.x * gv;
  const long long left = a.v - v0;
  const int nv = left < gv ? (int)left : gv;
  const int t = threadIdx.x;
  if (t < nv * 3) {
    const int g = t / 3, k = t - g * 3;
    const int n = deco_slots(a, v0 + g);
    if (k == 0) slots[g] = n;
    mean[t] = ((a.flags & GD3D_PD_CLUSTER_CENTER) != 0 && n > 0) ? deco_mean(a, v0 + g, n, k) : 0.0f;
  }
  __syncthreads();
  const unsigned W = (unsigned)a.width, per = (unsigned)a.P * W, total = (unsigned)nv * per;
  float* base = a.out + v0 * (long long)per;
  if (VEC) {
    for (unsigned e = t * 4u; e < total; e += BLOCK * 4u) {
      unsigned g = e / per;
      const unsigned r = e - g * per;
      unsigned p = r / W, col = r - p * W;
      const unsigned cnt = total - e < 4u ? total - e : 4u;
      float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (unsigned u = 0; u < 4; ++u) {
        if (u < cnt) {
          val[u] = (int)p < slots[g] ? deco_element(a, v0 + g, (int)p, (int)col, mean + 3 * g) : 0.0f;
          if (++col == W) {
            col = 0;
            if (++p == (unsigned)a.P) {
              p = 0;
              ++g;
            }
          }
        }
      }
      if (cnt == 4u) {
        *reinterpret_cast<float4*>(base + e) = make_float4(val[0], val[1], val[2], val[3]);
      } else {
        for (unsigned u = 0; u < cnt; ++u) base[e + u] = val[u];
      }
    }
  } else {
    for (unsigned e = t; e < total; e += BLOCK) {
      const unsigned g = e / per, r = e - g * per, p = r / W, col = r - p * W;
      base[e] = (int)p < slots[g] ? deco_element(a, v0 + g, (int)p, (int)col, mean + 3 * g) : 0.0f;
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace pillar_feat

using namespace pillar_feat;

extern "C" {

int gd3d_point_voxel_stats(const float* points, int64_t N, int64_t row_stride, int32_t C, const void* coors, int32_t coors_is_int64,
                           int32_t ndim, const int32_t* map, const int32_t* counts, const int32_t* order, const int32_t* seg,
                           int64_t V, const float* voxel_size, const float* offset, int32_t flags, float* table, float* out,
                           int64_t out_stride, void* stream) {
  StatsArgs a;
  const int rc = stats_make(points, N, row_stride, C, coors, coors_is_int64, ndim, map, counts, order, seg, V, voxel_size, offset,
                            flags, table, out, out_stride, &a);
  if (rc != 0 || N == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (stats_needs_table(flags) && V > 0) {
    const bool cov = (flags & GD3D_PVS_COVARIANCE) != 0;
    const long long per_wave = cov ? 4 : 16;                      // voxels per wave
    const long long waves = (V + per_wave - 1) / per_wave;
    const unsigned blocks = (unsigned)((waves + BLOCK / 64 - 1) / (BLOCK / 64));   // V < 2^31
    if (cov) hipLaunchKernelGGL(table_kernel<true>, dim3(blocks), dim3(BLOCK), 0, s, a, table);
    else hipLaunchKernelGGL(table_kernel<false>, dim3(blocks), dim3(BLOCK), 0, s, a, table);
  }
  // four consecutive flat elements lie one after the other in memory, 16-byte aligned, when the output is contiguous (a workgroup
  // starts at a multiple of 64 rows) or when a row and the row stride are whole 16-byte vectors
  const int W = a.start[8];
  const bool vec = aligned16(out) && (out_stride == W || (W % 4 == 0 && out_stride % 4 == 0));
  const unsigned blocks = (unsigned)((N + STATS_ROWS - 1) / STATS_ROWS);
  if (vec) hipLaunchKernelGGL(point_kernel<true>, dim3(blocks), dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL(point_kernel<false>, dim3(blocks), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

int gd3d_pillar_decorate(const float* features, const int32_t* num_points, const int32_t* coors, int64_t V, int32_t P, int32_t C,
                         const float* voxel_size, const float* offset, int32_t flags, float* out, void* stream) {
  DecoArgs a;
  const int rc = deco_make(features, num_points, coors, V, P, C, voxel_size, offset, flags, out, &a);
  if (rc != 0 || V == 0) return rc;
  const long long per = (long long)P * a.width;                   // <= 2^30
  int gv = (int)(DECO_ELEMS / per);
  gv = gv < 1 ? 1 : (gv > DECO_MAX_GV ? DECO_MAX_GV : gv);
  if (gv >= 4) gv &= ~3;                                          // a workgroup's run starts at a multiple of 4 floats
  const bool vec = aligned16(out) && ((long long)gv * per) % 4 == 0;
  const unsigned blocks = (unsigned)((V + gv - 1) / gv);
  if (vec) hipLaunchKernelGGL(decorate_kernel<true>, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, a, gv);
  else hipLaunchKernelGGL(decorate_kernel<false>, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, a, gv);
  return (int)hipGetLastError();
}

}  // extern "C"
