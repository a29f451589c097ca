// pib.hip — the point-in-rotated-box ops for gfx950 (include/gd3d.h, gd3d_pib_*, gd3d_roi_grid_points): mmdet3d 1.0's
// roiaware_pool3d `points_in_boxes_part` / `points_in_boxes_all` (a third-party CUDA extension the reference imports), the
// whole of PointwiseMaskHead.get_targets (models/roi_heads/mask_heads/pointwise_mask_head.py:62-92) in one launch, and
// Batch3DRoIGridExtractor.get_dense_grid_points (roi_extractors/batch_roigrid_extractor.py:56-71).
//
// Shapes:
//   first box (part, mask targets) : one lane per point, WG = 256 points of ONE sample per workgroup.  The sample's boxes pass
//                   through LDS in tiles of BOX_TILE as the constants (x, y, czm, hx, hy, hz, c, s) — for the mask targets the
//                   enlarged box's (czm, hx, hy, hz) next to them — computed once per workgroup.  Every lane walks the tile in
//                   ascending box index; all lanes read the same LDS address (a broadcast, no bank conflict).  A lane latches
//                   its first hit; a wave leaves the walk when every lane has latched, and when every wave has, no further
//                   tile is built.
//   all           : the kernel is write-bound, so the mapping follows the OUTPUT: a workgroup owns WG points x one tile of box
//                   columns; a lane owns a fixed run of E columns (E = 1 int32 / byte, E = 4 bytes packed into one dword store),
//                   keeps those boxes' constants in registers, and walks down the rows; consecutive lanes store consecutive
//                   addresses and the rows of one pass are adjacent.  Columns past box_cnt[b] carry all-zero constants, which
//                   contain nothing, so they are written 0 by the same code.
//   grid points   : one wave per RoI; its (G^3, 3) block is written as the contiguous run it is.
// Compiled with -ffp-contract=off: every decision and every grid point replays bit for bit in csrc/pib_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "pib_common.h"

namespace pib {

struct FirstArgs {
  const float* pts;
  const int32_t* pcnt;
  const float* boxes;      // (B, T, 7)
  const int64_t* labels;   // (B, T), MASK only
  const int32_t* box_cnt;  // nullable
  int B, T;
  long long N;
  float extra_width;
  long long num_classes;
  int64_t* seg;            // MASK only
  int32_t* box_idx;        // nullable when MASK
};

template <bool MASK>
__global__ __launch_bounds__(WG) void first_box_kernel(const FirstArgs a) {
  constexpr int W = MASK ? 12 : 8;   // floats per box in LDS: x y c s | czm hx hy hz | enlarged czm hx hy hz
  __shared__ __attribute__((aligned(16))) float cst[BOX_TILE * W];
  const int tid = threadIdx.x;
  int b = 0, np = 0;
  long long p0 = 0;
  if (!point_block(a.pcnt, a.B, a.N, (long long)blockIdx.x, b, p0, np)) return;   // block-uniform
  const int Tb = b < a.B ? boxes_of(a.box_cnt, b, a.T) : 0;
  const bool valid = tid < np;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) {
    const float* p = a.pts + (p0 + tid) * 3;
    px = p[0];
    py = p[1];
    pz = p[2];
  }
  int hit = -1, ehit = -1;
  bool pending = valid;
  for (int t0 = 0; t0 < Tb; t0 += BOX_TILE) {
    // the barrier that frees the previous tile; no lane of the workgroup is still looking: no further tile is built
    if (!__syncthreads_or(pending ? 1 : 0)) break;
    const int tn = (Tb - t0) < BOX_TILE ? (Tb - t0) : BOX_TILE;
    for (int j = tid; j < tn; j += WG) {
      const float* q = a.boxes + ((long long)b * a.T + t0 + j) * 7;
      const BoxC k = box_constants(q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
      float* o = cst + j * W;
      o[0] = k.x; o[1] = k.y; o[2] = k.c; o[3] = k.s;
      o[4] = k.czm; o[5] = k.hx; o[6] = k.hy; o[7] = k.hz;
      if (MASK) {
        const BoxC e = box_constants_enlarged(q[0], q[1], q[2], q[3], q[4], q[5], q[6], a.extra_width);
        o[8] = e.czm; o[9] = e.hx; o[10] = e.hy; o[11] = e.hz;
      }
    }
    __syncthreads();
    if (__ballot(pending) != 0ull) {   // wave-uniform: the walk below reads LDS at one address per step
      for (int k = 0; k < tn; ++k) {
        const float4 g = *reinterpret_cast<const float4*>(cst + k * W);
        const float4 h = *reinterpret_cast<const float4*>(cst + k * W + 4);
        const bool in = contains(g.x, g.y, h.x, h.y, h.z, h.w, g.z, g.w, px, py, pz);
        hit = (hit < 0 && in) ? t0 + k : hit;
        if (MASK) {
          const float4 e = *reinterpret_cast<const float4*>(cst + k * W + 8);
          const bool ein = contains(g.x, g.y, e.x, e.y, e.z, e.w, g.z, g.w, px, py, pz);
          ehit = (ehit < 0 && ein) ? t0 + k : ehit;
        }
        pending = valid && (hit < 0 || (MASK && ehit < 0));
        if (__ballot(pending) == 0ull) break;
      }
    }
  }
  if (!valid) return;   // past the last block-wide barrier
  const long long n = p0 + tid;
  if (MASK) {
    long long seg = hit >= 0 ? (long long)a.labels[(long long)b * a.T + hit] : a.num_classes;
    if ((hit >= 0) != (ehit >= 0)) seg = -1;   // the reference's xor: inside the enlarged box only (or, with a negative width, the original only)
    a.seg[n] = seg;
  }
  if (a.box_idx != nullptr) a.box_idx[n] = hit;
}

struct AllArgs {
  const float* pts;
  const int32_t* pcnt;
  const float* boxes;
  const int32_t* box_cnt;
  int B, T;
  long long N;
  void* out;   // (N, T)
};

template <typename OutT, int E>
__global__ __launch_bounds__(WG) void all_kernel(const AllArgs a) {
  __shared__ float cst[BOX_TILE * 8];
  __shared__ float spt[WG * 3];
  const int tid = threadIdx.x;
  int b = 0, np = 0;
  long long p0 = 0;
  if (!point_block(a.pcnt, a.B, a.N, (long long)blockIdx.x, b, p0, np)) return;   // block-uniform
  const int Tb = b < a.B ? boxes_of(a.box_cnt, b, a.T) : 0;
  const int t0 = blockIdx.y * BOX_TILE;
  const int tn = (a.T - t0) < BOX_TILE ? (a.T - t0) : BOX_TILE;   // columns of this workgroup: all T are written
  for (int j = tid; j < tn; j += WG) {
    BoxC k = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // hx = hy = 0: contains nothing
    if (t0 + j < Tb) {
      const float* q = a.boxes + ((long long)b * a.T + t0 + j) * 7;
      k = box_constants(q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
    }
    float* o = cst + j * 8;
    o[0] = k.x; o[1] = k.y; o[2] = k.czm; o[3] = k.hx; o[4] = k.hy; o[5] = k.hz; o[6] = k.c; o[7] = k.s;
  }
  for (int i = tid; i < np * 3; i += WG) spt[i] = a.pts[p0 * 3 + i];
  __syncthreads();
  const int slots = tn / E;          // runs of E columns per row (E == 4: T % 4 == 0, so tn % 4 == 0)
  const int rows = WG / slots;       // rows of one pass
  const int rr = tid / slots, d = tid - rr * slots;
  if (rr >= rows) return;            // no barrier below
  BoxC k[E];
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const float* o = cst + (d * E + u) * 8;
    k[u].x = o[0]; k[u].y = o[1]; k[u].czm = o[2]; k[u].hx = o[3]; k[u].hy = o[4]; k[u].hz = o[5]; k[u].c = o[6]; k[u].s = o[7];
  }
  OutT* const out = reinterpret_cast<OutT*>(a.out) + p0 * a.T + t0 + d * E;
#pragma unroll 2
  for (int p = rr; p < np; p += rows) {   // two rows in flight; more only spends registers (the stores set the pace)
    const float px = spt[3 * p], py = spt[3 * p + 1], pz = spt[3 * p + 2];
    if (E == 1) {
      out[(long long)p * a.T] = (OutT)(contains(k[0], px, py, pz) ? 1 : 0);
    } else {
      uint32_t v = 0;
#pragma unroll
      for (int u = 0; u < E; ++u) v |= (contains(k[u], px, py, pz) ? 1u : 0u) << (8 * u);
      *reinterpret_cast<uint32_t*>(out + (long long)p * a.T) = v;   // 4-byte aligned: base, T, t0 and d * E all are
    }
  }
}

struct GridArgs {
  const float* rois;
  long long R;
  int stride, first, G, clockwise;
  float* out;
};

constexpr int GW = 4;   // waves = RoIs per workgroup

__global__ __launch_bounds__(GW * 64) void roi_grid_kernel(const GridArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * GW + w;
  if (r >= a.R) return;
  const RoiC k = roi_constants(a.rois + r * a.stride + a.first);   // wave-uniform
  const int G = a.G, G2 = G * G, n = 3 * G2 * G;
  const float g = (float)G;
  float* const o = a.out + r * n;
  for (int f = lane; f < n; f += 64) {
    const int pt = f / 3, comp = f - pt * 3;
    const int i = pt / G2, rem = pt - i * G2;
    const int j = rem / G, kk = rem - j * G;
    o[f] = grid_coord(k, i, j, kk, g, a.clockwise, comp);
  }
}

static long long point_blocks(long long N, int B) { return (N + WG - 1) / WG + B + 1; }   // >= sum of ceil(n_b / WG), the uncovered tail included

template <bool MASK>
static int launch_first(const FirstArgs& a, hipStream_t s) {
  const long long blocks = point_blocks(a.N, a.B);
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipLaunchKernelGGL((first_box_kernel<MASK>), dim3((unsigned)blocks), dim3(WG), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace pib

using namespace pib;

extern "C" {

int gd3d_pib_box_tile(void) { return BOX_TILE; }
int gd3d_pib_workgroup_points(void) { return WG; }

int gd3d_pib_part(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt, int32_t B, int64_t N,
                  int32_t T, int32_t* box_idx, void* stream) {
  if (B < 0 || N < 0 || T < 0) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || box_idx == nullptr || (B > 0 && pts_batch_cnt == nullptr) || (B > 0 && T > 0 && boxes == nullptr)) return GD3D_E_BADARG;
  FirstArgs a;
  a.pts = points; a.pcnt = pts_batch_cnt; a.boxes = boxes; a.labels = nullptr; a.box_cnt = box_cnt;
  a.B = B; a.T = T; a.N = N; a.extra_width = 0.0f; a.num_classes = 0; a.seg = nullptr; a.box_idx = box_idx;
  return launch_first<false>(a, (hipStream_t)stream);
}

int gd3d_pib_mask_targets(const float* points, const int32_t* pts_batch_cnt, const float* gt_boxes, const int64_t* gt_labels,
                          const int32_t* box_cnt, int32_t B, int64_t N, int32_t T, float extra_width, int32_t num_classes,
                          int64_t* seg_targets, int32_t* box_idx, void* stream) {
  if (B < 0 || N < 0 || T < 0) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || seg_targets == nullptr || (B > 0 && pts_batch_cnt == nullptr)) return GD3D_E_BADARG;
  if (B > 0 && T > 0 && (gt_boxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  FirstArgs a;
  a.pts = points; a.pcnt = pts_batch_cnt; a.boxes = gt_boxes; a.labels = gt_labels; a.box_cnt = box_cnt;
  a.B = B; a.T = T; a.N = N; a.extra_width = extra_width; a.num_classes = num_classes; a.seg = seg_targets; a.box_idx = box_idx;
  return launch_first<true>(a, (hipStream_t)stream);
}

int gd3d_pib_all(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt, int32_t B, int64_t N,
                 int32_t T, void* flags, int32_t elem_size, void* stream) {
  if (B < 0 || N < 0 || T < 0 || (elem_size != 1 && elem_size != 4)) return GD3D_E_BADARG;
  if (N == 0 || T == 0) return 0;
  if (points == nullptr || flags == nullptr || (B > 0 && (pts_batch_cnt == nullptr || boxes == nullptr))) return GD3D_E_BADARG;
  const long long blocks = point_blocks(N, B);
  const long long tiles = ((long long)T + BOX_TILE - 1) / BOX_TILE;
  if (blocks > 0x7fffffffLL || tiles > 65535) return GD3D_E_TOOLARGE;
  AllArgs a;
  a.pts = points; a.pcnt = pts_batch_cnt; a.boxes = boxes; a.box_cnt = box_cnt; a.B = B; a.T = T; a.N = N; a.out = flags;
  const dim3 grid((unsigned)blocks, (unsigned)tiles);
  hipStream_t s = (hipStream_t)stream;
  if (elem_size == 4)
    hipLaunchKernelGGL((all_kernel<int32_t, 1>), grid, dim3(WG), 0, s, a);
  else if (T % 4 == 0 && (reinterpret_cast<uintptr_t>(flags) & 3) == 0)
    hipLaunchKernelGGL((all_kernel<uint8_t, 4>), grid, dim3(WG), 0, s, a);
  else   // rows that do not start on a dword: one byte per lane, still consecutive lanes on consecutive addresses
    hipLaunchKernelGGL((all_kernel<uint8_t, 1>), grid, dim3(WG), 0, s, a);
  return (int)hipGetLastError();
}

int gd3d_roi_grid_points(const float* rois, int32_t roi_stride, int32_t first_col, int64_t R, int32_t G, int32_t clockwise, float* out,
                         void* stream) {
  if (R < 0 || roi_stride < 7 || first_col < 0 || first_col + 7 > roi_stride || G < 1 || G > MAX_GRID) return GD3D_E_BADARG;
  if (R == 0) return 0;
  if (rois == nullptr || out == nullptr) return GD3D_E_BADARG;
  const long long blocks = (R + GW - 1) / GW;
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  GridArgs a;
  a.rois = rois; a.R = R; a.stride = roi_stride; a.first = first_col; a.G = G; a.clockwise = clockwise != 0; a.out = out;
  hipLaunchKernelGGL(roi_grid_kernel, dim3((unsigned)blocks), dim3(GW * 64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
