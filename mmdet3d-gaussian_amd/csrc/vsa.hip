// vsa.hip — PV-RCNN's voxel-set-abstraction ops for gfx950: stacked ball query, point grouping (forward, backward), the
// two fused, and furthest point sampling (include/gd3d.h, gd3d_vsa_*).  Replaces the reference's CUDA extension
//   /root/reference/mmdet3d_gaussian/ops/vsa/src/ball_query.cu:12-72, src/group_points.cu:14-90, src/sampling.cu:22-152
// behind ops/vsa/group_points.py (`QueryAndGroup`) and ops/vsa/sample_points.py (`furthest_point_sample`).
//
// Shapes:
//   scan / gather : one wave per query, QW queries of ONE sample per workgroup.  The sample's points pass through LDS in tiles
//                   of TILE points that the workgroup's waves share; a wave tests 64 consecutive points per step, a ballot and
//                   a lane prefix count give every member its slot (ascending index by construction), and a wave that has its
//                   nsample members scans no further; when every wave has, no further tile is loaded.  The fused form then
//                   gathers: feature rows are read as contiguous runs, transposed through a per-wave LDS buffer (rows padded to
//                   an odd stride) and the query's (3 + C, nsample) block is written as the contiguous run it is.
//   backward      : one wave per query; the (C, nsample) gradient block is read contiguously, transposed through LDS, the padded
//                   tail folded into the first member's row, and added with float atomics whose wave instruction covers
//                   contiguous floats of one feature row (MI355X: 256 B or 2 x 128 B per instruction run at the full atomic rate,
//                   one lane per row 17x slower).
//   FPS           : one workgroup of 1024 threads per sample; 16 points per thread and their running minimum live in registers
//                   (the rest, beyond 16384 points, in a global workspace); per pick: update, per-thread best, wave arg max by
//                   DPP, one LDS slot per wave (double-buffered: ONE barrier per pick), every wave reduces the 16 slots itself.
// Compiled with -ffp-contract=off: membership and arg-max decisions replay bit for bit in csrc/vsa_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "vsa_common.h"
#include "vsa_gather.h"

namespace vsa {

constexpr int QW = 8;                    // waves = queries per workgroup (scan / gather kernel)
constexpr int QTHREADS = QW * 64;
constexpr int TILE = 1024;               // points per LDS tile: 12 KiB, kept as they lie in memory (x y z x y z ...)
constexpr int BW = 4;                    // waves = queries per workgroup (backward kernel)

enum { MODE_QUERY = 0, MODE_QUERY_GROUP = 1, MODE_GROUP = 2 };

struct QagArgs {
  const float* xyz;
  const int32_t* xyz_cnt;
  const float* new_xyz;
  const int32_t* new_cnt;
  const float* feats;
  const int32_t* idx_in;   // MODE_GROUP
  int B;
  long long N, M;
  int C, nsample, c_xyz;   // c_xyz: 3 when the xyz channels are written, else 0
  int cc;                  // feature channels per pass through the transpose buffer
  unsigned magic_ns;       // floor(2^32 / nsample) + 1: e / nsample == __umulhi(e, magic_ns) for e < 2^32 / nsample (nsample > 1)
  float radius2;
  float* out;
  int32_t* idx;
  int32_t* cnt;
  uint8_t* mask;
};

template <int MODE>
__global__ __launch_bounds__(QTHREADS) void qag_kernel(const QagArgs a) {
  constexpr bool SCAN = MODE != MODE_GROUP;
  constexpr bool GROUP = MODE != MODE_QUERY;
  extern __shared__ float lds_f[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long q0 = 0, p0 = 0;
  int nq = 0, np = 0;
  if (!item_segment<QW>(a.xyz_cnt, a.new_cnt, a.B, a.N, a.M, (long long)blockIdx.x, q0, nq, p0, np)) return;  // block-uniform
  const bool has_q = w < nq;
  const long long m = q0 + w;
  const int nsample = a.nsample;
  float* const tile = lds_f;
  int* const lidx = reinterpret_cast<int*>(lds_f + (SCAN ? 3 * TILE : 0)) + w * nsample;
  float* const xp = reinterpret_cast<float*>(reinterpret_cast<int*>(lds_f + (SCAN ? 3 * TILE : 0)) + QW * nsample) + w * XP;
  int found = 0;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (SCAN) {
    if (has_q) {
      cx = a.new_xyz[m * 3 + 0];
      cy = a.new_xyz[m * 3 + 1];
      cz = a.new_xyz[m * 3 + 2];
    }
    bool done = !has_q;
    for (int t0 = 0; t0 < np; t0 += TILE) {
      // the barrier that frees the previous tile; no wave needs more points: no further tile is loaded
      if (!__syncthreads_or(done ? 0 : 1)) break;
      const int tn = (np - t0) < TILE ? (np - t0) : TILE;
      const float* src = a.xyz + (p0 + t0) * 3;
      for (int i = tid; i < tn * 3; i += QTHREADS) tile[i] = src[i];
      __syncthreads();
      if (!done) {
        for (int k = 0; k < tn; k += 64) {
          const int p = k + lane;
          bool member = false;
          if (p < tn) member = dist2(cx, cy, cz, tile[3 * p], tile[3 * p + 1], tile[3 * p + 2]) < a.radius2;
          const unsigned long long bal = __ballot(member);
          if (bal != 0ull) {
            const int slot = found + __popcll(bal & ((1ull << lane) - 1ull));
            if (member && slot < nsample) lidx[slot] = t0 + p;
            found += __popcll(bal);
            if (found >= nsample) {   // early stop: later points cannot change idx, cnt or the mask
              found = nsample;
              done = true;
              break;
            }
          }
        }
      }
    }
    if (!has_q) return;   // past the last block-wide barrier
  } else {
    if (!has_q) return;
    found = np > 0 ? nsample : 0;   // a sample without points has nothing to gather: zeros
    if (found)
      for (int s = lane; s < nsample; s += 64) lidx[s] = clamp_index(a.idx_in[m * nsample + s], np);
  }
  write_query<SCAN, GROUP>(a, m, p0, lidx, xp, found, cx, cy, cz, lane);   // csrc/vsa_gather.h: shared with csrc/voxel_query.hip
}

// ---------------------------------------------------------------------------------------------------------------- backward
struct BwdArgs {
  const float* gout;        // (M, ct, nsample)
  const int32_t* idx;       // (M, nsample)
  const int32_t* cnt;       // (M) or NULL: every slot is a contribution of its own
  const int32_t* feat_cnt;
  const int32_t* idx_cnt;
  int B;
  long long N, M;
  int C, nsample, ct, c_off, cc;
  unsigned magic_ns;
  float* gfeat;             // (N, C), zero-filled
};

__global__ __launch_bounds__(BW * 64) void group_backward_kernel(const BwdArgs a) {
  extern __shared__ float lds_f[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long m = (long long)blockIdx.x * BW + w;
  if (m >= a.M) return;   // no block-wide barrier below
  long long p0 = 0;
  int np = 0;
  if (!row_segment(a.feat_cnt, a.idx_cnt, a.B, a.N, a.M, m, p0, np) || np <= 0) return;
  const int nsample = a.nsample;
  int found = nsample;
  if (a.cnt != nullptr) {
    found = a.cnt[m];
    found = found < 0 ? 0 : (found > nsample ? nsample : found);
  }
  if (found == 0) return;   // empty ball: no gradient
  int* const lidx = reinterpret_cast<int*>(lds_f) + w * nsample;
  float* const xp = reinterpret_cast<float*>(reinterpret_cast<int*>(lds_f) + BW * nsample) + w * XP;
  for (int s = lane; s < found; s += 64) lidx[s] = clamp_index(a.idx[m * nsample + s], np);
  const int pad = nsample | 1;
  const float* const g = a.gout + (m * a.ct + a.c_off) * nsample;
  for (int c0 = 0; c0 < a.C; c0 += a.cc) {
    const int cw = (a.C - c0) < a.cc ? (a.C - c0) : a.cc;
    const float* const gc = g + (long long)c0 * nsample;
    for (int e = lane; e < cw * nsample; e += 64) {   // the block as the contiguous run it is
      const int ch = div_nsample(e, nsample, a.magic_ns);
      xp[ch * pad + (e - ch * nsample)] = gc[e];
    }
    wave_sync();
    if (found < nsample) {   // the padded slots all name the first member: one sum, one add
      for (int ch = lane; ch < cw; ch += 64) {
        float acc = xp[ch * pad];
        for (int s = found; s < nsample; ++s) acc += xp[ch * pad + s];
        xp[ch * pad] = acc;
      }
      wave_sync();
    }
    const int r = cw >= 64 ? 1 : 64 / cw;
    const int sub = cw >= 64 ? 0 : lane / cw;
    const int ch0 = lane - sub * cw;
    if (sub < r) {
      for (int s = sub; s < found; s += r) {
        float* const row = a.gfeat + (p0 + lidx[s]) * a.C + c0;
        for (int ch = ch0; ch < cw; ch += 64) atomicAdd(row + ch, xp[ch * pad + s]);   // contiguous floats of one row per instruction
      }
    }
    wave_sync();
  }
}

// Clears a buffer from a KERNEL (this library puts no memset node into paths a caller may capture: csrc/voxel_scatter.hip).
__global__ __launch_bounds__(256) void zero_floats_kernel(float* __restrict__ p, long long n) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = 0.0f;
}

static int zero_floats(float* p, long long n, hipStream_t s) {
  if (n <= 0) return 0;
  long long blocks = (n + 1023) / 1024;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(zero_floats_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, n);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------------- FPS
// arg-max key: (distance, LOWEST index); a total order, so every reduction tree gives the same winner
template <int CTRL>
__device__ __forceinline__ void key_max_dpp(float& d, int& i) {
  const float od = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(d), __float_as_int(d), CTRL, 0xf, 0xf, false));
  const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false);
  const bool take = od > d || (od == d && oi < i);
  d = take ? od : d;
  i = take ? oi : i;
}
// after it every lane of a row of 16 holds the row's maximum
__device__ __forceinline__ void key_max_row16(float& d, int& i) {
  key_max_dpp<0xB1>(d, i);    // quad_perm [1,0,3,2]
  key_max_dpp<0x4E>(d, i);    // quad_perm [2,3,0,1]
  key_max_dpp<0x141>(d, i);   // row_half_mirror
  key_max_dpp<0x140>(d, i);   // row_mirror
}
__device__ __forceinline__ void key_max_take(float& d, int& i, float od, int oi) {
  const bool take = od > d || (od == d && oi < i);
  d = take ? od : d;
  i = take ? oi : i;
}

template <typename OutT>
__global__ __launch_bounds__(FPS_THREADS) void fps_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ cnt, int B,
                                                          long long N, int n_fixed, int npoint, OutT* __restrict__ out,
                                                          float* __restrict__ ws) {
  __shared__ float s_d[2][16], s_x[2][16], s_y[2][16], s_z[2][16];
  __shared__ int s_i[2][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x;
  long long p0 = 0;
  int n = n_fixed;
  if (cnt != nullptr) {
    for (int k = 0; k < b; ++k) p0 += clamp_count(cnt[k], N - p0);
    n = (int)clamp_count(cnt[b], N - p0);
  } else {
    p0 = (long long)b * n_fixed;
  }
  OutT* const o = out + (long long)b * npoint;
  if (n <= 0) {   // block-uniform
    for (int j = tid; j < npoint; j += FPS_THREADS) o[j] = (OutT)0;
    return;
  }
  const float* const P = xyz + p0 * 3;
  float* const T = ws + p0;   // running minimum of the points beyond the registers
  float x[FPS_PPT], y[FPS_PPT], z[FPS_PPT], t[FPS_PPT];
#pragma unroll
  for (int j = 0; j < FPS_PPT; ++j) {
    const int k = j * FPS_THREADS + tid;
    const bool valid = k < n;
    x[j] = valid ? P[3 * k + 0] : 0.0f;
    y[j] = valid ? P[3 * k + 1] : 0.0f;
    z[j] = valid ? P[3 * k + 2] : 0.0f;
    t[j] = valid ? FPS_FAR : -1.0f;   // -1: below every distance, never updated (d < -1 is false), never picked
  }
  for (int k = FPS_CAP + tid; k < n; k += FPS_THREADS) T[k] = FPS_FAR;   // read back by this same thread only
  float px = P[0], py = P[1], pz = P[2];
  const int picks = npoint < n ? npoint : n;
  if (tid == 0)
    for (int q = 0; q < npoint; q += n) o[q] = (OutT)0;   // pick 0 and its cyclic copies
  for (int p = 1; p < picks; ++p) {
    float bd = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < FPS_PPT; ++j) {   // ascending index inside the thread: strict > keeps the lowest
      const float d = dist2(px, py, pz, x[j], y[j], z[j]);
      const float tt = d < t[j] ? d : t[j];
      t[j] = tt;
      const bool better = tt > bd;
      bd = better ? tt : bd;
      bi = better ? j * FPS_THREADS + tid : bi;
      bx = better ? x[j] : bx;
      by = better ? y[j] : by;
      bz = better ? z[j] : bz;
    }
    for (int k = FPS_CAP + tid; k < n; k += FPS_THREADS) {
      const float xk = P[3 * k + 0], yk = P[3 * k + 1], zk = P[3 * k + 2];
      const float d = dist2(px, py, pz, xk, yk, zk);
      const float tk = T[k];
      const float tt = d < tk ? d : tk;
      T[k] = tt;
      const bool better = tt > bd;
      bd = better ? tt : bd;
      bi = better ? k : bi;
      bx = better ? xk : bx;
      by = better ? yk : by;
      bz = better ? zk : bz;
    }
    float wd = bd;
    int wi = bi;
    key_max_row16(wd, wi);
    {
      float d0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wd), 0));
      int i0 = __builtin_amdgcn_readlane(wi, 0);
      key_max_take(d0, i0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wd), 16)), __builtin_amdgcn_readlane(wi, 16));
      key_max_take(d0, i0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wd), 32)), __builtin_amdgcn_readlane(wi, 32));
      key_max_take(d0, i0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wd), 48)), __builtin_amdgcn_readlane(wi, 48));
      wd = d0;
      wi = i0;
    }
    const int buf = p & 1;
    if (bi == wi) {   // the lane that owns the wave's winner (indices are unique; a wave without points writes its zeros)
      s_d[buf][w] = wd;
      s_i[buf][w] = wi;
      s_x[buf][w] = bx;
      s_y[buf][w] = by;
      s_z[buf][w] = bz;
    }
    __syncthreads();   // the only barrier of a pick: the next pick writes the other buffer
    float gd = s_d[buf][lane & 15];
    int gi = s_i[buf][lane & 15];
    key_max_row16(gd, gi);
    const int ww = (gi >> 6) & 15;   // the wave that owns point gi (index = j * 1024 + thread)
    px = s_x[buf][ww];
    py = s_y[buf][ww];
    pz = s_z[buf][ww];
    if (tid == 0)
      for (int q = p; q < npoint; q += n) o[q] = (OutT)gi;
  }
}

// Dynamic LDS of a qag_kernel<MODE> launch: the point tile (scanning modes, 12288 B), the waves' idx rows (32 * nsample B) and
// the waves' transpose buffers (grouping modes, 34816 B):
//   MODE_QUERY        12288 + 32 * nsample  <= 45056 B
//   MODE_QUERY_GROUP  47104 + 32 * nsample  >  64 KiB from nsample 577 on, 79872 B at MAX_NSAMPLE
//   MODE_GROUP        34816 + 32 * nsample  >  64 KiB from nsample 961 on, 67584 B at MAX_NSAMPLE
// (the backward: 17408 + 16 * nsample <= 33792 B).
template <int MODE>
constexpr size_t qag_lds_bytes(int nsample) {
  return ((MODE != MODE_GROUP ? 3 * TILE : 0) + (size_t)QW * nsample + (MODE != MODE_QUERY ? (size_t)QW * XP : 0)) * 4;
}
static_assert(qag_lds_bytes<MODE_QUERY>(MAX_NSAMPLE) <= 65536, "the stand-alone query needs no raised dynamic-LDS limit");
static_assert(qag_lds_bytes<MODE_QUERY_GROUP>(MAX_NSAMPLE) <= 160 * 1024 && qag_lds_bytes<MODE_GROUP>(MAX_NSAMPLE) <= 160 * 1024,
              "the largest request must fit the 160 KiB LDS of a gfx950 CU");

template <int MODE>
static int launch_qag(const QagArgs& a, hipStream_t s) {
  const long long blocks = (a.M + QW - 1) / QW + a.B + 1;   // sum over samples of ceil(M_b / QW), bounded without reading the counts
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  const size_t lds = qag_lds_bytes<MODE>(a.nsample);
  if (lds > 65536) {   // beyond the default limit: raised once per device and instance, sized for MAX_NSAMPLE (a captured launch
                       // never calls it: the warm-up did)
    static bool attr_set[64] = {};
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess) return GD3D_E_BADARG;
    if (devid < 0 || devid >= 64 || !attr_set[devid]) {
      const hipError_t e = hipFuncSetAttribute((const void*)qag_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)qag_lds_bytes<MODE>(MAX_NSAMPLE));
      if (e != hipSuccess) return (int)e;
      if (devid >= 0 && devid < 64) attr_set[devid] = true;
    }
  }
  hipLaunchKernelGGL((qag_kernel<MODE>), dim3((unsigned)blocks), dim3(QTHREADS), lds, s, a);
  return (int)hipGetLastError();
}

static int launch_backward(const float* grad_out, const int32_t* idx, const int32_t* cnt, const int32_t* idx_cnt,
                           const int32_t* feat_cnt, int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample, int32_t ct,
                           int32_t c_off, float* grad_features, void* stream) {
  if (B < 0 || N < 0 || M < 0 || C < 0 || nsample <= 0 || c_off < 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE) return GD3D_E_TOOLARGE;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || C == 0) return 0;
  if (grad_features == nullptr) return GD3D_E_BADARG;
  const int e = zero_floats(grad_features, (long long)N * C, s);
  if (e != 0 || M == 0 || B == 0) return e;
  if (grad_out == nullptr || idx == nullptr || idx_cnt == nullptr || feat_cnt == nullptr) return GD3D_E_BADARG;
  const long long blocks = (M + BW - 1) / BW;
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  BwdArgs a;
  a.gout = grad_out; a.idx = idx; a.cnt = cnt; a.feat_cnt = feat_cnt; a.idx_cnt = idx_cnt;
  a.B = B; a.N = N; a.M = M; a.C = C; a.nsample = nsample; a.ct = ct; a.c_off = c_off;
  a.cc = channels_per_pass(C, nsample);
  a.magic_ns = magic_of(nsample);
  a.gfeat = grad_features;
  const size_t lds = ((size_t)BW * nsample + (size_t)BW * XP) * 4;
  hipLaunchKernelGGL(group_backward_kernel, dim3((unsigned)blocks), dim3(BW * 64), lds, s, a);
  return (int)hipGetLastError();
}

}  // namespace vsa

using namespace vsa;

extern "C" {

int gd3d_vsa_ball_query(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz, const int32_t* new_xyz_batch_cnt,
                        int32_t B, int64_t N, int64_t M, float radius, int32_t nsample, int32_t* idx, int32_t* cnt,
                        uint8_t* empty_mask, void* stream) {
  return gd3d_vsa_query_and_group(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, nullptr, B, N, M, 0, radius, nsample, 0, nullptr,
                                  idx, cnt, empty_mask, stream);
}

int gd3d_vsa_query_and_group(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                             const int32_t* new_xyz_batch_cnt, const float* features, int32_t B, int64_t N, int64_t M, int32_t C,
                             float radius, int32_t nsample, int32_t use_xyz, float* out, int32_t* idx, int32_t* cnt,
                             uint8_t* empty_mask, void* stream) {
  if (B < 0 || N < 0 || M < 0 || C < 0 || nsample <= 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE) return GD3D_E_TOOLARGE;
  if (M == 0) return 0;
  if (new_xyz == nullptr || idx == nullptr || (B > 0 && (xyz_batch_cnt == nullptr || new_xyz_batch_cnt == nullptr))) return GD3D_E_BADARG;
  if (N > 0 && xyz == nullptr) return GD3D_E_BADARG;
  if (C > 0 && features == nullptr && N > 0) return GD3D_E_BADARG;
  const bool group = out != nullptr;
  if (group && !use_xyz && C == 0) return GD3D_E_BADARG;   // nothing to write
  if ((long long)((use_xyz ? 3 : 0) + C) * nsample > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  QagArgs a;
  a.xyz = xyz; a.xyz_cnt = xyz_batch_cnt; a.new_xyz = new_xyz; a.new_cnt = new_xyz_batch_cnt; a.feats = features; a.idx_in = nullptr;
  a.B = B; a.N = N; a.M = M; a.C = group ? C : 0; a.nsample = nsample; a.c_xyz = (group && use_xyz) ? 3 : 0;
  a.cc = channels_per_pass(C, nsample);
  a.magic_ns = magic_of(nsample);
  a.radius2 = radius * radius;
  a.out = out; a.idx = idx; a.cnt = cnt; a.mask = empty_mask;
  return group ? launch_qag<MODE_QUERY_GROUP>(a, (hipStream_t)stream) : launch_qag<MODE_QUERY>(a, (hipStream_t)stream);
}

int gd3d_vsa_group(const float* features, const int32_t* features_batch_cnt, const int32_t* idx, const int32_t* idx_batch_cnt,
                   int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample, float* out, void* stream) {
  if (B < 0 || N < 0 || M < 0 || C <= 0 || nsample <= 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE || (long long)C * nsample > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (M == 0) return 0;
  if (idx == nullptr || out == nullptr || (B > 0 && (features_batch_cnt == nullptr || idx_batch_cnt == nullptr))) return GD3D_E_BADARG;
  if (N > 0 && features == nullptr) return GD3D_E_BADARG;
  QagArgs a;
  a.xyz = nullptr; a.xyz_cnt = features_batch_cnt; a.new_xyz = nullptr; a.new_cnt = idx_batch_cnt; a.feats = features; a.idx_in = idx;
  a.B = B; a.N = N; a.M = M; a.C = C; a.nsample = nsample; a.c_xyz = 0;
  a.cc = channels_per_pass(C, nsample);
  a.magic_ns = magic_of(nsample);
  a.radius2 = 0.0f;
  a.out = out; a.idx = nullptr; a.cnt = nullptr; a.mask = nullptr;
  return launch_qag<MODE_GROUP>(a, (hipStream_t)stream);
}

int gd3d_vsa_group_backward(const float* grad_out, const int32_t* idx, const int32_t* idx_batch_cnt, const int32_t* features_batch_cnt,
                            int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample, float* grad_features, void* stream) {
  return launch_backward(grad_out, idx, nullptr, idx_batch_cnt, features_batch_cnt, B, N, M, C, nsample, C, 0, grad_features, stream);
}

int gd3d_vsa_query_and_group_backward(const float* grad_out, const int32_t* idx, const int32_t* cnt, const int32_t* new_xyz_batch_cnt,
                                      const int32_t* xyz_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample,
                                      int32_t c_off, float* grad_features, void* stream) {
  if (cnt == nullptr && M > 0 && N > 0 && C > 0) return GD3D_E_BADARG;
  return launch_backward(grad_out, idx, cnt, new_xyz_batch_cnt, xyz_batch_cnt, B, N, M, C, nsample, c_off + C, c_off, grad_features, stream);
}

int gd3d_vsa_fps_register_points(void) { return FPS_CAP; }

size_t gd3d_vsa_fps_workspace_bytes(int64_t N) {
  const size_t n = N > 0 ? (size_t)N : 0;
  return ((n * sizeof(float) + 255) / 256 + 1) * 256;
}

int gd3d_vsa_fps(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* out, void* workspace, void* stream) {
  if (B < 0 || n < 0 || npoint < 0) return GD3D_E_BADARG;
  if (B == 0 || npoint == 0) return 0;
  if (out == nullptr || workspace == nullptr || (n > 0 && xyz == nullptr)) return GD3D_E_BADARG;
  hipLaunchKernelGGL((fps_kernel<int32_t>), dim3((unsigned)B), dim3(FPS_THREADS), 0, (hipStream_t)stream, xyz, (const int32_t*)nullptr,
                     (int)B, (long long)B * n, (int)n, (int)npoint, out, (float*)workspace);
  return (int)hipGetLastError();
}

int gd3d_vsa_fps_stacked(const float* xyz, const int32_t* xyz_batch_cnt, int32_t B, int64_t N, int32_t npoint, int64_t* out,
                         void* workspace, void* stream) {
  if (B < 0 || N < 0 || npoint < 0) return GD3D_E_BADARG;
  if (B == 0 || npoint == 0) return 0;
  if (out == nullptr || workspace == nullptr || xyz_batch_cnt == nullptr || (N > 0 && xyz == nullptr)) return GD3D_E_BADARG;
  hipLaunchKernelGGL((fps_kernel<int64_t>), dim3((unsigned)B), dim3(FPS_THREADS), 0, (hipStream_t)stream, xyz, xyz_batch_cnt, (int)B,
                     (long long)N, 0, (int)npoint, out, (float*)workspace);
  return (int)hipGetLastError();
}

}  // extern "C"
