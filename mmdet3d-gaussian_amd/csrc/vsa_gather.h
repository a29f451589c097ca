// vsa_gather.h — the gather stage of the query-and-group kernels, ONE definition for csrc/vsa.hip (ball query over a sample's
// points) and csrc/voxel_query.hip (voxel query over a cell window): once a wave holds its query's member rows in LDS it writes
// idx / cnt / the mask, the grouped xyz minus the centre, the feature rows transposed through the wave's LDS buffer, the padded tail
// and the zeros of an empty query.  Device only; every function is per wave, no block-wide barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vsa {

constexpr int XP = 1024 + 64;            // floats of a wave's transpose buffer (>= MAX_NSAMPLE | 1)

// LDS written by some lanes of a wave and read by others of the SAME wave: the accesses of one wave reach the LDS in program
// order; this keeps the compiler from moving them across the point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// e / nsample for the small e of a query's block (the magic of 1 does not fit 32 bits)
__device__ __forceinline__ int div_nsample(int e, int nsample, unsigned magic) {
  return nsample == 1 ? e : (int)__umulhi((unsigned)e, magic);
}

// rows[s] (s < found) x cw channels from `src` (row stride C) into xp[ch * pad + s]: lanes run along a row (contiguous
// floats), 64 / cw rows per wave instruction when a row is shorter than the wave, four rows in flight per lane.
__device__ __forceinline__ void gather_rows(const float* __restrict__ src, long long p0, int C, const int* lidx, int found,
                                            int cw, int pad, float* xp, int lane) {
  const int r = cw >= 64 ? 1 : 64 / cw;
  const int sub = cw >= 64 ? 0 : lane / cw;
  const int ch0 = lane - sub * cw;
  if (sub >= r) return;
  for (int ch = ch0; ch < cw; ch += 64) {
    for (int s = sub; s < found; s += 4 * r) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int su = s + u * r;
        v[u] = su < found ? src[(p0 + lidx[su]) * C + ch] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int su = s + u * r;
        if (su < found) xp[ch * pad + su] = v[u];
      }
    }
  }
}

// What a wave writes for query row m once lidx[0 .. found) holds its members (rows of xyz / feats counted from p0), the wave's LDS
// writes of them still pending.  `a` is the kernel's argument block: xyz, feats, C, nsample, c_xyz, cc, magic_ns, out, idx, cnt, mask.
// WRITE_IDX: idx / cnt / mask are outputs of this launch; GROUP: the (c_xyz + C, nsample) block is.
template <bool WRITE_IDX, bool GROUP, class Args>
__device__ __forceinline__ void write_query(const Args& a, long long m, long long p0, const int* lidx, float* xp, int found, float cx,
                                            float cy, float cz, int lane) {
  const int nsample = a.nsample;
  wave_sync();
  if (WRITE_IDX) {
    const int first = found > 0 ? lidx[0] : 0;
    for (int s = lane; s < nsample; s += 64) a.idx[m * nsample + s] = s < found ? lidx[s] : first;
    if (lane == 0) {
      if (a.cnt != nullptr) a.cnt[m] = found;
      if (a.mask != nullptr) a.mask[m] = found == 0 ? 1 : 0;
    }
  }
  if (!GROUP) return;
  const int ct = a.c_xyz + a.C;
  float* const o = a.out + m * ct * nsample;
  if (found == 0) {   // empty ball: every channel zero
    for (int e = lane; e < ct * nsample; e += 64) o[e] = 0.0f;
    return;
  }
  if (a.c_xyz) {   // grouped xyz minus the centre: 3 * nsample outputs, written as one run
    for (int e = lane; e < 3 * nsample; e += 64) {
      const int k = div_nsample(e, nsample, a.magic_ns);
      const int s = e - k * nsample;
      const int p = lidx[s < found ? s : 0];
      const float v = a.xyz[(p0 + p) * 3 + k];
      o[e] = v - (k == 0 ? cx : (k == 1 ? cy : cz));
    }
  }
  const int pad = nsample | 1;   // odd row stride: lanes along a channel column hit different banks
  for (int c0 = 0; c0 < a.C; c0 += a.cc) {
    const int cw = (a.C - c0) < a.cc ? (a.C - c0) : a.cc;
    gather_rows(a.feats + c0, p0, a.C, lidx, found, cw, pad, xp, lane);
    wave_sync();
    float* const oc = o + (a.c_xyz + c0) * nsample;
    for (int e = lane; e < cw * nsample; e += 64) {
      const int ch = div_nsample(e, nsample, a.magic_ns);
      const int s = e - ch * nsample;
      oc[e] = xp[ch * pad + (s < found ? s : 0)];   // the padded tail repeats the first member
    }
    wave_sync();
  }
}

inline unsigned magic_of(int d) { return (unsigned)(0x100000000ULL / (unsigned)d) + 1u; }

inline int channels_per_pass(int C, int nsample) {
  int cc = XP / (nsample | 1);
  cc = cc < 1 ? 1 : cc;
  return cc > C ? (C > 0 ? C : 1) : cc;
}

}  // namespace vsa
