// vsa_common.h — what csrc/vsa.hip (gfx950 kernels) and csrc/vsa_cpu.cpp (their `_cpu` twins) share: the squared distance as ONE
// fixed sequence of fp32 operations and the resolution of a stacked batch into clamped segments.  Both units are compiled with
// -ffp-contract=off, so every `d2 < radius2` and every arg-max decision is the same bit on the device and on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VSA_HD __host__ __device__ __forceinline__
#else
#define VSA_HD inline
#endif

namespace vsa {

constexpr int MAX_NSAMPLE = 1024;          // idx rows are staged per wave in LDS
constexpr int FPS_THREADS = 1024;          // one workgroup per sample
constexpr int FPS_PPT = 16;                // points a thread keeps in registers
constexpr int FPS_CAP = FPS_THREADS * FPS_PPT;
constexpr float FPS_FAR = 1e10f;           // initial running minimum (ops/vsa/sample_points.py:23)

// (ax-x)*(ax-x) + (ay-y)*(ay-y) + (az-z)*(az-z), left to right: ((xx + yy) + zz), five roundings, no fma
VSA_HD float dist2(float ax, float ay, float az, float x, float y, float z) {
  const float dx = ax - x, dy = ay - y, dz = az - z;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

VSA_HD long long clamp_count(int c, long long room) {
  const long long v = c < 0 ? 0 : (long long)c;
  return v < room ? v : room;
}

// Work item j of a launch that gives every sample ceil(queries / PER) consecutive items -> the item's first query row q0,
// its nq <= PER queries and its sample's points [p0, p0 + np).  Rows of the query array beyond the counts' sum form one more
// segment without points.  False: j is past the last item.
template <int PER>
VSA_HD bool item_segment(const int32_t* pcnt, const int32_t* qcnt, int B, long long N, long long M, long long j,
                         long long& q0, int& nq, long long& p0, int& np) {
  long long qs = 0, ps = 0;
  for (int b = 0; b <= B; ++b) {
    const long long mq = b < B ? clamp_count(qcnt[b], M - qs) : M - qs;
    const long long pn = b < B ? clamp_count(pcnt[b], N - ps) : 0;
    const long long items = (mq + PER - 1) / PER;
    if (j < items) {
      q0 = qs + j * PER;
      const long long left = mq - j * PER;
      nq = (int)(left < PER ? left : PER);
      p0 = ps;
      np = (int)pn;
      return true;
    }
    j -= items;
    qs += mq;
    ps += pn;
  }
  return false;
}

// The sample of query row m: its points [p0, p0 + np).  False: no count covers the row.
VSA_HD bool row_segment(const int32_t* pcnt, const int32_t* qcnt, int B, long long N, long long M, long long m, long long& p0,
                        int& np) {
  long long qs = 0, ps = 0;
  for (int b = 0; b < B; ++b) {
    const long long mq = clamp_count(qcnt[b], M - qs);
    const long long pn = clamp_count(pcnt[b], N - ps);
    if (m < qs + mq) {
      p0 = ps;
      np = (int)pn;
      return true;
    }
    qs += mq;
    ps += pn;
  }
  return false;
}

VSA_HD int clamp_index(int v, int np) { return v < 0 ? 0 : (v >= np ? np - 1 : v); }

}  // namespace vsa
