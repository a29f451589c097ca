// eval_ap.hip — the accumulate stage of the flexible mAP evaluation on gfx950 (include/gd3d.h "Flexible mAP"):
//   eval_tp_records     one matcher result -> D records (group, score, tp_bits, msk_bits), one launch;
//   eval_ap_accumulate  n records -> num_det, recall, ap of every (group, threshold), without a read-back or a float atomic:
//     key kernel     64-bit key (group | score word of eval_ap_common.h) and the row index of every record;
//     sort           device_sort.h's stable radix sort over the key's live bits: the rank order of the header;
//     gather kernel  the sorted rows' group, msk and tp & msk words, streamed by everything below; per (tile, t) the counts of the
//                    tile's LAST segment (a segment = the rows of one group);
//     carry scan     one workgroup per t walks the tiles in chunks: segmented sum of those counts -> what each tile inherits;
//     max kernel     per (tile, t) the segmented counts of every row (wave scans, four wave totals through LDS), the precisions
//                    c / j, and the largest one in the tile's FIRST segment;
//     carry scan     the same walk backwards: segmented maximum -> the envelope each tile inherits from the tiles after it;
//     sum kernel     per (tile, t) counts and precisions again, the envelope e_j backwards, and the segmented sum of the e_j's
//                    2^-84 units as integer limbs: a segment that lies inside the tile is stored per group, the tile's first and last
//                    segment per tile; the row that ends a group stores its counts and its range;
//     finish kernel  one wave per (group, t) adds the limbs of the group's tiles (integers: any order), rounds once, divides.
// Compiled with -ffp-contract=off; fp64 division is correctly rounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_sort.h"
#include "eval_ap_common.h"
#include "gd3d_workspace.h"

namespace eval_ap {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int RPT = TILE_ROWS / BLOCK;   // consecutive rows of a thread: one 16-byte load per column
static_assert(RPT == 4, "the columns are read as uint4");
static_assert(SCAN_CHUNK == BLOCK, "the carry scans run the workgroup scan of the tile kernels");

// ---- records ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void records_kernel(const int32_t* __restrict__ matched, const uint8_t* __restrict__ det_flag,
                                                        const uint8_t* __restrict__ gt_flag, const float* __restrict__ score, int32_t g,
                                                        long long D, long long G, int T, int32_t* __restrict__ o_group,
                                                        float* __restrict__ o_score, uint32_t* __restrict__ o_tp, uint32_t* __restrict__ o_msk) {
  const long long d = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (d >= D) return;
  const bool df = det_flag[d] != 0;
  uint32_t tp = 0, msk = 0;
  for (int t = 0; t < T; ++t) {
    const int32_t m = matched != nullptr ? clamp_match(matched[(long long)t * D + d], G) : -1;
    const bool hit = m > -1;
    const bool in = hit ? gt_flag[m] != 0 : df;
    tp |= (uint32_t)hit << t;
    msk |= (uint32_t)in << t;
  }
  o_group[d] = g;
  o_score[d] = score[d];
  o_tp[d] = tp;
  o_msk[d] = msk;
}

// ---- keys and the gather --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void key_kernel(const int32_t* __restrict__ group, const float* __restrict__ score, long long n, int32_t K,
                                                    long long* __restrict__ key, int* __restrict__ val) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  key[i] = (long long)record_key(group[i], score[i], K);
  val[i] = (int)i;
}

// Sorted columns, padded to whole tiles with rows of group K that count for nothing, and tail[t][tile] = (msk rows, tp rows) of the
// tile's last segment.
__global__ __launch_bounds__(BLOCK) void gather_kernel(const long long* __restrict__ skey, const int* __restrict__ srow,
                                                       const uint32_t* __restrict__ tp_bits, const uint32_t* __restrict__ msk_bits, long long n,
                                                       int32_t K, int T, long long tiles, int32_t* __restrict__ sgrp, uint32_t* __restrict__ smsk,
                                                       uint32_t* __restrict__ stp, uint2* __restrict__ tail) {
  __shared__ uint32_t wcnt[WAVES][MAX_T][2];
  __shared__ int32_t last_group;
  const long long tile = blockIdx.x, base = tile * TILE_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t g[RPT];
  uint32_t m[RPT], c[RPT];
  for (int j = 0; j < RPT; ++j) {
    const long long i = base + j * BLOCK + tid;
    g[j] = K;
    m[j] = c[j] = 0;
    if (i < n) {
      const int r = srow[i];
      g[j] = (int32_t)((unsigned long long)skey[i] >> 32);
      m[j] = msk_bits[r];
      c[j] = tp_bits[r] & m[j];
    }
    sgrp[i] = g[j];
    smsk[i] = m[j];
    stp[i] = c[j];
  }
  if (tid == BLOCK - 1) last_group = g[RPT - 1];
  __syncthreads();
  const int32_t lg = last_group;
  for (int t = 0; t < T; ++t) {
    uint32_t cm = 0, cc = 0;
    for (int j = 0; j < RPT; ++j) {
      const bool in = g[j] == lg;
      cm += (uint32_t)__popcll(__ballot(in && ((m[j] >> t) & 1u)));
      cc += (uint32_t)__popcll(__ballot(in && ((c[j] >> t) & 1u)));
    }
    if (lane == 0) {
      wcnt[wave][t][0] = cm;
      wcnt[wave][t][1] = cc;
    }
  }
  __syncthreads();
  if (tid < T) {
    uint2 s = make_uint2(0u, 0u);
    for (int w = 0; w < WAVES; ++w) {
      s.x += wcnt[w][tid][0];
      s.y += wcnt[w][tid][1];
    }
    tail[(long long)tid * tiles + tile] = s;
  }
}

// ---- segmented scans over the threads of a workgroup ------------------------------------------------------------------------------
// An element is (flag, value): the flag says that a segment boundary lies inside the element, the value covers the element's part
// after its last boundary.  combine(earlier, later) = (either flag, later.flag ? later.value : earlier.value + later.value).  The
// forward scans run over ascending lanes and waves with `+` on counts or limbs; the backward one over descending lanes and waves
// with max on precisions.  Each returns the thread's EXCLUSIVE result, seeded with what the tile inherits.

struct Cnt {
  uint32_t m, c;
};
__device__ __forceinline__ Cnt join(const Cnt& a, const Cnt& b) { return {a.m + b.m, a.c + b.c}; }
__device__ __forceinline__ Cnt shift(const Cnt& v, int d, bool up) {
  return {up ? __shfl_up(v.m, d) : __shfl_down(v.m, d), up ? __shfl_up(v.c, d) : __shfl_down(v.c, d)};
}
struct Sum4 {
  uint32_t l[4];
};
__device__ __forceinline__ Sum4 join(const Sum4& a, const Sum4& b) { return {{a.l[0] + b.l[0], a.l[1] + b.l[1], a.l[2] + b.l[2], a.l[3] + b.l[3]}}; }
__device__ __forceinline__ Sum4 shift(const Sum4& v, int d, bool up) {
  Sum4 r;
  for (int k = 0; k < 4; ++k) r.l[k] = up ? __shfl_up(v.l[k], d) : __shfl_down(v.l[k], d);
  return r;
}
struct Max1 {
  double x;
};
__device__ __forceinline__ Max1 join(const Max1& a, const Max1& b) { return {a.x > b.x ? a.x : b.x}; }
__device__ __forceinline__ Max1 shift(const Max1& v, int d, bool up) { return {up ? __shfl_up(v.x, d) : __shfl_down(v.x, d)}; }

template <class V>
struct ScanLds {
  V v[WAVES];
  int f[WAVES];
};

// FWD: over ascending threads; otherwise over descending ones.  (f, v): the thread's element; seed: the inherited value (flag clear).
// On return (f, v) is the exclusive result.  Two barriers; `lds` may be reused by the next call.
template <bool FWD, class V>
__device__ __forceinline__ void block_seg_scan(bool& f, V& v, const V& seed, const V& zero, ScanLds<V>& lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = FWD ? lane : 63 - lane;     // the element's place in scan order inside its wave
  int fi = f ? 1 : 0;
  for (int d = 1; d < 64; d <<= 1) {
    const int pf = FWD ? __shfl_up(fi, d) : __shfl_down(fi, d);
    const V pv = shift(v, d, FWD);
    if (pos >= d) {
      if (!fi) v = join(pv, v);
      fi |= pf;
    }
  }
  __syncthreads();                            // the previous call's readers are done
  if (pos == 63) {
    lds.v[wave] = v;
    lds.f[wave] = fi;
  }
  // exclusive inside the wave
  int ef = FWD ? __shfl_up(fi, 1) : __shfl_down(fi, 1);
  V ev = shift(v, 1, FWD);
  if (pos == 0) {
    ef = 0;
    ev = zero;
  }
  __syncthreads();
  // what precedes the wave: the seed, then the waves before it in scan order
  int pf = 0;
  V pv = seed;
  for (int k = 0; k < WAVES; ++k) {
    const int w = FWD ? k : WAVES - 1 - k;
    const bool before = FWD ? w < wave : w > wave;
    if (before) {
      pv = lds.f[w] ? lds.v[w] : join(pv, lds.v[w]);
      pf |= lds.f[w];
    }
  }
  v = ef ? ev : join(pv, ev);
  f = (ef | pf) != 0;
}

// What a thread knows of its four rows.  hd: a group starts at row j (not counting the tile's first row); en: a group ends at
// row j (not counting the tile's last row); head0 / end_last: the same for those two rows, which decide what the tile inherits.
struct Rows {
  int32_t g[RPT];
  uint32_t m[RPT], c[RPT];
  bool hd[RPT], en[RPT];
  bool head0, end_last;
  long long first;   // sorted position of row 0 of the thread
};

__device__ __forceinline__ void load_rows(const int32_t* __restrict__ sgrp, const uint32_t* __restrict__ smsk, const uint32_t* __restrict__ stp,
                                          long long tile, long long tiles, Rows& r) {
  const int tid = threadIdx.x;
  const long long base = tile * TILE_ROWS;
  r.first = base + (long long)tid * RPT;
  const int4 g4 = *reinterpret_cast<const int4*>(sgrp + r.first);
  const uint4 m4 = *reinterpret_cast<const uint4*>(smsk + r.first);
  const uint4 c4 = *reinterpret_cast<const uint4*>(stp + r.first);
  r.g[0] = g4.x; r.g[1] = g4.y; r.g[2] = g4.z; r.g[3] = g4.w;
  r.m[0] = m4.x; r.m[1] = m4.y; r.m[2] = m4.z; r.m[3] = m4.w;
  r.c[0] = c4.x; r.c[1] = c4.y; r.c[2] = c4.z; r.c[3] = c4.w;
  const int32_t prev = tid > 0 ? sgrp[r.first - 1] : r.g[0];
  const int32_t next = tid < BLOCK - 1 ? sgrp[r.first + RPT] : r.g[RPT - 1];
  for (int j = 0; j < RPT; ++j) {
    r.hd[j] = r.g[j] != (j > 0 ? r.g[j - 1] : prev);
    r.en[j] = r.g[j] != (j < RPT - 1 ? r.g[j + 1] : next);
  }
  r.head0 = tile == 0 || sgrp[base - 1] != sgrp[base];
  r.end_last = tile == tiles - 1 || sgrp[base + TILE_ROWS] != sgrp[base + TILE_ROWS - 1];
}

// Forward pass of one threshold: M[j], C[j] = the segmented inclusive counts of msk and tp rows at row j; seen[j] = a group started
// in the tile after its first row, at or before row j (the row is not in the tile's first segment).
__device__ __forceinline__ void forward_counts(const Rows& r, int t, const Cnt& inherit, ScanLds<Cnt>& lds, uint32_t (&M)[RPT], uint32_t (&C)[RPT],
                                               bool (&seen)[RPT]) {
  Cnt v = {0u, 0u};
  bool f = false;
  for (int j = 0; j < RPT; ++j) {
    if (r.hd[j]) {
      v = {0u, 0u};
      f = true;
    }
    v.m += (r.m[j] >> t) & 1u;
    v.c += (r.c[j] >> t) & 1u;
  }
  const Cnt seed = r.head0 ? Cnt{0u, 0u} : inherit;
  block_seg_scan<true>(f, v, seed, Cnt{0u, 0u}, lds);
  for (int j = 0; j < RPT; ++j) {
    if (r.hd[j]) {
      v = {0u, 0u};
      f = true;
    }
    v.m += (r.m[j] >> t) & 1u;
    v.c += (r.c[j] >> t) & 1u;
    M[j] = v.m;
    C[j] = v.c;
    seen[j] = f;
  }
}

// head_max[t][tile] = the largest precision among the msk rows of the tile's first segment (0 without one)
__global__ __launch_bounds__(BLOCK) void max_kernel(const int32_t* __restrict__ sgrp, const uint32_t* __restrict__ smsk,
                                                    const uint32_t* __restrict__ stp, const uint2* __restrict__ carry, int T, long long tiles,
                                                    double* __restrict__ head_max) {
  __shared__ ScanLds<Cnt> lds;
  __shared__ double wmax[2][WAVES];
  const long long tile = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Rows r;
  load_rows(sgrp, smsk, stp, tile, tiles, r);
  for (int t = 0; t < T; ++t) {
    const uint2 cin = carry[(long long)t * tiles + tile];
    uint32_t M[RPT], C[RPT];
    bool seen[RPT];
    forward_counts(r, t, Cnt{cin.x, cin.y}, lds, M, C, seen);
    double best = 0.0;
    for (int j = 0; j < RPT; ++j)
      if (((r.m[j] >> t) & 1u) && !seen[j]) {
        const double p = (double)C[j] / (double)M[j];
        best = p > best ? p : best;
      }
    for (int d = 32; d > 0; d >>= 1) {
      const double o = __shfl_down(best, d);
      best = o > best ? o : best;
    }
    if (lane == 0) wmax[t & 1][wave] = best;   // two slots: the next threshold's writers do not wait for this one's reader
    __syncthreads();
    if (tid == 0) {
      double b = wmax[t & 1][0];
      for (int w = 1; w < WAVES; ++w) b = wmax[t & 1][w] > b ? wmax[t & 1][w] : b;
      head_max[(long long)t * tiles + tile] = b;
    }
  }
}

// Per (tile, t): the envelope, and the integer limbs of its sum per segment.  A segment inside the tile is complete: stored per
// group (inner).  The first segment's limbs go to edge[t][tile][0], the last one's (when it is another one) to edge[t][tile][1].
// The row that ends a group stores the group's counts; the rows that start and end it store its range.
__global__ __launch_bounds__(BLOCK) void sum_kernel(const int32_t* __restrict__ sgrp, const uint32_t* __restrict__ smsk,
                                                    const uint32_t* __restrict__ stp, const uint2* __restrict__ carry,
                                                    const double* __restrict__ carry_max, int32_t K, int T, long long tiles,
                                                    uint4* __restrict__ edge, uint4* __restrict__ inner, uint2* __restrict__ total,
                                                    uint2* __restrict__ range) {
  __shared__ ScanLds<Cnt> lds_c;
  __shared__ ScanLds<Max1> lds_x;
  __shared__ ScanLds<Sum4> lds_s;
  const long long tile = blockIdx.x;
  const int tid = threadIdx.x;
  Rows r;
  load_rows(sgrp, smsk, stp, tile, tiles, r);
  const bool last_thread = tid == BLOCK - 1;
  for (int j = 0; j < RPT; ++j) {
    const bool starts = r.hd[j] || (tid == 0 && j == 0 && r.head0);
    const bool ends = r.en[j] || (last_thread && j == RPT - 1 && r.end_last);
    if (r.g[j] < K) {
      if (starts) range[r.g[j]].x = (uint32_t)(r.first + j);
      if (ends) range[r.g[j]].y = (uint32_t)(r.first + j + 1);
    }
  }
  for (int t = 0; t < T; ++t) {
    const uint2 cin = carry[(long long)t * tiles + tile];
    uint32_t M[RPT], C[RPT];
    bool seen[RPT];
    forward_counts(r, t, Cnt{cin.x, cin.y}, lds_c, M, C, seen);
    double p[RPT];
    for (int j = 0; j < RPT; ++j) p[j] = ((r.m[j] >> t) & 1u) ? (double)C[j] / (double)M[j] : 0.0;
    // backwards: the envelope
    Max1 x = {0.0};
    bool f = false;
    for (int j = RPT - 1; j >= 0; --j) {
      if (r.en[j]) {
        x.x = 0.0;
        f = true;
      }
      x.x = p[j] > x.x ? p[j] : x.x;
    }
    const Max1 seed = {r.end_last ? 0.0 : carry_max[(long long)t * tiles + tile]};
    block_seg_scan<false>(f, x, seed, Max1{0.0}, lds_x);
    double e[RPT];
    bool to_end[RPT];      // the row's segment reaches the tile's last row
    for (int j = RPT - 1; j >= 0; --j) {
      if (r.en[j]) {
        x.x = 0.0;
        f = true;
      }
      x.x = p[j] > x.x ? p[j] : x.x;
      e[j] = x.x;
      to_end[j] = !f;
    }
    // forwards: the limbs of e over the tp rows
    Sum4 s = {{0u, 0u, 0u, 0u}};
    f = false;
    for (int j = 0; j < RPT; ++j) {
      if (r.hd[j]) {
        s = {{0u, 0u, 0u, 0u}};
        f = true;
      }
      if ((r.c[j] >> t) & 1u) {
        const Limbs q = limbs_of(e[j]);
        for (int k = 0; k < 4; ++k) s.l[k] += q.l[k];
      }
    }
    const Sum4 zero = {{0u, 0u, 0u, 0u}};
    block_seg_scan<true>(f, s, zero, zero, lds_s);
    for (int j = 0; j < RPT; ++j) {
      if (r.hd[j]) {
        s = zero;
        f = true;
      }
      if ((r.c[j] >> t) & 1u) {
        const Limbs q = limbs_of(e[j]);
        for (int k = 0; k < 4; ++k) s.l[k] += q.l[k];
      }
      const bool tile_end = last_thread && j == RPT - 1;
      if (r.en[j] || tile_end) {
        const uint4 out = make_uint4(s.l[0], s.l[1], s.l[2], s.l[3]);
        uint4* const ed = edge + ((long long)t * tiles + tile) * 2;
        if (!f) {
          ed[0] = out;
          if (tile_end) ed[1] = make_uint4(0u, 0u, 0u, 0u);
        } else if (to_end[j]) {
          ed[1] = out;
        } else if (r.g[j] < K) {
          inner[(long long)r.g[j] * T + t] = out;
        }
        if ((r.en[j] || r.end_last) && r.g[j] < K) total[(long long)r.g[j] * T + t] = make_uint2(M[j], C[j]);
      }
    }
  }
}

// ---- the tile-carry scans: one workgroup per threshold walks the tiles SCAN_CHUNK at a time ----------------------------------------

// carry[t][k] = (msk rows, tp rows) of the group of tile k's first row in the tiles before k (what applies when that row starts no group)
__global__ __launch_bounds__(SCAN_CHUNK) void carry_sum_kernel(const int32_t* __restrict__ sgrp, const uint2* __restrict__ tail, long long tiles,
                                                                uint2* __restrict__ carry) {
  __shared__ ScanLds<Cnt> lds;
  __shared__ Cnt running;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) running = {0u, 0u};
  __syncthreads();
  for (long long k0 = 0; k0 < tiles; k0 += SCAN_CHUNK) {
    const long long k = k0 + tid;
    Cnt v = {0u, 0u};
    bool f = false;
    if (k < tiles) {
      const uint2 x = tail[(long long)t * tiles + k];
      v = {x.x, x.y};
      // the tile's last segment starts inside the tile
      f = k == 0 || sgrp[k * TILE_ROWS - 1] != sgrp[k * TILE_ROWS + TILE_ROWS - 1];
    }
    const Cnt own = v;
    const bool own_f = f;
    const Cnt seed = running;
    block_seg_scan<true>(f, v, seed, Cnt{0u, 0u}, lds);
    if (k < tiles) carry[(long long)t * tiles + k] = make_uint2(v.m, v.c);
    __syncthreads();                        // everyone has read `running`
    if (tid == SCAN_CHUNK - 1) running = own_f ? own : join(v, own);
    __syncthreads();
  }
}

// carry_max[t][k] = the largest precision of the group of tile k's last row in the tiles after k
__global__ __launch_bounds__(SCAN_CHUNK) void carry_max_kernel(const int32_t* __restrict__ sgrp, const double* __restrict__ head_max,
                                                                long long tiles, double* __restrict__ carry_max) {
  __shared__ ScanLds<Max1> lds;
  __shared__ double running;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) running = 0.0;
  __syncthreads();
  const long long chunks = (tiles + SCAN_CHUNK - 1) / SCAN_CHUNK;
  for (long long c = chunks - 1; c >= 0; --c) {
    const long long k = c * SCAN_CHUNK + tid;
    Max1 v = {0.0};
    bool f = false;
    if (k < tiles) {
      v.x = head_max[(long long)t * tiles + k];
      // the tile's first segment ends inside the tile
      f = k == tiles - 1 || sgrp[k * TILE_ROWS] != sgrp[(k + 1) * TILE_ROWS];
    }
    const Max1 own = v;
    const bool own_f = f;
    const Max1 seed = {running};
    block_seg_scan<false>(f, v, seed, Max1{0.0}, lds);
    if (k < tiles) carry_max[(long long)t * tiles + k] = v.x;
    __syncthreads();
    if (tid == 0) running = own_f ? own.x : join(v, own).x;
    __syncthreads();
  }
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// one wave per (group, t)
__global__ __launch_bounds__(BLOCK) void finish_kernel(const uint4* __restrict__ edge, const uint4* __restrict__ inner, const uint2* __restrict__ total,
                                                       const uint2* __restrict__ range, const int64_t* __restrict__ num_gt, long long K, int T,
                                                       long long tiles, int64_t* __restrict__ num_det, double* __restrict__ recall,
                                                       double* __restrict__ ap) {
  const long long item = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (item >= K * T) return;
  const long long g = item / T;
  const int t = (int)(item - g * T);
  const uint2 rg = tiles > 0 ? range[g] : make_uint2(0u, 0u);
  unsigned long long l[4] = {0, 0, 0, 0};
  uint2 tot = make_uint2(0u, 0u);
  if (rg.y > rg.x) {
    tot = total[item];
    const long long s = rg.x, e = rg.y, ks = s / TILE_ROWS, ke = (e - 1) / TILE_ROWS;
    if (s > ks * TILE_ROWS && e < (ks + 1) * TILE_ROWS) {
      if (lane == 0) {
        const uint4 q = inner[item];
        l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
      }
    } else {
      for (long long k = ks + lane; k <= ke; k += 64) {
        const uint4 q = edge[((long long)t * tiles + k) * 2 + (k * TILE_ROWS >= s ? 0 : 1)];
        l[0] += q.x; l[1] += q.y; l[2] += q.z; l[3] += q.w;
      }
    }
  }
  for (int k = 0; k < 4; ++k) l[k] = wave_sum_u64(l[k]);
  if (lane == 0) {
    const double esum = limbs_to_double(l[0], l[1], l[2], l[3]);
    finish(tot.x, tot.y, esum, num_gt[g], num_det + item, recall + item, ap + item);
  }
}

// ---- the workspace: one carve gives the pointers and, at address 0, the size -------------------------------------------------------

struct Work {
  long long *key_in, *key_out;
  int *val_in, *val_out;
  char* sort_tmp;
  int32_t* sgrp;
  uint32_t *smsk, *stp;
  uint2 *tail, *carry;
  double *head_max, *carry_max;
  uint4 *edge, *inner;
  uint2 *total, *range;   // cleared before every run: an empty group stores nothing
  size_t sort_bytes = 0, bytes = 0, clear_bytes = 0;
  long long tiles = 0;
  hipError_t err;
  Work(void* workspace, int64_t n, int64_t K, int32_t T) {
    tiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    err = gd3d::sort_pairs_temp_bytes((size_t)(n > 0 ? n : 1), sort_bytes);
    if (err != hipSuccess) return;
    gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
    const size_t pad = (size_t)tiles * TILE_ROWS, tt = (size_t)tiles * T, kt = (size_t)K * T;
    key_in = c.take<long long>((size_t)n);
    key_out = c.take<long long>((size_t)n);
    val_in = c.take<int>((size_t)n);
    val_out = c.take<int>((size_t)n);
    sort_tmp = c.take<char>(sort_bytes);
    sgrp = c.take<int32_t>(pad);
    smsk = c.take<uint32_t>(pad);
    stp = c.take<uint32_t>(pad);
    tail = c.take<uint2>(tt);
    carry = c.take<uint2>(tt);
    head_max = c.take<double>(tt);
    carry_max = c.take<double>(tt);
    edge = c.take<uint4>(tt * 2);
    inner = c.take<uint4>(kt);
    total = c.take<uint2>(kt);
    range = c.take<uint2>((size_t)K);
    clear_bytes = (size_t)((char*)c.take<char>(0) - (char*)total);
    bytes = c.bytes();
  }
};

}  // namespace eval_ap

using namespace eval_ap;

extern "C" {

int32_t eval_ap_tile_rows(void) { return TILE_ROWS; }
int32_t eval_ap_scan_chunk_tiles(void) { return SCAN_CHUNK; }

size_t eval_ap_workspace_bytes(int64_t n, int64_t K, int32_t T) {
  if (n < 0 || n > MAX_N || K < 1 || K > MAX_K || T < 1 || T > MAX_T) return 0;
  const Work w(nullptr, n, K, T);
  return w.err == hipSuccess ? (w.bytes > 256 ? w.bytes : 256) : 0;
}

int eval_tp_records(const int32_t* matched, const uint8_t* det_flag, const uint8_t* gt_flag, const float* score, int32_t group, int64_t D,
                    int64_t G, int32_t T, int32_t* out_group, float* out_score, uint32_t* out_tp_bits, uint32_t* out_msk_bits, void* stream) {
  const int rc = check_records(det_flag, gt_flag, score, D, G, T, out_group, out_score, out_tp_bits, out_msk_bits);
  if (rc != 0 || D == 0) return rc;
  hipLaunchKernelGGL(records_kernel, dim3((unsigned)((D + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, matched, det_flag, gt_flag,
                     score, group, (long long)D, (long long)G, (int)T, out_group, out_score, out_tp_bits, out_msk_bits);
  return (int)hipGetLastError();
}

int eval_ap_accumulate(const int32_t* group, const float* score, const uint32_t* tp_bits, const uint32_t* msk_bits, const int64_t* num_gt,
                       int64_t n, int64_t K, int32_t T, int64_t* num_det, double* recall, double* ap, void* workspace, void* stream) {
  const int rc = check_accumulate(group, score, tp_bits, msk_bits, num_gt, n, K, T, num_det, recall, ap);
  if (rc != 0) return rc;
  if (workspace == nullptr || ((uintptr_t)workspace & 255) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const Work w(workspace, n, K, T);
  if (w.err != hipSuccess) return (int)w.err;
  const unsigned tiles = (unsigned)w.tiles;
  if (n > 0) {
    hipError_t he = hipMemsetAsync(w.total, 0, w.clear_bytes, s);
    if (he != hipSuccess) return (int)he;
    hipLaunchKernelGGL(key_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, group, score, (long long)n, (int32_t)K, w.key_in,
                       w.val_in);
    he = gd3d::sort_pairs(w.sort_tmp, w.sort_bytes, w.key_in, w.key_out, w.val_in, w.val_out, (size_t)n, (unsigned)(32 + gd3d::key_bits(K)), s);
    if (he != hipSuccess) return (int)he;
    hipLaunchKernelGGL(gather_kernel, dim3(tiles), dim3(BLOCK), 0, s, w.key_out, w.val_out, tp_bits, msk_bits, (long long)n, (int32_t)K, (int)T,
                       w.tiles, w.sgrp, w.smsk, w.stp, w.tail);
    hipLaunchKernelGGL(carry_sum_kernel, dim3((unsigned)T), dim3(SCAN_CHUNK), 0, s, w.sgrp, w.tail, w.tiles, w.carry);
    hipLaunchKernelGGL(max_kernel, dim3(tiles), dim3(BLOCK), 0, s, w.sgrp, w.smsk, w.stp, w.carry, (int)T, w.tiles, w.head_max);
    hipLaunchKernelGGL(carry_max_kernel, dim3((unsigned)T), dim3(SCAN_CHUNK), 0, s, w.sgrp, w.head_max, w.tiles, w.carry_max);
    hipLaunchKernelGGL(sum_kernel, dim3(tiles), dim3(BLOCK), 0, s, w.sgrp, w.smsk, w.stp, w.carry, w.carry_max, (int32_t)K, (int)T, w.tiles, w.edge,
                       w.inner, w.total, w.range);
  }
  const long long items = (long long)K * T;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(BLOCK), 0, s, w.edge, w.inner, w.total, w.range, num_gt,
                     (long long)K, (int)T, w.tiles, num_det, recall, ap);
  return (int)hipGetLastError();
}

}  // extern "C"
