// eval_ap_common.h — what csrc/eval_ap.hip (gfx950 kernels) and csrc/eval_ap_cpu.cpp (their `_cpu` twins) share: the sort key of a
// record (rank order of include/gd3d.h: group, descending score, NaN first, -0 == +0), the bit tests of eval_tp_records, the
// argument checks, and the summation of the precision envelope.  That sum is EXACT: every e_j is a fp64 in [2^-31, 1], hence a
// whole number of 2^-84; the units are added as integers (four 21-bit limbs, so that any order gives the same words) and the total
// is rounded to fp64 once, to nearest even.  Both units are compiled with -ffp-contract=off and correctly rounded fp64 division.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/gd3d.h"

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define EA_HD __host__ __device__ __forceinline__
#else
#define EA_HD inline
#endif

namespace eval_ap {

constexpr int TILE_ROWS = 1024;     // sorted rows per workgroup of the scan kernels (256 threads x 4 rows): eval_ap_tile_rows()
constexpr int SCAN_CHUNK = 256;     // tiles per iteration of the tile-carry scans (one workgroup loops): eval_ap_scan_chunk_tiles()
constexpr int MAX_T = 32;           // thresholds: one bit each of tp_bits / msk_bits
constexpr int64_t MAX_K = 1LL << 20;
constexpr int64_t MAX_N = 0x7fffffffLL;
constexpr int LIMB_BITS = 21;       // 4 limbs x 21 bits = the 84 fraction bits; 1024 rows of a tile sum below 2^32 in every limb
constexpr uint32_t LIMB_MASK = (1u << LIMB_BITS) - 1;

EA_HD uint32_t float_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// low key word: ascending order of this word is the rank order of the scores.  NaN -> 0 (first); otherwise the complement of the
// order-preserving map of the score with -0 folded to +0 (so +inf -> 0x007fffff, the smallest word of a number).
EA_HD uint32_t score_key(float v) {
  uint32_t u = float_bits(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  const uint32_t ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~ordered;
}

// the 64-bit sort key: [32 + bits(K)) group (rows of a group outside [0, K) take K and sort last) | [32) score word
EA_HD uint64_t record_key(int32_t group, float score, int32_t K) {
  const uint32_t g = (group >= 0 && group < K) ? (uint32_t)group : (uint32_t)K;
  return ((uint64_t)g << 32) | (uint64_t)score_key(score);
}

// eval_tp_records, one detection and one threshold: m = matched[t, d] (out of [-1, G): -1)
EA_HD int32_t clamp_match(int32_t m, int64_t G) { return (m >= 0 && (int64_t)m < G) ? m : -1; }

struct Limbs {
  uint32_t l[4];
};

// e in [2^-31, 1] (a quotient c / j of integers 1 <= c <= j < 2^31, rounded) or 0 -> its 2^-84 units as four 21-bit limbs
// (the top limb reaches 2^21 for e = 1)
EA_HD Limbs limbs_of(double e) {
  Limbs r = {{0u, 0u, 0u, 0u}};
  uint64_t b;
  memcpy(&b, &e, 8);
  const int ex = (int)((b >> 52) & 0x7ff);
  if (ex == 0) return r;                                        // e == 0 (no denormal can occur)
  const uint64_t mant = (b & ((1ull << 52) - 1)) | (1ull << 52);
  const int sh = ex - 991;                                      // 1 .. 32: units = mant << sh < 2^85
  const uint64_t lo = mant << sh, hi = mant >> (64 - sh);
  r.l[0] = (uint32_t)lo & LIMB_MASK;
  r.l[1] = (uint32_t)(lo >> 21) & LIMB_MASK;
  r.l[2] = (uint32_t)(lo >> 42) & LIMB_MASK;
  r.l[3] = (uint32_t)((lo >> 63) | (hi << 1));
  return r;
}

// limb sums (each below 2^53) -> the exact total of 2^-84 units, rounded once to fp64 (nearest even)
EA_HD double limbs_to_double(uint64_t l0, uint64_t l1, uint64_t l2, uint64_t l3) {
  // 128-bit total = l0 + l1 * 2^21 + l2 * 2^42 + l3 * 2^63 in (hi, lo)
  uint64_t lo = l0, hi = 0, t;
  t = l1 << 21; lo += t; hi += (lo < t) + (l1 >> 43);
  t = l2 << 42; lo += t; hi += (lo < t) + (l2 >> 22);
  t = l3 << 63; lo += t; hi += (lo < t) + (l3 >> 1);
  if (hi == 0) return (double)lo * 0x1p-84;                     // u64 -> fp64 rounds to nearest even; the scaling is exact
  int nb = 0;                                                   // bits of hi
  for (uint64_t h = hi; h != 0; h >>= 1) ++nb;                  // 1 .. 64 (the total stays below 2^116)
  // the top 64 bits, with everything shifted out jammed into the last one (64 > 53 + 2: the rounding sees the same thing)
  const uint64_t q = (nb == 64 ? hi : ((hi << (64 - nb)) | (lo >> nb))) | ((nb == 64 ? lo : (lo << (64 - nb))) != 0 ? 1ull : 0ull);
  double s = (double)q;
  for (int i = 0; i < nb; ++i) s *= 2.0;                        // exact
  return s * 0x1p-84;
}

// num_det, recall and ap of one (group, threshold) from its counts and its exact envelope sum
EA_HD void finish(uint32_t D, uint32_t C, double esum, int64_t num_gt, int64_t* num_det, double* recall, double* ap) {
  const double den = num_gt > 0 ? (double)num_gt : 1e-7;
  *num_det = (int64_t)D;
  *recall = D ? (double)C / den : 0.0;
  *ap = esum / den;
}

inline int check_accumulate(const void* group, const void* score, const void* tp, const void* msk, const void* num_gt, int64_t n, int64_t K,
                            int32_t T, const void* num_det, const void* recall, const void* ap) {
  if (n < 0 || K < 1 || T < 1 || T > MAX_T || num_gt == nullptr || num_det == nullptr || recall == nullptr || ap == nullptr)
    return GD3D_E_BADARG;
  if (n > MAX_N || K > MAX_K) return GD3D_E_TOOLARGE;
  if (n > 0 && (group == nullptr || score == nullptr || tp == nullptr || msk == nullptr)) return GD3D_E_BADARG;
  return 0;
}

inline int check_records(const void* det_flag, const void* gt_flag, const void* score, int64_t D, int64_t G, int32_t T, const void* o_group,
                         const void* o_score, const void* o_tp, const void* o_msk) {
  if (D < 0 || G < 0 || T < 1 || T > MAX_T) return GD3D_E_BADARG;
  if (D > MAX_N || G > MAX_N) return GD3D_E_TOOLARGE;
  if (D > 0 && (det_flag == nullptr || score == nullptr || o_group == nullptr || o_score == nullptr || o_tp == nullptr || o_msk == nullptr))
    return GD3D_E_BADARG;
  if (G > 0 && gt_flag == nullptr) return GD3D_E_BADARG;
  return 0;
}

}  // namespace eval_ap
