// roi_sample_common.h — what csrc/roi_sample.hip (gfx950 kernels) and csrc/roi_sample_cpu.cpp (their `_cpu` twins) share: the 3D
// IoU of the iou3d family (BEV overlap of csrc/rbox_device.h times the height overlap) as ONE sequence of fp32 operations, and
// every decision of PVRCNNROIHead._assign_and_sample (models/roi_heads/pvrcnn_roi_head.py:225-297) that is not a loop over rows:
// the MaxIoUAssigner's first three rules, the stratum of a proposal, the order key of a draw, the plan of the piecewise negative
// sampler and the member a fill slot takes.  Both units are compiled with -ffp-contract=off, and sin / cos / atan2 are the
// project's fixed polynomial sequences (fx_sincosf, fx_atan2f), so the IoU — hence every decision below — is the same bits on
// the device and on the host.
#pragma once
#include "rbox_device.h"

#include <stdint.h>

namespace roi_sample {

using rbox::OBox;
using rbox::VertexScratch;

constexpr int WG = 1024;            // threads of a sample's workgroup (csrc/lds_sort.h is written for 1024)
constexpr int NT = 256;             // of which this many evaluate box pairs: VertexScratch<NT> is 192 * NT bytes of LDS
constexpr int MAX_PROPS = 4096;     // proposal rows of one sample (12 index bits in a draw's order key)
constexpr int MAX_GTS = 1024;       // gt rows of one sample (their rows and maxima live in LDS)
constexpr int MAX_NUM = 1024;       // sampler.num
constexpr int MAX_PIECES = 8;       // len(neg_iou_piece_thrs)
constexpr int MAX_CLASSES = 16;     // assigners
constexpr int MAX_SAMPLES = 1024;   // samples whose segment starts the packing kernel keeps in LDS
constexpr long long MAX_ROWS = 1LL << 24;
constexpr int FLAG_LOW_QUALITY = 1, FLAG_ASSIGN_ALL = 2;

struct Rules {
  int C;
  float pos[MAX_CLASSES], neg[MAX_CLASSES], min_pos[MAX_CLASSES];
  int flags[MAX_CLASSES];
  int num, npos, K;
  float piece_thr[MAX_PIECES];
  double piece_frac[MAX_PIECES];
};

// the entry points' argument checks and the Rules record (csrc/roi_sample_cpu.cpp): one text for the launch and for the twin
int make_rules(int64_t N, int64_t G, int32_t B, int32_t C, const float* pos_iou_thr, const float* neg_iou_thr, const float* min_pos_iou,
               const int32_t* assign_flags, int32_t num, int32_t npos, int32_t K, const double* neg_piece_fractions,
               const float* neg_iou_piece_thrs, Rules& r);

// the plan of one sample's draws, from the sizes of its strata alone
struct Plan {
  int npos;               // positives drawn
  int take[MAX_PIECES];   // negatives each piece gives, in (key, index) order
  int off[MAX_PIECES];    // where a piece's negatives start among the negatives of the output
  int chosen;             // their sum
  int fill;               // slots filled with replacement after them
  int fill_from_last;     // from the last piece in index order (1) or from the chosen negatives in output order (0)
  int m;                  // length of that list
};

// [x, y, z, dx, dy, dz, yaw] -> the BEV rectangle xywhr2xyxyr makes of [x, y, dx, dy, yaw], as the pair test consumes it
RB_DEV void bev_obox(const float* b, OBox& o) {
  const float hw = b[3] / 2.0f, hh = b[4] / 2.0f;
  const float r[5] = {b[0] - hw, b[1] - hh, b[0] + hw, b[1] + hh, b[6]};
  rbox::obox_make(r, o);
}

// BboxOverlaps3D(coordinate='lidar'): z is the bottom face
template <int N>
RB_DEV float iou3d(const float* a, const OBox& A, const float* b, const OBox& B, VertexScratch<N>& vs, int t) {
  const float ov_bev = rbox::box_overlap<N>(A, B, vs, t);
  const float top = rbox::fmin2(a[2] + a[5], b[2] + b[5]);
  const float bottom = rbox::fmax2(a[2], b[2]);
  const float ov_h = rbox::fmax2(top - bottom, 0.0f);
  const float ov = ov_bev * ov_h;
  const float va = a[3] * a[4] * a[5];
  const float vb = b[3] * b[4] * b[5];
  return ov / rbox::fmax2(va + vb - ov, 1e-8f);
}

// what the assigner sees of an IoU: NaN and negative values (NaN boxes, negative extents) count as no overlap, so the per-gt
// maximum is a maximum of non-negative floats — order free as an unsigned maximum of the bit patterns
RB_DEV float clean_iou(float v) { return v > 0.0f ? v : 0.0f; }

// What decides, before any clipping, that clean_iou(iou3d) of a pair is exactly 0: the bounding-circle early-out of
// rbox::box_overlap, on the very operations it performs on the OBox of bev_obox (overlap 0, hence IoU 0 or 0 / NaN), and an
// empty height overlap (ov = ov_bev * 0: 0 or NaN).  A NaN anywhere fails both tests and leaves the pair to the full sequence.
struct Lite {
  float cx, cy, ra, z0, z1;
};
RB_DEV void lite_of(const float* b, Lite& l) {
  const float hw = b[3] / 2.0f, hh = b[4] / 2.0f;
  const float x1 = b[0] - hw, y1 = b[1] - hh, x2 = b[0] + hw, y2 = b[1] + hh;
  l.cx = (x1 + x2) / 2.0f;
  l.cy = (y1 + y2) / 2.0f;
  l.ra = fabsf(x2 - x1) + fabsf(y2 - y1);
  l.z0 = b[2];
  l.z1 = b[2] + b[5];
}
RB_DEV bool may_overlap(const Lite& a, const Lite& b) {
  const float ddx = a.cx - b.cx, ddy = a.cy - b.cy;
  const float reach = 0.5f * (a.ra + b.ra) + 1e-2f;
  if (ddx * ddx + ddy * ddy > reach * reach * 1.0001f) return false;
  const float top = rbox::fmin2(a.z1, b.z1), bottom = rbox::fmax2(a.z0, b.z0);
  return rbox::fmax2(top - bottom, 0.0f) != 0.0f;
}

RB_DEV unsigned f32_bits(float v) { return __builtin_bit_cast(unsigned, v); }
RB_DEV float bits_f32(unsigned v) { return __builtin_bit_cast(float, v); }

// a draw's key as an unsigned that orders as the float does on [0, 1); anything else (NaN, negative, >= 1) is clamped into it
RB_DEV unsigned key_bits(float k) {
  if (!(k >= 0.0f)) return 0u;
  if (k >= 1.0f) return 0x3f7fffffu;
  return f32_bits(k + 0.0f);
}

// MaxIoUAssigner.assign_wrt_overlaps, rules 1-3, for a proposal that met at least one gt of its class
RB_DEV int assign_first(float max_overlap, int argmax, float pos_thr, float neg_thr) {
  int gi = -1;
  if (max_overlap >= 0.0f && max_overlap < neg_thr) gi = 0;
  if (max_overlap >= pos_thr) gi = argmax + 1;
  return gi;
}

// 0: a positive; 1 + i: a negative of piece i; -1: sampled by neither side
RB_DEV int stratum_of(int gt_ind, float max_overlap, const Rules& r) {
  if (gt_ind > 0) return 0;
  if (gt_ind < 0) return -1;
  for (int i = 0; i < r.K; ++i) {
    const float lo = i + 1 < r.K ? r.piece_thr[i + 1] : 0.0f;
    if (max_overlap >= lo && max_overlap < r.piece_thr[i]) return 1 + i;
  }
  return -1;
}

// (stratum, key, index) ascending == these 64-bit entries DESCENDING; no entry is 0
RB_DEV unsigned long long draw_entry(int stratum, float key, int n) {
  return ~(((unsigned long long)stratum << 44) | ((unsigned long long)key_bits(key) << 12) | (unsigned long long)n);
}
RB_DEV int entry_stratum(unsigned long long e) { return (int)((~e >> 44) & 0xfull); }
RB_DEV int entry_index(unsigned long long e) { return (int)(~e & 0xfffull); }

// IoUNegPiecewiseSampler's bookkeeping; cnt[0] positives, cnt[1 + i] negatives of piece i.  A piece never takes more than what is
// left of `expected` (the reference's doubled carry can ask for more; the output has `num` rows per sample).
RB_DEV void make_plan(const int* cnt, const Rules& r, Plan& p) {
  p.npos = cnt[0] < r.npos ? cnt[0] : r.npos;
  const int expected = r.num - p.npos;
  int chosen = 0, carry = 0;
  for (int i = 0; i < MAX_PIECES; ++i) p.take[i] = p.off[i] = 0;
  for (int i = 0; i < r.K; ++i) {
    const bool last = i + 1 == r.K;
    const int room = expected - chosen;
    const int e = last ? room : (int)((double)expected * r.piece_frac[i]) + carry;
    const int c = cnt[1 + i];
    int take;
    if (c < e) {
      take = c;
      carry += e - c;
    } else {
      take = e;
      carry = 0;
    }
    take = take < room ? take : room;
    take = take < 0 ? 0 : take;
    p.take[i] = take;
    p.off[i] = chosen;
    chosen += take;
  }
  p.chosen = chosen;
  const int c_last = r.K > 0 ? cnt[r.K] : 0;
  p.fill = expected - chosen;
  p.fill_from_last = c_last > 0 ? 1 : 0;
  p.m = c_last > 0 ? c_last : chosen;
  if (p.m == 0) p.fill = 0;   // nothing to repeat: the sample comes out short
}

// the member a fill slot takes of a list of m: min(floor(key * m), m - 1); a NaN or negative product takes member 0
RB_DEV int fill_member(float key, int m) {
  const float f = key * (float)m;
  if (!(f >= 0.0f)) return 0;
  if (f >= (float)m) return m - 1;
  return (int)f;
}

RB_DEV int clamp_count(int c, int room) {
  const int v = c < 0 ? 0 : c;
  return v < room ? v : room;
}

// the b with s[b] <= i < s[b + 1] among the segment starts s[0] <= .. <= s[B]; B for a row past s[B]
RB_DEV int sample_of(const int* s, int B, int i) {
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid + 1] > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

}  // namespace roi_sample
