// simota_common.h — what csrc/simota.hip (gfx950 kernels) and csrc/simota_cpu.cpp (their `_cpu` twin) share: every decision of
// SimOTABEVAssigner.assign (core/bbox/assigners/sim_ota_3d_assigner.py:34-211) that is not a loop over rows, each as ONE fixed
// sequence of fp32 operations: the BEV membership of a prior (the x / y part of pib::contains), the centre test, the
// classification cost on fx_logf (csrc/fx_log.h), the pair cost, the order keys of the two bounded selections and the dynamic k.
// The IoU is roi_sample::iou3d behind its may_overlap early-out (csrc/roi_sample_common.h): the bits of bbox_overlaps_3d.  Both
// units are compiled with -ffp-contract=off, so every decision is the same on the device and on the host.
#pragma once
#include "fx_log.h"
#include "gd3d_workspace.h"
#include "roi_sample_common.h"

#include <stddef.h>
#include <stdint.h>

namespace simota {

using rbox::OBox;
using rbox::VertexScratch;
using roi_sample::bev_obox;
using roi_sample::bits_f32;
using roi_sample::clean_iou;
using roi_sample::f32_bits;
using roi_sample::iou3d;
using roi_sample::Lite;
using roi_sample::lite_of;
using roi_sample::may_overlap;

constexpr int WG = 1024;              // threads of every workgroup (csrc/lds_sort.h is written for 1024)
constexpr int NT = 256;               // of which this many clip box pairs: VertexScratch<NT> is 192 * NT bytes of LDS
constexpr int GT_TILE = 256;          // gts whose constants the flag kernel holds in LDS at a time
constexpr int MAX_GTS = 1024;         // gts of one sample
constexpr int MAX_TOPK = 32;          // candidate_topk
constexpr int MAX_CLASSES = 32;
constexpr int MAX_SAMPLES = 1024;
constexpr int MAX_MATCHES = 16384;    // G_cap * candidate_topk: the matches of a sample are sorted in LDS
constexpr long long MAX_ROWS = 1LL << 24;

struct Params {
  int C, K;                           // classes, candidate_topk
  float radius, iou_w, cls_w, match_init;
};

// ---- the launches' arguments and the workspace, sized from shapes alone (csrc/simota_cpu.cpp: gd3d_simota_workspace_bytes) --------
struct Args {
  const float* scores;        // (P, C)
  const float* boxes;         // (P, 7)
  const float* priors;        // (prior_rows, stride)
  long long prior_rows, prior_stride;
  int shared;
  const int32_t* pcnt;        // (B)
  long long P;
  const float* gt;            // (G, 7)
  const int64_t* glabel;      // (G)
  const int32_t* gcnt;        // (B)
  long long G;
  int B, G_cap;
  Params prm;
  int64_t* gt_inds;           // (P)
  int64_t* labels;            // (P)
  float* max_overlaps;        // (P)
  int32_t* pos_cnt;           // (B)
  int64_t* pos_inds;          // (B, G_cap * K)
  int64_t* pos_gt_inds;       // (B, G_cap * K)
  // the workspace (carve):
  int32_t* cand_cnt;          // [B]              candidates of a sample
  int32_t* cand;              // [P]              their prior indices within the sample, in the sample's own rows, in no order
  int32_t* match_prior;       // [B * G_cap * K]  the priors gt g took, -1 beyond its k
  float* match_iou;           // [B * G_cap * K]  their IoU with g
  int32_t* conflict;          // [B * G_cap * K]  (prior, rank) of the priors more than one gt took
};

// The workspace cut into a's buffers, every buffer once; the base is rounded up to 256 bytes here.  Returns the size the entry asks
// of its caller: at address 0 it is the size function.
inline size_t carve(Args& a, void* workspace, int64_t P, int32_t B, int32_t G_cap, int32_t K) {
  const size_t m = (size_t)B * (size_t)G_cap * (size_t)K;
  gd3d::Carver c(workspace, gd3d::Carver::SELF_ALIGNING);
  a.cand_cnt = c.take<int32_t>((size_t)B);
  a.cand = c.take<int32_t>((size_t)P);
  a.match_prior = c.take<int32_t>(m);
  a.match_iou = c.take<float>(m);
  a.conflict = c.take<int32_t>(m);
  return c.bytes();
}

// the entry points' argument checks (csrc/simota_cpu.cpp): one text for the launch and for the twin
int check_args(int64_t P, int64_t prior_rows, int64_t prior_stride, int32_t shared_priors, int64_t G, int32_t B, int32_t C, int32_t G_cap,
               float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight, float match_init, Params& p);

// ---- membership ---------------------------------------------------------------------------------------------------------------
// what the two tests consume of a gt [x, y, z, dx, dy, dz, yaw]: pib::box_constants without its z terms
struct GtC {
  float x, y, hx, hy, c, s;
};
RB_DEV GtC gt_constants(const float* g) {
  GtC k;
  k.x = g[0];
  k.y = g[1];
  k.hx = g[3] * 0.5f;
  k.hy = g[4] * 0.5f;
  rbox::fx_sincosf(-g[6], k.s, k.c);
  return k;
}
// the x / y part of pib::contains, operation for operation: strict faces, a NaN coordinate is in nothing
RB_DEV bool in_gt(const GtC& k, float px, float py) {
  const float sx = px - k.x, sy = py - k.y;
  const float ns = -k.s;
  const float a0 = sx * k.c, a1 = sy * ns;
  const float b0 = sx * k.s, b1 = sy * k.c;
  const float lx = a0 + a1, ly = b0 + b1;
  return lx > -k.hx && lx < k.hx && ly > -k.hy && ly < k.hy;
}
// max(|x - gx|, |y - gy|) < radius
RB_DEV bool in_ct(const GtC& k, float px, float py, float radius) {
  const float dx = px - k.x, dy = py - k.y;
  return (dx < 0.0f ? -dx : dx) < radius && (dy < 0.0f ? -dy : dy) < radius;
}

// ---- costs ----------------------------------------------------------------------------------------------------------------------
// a probability as binary_cross_entropy accepts it: clamped into [0, 1], NaN to 0
RB_DEV float clamp_score(float v) { return v >= 0.0f ? (v <= 1.0f ? v : 1.0f) : 0.0f; }

// the two logarithms BCE takes of s = sqrt(score), floored at -100
RB_DEV void cls_terms(float score, float& la, float& lb) {
  const float s = sqrtf(clamp_score(score));
  la = rbox::fmax2(rbox::fx_logf(s), -100.0f);
  lb = rbox::fmax2(rbox::fx_logf(1.0f - s), -100.0f);
}

// sum over the classes, ascending, into +0 of -(t log s + (1 - t) log(1 - s)), t = [c == label]; a label outside [0, C) has t = 0
RB_DEV float cls_cost(const float* scores, int C, int64_t label) {
  float sum = 0.0f;
  for (int c = 0; c < C; ++c) {
    float la, lb;
    cls_terms(scores[c], la, lb);
    const float t = (int64_t)c == label ? 1.0f : 0.0f;
    sum = sum + (-(t * la + (1.0f - t) * lb));
  }
  return sum;
}

// cls * cls_weight + (-log(iou + 1e-8)) * iou_weight, each operation rounded; min(cost, match_init) inside box AND centre (a NaN
// cost becomes match_init there)
RB_DEV float pair_cost(float cls, float iou, bool both, const Params& p) {
  const float ic = -rbox::fx_logf(iou + 1e-8f);
  const float cost = cls * p.cls_w + ic * p.iou_w;
  return both ? rbox::fmin2(cost, p.match_init) : cost;
}

// an unsigned that orders as the cost does: -0 == +0, NaN above everything
RB_DEV unsigned cost_key(float c) {
  if (c != c) return 0xffffffffu;
  const unsigned u = f32_bits(c + 0.0f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// 64-bit entries of the two bounded selections; the LARGEST entries win, none is 0.
//   IoU  : (IoU bits, ~prior)   — IoUs are clean (>= +0 or +inf), so the bits order as the values; only IoU > 0 is entered
//   cost : (~cost key, ~prior)  — the smallest cost, then the lowest prior index
RB_DEV unsigned long long iou_entry(float iou, unsigned prior) {
  return ((unsigned long long)f32_bits(iou) << 32) | (unsigned long long)(0xffffffffu - prior);
}
RB_DEV unsigned long long cost_entry(float cost, unsigned prior) {
  return ((unsigned long long)(~cost_key(cost)) << 32) | (unsigned long long)(0xffffffffu - prior);
}
RB_DEV unsigned entry_prior(unsigned long long e) { return 0xffffffffu - (unsigned)e; }

// min(max((int)sum, 1), Kc) without a conversion that can overflow: a NaN sum gives 1, +inf gives Kc
RB_DEV int dynamic_k(float sum, int Kc) {
  if (!(sum >= 1.0f)) return 1 < Kc ? 1 : Kc;
  if (sum >= (float)Kc) return Kc;
  return (int)sum;
}

// ---- segments ---------------------------------------------------------------------------------------------------------------------
RB_DEV long long clamp_count(int c, long long room) {
  const long long v = c < 0 ? 0 : (long long)c;
  return v < room ? v : room;
}

// rows [start, start + n) of sample b among N rows: every count clamped to the rows left
RB_DEV void segment_of(const int32_t* cnt, int b, long long N, long long& start, long long& n) {
  long long s = 0, c = 0;
  for (int i = 0; i <= b; ++i) {
    s += c;
    c = clamp_count(cnt[i], N - s);
  }
  start = s;
  n = c;
}

// Work item j of a launch that gives every sample ceil(rows / WG) consecutive items -> the sample b, the item's first row and its
// np <= WG rows.  Rows beyond the counts' sum form one more segment, b == B, that has no gts.  False: j is past the last item.
RB_DEV bool row_block(const int32_t* pcnt, int B, long long N, long long j, int& b, long long& p0, long long& first, int& np) {
  long long ps = 0;
  for (int s = 0; s <= B; ++s) {
    const long long pn = s < B ? clamp_count(pcnt[s], N - ps) : N - ps;
    const long long items = (pn + WG - 1) / WG;
    if (j < items) {
      b = s;
      p0 = ps;
      first = j * WG;
      const long long left = pn - j * WG;
      np = (int)(left < WG ? left : WG);
      return true;
    }
    j -= items;
    ps += pn;
  }
  return false;
}

// the xy of prior n of the sample whose rows start at p0; false: a shared prior tensor has no such row
RB_DEV bool prior_xy(const float* priors, long long stride, int shared, long long prior_rows, long long p0, long long n, float& x, float& y) {
  const long long row = shared ? n : p0 + n;
  if (row >= prior_rows) return false;
  x = priors[row * stride];
  y = priors[row * stride + 1];
  return true;
}

}  // namespace simota
