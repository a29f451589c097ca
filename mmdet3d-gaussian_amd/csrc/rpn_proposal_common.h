// rpn_proposal_common.h — what csrc/rpn_proposal.hip (gfx950 kernels) and csrc/rpn_proposal_cpu.cpp (their `_cpu` twin) share:
// every value and decision of the RPN proposal stage (mmdet3d's PartA2RPNHead.get_bboxes_single + class_agnostic_nms, restated in
// include/gd3d.h) that is not a loop over anchors, each as ONE fixed sequence of fp32 operations: the per-anchor reduction and
// its order key, the sigmoid on fx_expf (csrc/fx_exp.h), the DeltaXYZWLHR decode with the NMS box, the direction fix, the
// argument checks, the launches' arguments and the carve of the workspace.  Both units are compiled with -ffp-contract=off, so
// every output is the same bits on the device and on the host.
#pragma once
#include "fx_exp.h"
#include "gd3d_workspace.h"

#include <stddef.h>
#include <stdint.h>

namespace rpn_proposal {

constexpr int MAX_CLASSES = 16;
constexpr int MAX_CAND = 16384;       // candidates of a sample: rnms_scored_max_n(), the largest NMS problem the library runs
constexpr int MAX_SAMPLES = 1024;
constexpr int RADIX_BITS = 8, BINS = 1 << RADIX_BITS, LEVELS = 32 / RADIX_BITS;   // the radix select: 4 levels of 256 bins
constexpr int WG = 256;               // threads of every workgroup
constexpr int SPAN = 16 * WG;         // keys one workgroup of the histogram / compaction launches covers
constexpr int RANK_I = 64;            // survivors one workgroup of the ordering launch ranks
constexpr float PI_F = 3.14159265358979323846f;

struct Params {
  int B, A, C, H, W, HW, N, cap, M;   // N = H W A anchors; cap = min(nms_pre, N) candidates; M = min(nms_post, max_num) rows
  int rotate;
  float nms_thr, score_thr, dir_offset, dir_limit_offset;
};

// ---- the launches' arguments and the workspace, sized from shapes alone --------------------------------------------------------
struct Args {
  const float* cls;        // (B, A*C, H, W)
  const float* bbox;       // (B, A*7, H, W)
  const float* dirp;       // (B, A*2, H, W)
  const float* anchors;    // (N, 7)
  Params p;
  int nblk;                // spans of SPAN keys in a sample
  // the workspace (carve):
  int* hist;               // [B][LEVELS][BINS]  keys per digit under the prefix the levels above resolved
  int* nsurv;              // [B]                survivors above the boundary key appended so far
  int* cnt;                // [B]                candidates with score > score_thr
  unsigned* keys;          // [B][N]             order keys, 0 for an anchor that is no candidate
  int* tiecnt;             // [B][nblk]          keys equal to the boundary key in each span
  unsigned long long* surv;   // [B][cap]        (key, ~index) of the survivors, in no order
  int* sel;                // [B][cap]           their anchor indices in the selection order
  float* box7;             // per candidate, in the selection order: box7 .. dir
  float* bev5;
  float* score;
  int* label;
  int* dir;
  long long* order;        // the operands of rnms_batched: order, cnt, thresh, keep, num_keep
  float* thresh;
  const long long* keep;
  const long long* num_keep;
  float* boxes_3d;
  float* scores_3d;
  long long* labels_3d;
  float* cls_preds;
  float* rois;
  int* batch_cnt;
  long long* cand_inds;    // nullable
  int* cand_cnt;           // nullable
};

// What of the workspace is no kernel argument: the block one fill clears (hist, nsurv, cnt: contiguous and first), the workspace of
// rnms_batched, the size the entry asks of its caller.
struct Carved {
  size_t zero_bytes;
  void* nms;
  size_t bytes;
};

// The workspace of a.p (B, N, cap) cut into a's buffers, every buffer once; the base is rounded up to 256 bytes here.  At address 0
// it is the size function.
inline Carved carve(Args& a, void* workspace, size_t nms_bytes) {
  const size_t B = (size_t)a.p.B, N = (size_t)a.p.N, cap = (size_t)a.p.cap;
  gd3d::Carver c(workspace, gd3d::Carver::SELF_ALIGNING);
  Carved r;
  a.nblk = (int)((N + SPAN - 1) / SPAN);
  a.hist = c.take<int>(B * LEVELS * BINS);
  a.nsurv = c.take<int>(B);
  a.cnt = c.take<int>(B);
  a.keys = c.take<unsigned>(B * N);
  r.zero_bytes = (size_t)((uintptr_t)a.keys - (uintptr_t)a.hist);
  a.tiecnt = c.take<int>(B * (size_t)a.nblk);
  a.surv = c.take<unsigned long long>(B * cap);
  a.sel = c.take<int>(B * cap);
  a.box7 = c.take<float>(B * cap * 7);
  a.bev5 = c.take<float>(B * cap * 5);
  a.score = c.take<float>(B * cap);
  a.label = c.take<int>(B * cap);
  a.dir = c.take<int>(B * cap);
  a.order = c.take<long long>(B * cap);
  a.thresh = c.take<float>(B);
  a.keep = c.take<long long>(B * cap);
  a.num_keep = c.take<long long>(B);
  r.nms = c.take<char>(nms_bytes);
  r.bytes = c.bytes();
  return r;
}

// the entry points' argument checks (csrc/rpn_proposal_cpu.cpp): one text for the launches and for the twin
int check_args(int32_t B, int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num, float nms_thr,
               float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset, Params& p);

// ---- the per-anchor reduction ------------------------------------------------------------------------------------------------------
// order-preserving 32-bit key of a logit: a < b  <=>  key(a) < key(b), -0 and +0 share a key; 0 is no logit's key (-inf has
// 0x007fffff) and marks an anchor that is no candidate
RB_DEV unsigned key_of(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the C class logits of one anchor, `stride` floats apart: best = the maximum, label = the lowest class attaining it; false when
// a logit is NaN (the anchor is never a candidate)
RB_DEV bool anchor_best(const float* logit, size_t stride, int C, float& best, int& label) {
  float m = logit[0];
  bool ok = m == m;
  int l = 0;
  for (int c = 1; c < C; ++c) {
    const float v = logit[(size_t)c * stride];
    ok = ok && v == v;
    if (v > m) {
      m = v;
      l = c;
    }
  }
  best = m;
  label = l;
  return ok;
}

RB_DEV float sigmoid(float x) { return 1.0f / (1.0f + rbox::fx_expf(-x)); }

// ---- per candidate -----------------------------------------------------------------------------------------------------------------
// DeltaXYZWLHRBBoxCoder.decode, operation by operation, and xywhr2xyxyr of [x, y, dx, dy, r]; t: the 7 deltas, an: the anchor
RB_DEV void decode(const float* an, const float* t, float* box7, float* bev5) {
  const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
  const float za = an[2] + ha / 2.0f;
  const float diagonal = sqrtf(la * la + wa * wa);
  const float xg = t[0] * diagonal + xa;
  const float yg = t[1] * diagonal + ya;
  float zg = t[2] * ha + za;
  const float lg = rbox::fx_expf(t[4]) * la;
  const float wg = rbox::fx_expf(t[3]) * wa;
  const float hg = rbox::fx_expf(t[5]) * ha;
  const float rg = t[6] + ra;
  zg = zg - hg / 2.0f;
  box7[0] = xg; box7[1] = yg; box7[2] = zg; box7[3] = wg; box7[4] = lg; box7[5] = hg; box7[6] = rg;
  const float hw = wg / 2.0f, hl = lg / 2.0f;
  bev5[0] = xg - hw; bev5[1] = yg - hl; bev5[2] = xg + hw; bev5[3] = yg + hl; bev5[4] = rg;
}

// yaw = limit_period(yaw - dir_offset, dir_limit_offset, pi) + dir_offset + pi * dir
RB_DEV float dir_fix(float yaw, int dir, float dir_offset, float dir_limit_offset) {
  const float val = yaw - dir_offset;
  const float dir_rot = val - floorf(val / PI_F + dir_limit_offset) * PI_F;
  return dir_rot + dir_offset + PI_F * (float)dir;
}

// rows a sample contributes: the scan's failure mark passes through as -1
RB_DEV int rows_of(long long num_keep, int M) { return num_keep < 0 ? -1 : (num_keep < (long long)M ? (int)num_keep : M); }

}  // namespace rpn_proposal
