// eval_frames.hip — the per-frame stage of the flexible mAP evaluation for a whole BATCH of frames on gfx950 (include/gd3d.h "Flexible
// mAP, a batch of frames").  A problem is one (frame, class) pair; eval_frames_records turns every problem, every
// breakdown row and every threshold of the batch into records in THREE launches, whatever P, R, T and the frames are:
//   pair kernel     one thread per (detection, gt) pair of the batch; the thread finds its problem by binary search in pair_off and
//                   writes the (negated) affinity: eval_iou of rbox_device.h, or the centre distance in trans_bev_kernel's expression;
//   match kernel    one wave per (problem, breakdown row, threshold) runs the matcher body of eval_match_device.h — the code of
//                   eval_match_coco's kernels — on the problem's slice of the pair buffer; ONE form per launch, picked from max_gt:
//                   <= 64 gts and <= 256 gts (the sets are lane masks), <= 2048 gts (taken bits in a register);
//   records kernel  one thread per (breakdown row, detection) packs the T bits as eval_tp_records does; with alias_tp the tp bits
//                   come from the matcher result of the problem's LAST applicable row, so nothing is copied and nothing can race.
// A batch without a single (detection, gt) pair has no pair grid: it runs the records kernel alone (host-known from the shapes).
// No host read, no atomic, static shapes.  Compiled with -ffp-contract=off, as rbox.hip and eval_match.hip are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eval_frames_common.h"
#include "eval_match_device.h"
#include "gd3d_workspace.h"
#include "rbox_device.h"

namespace eval_frames {

constexpr int PAIR_T = 128;   // threads of the pair kernel: HullScratch<128> is 60 KiB of LDS, as in riou_eval_kernel
constexpr int REC_T = 256;

// largest p in [0, P) with off[p] <= x, for an ascending table off[0 .. P] with off[0] <= x < off[P]: the problem that owns x.
// Empty problems (off[p] == off[p + 1]) are stepped over; the result stays in [0, P) whatever the table holds.
template <class I>
__device__ __forceinline__ int owner(const I* __restrict__ off, int P, long long x) {
  int lo = 0, hi = P;   // invariant: off[lo] <= x (assumed for lo = 0), off[hi] > x (assumed for hi = P)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long long)off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// MODE 0: iou_3d, 1: iou_bev, 2: BEV centre distance
template <int MODE>
__global__ __launch_bounds__(PAIR_T) void pair_kernel(const float* __restrict__ det, const int32_t* __restrict__ det_seg, long long ND,
                                                      const float* __restrict__ gt, const int32_t* __restrict__ gt_seg, long long NG,
                                                      const int64_t* __restrict__ pair_off, long long pairs, int P, float z_offset, int negate,
                                                      float* __restrict__ cost) {
  __shared__ rbox::HullScratch<MODE == 2 ? 1 : PAIR_T> hs;
  const long long idx = (long long)blockIdx.x * PAIR_T + threadIdx.x;
  if (idx >= pairs) return;
  const int p = owner(pair_off, P, idx);
  const long long local = idx - pair_off[p];
  const long long ds = det_seg[p], gs = gt_seg[p], nd = det_seg[p + 1] - ds, ng = gt_seg[p + 1] - gs;
  if (local < 0 || nd <= 0 || ng <= 0) return;                   // tables that disagree: nothing is read out of range
  const long long di = local / ng, gi = local - di * ng;
  if (di >= nd || ds < 0 || gs < 0 || ds + nd > ND || gs + ng > NG) return;
  const float* __restrict__ dr = det + (ds + di) * 7;
  const float* __restrict__ gr = gt + (gs + gi) * 7;
  float v;
  if constexpr (MODE == 2) {
    const float dx = dr[0] - gr[0], dy = dr[1] - gr[1];
    v = sqrtf(dx * dx + dy * dy);   // trans_bev_kernel's expression (correctly rounded)
  } else {
    float d[7], g[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      d[k] = dr[k];
      g[k] = gr[k];
    }
    v = rbox::eval_iou<MODE == 0, (MODE == 2 ? 1 : PAIR_T)>(d, g, z_offset, hs, threadIdx.x);
  }
  cost[idx] = negate ? -v : v;      // exact
}

// the flags of one breakdown row: a gt outside the row is ignored; no crowd array means no crowd gt
struct RowFlags {
  const uint8_t* __restrict__ in_row;
  const uint8_t* __restrict__ is_crowd;
  __device__ __forceinline__ bool ignore(int g) const { return in_row[g] == 0; }
  __device__ __forceinline__ bool crowd(int g) const { return is_crowd != nullptr && is_crowd[g] != 0; }
};

// FORM 0: every problem has <= 64 gts, 1: <= 256, 2: <= 2048.  matched is (R, T, ND): row (b, t) holds the detections of all problems.
template <int FORM>
__global__ __launch_bounds__(64) void match_kernel(const float* __restrict__ cost, const float* __restrict__ thrs, int negate,
                                                   const int32_t* __restrict__ det_seg, long long ND, const int32_t* __restrict__ gt_seg,
                                                   long long NG, const int64_t* __restrict__ pair_off, long long pairs,
                                                   const int32_t* __restrict__ group, const uint8_t* __restrict__ gt_flag,
                                                   const uint8_t* __restrict__ gt_crowd, int R, int T, int32_t* __restrict__ matched) {
  constexpr int CAP = FORM == 0 ? 64 : FORM == 1 ? 256 : (int)MAX_GT;
  const int item = blockIdx.x;
  const int t = item % T, pb = item / T, b = pb % R, p = pb / R;
  if (group[(long long)p * R + b] < 0) return;                                   // the row does not apply: nothing is matched
  const long long ds = det_seg[p], gs = gt_seg[p], nd = det_seg[p + 1] - ds, ng = gt_seg[p + 1] - gs, po = pair_off[p];
  if (nd <= 0 || ng <= 0 || ng > CAP) return;                                    // no rows, or the no-match branch of the records
  if (ds < 0 || gs < 0 || ds + nd > ND || gs + ng > NG || po < 0 || po + nd * ng > pairs) return;
  const float thr = negate ? -thrs[t] : thrs[t];
  const RowFlags fl = {gt_flag + (long long)b * NG + gs, gt_crowd != nullptr ? gt_crowd + gs : nullptr};
  int* const out = matched + ((size_t)b * T + t) * (size_t)ND + ds;
  if (FORM == 0) evalm::match_coco_small_wave<1>(cost + po, thr, fl, (int)nd, (int)ng, out);
  else if (FORM == 1) evalm::match_coco_small_wave<4>(cost + po, thr, fl, (int)nd, (int)ng, out);
  else evalm::match_coco_wave<true, true>(cost + po, thr, fl, (int)nd, (int)ng, nullptr, out);
}

__global__ __launch_bounds__(REC_T) void records_kernel(const int32_t* __restrict__ matched, const int32_t* __restrict__ det_seg,
                                                        const int32_t* __restrict__ gt_seg, const int32_t* __restrict__ group,
                                                        const uint8_t* __restrict__ det_flag, const uint8_t* __restrict__ gt_flag,
                                                        const float* __restrict__ score, long long ND, long long NG, int P, int R, int T,
                                                        int alias_tp, int32_t* __restrict__ o_group, float* __restrict__ o_score,
                                                        uint32_t* __restrict__ o_tp, uint32_t* __restrict__ o_msk) {
  const long long idx = (long long)blockIdx.x * REC_T + threadIdx.x;
  if (idx >= (long long)R * ND) return;
  const int b = (int)(idx / ND);
  const long long i = idx - (long long)b * ND;
  const int p = owner(det_seg, P, i);
  const int32_t g = group[(long long)p * R + b];
  uint32_t tp = 0, msk = 0;
  if (g >= 0) {
    long long gs = gt_seg[p], ng = gt_seg[p + 1] - gs;
    if (gs < 0 || ng < 0 || gs + ng > NG || matched == nullptr) ng = 0;           // the no-match branch
    int bl = b;                                                                  // the row whose matcher result gives the tp bits
    if (alias_tp)
      for (int k = R - 1; k > b; --k)
        if (group[(long long)p * R + k] >= 0) {
          bl = k;
          break;
        }
    const bool df = det_flag[idx] != 0;
    const uint8_t* __restrict__ gf = gt_flag + (long long)b * NG + gs;
    for (int t = 0; t < T; ++t) {
      const int32_t m = ng > 0 ? eval_ap::clamp_match(matched[((size_t)b * T + t) * (size_t)ND + i], ng) : -1;
      const int32_t ml = (ng > 0 && bl != b) ? eval_ap::clamp_match(matched[((size_t)bl * T + t) * (size_t)ND + i], ng) : m;
      const bool in = m > -1 ? gf[m] != 0 : df;
      tp |= (uint32_t)(ml > -1) << t;
      msk |= (uint32_t)in << t;
    }
  }
  o_group[idx] = g < 0 ? -1 : g;
  o_score[idx] = score[i];
  o_tp[idx] = tp;
  o_msk[idx] = msk;
}

// the workspace: one carve gives the pointers and, at address 0, the size
struct Work {
  float* cost;
  int32_t* matched;
  size_t bytes;
  Work(void* workspace, int64_t ND, int64_t pairs, int32_t R, int32_t T) {
    gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
    cost = c.take<float>((size_t)pairs);
    matched = c.take<int32_t>((size_t)R * (size_t)T * (size_t)ND);
    bytes = c.bytes();
  }
};

}  // namespace eval_frames

using namespace eval_frames;

extern "C" {

size_t eval_frames_workspace_bytes(int64_t ND, int64_t pairs, int32_t R, int32_t T) {
  if (ND < 0 || pairs < 0 || R < 1 || T < 1 || T > eval_ap::MAX_T || ND > MAX_I32 || pairs > MAX_I32 || (int64_t)R * ND > MAX_I32) return 0;
  const Work w(nullptr, ND, pairs, R, T);
  return w.bytes > 256 ? w.bytes : 256;
}

int eval_frames_records(int32_t mode, float z_offset, int32_t negate, const float* det, const float* score, const int32_t* det_seg, int64_t ND,
                        const float* gt, const int32_t* gt_seg, int64_t NG, const uint8_t* gt_crowd, const int64_t* pair_off, int64_t pairs,
                        int64_t max_gt, const uint8_t* det_flag, const uint8_t* gt_flag, const int32_t* group, const float* thrs, int32_t P,
                        int32_t R, int32_t T, int32_t alias_tp, int32_t* out_group, float* out_score, uint32_t* out_tp_bits,
                        uint32_t* out_msk_bits, void* workspace, void* stream) {
  const int rc = check_frames(mode, det, score, det_seg, ND, gt, gt_seg, NG, pair_off, pairs, max_gt, det_flag, gt_flag, group, thrs, P, R, T,
                              out_group, out_score, out_tp_bits, out_msk_bits);
  if (rc != 0 || ND == 0) return rc;
  if (workspace == nullptr || ((uintptr_t)workspace & 255) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const Work w(workspace, ND, pairs, R, T);
  if (pairs > 0) {
    const dim3 pg((unsigned)((pairs + PAIR_T - 1) / PAIR_T)), pb(PAIR_T);
#define GD3D_PAIR(MODE)                                                                                                                       \
  hipLaunchKernelGGL((pair_kernel<MODE>), pg, pb, 0, s, det, det_seg, (long long)ND, gt, gt_seg, (long long)NG, pair_off, (long long)pairs, \
                     (int)P, z_offset, (int)negate, w.cost)
    if (mode == 0) GD3D_PAIR(0);
    else if (mode == 1) GD3D_PAIR(1);
    else GD3D_PAIR(2);
#undef GD3D_PAIR
    const dim3 mg((unsigned)((int64_t)P * R * T)), mb(64);
#define GD3D_MATCH(FORM)                                                                                                                   \
  hipLaunchKernelGGL((match_kernel<FORM>), mg, mb, 0, s, w.cost, thrs, (int)negate, det_seg, (long long)ND, gt_seg, (long long)NG, pair_off, \
                     (long long)pairs, group, gt_flag, gt_crowd, (int)R, (int)T, w.matched)
    if (max_gt <= 64) GD3D_MATCH(0);
    else if (max_gt <= 256) GD3D_MATCH(1);
    else GD3D_MATCH(2);
#undef GD3D_MATCH
  }
  const long long rows = (long long)R * ND;
  hipLaunchKernelGGL(records_kernel, dim3((unsigned)((rows + REC_T - 1) / REC_T)), dim3(REC_T), 0, s, pairs > 0 ? w.matched : nullptr, det_seg,
                     gt_seg, group, det_flag, gt_flag, score, (long long)ND, (long long)NG, (int)P, (int)R, (int)T, (int)alias_tp, out_group,
                     out_score, out_tp_bits, out_msk_bits);
  return (int)hipGetLastError();
}

}  // extern "C"
