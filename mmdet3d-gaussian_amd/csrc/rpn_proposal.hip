// rpn_proposal.hip — PV-RCNN's RPN proposal stage (mmdet3d's PartA2RPNHead.get_bboxes_single + class_agnostic_nms, restated in
// include/gd3d.h, gd3d_rpn_proposals) for gfx950: the proposals of a whole batch as one fill, nine launches of this file and the
// batched NMS of rbox.hip, without a host read, a data-dependent shape or launch, so the call captures in a hipGraph on one stream.
//   key_kernel      a thread per BEV cell: the A * C class logits of the cell, each load coalesced along w, are read ONCE; per
//                   anchor the order key of the best logit (0: a NaN logit, no candidate) goes to the workspace in the
//                   reference's anchor order (h, w, a), and the keys' top digit to the sample's first histogram;
//   hist_kernel     x3: the radix select, 8 bits a level.  Every workgroup re-derives the prefix the levels above resolved from
//                   their 256-bin histograms (a thread per bin, one shuffle scan per level: cheaper than a launch that would do
//                   it once) and counts the next digit of the keys under that prefix in its span of SPAN keys;
//   compact_kernel  with all 32 bits resolved the boundary key tau and the number of its holders to take are known: the keys
//                   above tau are gathered in LDS and appended with ONE integer atomic per workgroup (their order never reaches
//                   an output: 3300 same-address atomics a sample took 137 us), the holders of tau are counted per span;
//   tie_kernel      the holders of tau by ASCENDING anchor index: a span's holders rank behind those of the spans before it
//                   (sum of the span counts) and in index order inside it; the first `need` take the list's last places;
//   rank_kernel     orders the at most 16 384 survivors by COUNTING: the rank of a survivor is the number of survivors with a
//                   greater (key, ~index), tiles of 256 through LDS, 64 survivors a workgroup.  A permutation by construction: no
//                   sort, no atomics;
//   gather_kernel   per candidate in the selection order: label, score = sigmoid(best), direction bin, the 7 deltas and the
//                   anchor -> decode, the NMS row, the operands of rnms_batched and the count of scores above score_thr;
//   rnms_batched    (rbox.hip) B groups, device counts;
//   finish_kernel   a workgroup per sample: the exclusive scan of the B row counts, then the sample's kept rows back to back:
//                   the cut, the direction fix, the class scores (sigmoid of the kept anchors' logits) and the rois; the rows
//                   past the counts' sum get batch id -1, label -1 and zeros.
// Every output element is written by exactly one thread; the same bits on every run and in csrc/rpn_proposal_cpu.cpp.
// Compiled with -ffp-contract=off (csrc/rpn_proposal_common.h).
#include <hip/hip_runtime.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "rpn_proposal_common.h"

namespace rpn_proposal {

static_assert(WG == BINS && WG == 4 * 64 && RANK_I == 64, "a thread per bin; four waves share a tile; a lane per ranked survivor");

// histogram add with two rounds of peer aggregation (trained maps put most anchors into a handful of exponent bins, and 64 lanes
// adding to one LDS word are served one after the other); every lane of the wave calls it
__device__ __forceinline__ void hist_add(int* hist, int bin, bool valid) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (todo == 0) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(valid && bin == lb) & todo;
    if (lane == leader) atomicAdd(&hist[lb], __popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&hist[bin], 1);
}

struct Sel {
  unsigned prefix;   // the digits resolved so far, right-aligned; with all LEVELS: the boundary key tau
  int need;          // candidates still to take under the prefix; with all LEVELS: holders of tau to take
  int total;         // candidates of the sample: min(cap, anchors without a NaN logit)
};

// v summed over the workgroup's WG threads (wave shuffles + one LDS hop): returns the sum over the threads ABOVE this one
// (tid' > tid), *total = the sum over all.  s_w: WG / 64 ints of LDS.  Two barriers.
__device__ __forceinline__ int sum_above(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_down(x, off, 64);
    if (lane + off < 64) x += y;
  }
  __syncthreads();                           // the previous use of s_w is over
  if (lane == 0) s_w[wave] = x;
  __syncthreads();
  int above = x - v, tot = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    const int p = s_w[w];
    above += w > wave ? p : 0;
    tot += p;
  }
  *total = tot;
  return above;
}

// The selection state after `levels` levels, from the sample's histograms (a thread per bin: WG == BINS); every thread of the
// workgroup calls it and gets the same answer.  s_h: WG / 64 ints, s_o: 2 ints of LDS.  total == 0: nothing is selected (prefix
// and need are void).
__device__ Sel resolve(const int* hist, int cap, int levels, int* s_h, int* s_o) {
  const int tid = threadIdx.x;
  Sel s;
  s.prefix = 0u;
  s.need = 0;
  s.total = 0;
  for (int l = 0; l < (levels > 0 ? levels : 1); ++l) {   // level l is decided on histogram l; the total comes from histogram 0
    const int v = hist[l * BINS + tid];
    int tot;
    const int above = sum_above(v, s_h, &tot);
    if (l == 0) {
      s.total = s.need = tot < cap ? tot : cap;
      if (s.total == 0 || levels == 0) return s;
    }
    if (s.need > above && s.need <= above + v) {   // exactly one bin: the counts under the prefix sum to >= need
      s_o[0] = tid;
      s_o[1] = s.need - above;
    }
    __syncthreads();
    s.prefix = (s.prefix << RADIX_BITS) | (unsigned)s_o[0];
    s.need = s_o[1];
  }
  return s;
}

__global__ __launch_bounds__(WG) void key_kernel(const Args a) {
  __shared__ int s_hist[BINS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cell = blockIdx.x * WG + tid;
  const bool in = cell < a.p.HW;
  s_hist[tid] = 0;
  __syncthreads();
  const size_t HW = (size_t)a.p.HW;
  const float* base = a.cls + (size_t)b * a.p.A * a.p.C * HW + (in ? cell : 0);
  unsigned* out = a.keys + (size_t)b * a.p.N + (size_t)(in ? cell : 0) * a.p.A;
  for (int an = 0; an < a.p.A; ++an) {
    unsigned key = 0u;
    if (in) {
      float best;
      int label;
      if (anchor_best(base + (size_t)an * a.p.C * HW, HW, a.p.C, best, label)) key = key_of(best);
      out[an] = key;
    }
    hist_add(s_hist, (int)(key >> (32 - RADIX_BITS)), key != 0u);
  }
  __syncthreads();
  if (s_hist[tid] != 0) atomicAdd(&a.hist[(size_t)b * LEVELS * BINS + tid], s_hist[tid]);
}

// level: 1 .. LEVELS - 1
__global__ __launch_bounds__(WG) void hist_kernel(const Args a, const int level) {
  __shared__ int s_hist[BINS], s_h[BINS], s_o[3];
  const int b = blockIdx.y, tid = threadIdx.x;
  int* hist = a.hist + (size_t)b * LEVELS * BINS;
  const Sel s = resolve(hist, a.p.cap, level, s_h, s_o);
  if (s.total == 0) return;
  s_hist[tid] = 0;
  __syncthreads();
  const unsigned* keys = a.keys + (size_t)b * a.p.N;
  const int i0 = blockIdx.x * SPAN;
  const int hi_shift = 32 - RADIX_BITS * level, lo_shift = hi_shift - RADIX_BITS;
  for (int it = 0; it < SPAN / WG; ++it) {
    const int i = i0 + it * WG + tid;
    const unsigned key = i < a.p.N ? keys[i] : 0u;
    hist_add(s_hist, (int)((key >> lo_shift) & (BINS - 1)), key != 0u && (key >> hi_shift) == s.prefix);
  }
  __syncthreads();
  if (s_hist[tid] != 0) atomicAdd(&hist[level * BINS + tid], s_hist[tid]);
}

__device__ __forceinline__ unsigned long long pack(unsigned key, int idx) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)idx);
}

__global__ __launch_bounds__(WG) void compact_kernel(const Args a) {
  __shared__ unsigned long long s_list[SPAN];     // the span's keys above tau: ONE global atomic per workgroup places them
  __shared__ int s_h[BINS], s_o[3], s_ties, s_n, s_base;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const Sel s = resolve(a.hist + (size_t)b * LEVELS * BINS, a.p.cap, LEVELS, s_h, s_o);
  if (tid == 0) s_ties = s_n = 0;
  __syncthreads();
  if (s.total == 0) {
    if (tid == 0) a.tiecnt[(size_t)b * a.nblk + blockIdx.x] = 0;
    return;
  }
  const unsigned tau = s.prefix;          // > 0: the key of a candidate
  const unsigned* keys = a.keys + (size_t)b * a.p.N;
  const int i0 = blockIdx.x * SPAN;
  int ties = 0;
  for (int it = 0; it < SPAN / WG; ++it) {
    const int i = i0 + it * WG + tid;
    const unsigned key = i < a.p.N ? keys[i] : 0u;
    ties += key == tau ? 1 : 0;
    const bool take = key > tau;
    const unsigned long long m = __ballot(take);
    if (m != 0) {
      const int leader = __ffsll((long long)m) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&s_n, __popcll(m));
      base = __shfl(base, leader, 64);
      if (take) s_list[base + __popcll(m & ((1ull << lane) - 1ull))] = pack(key, i);     // at most SPAN entries: one per key
    }
  }
  if (ties != 0) atomicAdd(&s_ties, ties);
  __syncthreads();
  if (tid == 0) {
    a.tiecnt[(size_t)b * a.nblk + blockIdx.x] = s_ties;
    s_base = s_n != 0 ? atomicAdd(&a.nsurv[b], s_n) : 0;
  }
  __syncthreads();
  unsigned long long* surv = a.surv + (size_t)b * a.p.cap;
  for (int j = tid; j < s_n; j += WG)
    if (s_base + j < a.p.cap) surv[s_base + j] = s_list[j];     // fewer than `total` keys lie above tau: always inside
}

__global__ __launch_bounds__(WG) void tie_kernel(const Args a) {
  __shared__ int s_h[BINS], s_o[3], s_base;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int* tiecnt = a.tiecnt + (size_t)b * a.nblk;
  if (tiecnt[blockIdx.x] == 0) return;
  const Sel s = resolve(a.hist + (size_t)b * LEVELS * BINS, a.p.cap, LEVELS, s_h, s_o);
  if (s.total == 0) return;
  if (tid == 0) s_base = 0;
  __syncthreads();
  int part = 0;
  for (int j = tid; j < (int)blockIdx.x; j += WG) part += tiecnt[j];
  if (part != 0) atomicAdd(&s_base, part);
  __syncthreads();
  const int base = s_base;                 // holders of tau in the spans before this one
  if (base >= s.need) return;
  const unsigned tau = s.prefix;
  const unsigned* keys = a.keys + (size_t)b * a.p.N;
  // thread t owns the SPAN / WG consecutive keys from i0: ascending index inside the span is ascending (thread, u)
  const int i0 = blockIdx.x * SPAN + tid * (SPAN / WG);
  unsigned mask = 0u;
  for (int u = 0; u < SPAN / WG; ++u) {
    const int i = i0 + u;
    if (i < a.p.N && keys[i] == tau) mask |= 1u << u;
  }
  int span_ties;
  const int mine = __popc(mask);
  const int r0 = sum_above(mine, s_h, &span_ties);
  int r = base + (span_ties - r0 - mine);     // holders before this thread's keys
  const int first = s.total - s.need;      // the keys above tau fill the places before
  unsigned long long* surv = a.surv + (size_t)b * a.p.cap;
  for (int u = 0; u < SPAN / WG && r < s.need; ++u) {
    if ((mask >> u) & 1u) {
      surv[first + r] = pack(tau, i0 + u);
      ++r;
    }
  }
}

// A workgroup ranks RANK_I = 64 survivors, a lane each; its WG / 64 waves share every 256-entry tile of the list between them, so
// ceil(cap / 64) * B workgroups work (one survivor a thread and the whole list a wave left three quarters of the chip idle: 198 us
// at cap = 9000).  The first pass compares the 32-bit keys alone (two instructions an entry) and counts the equal ones; only when
// some survivor of the workgroup shares its key — rare: logits are fp32 values — a second pass counts the equal keys of lower index.
__global__ __launch_bounds__(WG) void rank_kernel(const Args a) {
  __shared__ uint2 s_tile[WG];              // (~index, key)
  __shared__ int s_part[WG];
  __shared__ int s_h[BINS], s_o[3];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = resolve(a.hist + (size_t)b * LEVELS * BINS, a.p.cap, 0, s_h, s_o).total;
  if (blockIdx.x * RANK_I >= n) return;
  const int i = blockIdx.x * RANK_I + lane;
  const unsigned long long* surv = a.surv + (size_t)b * a.p.cap;
  const unsigned long long mine = i < n ? surv[i] : 0ull;
  const unsigned mh = (unsigned)(mine >> 32), ml = (unsigned)mine;
  const uint2* part = s_tile + wave * 64;   // this wave's share of a tile
  int gt = 0, eq = 0;
  for (int j0 = 0; j0 < n; j0 += WG) {
    __syncthreads();
    const unsigned long long e = j0 + tid < n ? surv[j0 + tid] : 0ull;     // padding: key 0 is no survivor's
    s_tile[tid] = make_uint2((unsigned)e, (unsigned)(e >> 32));
    __syncthreads();
#pragma unroll 16
    for (int j = 0; j < 64; ++j) {
      const unsigned k = part[j].y;
      gt += k > mh ? 1 : 0;
      eq += k == mh ? 1 : 0;
    }
  }
  __syncthreads();
  s_part[tid] = eq;
  __syncthreads();
  const int holders = s_part[lane] + s_part[64 + lane] + s_part[128 + lane] + s_part[192 + lane];      // itself included
  if (__syncthreads_or(i < n && holders > 1)) {
    for (int j0 = 0; j0 < n; j0 += WG) {
      __syncthreads();
      const unsigned long long e = j0 + tid < n ? surv[j0 + tid] : 0ull;
      s_tile[tid] = make_uint2((unsigned)e, (unsigned)(e >> 32));
      __syncthreads();
#pragma unroll 16
      for (int j = 0; j < 64; ++j) gt += ((part[j].y == mh) & (part[j].x > ml)) ? 1 : 0;      // a greater ~index: a lower index
    }
  }
  __syncthreads();
  s_part[tid] = gt;
  __syncthreads();
  if (wave == 0 && i < n) {
    const int rank = s_part[lane] + s_part[64 + lane] + s_part[128 + lane] + s_part[192 + lane];
    a.sel[(size_t)b * a.p.cap + rank] = (int)(0xffffffffu - ml);
  }
}

__global__ __launch_bounds__(WG) void gather_kernel(const Args a) {
  __shared__ int s_h[BINS], s_o[3];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n = resolve(a.hist + (size_t)b * LEVELS * BINS, a.p.cap, 0, s_h, s_o).total;
  const int s = blockIdx.x * WG + tid;
  const size_t slot = (size_t)b * a.p.cap + s;
  const bool in = s < a.p.cap, live = s < n;
  if (in) a.order[slot] = (long long)slot;
  if (s == 0) a.thresh[b] = a.p.nms_thr;
  bool pass = false;
  int anchor = -1;
  if (live) {
    anchor = a.sel[slot];
    if ((unsigned)anchor >= (unsigned)a.p.N) anchor = 0;     // never taken: rank_kernel wrote a permutation of the survivors
    const size_t HW = (size_t)a.p.HW;
    const size_t cell = (size_t)(anchor / a.p.A), an = (size_t)(anchor % a.p.A);
    float best, t[7], an7[7];
    int label;
    anchor_best(a.cls + ((size_t)b * a.p.A + an) * a.p.C * HW + cell, HW, a.p.C, best, label);
    const float sc = sigmoid(best);
    const float* dr = a.dirp + ((size_t)b * a.p.A + an) * 2 * HW + cell;
    a.dir[slot] = dr[HW] > dr[0] ? 1 : 0;
    const float* bp = a.bbox + ((size_t)b * a.p.A + an) * 7 * HW + cell;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      t[j] = bp[(size_t)j * HW];
      an7[j] = a.anchors[(size_t)anchor * 7 + j];
    }
    float o7[7], o5[5];
    decode(an7, t, o7, o5);
#pragma unroll
    for (int j = 0; j < 7; ++j) a.box7[slot * 7 + j] = o7[j];
#pragma unroll
    for (int j = 0; j < 5; ++j) a.bev5[slot * 5 + j] = o5[j];
    a.score[slot] = sc;
    a.label[slot] = label;
    pass = sc > a.p.score_thr;
  }
  if (in && a.cand_inds != nullptr) a.cand_inds[slot] = (long long)anchor;
  const unsigned long long m = __ballot(pass);
  if (m != 0 && lane == __ffsll((long long)m) - 1) atomicAdd(&a.cnt[b], __popcll(m));
}

__global__ __launch_bounds__(WG) void finish_kernel(const Args a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = a.p.M, C = a.p.C;
  int off = 0, total = 0;
  for (int g = 0; g < a.p.B; ++g) {        // the exclusive scan of the B row counts: B is small, every thread takes it
    const int m = rows_of(a.num_keep[g], M);
    off += g < b && m > 0 ? m : 0;
    total += m > 0 ? m : 0;
  }
  const int m = rows_of(a.num_keep[b], M);
  if (tid == 0) {
    a.batch_cnt[b] = m;
    if (a.cand_cnt != nullptr) a.cand_cnt[b] = a.cnt[b] < a.p.cap ? a.cnt[b] : a.p.cap;
  }
  const size_t HW = (size_t)a.p.HW;
  for (int r = tid; r < m; r += WG) {
    const size_t slot = (size_t)a.keep[(size_t)b * a.p.cap + r];     // b cap + the candidate's place in the selection order
    const size_t row = (size_t)off + r;
    int anchor = a.sel[slot];
    if ((unsigned)anchor >= (unsigned)a.p.N) anchor = 0;
    const size_t cell = (size_t)(anchor / a.p.A), an = (size_t)(anchor % a.p.A);
    float o[7];
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = a.box7[slot * 7 + j];
    o[6] = dir_fix(a.box7[slot * 7 + 6], a.dir[slot], a.p.dir_offset, a.p.dir_limit_offset);
    a.rois[row * 8] = (float)b;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      a.boxes_3d[row * 7 + j] = o[j];
      a.rois[row * 8 + 1 + j] = o[j];
    }
    a.scores_3d[row] = a.score[slot];
    a.labels_3d[row] = a.label[slot];
    const float* cls = a.cls + ((size_t)b * a.p.A + an) * C * HW + cell;
    for (int c = 0; c < C; ++c) a.cls_preds[row * C + c] = sigmoid(cls[(size_t)c * HW]);
  }
  // the rows past the counts' sum, dealt round the B workgroups
  for (long long row = (long long)total + b + (long long)tid * a.p.B; row < (long long)a.p.B * M; row += (long long)WG * a.p.B) {
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      a.boxes_3d[row * 7 + j] = 0.0f;
      a.rois[row * 8 + 1 + j] = 0.0f;
    }
    a.rois[row * 8] = -1.0f;
    a.scores_3d[row] = 0.0f;
    a.labels_3d[row] = -1;
    for (int c = 0; c < C; ++c) a.cls_preds[row * C + c] = 0.0f;
  }
}

}  // namespace rpn_proposal

using namespace rpn_proposal;

extern "C" {

size_t gd3d_rpn_proposal_workspace_bytes(int32_t B, int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre) {
  Args a;
  if (check_args(B, A, C, H, W, nms_pre, 1, 1, 0.0f, 0.0f, 1, 0.0f, 0.0f, a.p) != 0) return 0;
  return carve(a, nullptr, rnms_batched_workspace_bytes(a.p.B, a.p.cap)).bytes;
}

int gd3d_rpn_proposals(const float* cls_score, const float* bbox_pred, const float* dir_cls_pred, const float* anchors, int32_t B,
                       int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num, float nms_thr,
                       float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset, float* boxes_3d,
                       float* scores_3d, int64_t* labels_3d, float* cls_preds, float* rois, int32_t* batch_cnt, int64_t* cand_inds,
                       int32_t* cand_cnt, void* workspace, size_t workspace_bytes, void* stream) {
  Args a;
  int rc = check_args(B, A, C, H, W, nms_pre, nms_post, max_num, nms_thr, score_thr, use_rotate_nms, dir_offset, dir_limit_offset, a.p);
  if (rc != 0) return rc;
  if (cls_score == nullptr || bbox_pred == nullptr || dir_cls_pred == nullptr || anchors == nullptr || boxes_3d == nullptr ||
      scores_3d == nullptr || labels_3d == nullptr || cls_preds == nullptr || rois == nullptr || batch_cnt == nullptr ||
      workspace == nullptr)
    return GD3D_E_BADARG;
  const Carved w = carve(a, workspace, rnms_batched_workspace_bytes(a.p.B, a.p.cap));
  if (workspace_bytes < w.bytes) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  a.cls = cls_score;
  a.bbox = bbox_pred;
  a.dirp = dir_cls_pred;
  a.anchors = anchors;
  a.boxes_3d = boxes_3d;
  a.scores_3d = scores_3d;
  a.labels_3d = (long long*)labels_3d;
  a.cls_preds = cls_preds;
  a.rois = rois;
  a.batch_cnt = batch_cnt;
  a.cand_inds = (long long*)cand_inds;
  a.cand_cnt = cand_cnt;
  rc = gd3d::fill_words(a.hist, w.zero_bytes, 0u, s);
  if (rc != 0) return rc;
  const dim3 wg(WG), ranks((unsigned)((a.p.cap + RANK_I - 1) / RANK_I), (unsigned)B), cells((unsigned)((a.p.HW + WG - 1) / WG), (unsigned)B), spans((unsigned)a.nblk, (unsigned)B),
      cands((unsigned)((a.p.cap + WG - 1) / WG), (unsigned)B);
  hipLaunchKernelGGL(key_kernel, cells, wg, 0, s, a);
  for (int level = 1; level < LEVELS; ++level) hipLaunchKernelGGL(hist_kernel, spans, wg, 0, s, a, level);
  hipLaunchKernelGGL(compact_kernel, spans, wg, 0, s, a);
  hipLaunchKernelGGL(tie_kernel, spans, wg, 0, s, a);
  hipLaunchKernelGGL(rank_kernel, ranks, wg, 0, s, a);
  hipLaunchKernelGGL(gather_kernel, cands, wg, 0, s, a);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  rc = rnms_batched(a.p.rotate ? 0 : 1, a.bev5, (const int64_t*)a.order, a.cnt, B, a.p.cap, a.thresh, (int64_t*)a.keep,
                    (int64_t*)a.num_keep, w.nms, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)B), wg, 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
