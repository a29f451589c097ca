// rbox_mask.h — NMS stage 2 (rbox.hip's head comment): the four kernels that build the suppression mask and the victim lists.
#pragma once
#include "rbox_nms_common.h"

namespace rbox {
// Axis-aligned and circle NMS (cheap predicates, no polygon scratch): one WAVE per (row box i, 64-box column block
// c >= block of i): lane l tests box i against box 64c + l and the wave-wide ballot IS the 64-bit mask word — no partial
// words, no barrier.  A wave walks `rows` (1, 2, 4 or 8; host-chosen) consecutive row boxes against the same 64 column
// boxes (loaded once): 1 keeps small problems latency-short, 8 keeps large ones from being workgroup-dispatch bound;
// blockIdx.x = (upper-triangle block pair) * (64 / rows) + row group; blockIdx.y = group.
// On a DIAGONAL block the lanes left of the row box are not idle: lane j < i evaluates the same predicate with the
// operands in greedy order (box j first, box i second — bit for bit what row j's wave computes for its lane i), so the
// ballot also yields "which earlier boxes of my block suppress box i".  That word goes to colm[i]; the scan resolves a
// 64-box block from these column words in a few wave-parallel steps instead of one scalar step per kept box.
// (Rotated boxes went through this kernel too until the compacted form below replaced it: n = 4096 99 -> 29 us,
// n = 9000 293 -> 97 us, n = 1000 25 -> 21 us, same mask bits.)
template <int MODE>
__global__ __launch_bounds__(64) void nms_mask_kernel(const NmsArgs a, const OBox* __restrict__ ob_,
                                                      unsigned long long* __restrict__ mask_,
                                                      unsigned long long* __restrict__ colm_, const QueueArgs q) {
  static_assert(MODE == MODE_NORMAL || MODE == MODE_CIRCLE, "rotated boxes: nms_mask_compact_kernel");
  const int lane = threadIdx.x;
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  const int cb = (n + 63) >> 6;
  const int rows = a.rows;
  const int groups = 64 / rows;
  const unsigned pair = blockIdx.x / groups;
  if (pair >= (unsigned)(cb * (cb + 1) / 2)) return;  // grid is sized for `cap`
  const int r0 = (int)(blockIdx.x % groups) * rows;
  const long long* order = a.order != nullptr ? a.order + (size_t)g * a.cap : nullptr;
  unsigned long long* mask = mask_ + (size_t)g * a.cap * a.cbs;
  const float thresh = a.thresh_dev != nullptr ? a.thresh_dev[g] : a.thresh;
  const double thresh_d = a.thresh_dev != nullptr ? (double)a.thresh_dev[g] : a.thresh_d;
  // pair -> (rb, c): pairs before row block rb: rb*cb - rb(rb-1)/2
  int rb = (int)((2.0f * cb + 1.0f - sqrtf((2.0f * cb + 1.0f) * (2.0f * cb + 1.0f) - 8.0f * (float)pair)) * 0.5f);
  rb = max(0, min(rb, cb - 1));
  while (rb > 0 && (unsigned)(rb * cb - rb * (rb - 1) / 2) > pair) --rb;
  while ((unsigned)((rb + 1) * cb - (rb + 1) * rb / 2) <= pair) ++rb;
  const int c = rb + (int)(pair - (unsigned)(rb * cb - rb * (rb - 1) / 2));
  const int j = c * 64 + lane;
  float braw[5];
  if (j < n) {
    const size_t sj = order != nullptr ? (size_t)order[j] : (size_t)j;
    if constexpr (MODE == MODE_NORMAL) {
#pragma unroll
      for (int k = 0; k < 5; ++k) braw[k] = a.boxes[sj * 5 + k];
    } else {
      braw[0] = a.boxes[sj * 2];
      braw[1] = a.boxes[sj * 2 + 1];
    }
  }
  unsigned hits = 0u;   // bit r: this lane's box is a hit of row r (rows <= 8)
  int total = 0;        // lane r: hits of row r
  for (int r = 0; r < rows; ++r) {
    const int i = rb * 64 + r0 + r;  // wave-uniform
    if (i >= n) break;
    const bool act = j < n && j != i;   // (off-diagonal blocks: j > i always)
    const bool low = j < i;             // diagonal block only: lane box precedes the row box -> it goes first
    bool hit = false;
    if constexpr (MODE == MODE_NORMAL) {
      if (act) {
        const size_t si = order != nullptr ? (size_t)order[i] : (size_t)i;
        float ar[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) ar[k] = a.boxes[si * 5 + k];
        hit = (low ? iou_normal(braw, ar) : iou_normal(ar, braw)) > thresh;
      }
    } else {
      if (act) {  // mmdet3d circle_nms: dist = (x_i - x_j)^2 + (y_i - y_j)^2 ; suppressed iff dist <= thresh
        const size_t si = order != nullptr ? (size_t)order[i] : (size_t)i;
        const float xi = a.boxes[si * 2], yi = a.boxes[si * 2 + 1];
        const float dx = low ? braw[0] - xi : xi - braw[0], dy = low ? braw[1] - yi : yi - braw[1];
        const float dist = dx * dx + dy * dy;
        hit = (double)dist <= thresh_d;
      }
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) {
      if (rb == c) {
        const int il = i & 63;
        const unsigned long long below = (1ull << il) - 1ull;
        mask[(size_t)i * a.cbs + c] = word & ~(below | (1ull << il));
        colm_[(size_t)g * a.cap + i] = word & below;
      } else {
        mask[(size_t)i * a.cbs + c] = word;
      }
    }
    // the list scan's victim lists: remembered per row (bit r of `hits`, the row's hit count in lane r), appended after the loop
    if (r < 8) {
      hits |= hit ? (1u << r) : 0u;
      if (lane == r) total = __popcll(word);
    }
  }
  // the list scan's victim lists (q.lists: counters and failure word were zeroed before this kernel): the hits of a LATER block go
  // to the row boxes' near or far lists.  ONE returning atomic for all of the wave's rows (lane r reserves row r's entries): a
  // counter update per row inside the loop above put a memory round trip between the rows (20 -> 25 us at n = 4096)
  if (q.lists != nullptr && rb != c) {   // uniform
    const bool far = c - rb > LIST_K;
    const int irow = rb * 64 + r0 + lane;   // lane r: row r of this wave
    unsigned base = 0u;
    if (lane < min(rows, 8) && total > 0) base = atomicAdd(&list_counts(q, g)[2 * irow + (far ? 1 : 0)], (unsigned)total);
    if (__ballot(hits != 0u) != 0ull) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (r < rows) {
          const unsigned long long word = __ballot((hits >> r) & 1u);
          const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)base, r);
          if ((hits >> r) & 1u) list_put(q, a, g, rb * 64 + r0 + r, j, far, b + (unsigned)__popcll(word & ((1ull << lane) - 1ull)));
        }
      }
    }
  }
}

// Rotated mode, compacted: the same mask words, with the expensive lanes packed densely.
// In nms_mask_kernel a wave pays a whole polygon-clipping pass whenever ANY of its 64 lanes survives the bounding-circle
// test; on score-sorted detector output ~1 % of the pairs do, i.e. about every second (row, 64 columns) wave runs a pass
// with one or two live lanes.  Here a wave owns `rows` (8..64) consecutive row boxes x one 64-box column block and works
// in two phases per 16-row chunk:
//   1. the circle test alone for every (row, lane) pair (~12 VALU per row, straight-line; the row boxes' centre / extent
//      are broadcast from lanes by v_readlane): every lane keeps the 16-bit candidate mask of ITS column, the survivors
//      are then appended to an LDS queue as (row << 6 | column) in bulk (DPP scan of the per-lane counts);
//   2. whenever >= 64 candidates are queued (and once more at the end) lane l takes candidate l: loads both 64-byte
//      records, runs the FULL predicate (iou_bev, which repeats the circle test — one code path, bit-identical
//      decisions) and ORs its bit into the row's word in LDS.  Every clipping pass but the last has 64 live lanes.
// The circle test is symmetric in its operands (squared differences, commutative sums), so on a DIAGONAL block it also
// selects the (earlier box, row box) pairs that are evaluated in greedy operand order for colm[] — as in the plain kernel.
// A pair that fails the circle test has overlap exactly 0 and IoU +0, which is "> thresh" only for thresh < 0: for such a
// threshold (or a NaN one) every valid pair is queued, so the result stays that of the plain kernel.
constexpr int CQ_ROWS = 16;                 // rows per chunk between drains (<= 32: one bit per row in a lane's mask)
constexpr int CQ_CAP = CQ_ROWS * 64 + 64;   // worst case of one chunk + the carried remainder (< 64)

struct CompactLds {
  VertexScratch<64> vs;
  unsigned short queue[CQ_CAP];
  unsigned long long words[64];
};

// one wave: `rows` row boxes (from row r0 of row block rb) x column block c of group g -> final mask words (and colm on a
// diagonal block).  The whole job of nms_mask_compact_kernel for one workgroup; also the overflow path of the queued form.
__device__ __forceinline__ void compact_pair(const NmsArgs& a, const OBox* __restrict__ ob, unsigned long long* __restrict__ mask,
                                             unsigned long long* __restrict__ colm, int n, int rb, int c, int r0, int rows,
                                             float thresh, CompactLds& L) {
  VertexScratch<64>& vs = L.vs;
  unsigned short* const queue = L.queue;
  unsigned long long* const words = L.words;
  const int lane = threadIdx.x & 63;
  const bool all_pairs = !(thresh >= 0.0f);
  const int i0 = rb * 64 + r0;  // first row box of this wave
  if (i0 >= n) return;
  const int nrows = min(rows, n - i0);
  const int j = c * 64 + lane;
  const bool jv = j < n;
  float bcx = 0.0f, bcy = 0.0f, bext = 0.0f;
  if (jv) {
    const OBox& B = ob[j];
    bcx = B.cx;
    bcy = B.cy;
    bext = fabsf(B.x2 - B.x1) + fabsf(B.y2 - B.y1);
  }
  // lane r also holds row box i0 + r's centre / extent: the row loop reads them with v_readlane instead of one
  // dependent scalar-load round trip per row (64 rows x ~500 cycles was most of phase 1)
  float rcx = 0.0f, rcy = 0.0f, rext = 0.0f;
  if (lane < nrows) {
    const OBox& R = ob[i0 + lane];
    rcx = R.cx;
    rcy = R.cy;
    rext = fabsf(R.x2 - R.x1) + fabsf(R.y2 - R.y1);
  }
  words[lane] = 0ull;
  __syncthreads();
  int qn = 0;  // queued candidates (wave-uniform)
  for (int rbase = 0; rbase < nrows; rbase += CQ_ROWS) {
    const int rend = min(rbase + CQ_ROWS, nrows);
    // circle tests of the chunk, straight-line: lane l (column box j) tests itself against the chunk's 16 row boxes
    // (centre / extent broadcast by v_readlane) and keeps ITS OWN 16-bit candidate mask — no ballot, no branch, no LDS
    // in the loop, rows independent of each other.  (A per-row ballot + divergent queue append ran at ~310 cycles per
    // row for a lone wave — mixed SALU/VALU dependencies and three branches per row — half of a wave's life.)
    unsigned colbits = 0u;
    const int jdiag = j - i0 - rbase;  // lane's column box IS row box (rbase + k)  <=>  k == jdiag
#pragma unroll
    for (int k = 0; k < CQ_ROWS; ++k) {
      const int r = rbase + k;  // < 64 always; rows >= nrows are masked off below
      const float acx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rcx), r));
      const float acy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rcy), r));
      const float aext = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rext), r));
      // box_overlap's early-out, same operations (it is symmetric in the two boxes)
      const float ddx = acx - bcx, ddy = acy - bcy;
      const float reach = 0.5f * (aext + bext) + 1e-2f;
      const bool near = !(ddx * ddx + ddy * ddy > reach * reach * 1.0001f);
      colbits |= (near && k != jdiag) ? (1u << k) : 0u;
    }
    if (all_pairs) colbits = ~(jdiag >= 0 && jdiag < CQ_ROWS ? (1u << jdiag) : 0u);
    colbits &= (rend - rbase >= 32) ? 0xffffffffu : ((1u << (rend - rbase)) - 1u);
    if (!jv) colbits = 0u;
    // queue append in bulk: inclusive scan of the 64 per-lane counts on the DPP network, then every lane walks the set
    // bits of its own mask (a handful at detector densities)
    const int cntl = __popc(colbits);
    int incl = cntl;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);   // row_shr:1 (out-of-row reads 0)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);   // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);   // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);   // row_shr:8
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    {
      unsigned w = colbits;
      int pos = qn + incl - cntl;
      while (w != 0u) {
        const int k = __builtin_ctz(w);
        w &= w - 1u;
        queue[pos++] = (unsigned short)(((rbase + k) << 6) | lane);
      }
    }
    qn += __builtin_amdgcn_readlane(incl, 63);
    __syncthreads();
    const bool last = rend >= nrows;
    int done = 0;
    while (qn - done >= 64 || (last && done < qn)) {
      const int q = done + lane;
      if (q < qn) {
        const int e = queue[q];
        const int r = e >> 6, jl = e & 63;
        const int i = i0 + r, jj = c * 64 + jl;
        const OBox A = ob[i];
        const OBox B = ob[jj];
        const bool low = jj < i;  // diagonal block only: the lane's box precedes the row box -> it goes first
        const OBox F = low ? B : A, S = low ? A : B;
        const bool hit = iou_bev<64>(F, S, vs, lane) > thresh;
        if (hit) atomicOr(&words[r], 1ull << jl);
      }
      done += 64;
    }
    if (!last && done > 0) {  // carry the < 64 leftover candidates to the front of the queue
      const int rem = qn - done;
      unsigned short v = 0;
      if (lane < rem) v = queue[done + lane];
      __syncthreads();
      if (lane < rem) queue[lane] = v;
      qn = rem;
    }
    __syncthreads();
  }
  if (lane < nrows) {
    const int i = i0 + lane;
    const unsigned long long word = words[lane];
    if (rb == c) {
      const int il = i & 63;
      const unsigned long long below = (1ull << il) - 1ull;
      mask[(size_t)i * a.cbs + c] = word & ~(below | (1ull << il));
      colm[i] = word & below;
    } else {
      mask[(size_t)i * a.cbs + c] = word;
    }
  }
}

__global__ __launch_bounds__(64) void nms_mask_compact_kernel(const NmsArgs a, const OBox* __restrict__ ob_,
                                                              unsigned long long* __restrict__ mask_,
                                                              unsigned long long* __restrict__ colm_) {
  __shared__ CompactLds L;
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  const int cb = (n + 63) >> 6;
  const int rows = a.rows;
  const int groups = 64 / rows;
  const unsigned pair = blockIdx.x / groups;
  if (pair >= (unsigned)(cb * (cb + 1) / 2)) return;  // grid is sized for `cap`
  int rb, c;
  pair_blocks(pair, cb, rb, c);
  const float thresh = a.thresh_dev != nullptr ? a.thresh_dev[g] : a.thresh;
  compact_pair(a, ob_ + (size_t)g * a.cap, mask_ + (size_t)g * a.cap * a.cbs, colm_ + (size_t)g * a.cap, n, rb, c,
               (int)(blockIdx.x % groups) * rows, rows, thresh, L);
}

// ---- Rotated mode, QUEUED (round 4): circle test and clipping as two kernels, every clipping pass full. -----------------------
// In the compacted kernel above every wave ends with one partly filled clipping pass (~1 % of a 64 x 64 block pair's 4096
// pairs survive the circle test: ~41 live lanes of 64) and the kernel lasts as long as its slowest waves (pairs with > 64
// survivors run two passes, the diagonal blocks evaluate every pair twice): profiles/r04_nms_pmc.txt.  Here
//   nms_circle_queue_kernel  one wave per block pair: zeroes the pair's mask words, runs ONLY the circle tests and appends the
//                            survivors (i << 16 | j, i < j) to a per-group queue in HBM (one wave-aggregated atomicAdd);
//                            a diagonal block queues every unordered pair ONCE (the compacted kernel evaluates it twice,
//                            as row i / lane j and as row j / lane i, with the same operand order and the same result);
//   nms_clip_queue_kernel    a fixed grid of waves walks the queue 64 entries at a time: lane l evaluates entry l with the
//                            full predicate and ORs its bit into mask[i][j / 64] — and, inside a diagonal block, into
//                            colm[j] as well (integer atomics: the words are the same whatever the order).
// Same predicate, same operand order (earlier box first), same bits.  A wave whose survivors do not fit the queue
// (128 entries per box over 64 shards; only pathological clouds get there) records its block pair instead and the clip kernel runs
// compact_pair() on it afterwards.
__global__ __launch_bounds__(64) void nms_circle_queue_kernel(const NmsArgs a, const OBox* __restrict__ ob_,
                                                              unsigned long long* __restrict__ mask_,
                                                              unsigned long long* __restrict__ colm_, const QueueArgs q) {
  const int lane = threadIdx.x;
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  const int cb = (n + 63) >> 6;
  const unsigned pair = blockIdx.x;
  if (pair >= (unsigned)(cb * (cb + 1) / 2)) return;  // grid is sized for `cap`
  int rb, c;
  pair_blocks(pair, cb, rb, c);
  const OBox* ob = ob_ + (size_t)g * a.cap;
  unsigned long long* mask = mask_ + (size_t)g * a.cap * a.cbs;
  const int i0 = rb * 64;
  const int nrows = min(64, n - i0);
  const int j = c * 64 + lane;
  const bool jv = j < n;
  float bcx = 0.0f, bcy = 0.0f, bext = 0.0f;
  if (jv) {
    const OBox& B = ob[j];
    bcx = B.cx;
    bcy = B.cy;
    bext = fabsf(B.x2 - B.x1) + fabsf(B.y2 - B.y1);
  }
  float rcx = 0.0f, rcy = 0.0f, rext = 0.0f;
  if (lane < nrows) {
    const OBox& R = ob[i0 + lane];
    rcx = R.cx;
    rcy = R.cy;
    rext = fabsf(R.x2 - R.x1) + fabsf(R.y2 - R.y1);
    mask[(size_t)(i0 + lane) * a.cbs + c] = 0ull;                 // the clip kernel ORs into these
    if (rb == c) {
      colm_[(size_t)g * a.cap + i0 + lane] = 0ull;
      if (q.lists != nullptr)   // the list scan's victim lists of this box: empty (the clip kernel appends)
        reinterpret_cast<uint2*>(list_counts(q, g))[i0 + lane] = make_uint2(0u, 0u);
    }
  }
  if (q.lists != nullptr && pair == 0 && lane == 0) *list_fail(q, a, g) = 0u;
  // circle tests, straight-line: lane l (column box j) against the 64 row boxes; bit r of `cand` = the pair (row i0 + r, column j)
  // survives.  On the diagonal block only the pairs with the column box AFTER the row box.  TWO ROWS PER INSTRUCTION (float2 ->
  // v_pk_add / v_pk_mul: the same IEEE operations per component as box_overlap's early-out, in its order), and the mask built by
  // shifting the compare's result in as a carry (w = w + w + carry: one instruction per row; rows descend so that row r ends in
  // bit r).  Left to itself the compiler packed the x / y components of ONE row and repacked between rows: 953 VALU instructions
  // per wave, more than the clipping kernel's 693 (profiles/r05_nms_pmc_counters.txt).
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 bcx2 = {bcx, bcx}, bcy2 = {bcy, bcy}, bext2 = {bext, bext};
  auto shift_in = [](unsigned w, unsigned long long carry) -> unsigned {
    unsigned out;
    unsigned long long co;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(out), "=s"(co) : "v"(w), "s"(carry));
    return out;
  };
  // the row boxes' (cx, cy, extent) go through LDS, laid out per PAIR of rows as the packed operands want them — [cx of row r + 1,
  // cx of row r, cy.., cy.., ext.., ext..] — and come back as broadcast reads (a uniform address: 2 LDS instructions per row pair
  // instead of 6 v_readlane, which are vector instructions: a quarter of the loop's)
  __shared__ __attribute__((aligned(16))) float srow[32][8];
  {
    float* const mypair = &srow[lane >> 1][1 - (lane & 1)];   // odd rows first
    mypair[0] = rcx;
    mypair[2] = rcy;
    mypair[4] = rext;
  }
  __syncthreads();
  unsigned wlo = 0u, whi = 0u;
#pragma unroll
  for (int r = 62; r >= 0; r -= 2) {   // rows r + 1 and r
    const float4 xy = *reinterpret_cast<const float4*>(&srow[r >> 1][0]);
    const float2 ex = *reinterpret_cast<const float2*>(&srow[r >> 1][4]);
    const f2 acx = {xy.x, xy.y}, acy = {xy.z, xy.w}, aext = {ex.x, ex.y};
    const f2 ddx = acx - bcx2, ddy = acy - bcy2;   // box_overlap's early-out, same operations (symmetric in the boxes)
    const f2 d2 = ddx * ddx + ddy * ddy;
    const f2 reach = 0.5f * (aext + bext2) + 1e-2f;
    const f2 lim = reach * reach * 1.0001f;
    const unsigned long long n1 = __ballot(!(d2.x > lim.x)), n0 = __ballot(!(d2.y > lim.y));
    if (r >= 32) {
      whi = shift_in(whi, n1);
      whi = shift_in(whi, n0);
    } else {
      wlo = shift_in(wlo, n1);
      wlo = shift_in(wlo, n0);
    }
  }
  unsigned long long cand = ((unsigned long long)whi << 32) | (unsigned long long)wlo;
  cand &= nrows >= 64 ? ~0ull : ((1ull << nrows) - 1ull);
  if (rb == c) cand &= (1ull << lane) - 1ull;        // rows r < lane only: i = i0 + r < j = i0 + lane
  if (!jv) cand = 0ull;
  const int cntl = __popcll(cand);
  int incl = cntl;
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);   // row_shr:1 (out-of-row reads 0)
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);   // row_shr:2
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);   // row_shr:4
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);   // row_shr:8
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  const int total = __builtin_amdgcn_readlane(incl, 63);
  unsigned* const ctl = q.ctl + (size_t)g * CTL_WORDS;
  unsigned* const novf = ctl + QUEUE_SHARDS * CTL_STRIDE;
  const float thresh = a.thresh_dev != nullptr ? a.thresh_dev[g] : a.thresh;
  if (!(thresh >= 0.0f)) {   // uniform: a negative or NaN threshold makes EVERY valid pair a candidate (IoU +0 > thresh):
    if (lane == 0) {   // compact_pair's all-pairs case
      const unsigned k = atomicAdd(novf, 1u);
      if (k < q.npairs) q.ovl[(size_t)g * q.npairs + k] = pair;
    }
    return;
  }
  if (total == 0) return;   // uniform
  const unsigned shard = pair % QUEUE_SHARDS;
  unsigned base = 0u;
  if (lane == 0) base = atomicAdd(&ctl[shard * CTL_STRIDE], (unsigned)total);
  base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
  unsigned* const queue = q.queue + ((size_t)g * QUEUE_SHARDS + shard) * q.scap;
  unsigned pos = base + (unsigned)(incl - cntl);
  if (base + (unsigned)total > q.scap) {   // uniform: does not fit -> this block pair goes to the overflow list,
    if (lane == 0) {   // what was reserved is voided
      const unsigned k = atomicAdd(novf, 1u);
      if (k < q.npairs) q.ovl[(size_t)g * q.npairs + k] = pair;
    }
    for (int k = 0; k < cntl; ++k, ++pos)
      if (pos < q.scap) queue[pos] = QUEUE_SENTINEL;
    return;
  }
  while (cand != 0ull) {
    const int r = __builtin_ctzll(cand);
    cand &= cand - 1ull;
    queue[pos++] = ((unsigned)(i0 + r) << 16) | (unsigned)j;
  }
}

__global__ __launch_bounds__(64) void nms_clip_queue_kernel(const NmsArgs a, const OBox* __restrict__ ob_,
                                                            unsigned long long* __restrict__ mask_,
                                                            unsigned long long* __restrict__ colm_, const QueueArgs q) {
  __shared__ CompactLds L;
  const int lane = threadIdx.x;
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  if (n == 0) return;
  const OBox* ob = ob_ + (size_t)g * a.cap;
  unsigned long long* mask = mask_ + (size_t)g * a.cap * a.cbs;
  unsigned long long* colm = colm_ + (size_t)g * a.cap;
  const float thresh = a.thresh_dev != nullptr ? a.thresh_dev[g] : a.thresh;
  const unsigned* const ctl = q.ctl + (size_t)g * CTL_WORDS;
  // wave w serves shard w % QUEUE_SHARDS (the grid is a multiple of QUEUE_SHARDS waves), every (grid / QUEUE_SHARDS)-th chunk of it
  const unsigned shard = blockIdx.x % QUEUE_SHARDS, per_shard = gridDim.x / QUEUE_SHARDS;
  // device-scope atomic loads: the counters were produced by the atomics of the previous kernel; a plain (scalar-cache) load of
  // a word that the same graph's previous replay also read is not guaranteed to be refetched
  const unsigned reserved = __hip_atomic_load(&ctl[shard * CTL_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned count = reserved < q.scap ? reserved : q.scap;
  const unsigned* const queue = q.queue + ((size_t)g * QUEUE_SHARDS + shard) * q.scap;
  for (unsigned b0 = (blockIdx.x / QUEUE_SHARDS) * 64u; b0 < count; b0 += per_shard * 64u) {   // uniform bounds
    const unsigned e = (b0 + lane < count) ? queue[b0 + lane] : QUEUE_SENTINEL;
    const int ei = (int)(e >> 16), ej = (int)(e & 0xffffu);
    if (e != QUEUE_SENTINEL && ei < ej && ej < n) {   // (the bounds cannot fail for an entry this call queued: they fence off garbage)
      const int i = ei, j = ej;   // i < j: the earlier box goes first, as in the greedy order
      const OBox A = ob[i];
      const OBox B = ob[j];
      if (iou_bev<64>(A, B, L.vs, lane) > thresh) {
        atomicOr(&mask[(size_t)i * a.cbs + (j >> 6)], 1ull << (j & 63));
        if ((i >> 6) == (j >> 6)) {
          atomicOr(&colm[j], 1ull << (i & 63));
        } else if (q.lists != nullptr) {   // i suppresses j of a later block: one more entry of i's near or far victim list
          const bool far = (j >> 6) - (i >> 6) > LIST_K;
          list_put(q, a, g, i, j, far, atomicAdd(&list_counts(q, g)[2 * i + (far ? 1 : 0)], 1u));
        }
      }
    }
  }
  unsigned novf = __hip_atomic_load(&ctl[QUEUE_SHARDS * CTL_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (novf == 0u) return;
  if (q.lists != nullptr && lane == 0) *list_fail(q, a, g) = 1u;   // pairs served by compact_pair() below write mask words only: no lists
  const int cb = (n + 63) >> 6;
  const unsigned npairs_now = (unsigned)(cb * (cb + 1) / 2);
  novf = novf < npairs_now ? novf : npairs_now;
  for (unsigned k = blockIdx.x; k < novf; k += gridDim.x) {   // block pairs that did not fit the queue: the compacted form
    const unsigned op = q.ovl[(size_t)g * q.npairs + k];
    if (op >= npairs_now) continue;   // (cannot happen for an entry this call recorded)
    int rb, c;
    pair_blocks(op, cb, rb, c);
    __syncthreads();
    compact_pair(a, ob, mask, colm, n, rb, c, 0, 64, thresh, L);
  }
}
}  // namespace rbox
