// rbox_nms_common.h — what the NMS stages (rbox_rank.h, rbox_mask.h, rbox_scan.h) and rbox.hip's host code share; no kernel here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rbox_device.h"

namespace rbox {
enum { MODE_ROT = 0, MODE_NORMAL = 1, MODE_CIRCLE = 2 };

// One launch serves G independent NMS problems ("groups": classes, samples, tasks) over a shared box array:
// group g owns order[g*cap .. g*cap + n_g), n_g = counts[g] read ON THE DEVICE (no host sync to size the launch;
// grids are sized for `cap` and surplus workgroups leave after one scalar load).  G = 1 with counts == NULL is the plain call.
struct NmsArgs {
  const float* boxes;          // (N,5) [x1,y1,x2,y2,r]; MODE_CIRCLE: (N,2) centres
  const long long* order;      // (G, cap) score order per group (indices into boxes); NULL (G = 1 only): identity
  const int* counts;           // (G) device, nullable
  const float* thresh_dev;     // (G) device, nullable -> thresh / thresh_d
  int n, cap, cbs, rows;       // cbs = ceil(cap / 64): mask row stride in words
  float thresh;
  double thresh_d;             // MODE_CIRCLE: numba compares the float32 distance with a float64 threshold
};

__device__ __forceinline__ int group_n(const NmsArgs& a, int g) {
  if (a.counts == nullptr) return a.n;
  const int c = a.counts[g];
  return c < 0 ? 0 : (c > a.cap ? a.cap : c);
}

// Victim lists of the LIST scan (round 5; one group of known size, n <= LIST_MAX_N: nms_list_body, rbox_scan.h).  Per box i two lists of
// 16-bit ids of boxes of LATER 64-blocks whose IoU with i exceeds the threshold, in any order, with a counter each (nothing is
// initialised but the counters; readers mask by the count):
//   near list: victims in the next LIST_K blocks (<= LIST_NEAR entries): marked by the scan's resolver wave itself;
//   far list : victims beyond (<= LIST_FAR entries): marked by helper waves.
constexpr int LIST_K = 8;   // (measured, scan kernel: n = 4096 thr 0.25: 17.9 / 16.5 / 16.2 / 16.4 us at 4 / 6 / 8 / 12; n = 9000 thr 0.7: 30.7 / 29.7 / 28.8 at 4 / 8 / 12)
constexpr int LIST_NEAR = 16;
constexpr int LIST_FAR = 64;
constexpr unsigned LIST_MAX_N = 16384;          // the list scan keeps one state BYTE per box in LDS
constexpr unsigned short LIST_DUMMY = 0x4040u;  // first of 64 scratch state bytes (never boxes), four bytes apart, one per lane
struct QueueArgs {
  unsigned* queue;   // (G, QUEUE_SHARDS, scap)
  unsigned* ctl;     // (G, CTL_WORDS): [s * CTL_STRIDE] entries reserved in shard s (may exceed scap); [QUEUE_SHARDS * CTL_STRIDE] overflowed block pairs
  unsigned* ovl;     // (G, npairs) overflowed block pair ids
  unsigned scap, npairs;   // scap: entries per shard
  unsigned short* lists;   // per group: (cap, LIST_NEAR) near lists, then (cap, LIST_FAR) far lists — or nullptr: no lists wanted
  unsigned* lcnt;          // per group a block of `lblock` words: (cap, 2) entries appended per box to its near / far list (may exceed the
                           // capacity: the list is then incomplete), then the group's FAILURE WORD (+ padding): set when the lists cannot
                           // be used — a full list, or block pairs that went to the overflow list
  unsigned lblock;
};
__device__ __forceinline__ unsigned* list_counts(const QueueArgs& q, int g) { return q.lcnt + (size_t)g * q.lblock; }
__device__ __forceinline__ unsigned* list_fail(const QueueArgs& q, const NmsArgs&, int g) { return list_counts(q, g) + (q.lblock - 64u); }

// one more entry of box i's near or far victim list (j: a box of a LATER 64-block that i suppresses if i is kept); `pos` from the
// counter (the caller's atomicAdd: per pair, or wave-aggregated)
__device__ __forceinline__ void list_put(const QueueArgs& q, const NmsArgs& a, int g, int i, int j, bool far, unsigned pos) {
  unsigned short* const glists = q.lists + (size_t)g * a.cap * (LIST_NEAR + LIST_FAR);
  if (far) {
    if (pos < (unsigned)LIST_FAR) glists[(size_t)a.cap * LIST_NEAR + (size_t)i * LIST_FAR + pos] = (unsigned short)j;
    else *list_fail(q, a, g) = 1u;   // the list is incomplete: the list scan must not run (the classic scan does)
  } else {
    if (pos < (unsigned)LIST_NEAR) glists[(size_t)i * LIST_NEAR + pos] = (unsigned short)j;
    else *list_fail(q, a, g) = 1u;
  }
}

constexpr unsigned QUEUE_SENTINEL = 0xffffffffu;   // (65535, 65535): never a queued pair (i < j)
// The queue is cut into QUEUE_SHARDS sub-queues (block pair p appends to shard p % QUEUE_SHARDS), each with its own counter in
// its own 128-byte line: returning atomics on ONE word saturate at ~88 per us on this chip (MI355X_MICROARCH.md, "dequeue"), and
// the 2080 appends of an n = 4096 call through one counter cost 24 us — more than the clipping they were meant to feed.
constexpr unsigned QUEUE_SHARDS = 64;
constexpr unsigned CTL_STRIDE = 32;                                  // words: one 128-byte line per counter
constexpr unsigned CTL_WORDS = (QUEUE_SHARDS + 1) * CTL_STRIDE;      // per group: shard counters, then the overflow counter

// block pair index of the upper triangle (row-major over row blocks) -> (row block rb, column block c >= rb)
__device__ __forceinline__ void pair_blocks(unsigned pair, int cb, int& rb, int& c) {
  rb = (int)((2.0f * cb + 1.0f - sqrtf((2.0f * cb + 1.0f) * (2.0f * cb + 1.0f) - 8.0f * (float)pair)) * 0.5f);
  rb = max(0, min(rb, cb - 1));
  while (rb > 0 && (unsigned)(rb * cb - rb * (rb - 1) / 2) > pair) --rb;
  while ((unsigned)((rb + 1) * cb - (rb + 1) * rb / 2) <= pair) ++rb;
  c = rb + (int)(pair - (unsigned)(rb * cb - rb * (rb - 1) / 2));
}

// Two-level form (win.gremv != nullptr; n > 8448): the box range is cut into super-blocks of SCAN_SB 64-box blocks.  One
// launch of nms_scan_kernel (rbox_scan.h) resolves ONE super-block [c_begin, c_end): its removed-set starts from the global words gremv
// (what earlier super-blocks suppressed), rows are propagated only to words inside the super-block (<= SCAN_SB words per
// row: short loads, one chunk), the kept words of its blocks go to gkept, the running keep count lives in num_keep.
// nms_propagate_kernel then ORs the kept rows into gremv for all words right of the super-block with the whole chip.
struct ScanWindow {
  int c_begin, c_end;               // blocks; c_end is clamped to the group's block count
  unsigned long long* gremv;        // (G, cbs) global removed-set, nullptr = single-level scan over all blocks
  unsigned long long* gkept;        // (G, cbs) kept word per block
  long long* gcount;                // (G) running keep count between the launches of a two-level scan
};
}  // namespace rbox
