// rbox.hip — rotated BEV NMS and pairwise rotated IoU kernels for gfx950 + their C-ABI entry points
// (include/gd3d.h).  Geometry: rbox_device.h.  Compiled with -ffp-contract=off (see build.py).
//
// NMS (replaces mmdet3d iou3d_cuda.nms_gpu, whose mask goes D->H and is scanned on the host):
//   0. rbox_rank.h (nms_gpu path, <= 16384 candidates) rank_place_kernel: the score order by counting larger (score, -index) keys — no
//      sort — with the per-box prep scattered straight to its rank, one launch.
//   1. rbox_rank.h obox_prep_kernel (pre-sorted / caller-ordered paths): one thread per box: sin/cos + rotated corners once ->
//      64-byte OBox records.
//   2. rbox_mask.h nms_mask_compact_kernel (rotated) / nms_mask_kernel (axis-aligned, circle): one wave per (8..64 row boxes,
//      64-box column block at or right of their own block).  Rotated: the cheap bounding-circle test for every pair
//      first, survivors queued in LDS, then the full polygon-clipping predicate with the live lanes packed densely;
//      per-thread polygon vertices live in LDS [slot][thread] (12 KiB per wave).  VALU-throughput-bound integer+fp32
//      work (no HBM roofline: N=4096 reads 256 KB, writes 1 MB).
//      From 768 boxes on (rotated): the QUEUED form — nms_circle_queue_kernel (circle tests only, survivors to a queue in HBM) and
//      nms_clip_queue_kernel (the full predicate, every pass full), which also appends each positive pair of different blocks to the
//      earlier box's near / far VICTIM LIST.
//   3. rbox_scan.h the greedy scan, ONE 16-wave workgroup per group that never leaves the device:
//      nms_list_or_scan_kernel (groups of <= 16384 boxes): the LIST scan — one state byte per box in LDS, a resolver wave per block
//      (alive bytes -> in-block fixed point -> kept; marks the kept boxes' near victims through addresses from an LDS ring), twelve
//      helper waves (far victims, ring fill, kept ids); no mask rows, no barrier in the loop.  A full victim list makes the same
//      launch run the classic scan:
//      nms_scan_kernel (classic; also beyond 16384 boxes, two-level with nms_propagate_kernel): a resolver wave solves each block
//      from an LDS ring, three phase-shifted groups of row waves OR the mask rows of the boxes just kept into the removed-set (LDS);
//      one LDS-only barrier per block.
// ONE translation unit: the headers hold their stages' kernels, rbox_nms_common.h what they share; this file keeps the IoU kernels
// and the NMS host side — workspace view (NmsWorkspace), launch plan (nms_plan), runner (nms_run) — behind the C ABI.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdlib.h>

#include "../../include/gd3d.h"
#include "gd3d_fill.h"
#include "rbox_rank.h"
#include "rbox_mask.h"
#include "rbox_scan.h"

namespace rbox {

// pairwise IoU matrices ------------------------------------------------------------------
constexpr int IOU_T = 256;
__global__ __launch_bounds__(IOU_T) void riou_xyxyr_kernel(const float* __restrict__ a, long long na,
                                                           const float* __restrict__ b, long long nb,
                                                           float* __restrict__ out) {
  __shared__ VertexScratch<IOU_T> vs;
  const long long idx = (long long)blockIdx.x * IOU_T + threadIdx.x;
  if (idx >= na * nb) return;
  const long long i = idx / nb, j = idx - i * nb;
  float ra[5], rb[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    ra[k] = a[i * 5 + k];
    rb[k] = b[j * 5 + k];
  }
  OBox A, B;
  obox_make(ra, A);
  obox_make(rb, B);
  out[idx] = iou_bev<IOU_T>(A, B, vs, threadIdx.x);
}

constexpr int EVAL_T = 128;
// affinity.cpp:8-81
template <bool IS3D>
__global__ __launch_bounds__(EVAL_T) void riou_eval_kernel(const float* __restrict__ det, long long nd,
                                                           const float* __restrict__ gt, long long ng, float z_offset,
                                                           float* __restrict__ out) {
  __shared__ HullScratch<EVAL_T> hs;
  const long long idx = (long long)blockIdx.x * EVAL_T + threadIdx.x;
  if (idx >= nd * ng) return;
  const long long di = idx / ng, gi = idx - di * ng;
  float d[7], g[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    d[k] = det[di * 7 + k];
    g[k] = gt[gi * 7 + k];
  }
  out[idx] = eval_iou<IS3D, EVAL_T>(d, g, z_offset, hs, threadIdx.x);
}


static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace rbox

using namespace rbox;

static const int64_t RNMS_MAX_N = 65536;  // 1024 mask words per row; removed-set = 8 KiB of LDS; queue entries hold two 16-bit box indices
static const int64_t QUEUE_MIN_N = 768;   // below: the compacted one-kernel form (3 us faster at 128-256 boxes, equal at 512-768,
                                          // 1 us slower at 1000, 4 at 4096, 34 at 9000: sweep in profiles/r04_nms_queue_ab.txt)
constexpr size_t QUEUE_PER_BOX = 128;

// ---- the workspace of G groups of up to `cap` boxes, as typed pointers; built once per entry-point call ---------------------------
//   OBox records | mask (cap x cbs words) | colm (cap words) | gremv, gkept (cbs words each: two-level scan), one running count per
//   group | candidate queue of the queued mask form (QUEUE_PER_BOX entries per box) | its control words | overflowed block pairs |
//   victim lists | list counters;  behind it, for the scored entry points: order (rnms_scored) | counts (batched scored forms)
struct NmsWorkspace {
  OBox* ob;
  unsigned long long *mask, *colm, *gremv, *gkept;   // colm: per box, the earlier boxes of its own 64-block that suppress it
  long long *gcount, *order;                         // order: (G, cap)
  unsigned *queue, *ctl, *ovl, *lcnt;
  unsigned short* lists;
  int* counts;                                       // (G)
  unsigned scap, npairs, lblock;                     // entries per queue shard; block pairs; list-counter words per group
  size_t bytes, bytes_with_order, bytes_with_counts;   // sizes, for the *_workspace_bytes entry points: NMS part; + order; + counts
  NmsWorkspace(void* workspace, size_t G, size_t cap) {
    const size_t cb = (cap + 63) / 64;
    uintptr_t at = (uintptr_t)workspace;   // (integers: the size functions lay out a workspace at address 0)
    auto take = [&at](auto*& p, size_t bytes) {
      p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(at);
      at += bytes;
    };
    scap = (unsigned)((cap * QUEUE_PER_BOX + QUEUE_SHARDS - 1) / QUEUE_SHARDS);
    npairs = (unsigned)(cb * (cb + 1) / 2);
    take(ob, align_up(G * cap * sizeof(OBox), 256));
    take(mask, align_up(G * cap * cb * sizeof(unsigned long long), 256));
    take(colm, align_up(G * cap * sizeof(unsigned long long), 256));
    take(gremv, G * cb * sizeof(unsigned long long));
    take(gkept, G * cb * sizeof(unsigned long long));
    take(gcount, align_up((2 * G * cb + G) * sizeof(unsigned long long), 256) - 2 * G * cb * sizeof(unsigned long long));
    take(queue, align_up(G * QUEUE_SHARDS * scap * sizeof(unsigned), 256));
    take(ctl, align_up(G * CTL_WORDS * sizeof(unsigned), 256));
    take(ovl, align_up(G * npairs * sizeof(unsigned), 256));
    // victim lists of the list scan (groups of at most LIST_MAX_N boxes only): ids, then per group one block of `lblock` words: the
    // (cap, 2) counters followed by the group's failure word in a 256-byte tail (group 0's — with one group: THE — failure word is
    // found 256 bytes before the end of the workspace: tests read it).  One zero fill per group clears counters and failure word.
    const bool wl = cap <= LIST_MAX_N;
    take(lists, align_up(wl ? G * cap * (LIST_NEAR + LIST_FAR) * sizeof(unsigned short) : 0, 256));
    lblock = wl ? (unsigned)(align_up(cap * 2 * sizeof(unsigned), 256) / sizeof(unsigned) + 64) : 64u;
    take(lcnt, G * (size_t)lblock * sizeof(unsigned));
    bytes = at - (uintptr_t)workspace;
    at = (uintptr_t)workspace + align_up(bytes, 256);
    take(order, align_up(G * cap * sizeof(long long), 256));
    bytes_with_order = at - (uintptr_t)workspace;
    take(counts, align_up(G * sizeof(int), 256));
    bytes_with_counts = at - (uintptr_t)workspace;
  }
};

// ---- the launch plan: which kernels a call runs, on which grids.  Host arithmetic only; every measured threshold lives here ----
enum MaskForm { MASK_PLAIN, MASK_COMPACT, MASK_QUEUED };      // nms_mask_kernel | nms_mask_compact_kernel | circle + clip queue kernels
enum ScanForm { SCAN_LIST, SCAN_SINGLE, SCAN_TWO_LEVEL };     // nms_list_or_scan_kernel | nms_scan_kernel | + nms_propagate_kernel
struct NmsPlan {
  int mode, groups, rows;    // rows: row boxes per wave of the plain / compacted mask kernel
  MaskForm mask;
  unsigned mask_grid;        // plain, compacted: block pairs x (64 / rows); queued: block pairs (the circle kernel's grid)
  unsigned clip_per_shard;   // queued: clipping waves per queue shard
  bool lists;                // the mask stage builds the victim lists (then the scan is SCAN_LIST)
  ScanForm scan;
  int chunks;                // 64-word chunks per mask row in flight in the list / single-level scan: 1 or 2
};

static int nms_plan(int mode, int64_t G, int64_t cap, float thresh, bool thresh_on_device, NmsPlan& p) {
  if (cap > RNMS_MAX_N || G > 65535) return GD3D_E_TOOLARGE;
  const int cbs = ((int)cap + 63) / 64;
  const long long pairs = (long long)cbs * (cbs + 1) / 2;
  p.mode = mode, p.groups = (int)G;
  // compacted kernel: 8..64 rows per wave, as many as keep >= 256 waves in the grid (measured, mask kernel alone:
  // n = 1000: 25 us at 8 rows, 21 at 32, 28 at 64; n = 4096: 47 at 16, 37 at 32, 29 at 64; n = 9000: 229 at 8, 97 at 64)
  p.rows = mode == MODE_ROT ? 64 : 1;
  if (mode == MODE_ROT) while (p.rows > 8 && pairs * G * (64 / p.rows) < 256) p.rows /= 2;
  else while (p.rows < 8 && pairs * G * 64 / (p.rows * 2) >= 16384) p.rows *= 2;  // plain kernel: keep >= ~16 K waves in the grid
  if (pairs * (64 / p.rows) > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  // queued form (circle tests and clipping as two kernels): from QUEUE_MIN_N boxes on, with a threshold every group shares and
  // that is a plain non-negative number (a negative or NaN threshold makes EVERY pair a candidate: the compacted kernel's case;
  // per-group device thresholds are checked in the kernel)
  p.mask = mode != MODE_ROT ? MASK_PLAIN : (cap >= QUEUE_MIN_N && (thresh_on_device || thresh >= 0.0f)) ? MASK_QUEUED : MASK_COMPACT;
  p.mask_grid = (unsigned)(p.mask == MASK_QUEUED ? pairs : pairs * (64 / p.rows));
  // clipping waves: a multiple of the shard count, about one per block pair, at most 4096 and at least 8 per shard: with few
  // block pairs few shards are in use, and one wave per shard walked its ~90 entries in two passes one after the other (n = 256:
  // 25 us for 900 candidates; waves that find their shard empty leave after one load).  The kernel is as long as a wave's passes
  // (memory round trips + one clipping pass each, vector units 27 % busy): more waves with one pass each beat 2048 waves with
  // three to four (n = 9000: 20.3 -> 18.0 us at 64 per shard; 128: the same — LDS holds ten waves per CU).
  const long long per = (pairs + QUEUE_SHARDS - 1) / QUEUE_SHARDS;
  p.clip_per_shard = (unsigned)(per < 8 ? 8 : (per > 64 ? 64 : per));
  // list scan (victim lists and state bytes instead of mask-row propagation): groups of QUEUE_MIN_N .. LIST_MAX_N boxes, rotated
  // (queued form) and axis-aligned boxes; a full list or an overflowed block pair (a negative / NaN device threshold included)
  // falls back to the classic scan on the device, per group
  static const float list_min_thr = [] {
    const char* e = getenv("RNMS_LIST_MIN_THR");   // test override (a value > 1 switches the list scan off)
    return e != nullptr ? (float)atof(e) : 0.0f;
  }();
  // (not for circle NMS: its mask kernel is so cheap that building the lists — 15.8 -> 21.9 us at n = 4096 — and clearing the
  // counters in a launch of their own — 4.4 us — cost what the list scan saves, 29.5 -> 18.0 us; axis-aligned: 62 -> 55 us)
  p.lists = list_min_thr <= 1.0f && cap >= QUEUE_MIN_N && cap <= (int64_t)LIST_MAX_N &&
            (mode == MODE_NORMAL || (p.mask == MASK_QUEUED && (thresh_on_device || thresh >= list_min_thr)));
  // n <= 8448: one launch resolves everything.  Beyond that the single workgroup's row propagation (three 64-word chunks
  // per kept row, one CU's miss bandwidth) dominates and the two-level form wins: r02, kernels of rnms_bev, single ->
  // two-level: n = 9000 339 -> 237 us (72 % kept), 208 -> 207 (25 % kept), 400 -> 237 (79 % kept); n = 16384 1052 -> 476 us;
  // it loses below (n = 6000: 117 -> 128 us: five launches instead of one) — profiles/r02_nms_scan_levels.txt.
  p.scan = p.lists ? SCAN_LIST : cbs <= 128 + 1 + SCAN_NU ? SCAN_SINGLE : SCAN_TWO_LEVEL;
  p.chunks = cbs <= 64 + 1 + SCAN_NU ? 1 : 2;   // one 64-word chunk right of any block (n <= 4352): 16 rows x 1 chunk in flight per row wave
  return 0;
}

// What the caller has already put into the workspace when the runner starts.  RECORDS: the OBox records (rotated mode), in score
// order.  CONTROL: the control words — what the mask stage expects to read as zero: in rotated mode the queue counters (CTL_WORDS
// per group at W.ctl), otherwise the list counters and failure word (W.lblock per group at W.lcnt) — are cleared.
enum NmsPrepared { PREPARED_NOTHING = 0, PREPARED_RECORDS = 1, PREPARED_CONTROL = 2, PREPARED_RECORDS_AND_CONTROL = 3 };

static NmsArgs nms_args(const float* boxes, const int64_t* order, const int32_t* counts, int64_t cap, float thresh, double thresh_d,
                        const float* thresh_dev) {
  return NmsArgs{boxes, (const long long*)order, (const int*)counts, thresh_dev, /*n=*/counts == nullptr ? (int)cap : 0, (int)cap,
                 /*cbs=*/((int)cap + 63) / 64, /*rows: the plan's, set by the runner*/ 0, thresh, thresh_d};
}

// issues the launches of plan `p` (made for a.cap, a's thresholds and p.groups groups)
static int nms_run(const NmsPlan& p, NmsArgs a, const NmsWorkspace& W, NmsPrepared done, int64_t* keep_, int64_t* num_keep_,
                   hipStream_t s) {
  long long *const keep = (long long*)keep_, *const num_keep = (long long*)num_keep_;
  const unsigned G = (unsigned)p.groups;
  a.rows = p.rows;
  const bool have_records = (done & PREPARED_RECORDS) != 0, have_control = (done & PREPARED_CONTROL) != 0;
  // built once for every form: only the queued kernels read queue / ctl / ovl (the plain ones: lists, lcnt, lblock)
  const QueueArgs q = {W.queue, W.ctl, W.ovl, W.scap, W.npairs, p.lists ? W.lists : nullptr, p.lists ? W.lcnt : nullptr, W.lblock};
  // the control words start at zero: cleared by whichever prep kernel ran (obox_prep_kernel here, or the scored paths'
  // rank_place_kernel); only a caller that prepared the records itself, and the plain form with lists, pay a fill in the stream
  // (4.4 us in the trace; a kernel, not a memset node)
  unsigned* const zero = p.mode == MODE_ROT ? W.ctl : W.lcnt;
  const int zero_n = p.mode == MODE_ROT ? (int)CTL_WORDS : (int)W.lblock;
  const dim3 pgrid(((unsigned)a.cap + 255) / 256, G), mgrid(p.mask_grid, G);
  if (p.mask == MASK_QUEUED) {
    if (!have_records) hipLaunchKernelGGL(obox_prep_kernel, pgrid, dim3(256), 0, s, a, W.ob, zero, zero_n);
    else if (!have_control) hipLaunchKernelGGL(zero_words_kernel, dim3(1, G), dim3(256), 0, s, zero, zero_n);
    hipLaunchKernelGGL(nms_circle_queue_kernel, mgrid, dim3(64), 0, s, a, W.ob, W.mask, W.colm, q);
    hipLaunchKernelGGL(nms_clip_queue_kernel, dim3(p.clip_per_shard * QUEUE_SHARDS, G), dim3(64), 0, s, a, W.ob, W.mask, W.colm, q);
  } else if (p.mask == MASK_COMPACT) {
    if (!have_records) hipLaunchKernelGGL(obox_prep_kernel, pgrid, dim3(256), 0, s, a, W.ob, (unsigned*)nullptr, 0);
    hipLaunchKernelGGL(nms_mask_compact_kernel, mgrid, dim3(64), 0, s, a, W.ob, W.mask, W.colm);
  } else {
    if (p.lists && !have_control) hipLaunchKernelGGL(zero_words_kernel, dim3(1, G), dim3(256), 0, s, zero, zero_n);
    hipLaunchKernelGGL(p.mode == MODE_NORMAL ? nms_mask_kernel<MODE_NORMAL> : nms_mask_kernel<MODE_CIRCLE>, mgrid, dim3(64), 0, s, a,
                       W.ob, W.mask, W.colm, q);
  }
  const dim3 sgrid(G), sblk(SCAN_T);
  const size_t slds = (size_t)a.cbs * sizeof(unsigned long long);
  ScanWindow win = {0, a.cbs, nullptr, nullptr, nullptr};   // every block, single-level
  if (p.scan == SCAN_LIST) {   // ONE launch: list scan, or — decided on the device from the clip kernel's failure word — the classic one
    hipLaunchKernelGGL(p.chunks == 1 ? nms_list_or_scan_kernel<1> : nms_list_or_scan_kernel<2>, sgrid, sblk, slds, s, a, W.mask, W.colm,
                       W.lists, W.lcnt, W.lblock, keep, num_keep, win);
  } else if (p.scan == SCAN_SINGLE) {
    hipLaunchKernelGGL((p.chunks == 1 ? nms_scan_kernel<SCAN_U, 1> : nms_scan_kernel<SCAN_U, 2>), sgrid, sblk, slds, s, a, W.mask, W.colm,
                       keep, num_keep, win);
  } else {
    // two-level scan: super-blocks of SCAN_SB blocks resolved one after the other by the scan workgroup (rows stay inside
    // the super-block: one chunk), the rows of the kept boxes spread to everything right of it by nms_propagate_kernel
    win = {0, 0, W.gremv, W.gkept, W.gcount};
    for (int c0 = 0; c0 < a.cbs; c0 += SCAN_SB) {
      win.c_begin = c0;
      win.c_end = c0 + SCAN_SB < a.cbs ? c0 + SCAN_SB : a.cbs;
      hipLaunchKernelGGL((nms_scan_kernel<SCAN_U, 1>), sgrid, sblk, slds, s, a, W.mask, W.colm, keep, num_keep, win);
      if (win.c_end < a.cbs) {
        const int wchunks = (a.cbs - win.c_end + 63) / 64;
        hipLaunchKernelGGL(nms_propagate_kernel, dim3((unsigned)((win.c_end - c0) * wchunks), G), dim3(256), 0, s, a, W.mask, win, wchunks);
      }
    }
  }
  return (int)hipGetLastError();
}

// plan, workspace view and run for a caller-ordered call (the scored entry points rank in between: ranked_nms)
static int ordered_nms(int mode, int32_t G, int64_t cap, const NmsArgs& a, NmsPrepared done, int64_t* keep, int64_t* num_keep,
                       void* workspace, void* stream) {
  NmsPlan p;
  if (const int e = nms_plan(mode, G, cap, a.thresh, a.thresh_dev != nullptr, p)) return e;   // (before a.cap, an int, is trusted)
  return nms_run(p, a, NmsWorkspace(workspace, (size_t)G, (size_t)cap), done, keep, num_keep, (hipStream_t)stream);
}

// The scored entry points: rank_place_kernel (one 16-wave workgroup per 16 boxes counts their ranks and places them: order and
// counts into the workspace's tail, the records of rotated boxes to their ranks; it also clears the control words), then the NMS.
// n: keys per group, cap: boxes that enter the NMS per group; valid / seg / gps as rank_place_kernel takes them.
static int ranked_nms(int mode, const float* boxes, const float* scores, const uint8_t* valid, const int32_t* seg, int32_t G,
                      int64_t n, int64_t cap, bool counts, int gps, float thresh, const float* thresh_dev, int64_t* keep,
                      int64_t* num_keep, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  NmsPlan p;
  if (const int e = nms_plan(mode, G, cap, thresh, thresh_dev != nullptr, p)) return e;
  const NmsWorkspace W(workspace, (size_t)G, (size_t)cap);
  const dim3 sg((unsigned)((n + 15) / 16), (unsigned)G);
  const dim3 sb(valid != nullptr && seg == nullptr ? 256u : 1024u);   // masked dense form: four waves per workgroup
  int* const cnt = counts ? W.counts : nullptr;
  const bool rot = mode == MODE_ROT;   // otherwise: no records, no queue; the list scan's counters and failure word are cleared instead
  hipLaunchKernelGGL(rot ? rank_place_kernel<true> : rank_place_kernel<false>, sg, sb, 0, s, boxes, scores, valid, seg, (int)n, (int)cap,
                     W.order, W.ob, cnt, gps, rot ? W.ctl : W.lcnt, rot ? (int)CTL_WORDS : (int)W.lblock);
  if (const hipError_t e = hipGetLastError()) return (int)e;
  return nms_run(p, nms_args(boxes, (const int64_t*)W.order, cnt, cap, thresh, 0.0, thresh_dev), W,
                 mode == MODE_ROT ? PREPARED_RECORDS_AND_CONTROL : PREPARED_CONTROL, keep, num_keep, s);
}

extern "C" {

size_t rnms_batched_workspace_bytes(int32_t groups, int64_t cap) {
  if (groups <= 0 || cap <= 0) return 16;
  return NmsWorkspace(nullptr, (size_t)groups, (size_t)cap).bytes;
}

size_t rnms_workspace_bytes(int64_t n) { return rnms_batched_workspace_bytes(1, n); }

static int rnms_impl(int mode, const float* boxes, const int64_t* order, int64_t n, float thresh, double thresh_d,
                     int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  if (n < 0 || num_keep == nullptr) return GD3D_E_BADARG;
  if (n == 0) return gd3d::fill_words(num_keep, sizeof(int64_t), 0u, (hipStream_t)stream);
  if (boxes == nullptr || keep == nullptr || workspace == nullptr) return GD3D_E_BADARG;
  return ordered_nms(mode, 1, n, nms_args(boxes, order, nullptr, n, thresh, thresh_d, nullptr), PREPARED_NOTHING, keep, num_keep,
                     workspace, stream);
}

static int rnms_batched_impl(int mode, const float* boxes, const int64_t* order, const int32_t* counts, int32_t groups, int64_t cap,
                             const float* thresh, NmsPrepared done, int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  if (groups == 0) return 0;
  if (num_keep == nullptr) return GD3D_E_BADARG;
  if (cap == 0) return gd3d::fill_words(num_keep, sizeof(int64_t) * (size_t)groups, 0u, (hipStream_t)stream);
  if (boxes == nullptr || order == nullptr || counts == nullptr || thresh == nullptr || keep == nullptr ||
      workspace == nullptr)
    return GD3D_E_BADARG;
  return ordered_nms(mode, groups, cap, nms_args(boxes, order, counts, cap, 0.0f, 0.0, thresh), done, keep, num_keep, workspace,
                     stream);
}

int rnms_batched(int32_t mode, const float* boxes, const int64_t* order, const int32_t* counts, int32_t groups, int64_t cap,
                 const float* thresh, int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  if (mode < MODE_ROT || mode > MODE_CIRCLE || groups < 0 || cap < 0) return GD3D_E_BADARG;
  return rnms_batched_impl(mode, boxes, order, counts, groups, cap, thresh, PREPARED_NOTHING, keep, num_keep, workspace, stream);
}

int rnms_batched_prepared(const float* boxes, const int64_t* order, const int32_t* counts, int32_t groups, int64_t cap,
                          const float* thresh, int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  if (groups < 0 || cap < 0) return GD3D_E_BADARG;
  return rnms_batched_impl(MODE_ROT, boxes, order, counts, groups, cap, thresh, PREPARED_RECORDS, keep, num_keep, workspace, stream);
}

int rnms_circle_ordered(const float* xy, const int64_t* order, int64_t n, double thresh, int64_t* keep, int64_t* num_keep,
                        void* workspace, void* stream) {
  return rnms_impl(MODE_CIRCLE, xy, order, n, (float)thresh, thresh, keep, num_keep, workspace, stream);
}

int rnms_bev(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep, int64_t* num_keep, void* workspace,
             void* stream) {
  return rnms_impl(MODE_ROT, boxes_sorted, nullptr, n, thresh, 0.0, keep, num_keep, workspace, stream);
}

int rnms_scored_max_n(void) { return RANK_MAX; }

size_t rnms_scored_workspace_bytes(int64_t n_all, int64_t n_keep) {
  return NmsWorkspace(nullptr, 1, (size_t)(n_keep < 1 ? 1 : n_keep)).bytes_with_order;   // NMS workspace | order
}

int rnms_scored(int32_t normal, const float* boxes, const float* scores, int64_t n_all, int64_t pre_max, float thresh,
                int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  if (n_all < 0 || num_keep == nullptr) return GD3D_E_BADARG;
  if (n_all > RANK_MAX) return GD3D_E_TOOLARGE;
  const int64_t n = (pre_max >= 0 && pre_max < n_all) ? pre_max : n_all;
  if (n == 0) return gd3d::fill_words(num_keep, sizeof(int64_t), 0u, (hipStream_t)stream);
  if (boxes == nullptr || scores == nullptr || keep == nullptr || workspace == nullptr) return GD3D_E_BADARG;
  return ranked_nms(normal ? MODE_NORMAL : MODE_ROT, boxes, scores, nullptr, nullptr, 1, n_all, n, /*counts=*/false, 0, thresh,
                    nullptr, keep, num_keep, workspace, stream);
}

size_t rnms_batched_scored_workspace_bytes(int32_t groups, int64_t n, int64_t cap) {
  return NmsWorkspace(nullptr, (size_t)(groups < 1 ? 1 : groups), (size_t)(cap < 1 ? 1 : cap)).bytes_with_counts;   // | order | counts
}

static int batched_scored_impl(int32_t mode, const float* boxes, const float* scores, const uint8_t* valid, const int32_t* seg,
                               int32_t groups, int64_t n, int64_t pre_max, const float* thresh, int64_t* keep,
                               int64_t* num_keep, void* workspace, void* stream, int gps) {
  if (mode < MODE_ROT || mode > MODE_CIRCLE || groups < 0 || n < 0) return GD3D_E_BADARG;
  if (groups == 0) return 0;
  if (num_keep == nullptr) return GD3D_E_BADARG;
  if (n > RANK_MAX || groups > 65535) return GD3D_E_TOOLARGE;
  const int64_t cap = (pre_max >= 0 && pre_max < n) ? pre_max : n;
  if (cap == 0) return gd3d::fill_words(num_keep, sizeof(int64_t) * (size_t)groups, 0u, (hipStream_t)stream);
  if (boxes == nullptr || scores == nullptr || thresh == nullptr || keep == nullptr || workspace == nullptr) return GD3D_E_BADARG;
  return ranked_nms(mode, boxes, scores, valid, seg, groups, n, cap, /*counts=*/true, gps, 0.0f, thresh, keep, num_keep, workspace,
                    stream);
}

int rnms_batched_scored(int32_t mode, const float* boxes, const float* scores, const uint8_t* valid, int32_t groups, int64_t n,
                        int64_t pre_max, const float* thresh, int64_t* keep, int64_t* num_keep, void* workspace, void* stream) {
  return batched_scored_impl(mode, boxes, scores, valid, nullptr, groups, n, pre_max, thresh, keep, num_keep, workspace, stream, 0);
}

int rnms_batched_scored_sets(int32_t mode, const float* boxes, const float* scores, const uint8_t* valid, int32_t sets,
                             int32_t groups_per_set, int64_t n, int64_t pre_max, const float* thresh, int64_t* keep, int64_t* num_keep,
                             void* workspace, void* stream) {
  if (sets < 0 || groups_per_set < 1 || (int64_t)sets * groups_per_set > 65535 || (int64_t)sets * n > 0x7fffffffLL) return GD3D_E_BADARG;
  return batched_scored_impl(mode, boxes, scores, valid, nullptr, sets * groups_per_set, n, pre_max, thresh, keep, num_keep, workspace,
                             stream, groups_per_set);
}

int rnms_segmented_scored(int32_t mode, const float* boxes, const float* scores, const int32_t* seg, int32_t groups,
                          int64_t max_seg, int64_t pre_max, const float* thresh, int64_t* keep, int64_t* num_keep,
                          void* workspace, void* stream) {
  if (groups > 0 && seg == nullptr) return GD3D_E_BADARG;
  return batched_scored_impl(mode, boxes, scores, nullptr, seg, groups, max_seg, pre_max, thresh, keep, num_keep, workspace,
                             stream, 0);
}

int rnms_bev_ordered(const float* boxes, const int64_t* order, int64_t n, float thresh, int64_t* keep, int64_t* num_keep,
                     void* workspace, void* stream) {
  if (n > 0 && order == nullptr) return GD3D_E_BADARG;
  return rnms_impl(MODE_ROT, boxes, order, n, thresh, 0.0, keep, num_keep, workspace, stream);
}

int rnms_normal_bev_ordered(const float* boxes, const int64_t* order, int64_t n, float thresh, int64_t* keep,
                            int64_t* num_keep, void* workspace, void* stream) {
  if (n > 0 && order == nullptr) return GD3D_E_BADARG;
  return rnms_impl(MODE_NORMAL, boxes, order, n, thresh, 0.0, keep, num_keep, workspace, stream);
}

int rnms_normal_bev(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep, int64_t* num_keep,
                    void* workspace, void* stream) {
  return rnms_impl(MODE_NORMAL, boxes_sorted, nullptr, n, thresh, 0.0, keep, num_keep, workspace, stream);
}

int riou_bev_xyxyr(const float* a, int64_t na, const float* b, int64_t nb, float* iou, void* stream) {
  if (na < 0 || nb < 0) return GD3D_E_BADARG;
  if (na == 0 || nb == 0) return 0;
  if (a == nullptr || b == nullptr || iou == nullptr) return GD3D_E_BADARG;
  const long long tot = (long long)na * nb;
  const long long blocks = (tot + IOU_T - 1) / IOU_T;
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipLaunchKernelGGL(riou_xyxyr_kernel, dim3((unsigned)blocks), dim3(IOU_T), 0, (hipStream_t)stream, a, (long long)na,
                     b, (long long)nb, iou);
  return (int)hipGetLastError();
}

static int riou_eval_impl(bool is3d, const float* det, int64_t nd, const float* gt, int64_t ng, float z_offset,
                          float* iou, void* stream) {
  if (nd < 0 || ng < 0) return GD3D_E_BADARG;
  if (nd == 0 || ng == 0) return 0;
  if (det == nullptr || gt == nullptr || iou == nullptr) return GD3D_E_BADARG;
  const long long tot = (long long)nd * ng;
  const long long blocks = (tot + EVAL_T - 1) / EVAL_T;
  if (blocks > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (is3d)
    hipLaunchKernelGGL((riou_eval_kernel<true>), dim3((unsigned)blocks), dim3(EVAL_T), 0, (hipStream_t)stream, det,
                       (long long)nd, gt, (long long)ng, z_offset, iou);
  else
    hipLaunchKernelGGL((riou_eval_kernel<false>), dim3((unsigned)blocks), dim3(EVAL_T), 0, (hipStream_t)stream, det,
                       (long long)nd, gt, (long long)ng, z_offset, iou);
  return (int)hipGetLastError();
}

int riou_eval_bev(const float* det, int64_t nd, const float* gt, int64_t ng, float* iou, void* stream) {
  return riou_eval_impl(false, det, nd, gt, ng, 0.5f, iou, stream);
}

int riou_eval_3d(const float* det, int64_t nd, const float* gt, int64_t ng, float z_offset, float* iou, void* stream) {
  return riou_eval_impl(true, det, nd, gt, ng, z_offset, iou, stream);
}

}  // extern "C"
