// roi_sample.hip — PVRCNNROIHead._assign_and_sample (models/roi_heads/pvrcnn_roi_head.py:225-297) for gfx950 (include/gd3d.h,
// gd3d_roi_iou3d / gd3d_roi_assign_sample): the per-class MaxIoUAssigner on BboxOverlaps3D(coordinate='lidar') and the
// IoUNegPiecewiseSampler of a whole batch without a host read.  The reference spends a Python loop over samples and classes,
// nonzero / pad / boolean assignment and a randperm / randint / unique chain on 512 proposals x a few dozen gts; here
//   * sample_kernel, ONE workgroup per sample: the gt rows and the per-gt maxima live in LDS; a thread per proposal sorts the
//     pairs of equal class into "IoU exactly 0" (bounding circles, height: no geometry) and a queue of pairs that NT lanes then
//     clip, all lanes busy; the maxima per proposal and per gt are unsigned 64-bit LDS maxima of (IoU bits, ~index) — order free,
//     and they carry the lowest-index argmax; rule 4 re-evaluates only the pairs that can tie a gt's maximum; the two
//     draws are ONE bitonic sort of (stratum, key, index) entries (csrc/lds_sort.h) and a plan made from the strata's sizes; the
//     ascending-index outputs (`.unique()`) come from a ballot / popcount rank.  It leaves the sample's chosen proposal indices
//     and its two counts in `stage`;
//   * pack_kernel, a second single-workgroup launch: packs the samples back to back by those counts and gathers every output row.
//     No workgroup ever waits for another one.
// Every output element is written by exactly one thread; keys in, the same bits out on every run and in csrc/roi_sample_cpu.cpp.
// Compiled with -ffp-contract=off (csrc/roi_sample_common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "lds_sort.h"
#include "roi_sample_common.h"

namespace roi_sample {

// ------------------------------------------------------------------ the pairwise op
__global__ __launch_bounds__(NT) void iou3d_kernel(const float* __restrict__ a, const float* __restrict__ b, long long pairs, int M,
                                                  float* __restrict__ out) {
  __shared__ VertexScratch<NT> vs;
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= pairs) return;
  const long long i = p / M, j = p - i * M;
  float ra[7], rb[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    ra[k] = a[i * 7 + k];
    rb[k] = b[j * 7 + k];
  }
  OBox A, B;
  bev_obox(ra, A);
  bev_obox(rb, B);
  out[p] = iou3d<NT>(ra, A, rb, B, vs, threadIdx.x);
}

// ------------------------------------------------------------------ one sample: assign, draw
struct SampleArgs {
  const float* prop;          // (N, 7)
  const int64_t* plabel;      // (N)
  const int32_t* pcnt;        // (B)
  const float* gt;            // (G, 7)
  const int64_t* glabel;      // (G)
  const int32_t* gcnt;        // (B)
  const float* keys;          // (N)
  const float* fill_keys;     // (B * num)
  int N, G, B;
  Rules r;
  int64_t* gt_inds;           // (N)
  float* max_overlaps;        // (N)
  int64_t* labels;            // (N)
  int32_t* stage;             // (B, 2 + num): positives drawn, rows, the chosen proposal indices
};

// the dynamic LDS block, every offset a multiple of 16
constexpr int SORT_BYTES = 8 * (MAX_PROPS + MAX_PROPS / 8 + 8);
constexpr int OFF_UNION = 0;                                             // VertexScratch<NT>, later the sort list
constexpr int UNION_BYTES = (int)sizeof(VertexScratch<NT>) > SORT_BYTES ? (int)sizeof(VertexScratch<NT>) : SORT_BYTES;
constexpr int OFF_GT = OFF_UNION + UNION_BYTES;                          // float [MAX_GTS][7]
constexpr int OFF_GBEST = OFF_GT + MAX_GTS * 7 * 4;                      // u64 [MAX_GTS]: (max IoU bits, ~lowest proposal)
constexpr int OFF_GLABEL = OFF_GBEST + MAX_GTS * 8;                      // int [MAX_GTS]
constexpr int OFF_STRAT = OFF_GLABEL + MAX_GTS * 4;                      // u8 [MAX_PROPS]
constexpr int OFF_SEL = OFF_STRAT + MAX_PROPS;                           // int [MAX_NUM]
constexpr int OFF_FILL = OFF_SEL + MAX_NUM * 4;                          // int [MAX_NUM]
constexpr int WL_CAP = 4096;                                             // pairs queued for clipping per round
constexpr int OFF_WL = OFF_FILL + MAX_NUM * 4;                           // u32 [WL_CAP]: (proposal << 10) | gt
constexpr int OFF_PBEST = OFF_WL + WL_CAP * 4;                           // u64 [WG]: (max IoU bits, ~lowest gt) of a chunk's proposals
constexpr int OFF_SMALL = OFF_PBEST + WG * 8;                            // int [64]: counts, starts, wave totals, queue control
constexpr int LDS_BYTES = OFF_SMALL + 64 * 4 + (int)sizeof(Plan) + 16;
static_assert(UNION_BYTES % 16 == 0 && OFF_GBEST % 16 == 0 && OFF_PBEST % 16 == 0 && OFF_SMALL % 16 == 0, "LDS carve offsets");
static_assert(LDS_BYTES <= 160 * 1024, "LDS of a CU");

constexpr int DRAWN = 0x80, NONE = 0x7f;

__device__ __forceinline__ float pair_iou(const float* pr, const OBox& A, const float* gts, int g, VertexScratch<NT>& vs, int t) {
  float gr[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) gr[k] = gts[g * 7 + k];
  OBox Bx;
  bev_obox(gr, Bx);
  return clean_iou(iou3d<NT>(pr, A, gr, Bx, vs, t));
}

__global__ __launch_bounds__(WG) void sample_kernel(const SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  VertexScratch<NT>& vs = *reinterpret_cast<VertexScratch<NT>*>(lds + OFF_UNION);
  unsigned long long* list = reinterpret_cast<unsigned long long*>(lds + OFF_UNION);
  float* gts = reinterpret_cast<float*>(lds + OFF_GT);
  unsigned long long* gbest = reinterpret_cast<unsigned long long*>(lds + OFF_GBEST);
  int* glab = reinterpret_cast<int*>(lds + OFF_GLABEL);
  unsigned char* strat = lds + OFF_STRAT;
  int* sel = reinterpret_cast<int*>(lds + OFF_SEL);
  int* fill_list = reinterpret_cast<int*>(lds + OFF_FILL);
  int* cnt = reinterpret_cast<int*>(lds + OFF_SMALL);        // [16] members per stratum
  int* start = cnt + 16;                                     // [16] where a stratum starts in the sorted list
  int* wave_cnt = cnt + 32;                                  // [2][WG / 64]
  int* ctl = start + 12;                                     // [2] queue length, "a pair is waiting" (start[] uses 10 words)
  unsigned* wl = reinterpret_cast<unsigned*>(lds + OFF_WL);
  unsigned long long* pbest = reinterpret_cast<unsigned long long*>(lds + OFF_PBEST);
  Plan& plan = *reinterpret_cast<Plan*>(lds + OFF_SMALL + 64 * 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const Rules& r = a.r;

  // this sample's clamped segments (B is small; the counts sit in a cache line or two)
  int p0 = 0, g0 = 0, pn = 0, gn = 0;
  for (int s = 0; s <= b; ++s) {
    p0 += pn;
    g0 += gn;
    pn = clamp_count(a.pcnt[s], a.N - p0);
    gn = clamp_count(a.gcnt[s], a.G - g0);
  }
  const int Np = pn < MAX_PROPS ? pn : MAX_PROPS;   // rows of the segment past MAX_PROPS / MAX_GTS take no part
  const int Ng = gn < MAX_GTS ? gn : MAX_GTS;
  const float* prop = a.prop + (long long)p0 * 7;

  for (int i = tid; i < Ng * 7; i += WG) gts[i] = a.gt[(long long)g0 * 7 + i];
  for (int g = tid; g < Ng; g += WG) {
    const int64_t l = a.glabel[g0 + g];
    glab[g] = (l >= 0 && l < r.C) ? (int)l : -1;
    gbest[g] = 0ull;
  }
  if (tid < 16) cnt[tid] = 0;
  __syncthreads();

  // ---- pass 1: max_overlap / argmax per proposal, the maximum per gt.  A thread per proposal walks the gts of its class with
  // the cheap tests only (bounding circles, height) and queues the pairs that can overlap; NT lanes then clip the queued pairs,
  // all of them busy.  (A lane per proposal clipping its own pairs leaves a wave waiting on whichever lanes clip: 440 us per
  // launch at 4 x 512 x 20.)  Both maxima are unsigned 64-bit LDS maxima of (IoU bits, ~index): order free, the lowest index on a tie.
  for (int base = 0; base < Np; base += WG) {          // block-uniform trip counts: every barrier is reached by every thread
    const int n = base + tid;
    int c = -1, g_next = 0;
    unsigned long long mine = 0ull;                    // (0, ~first gt of the class): what a proposal without overlap keeps
    Lite pa = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (n < Np) {
      const int64_t l = a.plabel[p0 + n];
      c = (l >= 0 && l < r.C) ? (int)l : -1;
      if (c >= 0) {
        float pr[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) pr[k] = prop[(long long)n * 7 + k];
        lite_of(pr, pa);
      }
    }
    pbest[tid] = 0ull;
    bool scanning = c >= 0;
    bool more;
    do {
      __syncthreads();
      if (tid == 0) ctl[0] = ctl[1] = 0;
      __syncthreads();
      if (scanning) {
        while (g_next < Ng) {
          const int g = g_next;
          if (glab[g] == c) {
            Lite gb;
            lite_of(gts + g * 7, gb);
            if (may_overlap(pa, gb)) {
              const int slot = atomicAdd(&ctl[0], 1);
              if (slot >= WL_CAP) {                    // the queue is full: this pair waits for the next round
                ctl[1] = 1;
                break;
              }
              wl[slot] = ((unsigned)n << 10) | (unsigned)g;
            } else {                                   // IoU exactly 0
              const unsigned long long cand = (unsigned long long)(0xffffffffu - (unsigned)n);
              if (gbest[g] < cand) atomicMax(&gbest[g], cand);
            }
            if (mine == 0ull) mine = (unsigned long long)(0xffffffffu - (unsigned)g);
          }
          ++g_next;
        }
        scanning = g_next < Ng;
      }
      __syncthreads();
      const int work = ctl[0] < WL_CAP ? ctl[0] : WL_CAP;
      more = ctl[1] != 0;
      if (tid < NT) {
        for (int i = tid; i < work; i += NT) {
          const unsigned e = wl[i];
          const int n2 = (int)(e >> 10), g = (int)(e & 1023u);
          float pr[7];
#pragma unroll
          for (int k = 0; k < 7; ++k) pr[k] = prop[(long long)n2 * 7 + k];
          OBox A;
          bev_obox(pr, A);
          const unsigned long long hi = (unsigned long long)f32_bits(pair_iou(pr, A, gts, g, vs, tid)) << 32;
          atomicMax(&pbest[n2 - base], hi | (unsigned long long)(0xffffffffu - (unsigned)g));
          atomicMax(&gbest[g], hi | (unsigned long long)(0xffffffffu - (unsigned)n2));
        }
      }
    } while (more);
    __syncthreads();
    if (n < Np) {
      const unsigned long long got = pbest[tid] > mine ? pbest[tid] : mine;
      a.max_overlaps[p0 + n] = got != 0ull ? bits_f32((unsigned)(got >> 32)) : 0.0f;
      a.gt_inds[p0 + n] = got != 0ull ? (int64_t)(0xffffffffu - (unsigned)got) : -1;      // the argmax for now: pass 2 reads it back
    }
  }
  __syncthreads();

  // ---- pass 2: the assigner's rules, the stratum of every proposal
  if (tid < NT) {
    for (int n = tid; n < Np; n += NT) {
      const float mo = a.max_overlaps[p0 + n];
      const int arg = (int)a.gt_inds[p0 + n];
      int gi = 0;
      if (arg >= 0) {
        const int c = glab[arg];
        gi = assign_first(mo, arg, r.pos[c], r.neg[c]);
        if (r.flags[c] & FLAG_LOW_QUALITY) {
          const bool all = (r.flags[c] & FLAG_ASSIGN_ALL) != 0;
          float pr[7];
          OBox A;
          Lite pa;
          bool have = false;
          for (int g = Ng - 1; g >= 0; --g) {   // ascending gts overwrite: the last match is the first one from the top
            if (glab[g] != c) continue;
            const unsigned long long gb = gbest[g];
            const float gmax = bits_f32((unsigned)(gb >> 32));
            if (!(gmax >= r.min_pos[c])) continue;
            bool match;
            if (!all) {
              match = (unsigned)gb == 0xffffffffu - (unsigned)n;
            } else if (g == arg) {
              match = mo == gmax;
            } else if (!(mo >= gmax)) {
              match = false;                    // iou[n, g] <= max_overlap[n] < gt_max[g]
            } else {
              if (!have) {
#pragma unroll
                for (int k = 0; k < 7; ++k) pr[k] = prop[(long long)n * 7 + k];
                bev_obox(pr, A);
                lite_of(pr, pa);
                have = true;
              }
              Lite gb;
              lite_of(gts + g * 7, gb);
              match = (may_overlap(pa, gb) ? pair_iou(pr, A, gts, g, vs, tid) : 0.0f) == gmax;
            }
            if (match) {
              gi = g + 1;
              break;
            }
          }
        }
      }
      a.gt_inds[p0 + n] = gi;
      a.labels[p0 + n] = gi > 0 ? a.glabel[g0 + gi - 1] : -1;
      const int s = stratum_of(gi, mo, r);
      strat[n] = (unsigned char)(s < 0 ? NONE : s);
      if (s >= 0) atomicAdd(&cnt[s], 1);
    }
  }
  for (int n = Np + tid; n < pn; n += WG) {   // rows of the segment beyond the limit
    a.gt_inds[p0 + n] = -1;
    a.max_overlaps[p0 + n] = 0.0f;
    a.labels[p0 + n] = -1;
  }
  __syncthreads();   // the vertex scratch is free from here on: the sort list takes its place

  // ---- the draws: one sort of (stratum, key, index), a plan from the strata's sizes
  if (tid == 0) {
    int s0 = 0;
    for (int s = 0; s <= r.K; ++s) {
      start[s] = s0;
      s0 += cnt[s];
    }
    start[r.K + 1] = s0;
    make_plan(cnt, r, plan);
  }
  for (int n = tid; n < Np; n += WG) {
    const int s = strat[n];
    list[ldssort::PH(n)] = s == NONE ? 0ull : draw_entry(s, a.keys[p0 + n], n);
  }
  __syncthreads();
  ldssort::bitonic_desc(list, Np);
  const int cands = start[r.K + 1];
  const int npos = plan.npos;
  for (int p = tid; p < cands; p += WG) {
    const unsigned long long e = list[ldssort::PH(p)];
    const int s = entry_stratum(e), n = entry_index(e), t = p - start[s];
    if (s == 0) {
      if (t < npos) strat[n] = DRAWN;
    } else if (t < plan.take[s - 1]) {
      sel[npos + plan.off[s - 1] + t] = n;
    }
  }
  __syncthreads();

  // ---- ascending index: the drawn positives, and the last piece as the list a fill repeats from
  const int last = r.K;
  const bool need_last = plan.fill > 0 && plan.fill_from_last;
  int run_p = 0, run_l = 0;
  int* wc_p = wave_cnt;
  int* wc_l = wave_cnt + WG / 64;
  for (int base = 0; base < Np; base += WG) {   // block-uniform trip count
    const int n = base + tid;
    const int s = n < Np ? (int)strat[n] : NONE;
    const unsigned long long mp = __ballot(s == DRAWN), ml = __ballot(need_last && s == last);
    if (lane == 0) {
      wc_p[wave] = __popcll(mp);
      wc_l[wave] = __popcll(ml);
    }
    __syncthreads();
    int before_p = 0, total_p = 0, before_l = 0, total_l = 0;
    for (int w = 0; w < WG / 64; ++w) {
      const int cp = wc_p[w], cl = wc_l[w];
      before_p += w < wave ? cp : 0;
      total_p += cp;
      before_l += w < wave ? cl : 0;
      total_l += cl;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (s == DRAWN) sel[run_p + before_p + __popcll(mp & below)] = n;
    if (need_last && s == last) {
      const int k = run_l + before_l + __popcll(ml & below);
      if (k < MAX_NUM) fill_list[k] = n;        // a short last piece has fewer than num members
    }
    run_p += total_p;
    run_l += total_l;
  }
  __syncthreads();

  // ---- the fill with replacement
  const int rows_before = npos + plan.chosen;
  for (int t = tid; t < plan.fill; t += WG) {
    const int j = rows_before + t;
    const int k = fill_member(a.fill_keys[(long long)b * r.num + j], plan.m);
    sel[j] = plan.fill_from_last ? fill_list[k] : sel[npos + k];
  }
  __syncthreads();
  const int rows = rows_before + plan.fill;
  int32_t* st = a.stage + (long long)b * (2 + r.num);
  if (tid == 0) {
    st[0] = npos;
    st[1] = rows;
  }
  for (int j = tid; j < r.num; j += WG) st[2 + j] = j < rows ? sel[j] : -1;
}

// ------------------------------------------------------------------ all samples: pack and gather
struct PackArgs {
  const float* prop;
  const int32_t* pcnt;
  const float* gt;
  const int32_t* gcnt;
  int N, G, B, num, npos;
  const int32_t* stage;
  int64_t* gt_inds;
  float* max_overlaps;
  int64_t* labels;
  float* rois;                // (B * num, 8)
  float* ious;                // (B * num)
  int64_t* inds;              // (B * num)
  float* pos_bboxes;          // (B * npos, 7)
  float* pos_gt_bboxes;       // (B * npos, 7)
  int64_t* pos_gt_inds;       // (B * npos)
  int32_t* pos_batch_cnt;     // (B)
  int32_t* roi_batch_cnt;     // (B)
};

__global__ __launch_bounds__(WG) void pack_kernel(const PackArgs a) {
  __shared__ int pstart[MAX_SAMPLES + 1], gstart[MAX_SAMPLES + 1], rstart[MAX_SAMPLES + 1], qstart[MAX_SAMPLES + 1];
  const int tid = threadIdx.x;
  const long long stride = 2 + a.num;
  if (tid == 0) {
    int p0 = 0, g0 = 0, r0 = 0, q0 = 0;
    pstart[0] = gstart[0] = rstart[0] = qstart[0] = 0;
    for (int b = 0; b < a.B; ++b) {
      p0 += clamp_count(a.pcnt[b], a.N - p0);
      g0 += clamp_count(a.gcnt[b], a.G - g0);
      q0 += clamp_count(a.stage[b * stride], a.npos);
      r0 += clamp_count(a.stage[b * stride + 1], a.num);
      pstart[b + 1] = p0;
      gstart[b + 1] = g0;
      rstart[b + 1] = r0;
      qstart[b + 1] = q0;
    }
  }
  __syncthreads();
  for (int b = tid; b < a.B; b += WG) {
    a.pos_batch_cnt[b] = qstart[b + 1] - qstart[b];
    a.roi_batch_cnt[b] = rstart[b + 1] - rstart[b];
  }
  for (int i = pstart[a.B] + tid; i < a.N; i += WG) {   // proposal rows past the counts' sum belong to no sample
    a.gt_inds[i] = -1;
    a.max_overlaps[i] = 0.0f;
    a.labels[i] = -1;
  }
  const int R = a.B * a.num, Q = a.B * a.npos;
  for (int row = tid; row < R; row += WG) {
    const int b = sample_of(rstart, a.B, row);
    float o[8] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float iou = 0.0f;
    int64_t ind = 0;
    if (b < a.B) {
      const int n = a.stage[b * stride + 2 + (row - rstart[b])];
      const long long src = (long long)pstart[b] + n;
      o[0] = (float)b;
#pragma unroll
      for (int k = 0; k < 7; ++k) o[1 + k] = a.prop[src * 7 + k];
      iou = a.max_overlaps[src];
      ind = n;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) a.rois[(long long)row * 8 + k] = o[k];
    a.ious[row] = iou;
    a.inds[row] = ind;
  }
  for (int row = tid; row < Q; row += WG) {
    const int b = sample_of(qstart, a.B, row);
    float pb[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, pg[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int64_t gi = 0;
    if (b < a.B) {
      const int n = a.stage[b * stride + 2 + (row - qstart[b])];
      const long long src = (long long)pstart[b] + n;
      gi = a.gt_inds[src] - 1;
      const long long gsrc = (long long)gstart[b] + gi;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        pb[k] = a.prop[src * 7 + k];
        pg[k] = a.gt[gsrc * 7 + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      a.pos_bboxes[(long long)row * 7 + k] = pb[k];
      a.pos_gt_bboxes[(long long)row * 7 + k] = pg[k];
    }
    a.pos_gt_inds[row] = gi;
  }
}

}  // namespace roi_sample

using namespace roi_sample;

extern "C" {

int gd3d_roi_iou3d(const float* bboxes1, int64_t n1, const float* bboxes2, int64_t n2, float* iou, void* stream) {
  if (n1 < 0 || n2 < 0) return GD3D_E_BADARG;
  if (n1 == 0 || n2 == 0) return 0;
  if (n1 > MAX_ROWS || n2 > MAX_ROWS || n1 * n2 > (1LL << 31) - NT) return GD3D_E_TOOLARGE;
  if (bboxes1 == nullptr || bboxes2 == nullptr || iou == nullptr) return GD3D_E_BADARG;
  const long long pairs = n1 * n2;
  hipLaunchKernelGGL(iou3d_kernel, dim3((unsigned)((pairs + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, bboxes1, bboxes2, pairs,
                     (int)n2, iou);
  return (int)hipGetLastError();
}

int gd3d_roi_assign_sample(const float* proposals, const int64_t* proposal_labels, const int32_t* prop_batch_cnt, int64_t N,
                           const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B,
                           const float* keys, const float* fill_keys, int32_t C, const float* pos_iou_thr, const float* neg_iou_thr,
                           const float* min_pos_iou, const int32_t* assign_flags, int32_t num, int32_t npos, int32_t K,
                           const double* neg_piece_fractions, const float* neg_iou_piece_thrs, float* rois, float* ious,
                           int64_t* inds, float* pos_bboxes, float* pos_gt_bboxes, int64_t* pos_assigned_gt_inds,
                           int32_t* pos_batch_cnt, int32_t* roi_batch_cnt, int64_t* gt_inds, float* max_overlaps, int64_t* labels,
                           int32_t* stage, void* stream) {
  SampleArgs s;
  const int rc = make_rules(N, G, B, C, pos_iou_thr, neg_iou_thr, min_pos_iou, assign_flags, num, npos, K, neg_piece_fractions,
                            neg_iou_piece_thrs, s.r);
  if (rc != 0) return rc;
  if (B == 0) return N == 0 ? 0 : GD3D_E_BADARG;
  if (prop_batch_cnt == nullptr || gt_batch_cnt == nullptr || fill_keys == nullptr || rois == nullptr || ious == nullptr ||
      inds == nullptr || pos_batch_cnt == nullptr || roi_batch_cnt == nullptr || stage == nullptr)
    return GD3D_E_BADARG;
  if (N > 0 && (proposals == nullptr || proposal_labels == nullptr || keys == nullptr || gt_inds == nullptr ||
                max_overlaps == nullptr || labels == nullptr))
    return GD3D_E_BADARG;
  if (G > 0 && (gt_bboxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  if (npos > 0 && (pos_bboxes == nullptr || pos_gt_bboxes == nullptr || pos_assigned_gt_inds == nullptr)) return GD3D_E_BADARG;
  static bool attr_set[64] = {};
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess) return GD3D_E_BADARG;
  if (devid < 0 || devid >= 64 || !attr_set[devid]) {
    const hipError_t e = hipFuncSetAttribute((const void*)sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    if (devid >= 0 && devid < 64) attr_set[devid] = true;
  }
  s.prop = proposals; s.plabel = proposal_labels; s.pcnt = prop_batch_cnt; s.gt = gt_bboxes; s.glabel = gt_labels;
  s.gcnt = gt_batch_cnt; s.keys = keys; s.fill_keys = fill_keys; s.N = (int)N; s.G = (int)G; s.B = B;
  s.gt_inds = gt_inds; s.max_overlaps = max_overlaps; s.labels = labels; s.stage = stage;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)B), dim3(WG), LDS_BYTES, (hipStream_t)stream, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  PackArgs p;
  p.prop = proposals; p.pcnt = prop_batch_cnt; p.gt = gt_bboxes; p.gcnt = gt_batch_cnt; p.N = (int)N; p.G = (int)G; p.B = B;
  p.num = num; p.npos = npos; p.stage = stage; p.gt_inds = gt_inds; p.max_overlaps = max_overlaps; p.labels = labels;
  p.rois = rois; p.ious = ious; p.inds = inds; p.pos_bboxes = pos_bboxes; p.pos_gt_bboxes = pos_gt_bboxes;
  p.pos_gt_inds = pos_assigned_gt_inds; p.pos_batch_cnt = pos_batch_cnt; p.roi_batch_cnt = roi_batch_cnt;
  hipLaunchKernelGGL(pack_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // extern "C"
