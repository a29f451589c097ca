// simota.hip — SimOTABEVAssigner.assign (core/bbox/assigners/sim_ota_3d_assigner.py:34-211) for gfx950 (include/gd3d.h,
// gd3d_simota_assign): the assignment of a whole batch as a fill and three launches, without a host read, a data-dependent
// allocation or a priors x gts matrix in memory.  The reference spends one host-synchronising topk per gt, two boolean
// compactions and (valid, G, C) repeats of the scores; here
//   * flag_kernel, a thread per prior: the gts' BEV constants pass through LDS in tiles of 256; writes the three default outputs and
//     appends the candidates' indices to the sample's list — ONE global atomic per workgroup that has candidates, the ranks inside
//     from ballots.  The list's order is free: every later key carries the prior index;
//   * select_kernel, a workgroup per (sample, gt), streams the candidates 1024 at a time: a thread per candidate makes the cheap
//     test (bounding circles, height) and either settles the pair at IoU 0 or queues it; NT lanes clip the queued pairs once more
//     than a round's worth wait (or the list ends), all busy.
//     The K largest IoUs and the K smallest (cost, prior) are two bounded selections of 64-bit entries: an entry that beats the
//     current K-th best is appended to an LDS buffer, a full buffer is sorted (csrc/lds_sort.h) and cut back to K.  Emits the k
//     matches of the gt;
//   * resolve_kernel, a workgroup per sample: sorts the sample's matches by prior, ranks the distinct priors by ballots, writes the
//     outputs and the padded positive lists, and re-evaluates the whole cost row of the priors more than one gt took — (prior, gt)
//     pairs spread over NT lanes, the row minimum an unsigned 64-bit LDS minimum of (cost key, gt).
// Every output element is written by exactly one thread per launch sequence; the same bits on every run and in csrc/simota_cpu.cpp.
// Compiled with -ffp-contract=off (csrc/simota_common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "lds_sort.h"
#include "simota_common.h"

namespace simota {

__device__ __forceinline__ void load7(const float* p, float (&r)[7]) {
#pragma unroll
  for (int k = 0; k < 7; ++k) r[k] = p[k];
}

// the cost of (prior n of the sample at p0, gt with constants gk and label) at IoU u
__device__ __forceinline__ float cost_at(const Args& a, long long p0, int n, const GtC& gk, int64_t label, float u) {
  float x = 0.0f, y = 0.0f;
  prior_xy(a.priors, a.prior_stride, a.shared, a.prior_rows, p0, n, x, y);
  const bool both = in_gt(gk, x, y) && in_ct(gk, x, y, a.prm.radius);
  return pair_cost(cls_cost(a.scores + (p0 + n) * a.prm.C, a.prm.C, label), u, both, a.prm);
}

// ------------------------------------------------------------------ candidates, default outputs
__global__ __launch_bounds__(WG) void flag_kernel(const Args a) {
  __shared__ GtC tile[GT_TILE];
  __shared__ int wave_cnt[WG / 64];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = 0, np = 0;
  long long p0 = 0, first = 0;
  if (!row_block(a.pcnt, a.B, a.P, blockIdx.x, b, p0, first, np)) return;   // block uniform
  const long long n = first + tid;
  const bool live = tid < np;
  if (live) {
    a.gt_inds[p0 + n] = 0;
    a.labels[p0 + n] = -1;
    a.max_overlaps[p0 + n] = -1e8f;
  }
  if (b >= a.B) return;                                                      // rows of no sample
  long long g0, gn_all;
  segment_of(a.gcnt, b, a.G, g0, gn_all);
  const int gn = (int)(gn_all < a.G_cap ? gn_all : a.G_cap);
  if (gn == 0) return;
  float x = 0.0f, y = 0.0f;
  const bool have = live && prior_xy(a.priors, a.prior_stride, a.shared, a.prior_rows, p0, n, x, y);
  bool any = false;
  for (int t0 = 0; t0 < gn; t0 += GT_TILE) {                                 // block-uniform trip count
    const int nt = gn - t0 < GT_TILE ? gn - t0 : GT_TILE;
    __syncthreads();
    if (tid < nt) tile[tid] = gt_constants(a.gt + (g0 + t0 + tid) * 7);
    __syncthreads();
    if (have && !any) {
      for (int g = 0; g < nt; ++g) {
        if (in_gt(tile[g], x, y) || in_ct(tile[g], x, y, a.prm.radius)) {
          any = true;
          break;
        }
      }
    }
  }
  const unsigned long long m = __ballot(any);
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < WG / 64; ++w) {
    const int c = wave_cnt[w];
    before += w < wave ? c : 0;
    total += c;
  }
  if (total == 0) return;                                                    // block uniform
  if (tid == 0) base_s = atomicAdd(&a.cand_cnt[b], total);
  __syncthreads();
  if (any) a.cand[p0 + base_s + before + __popcll(m & ((1ull << lane) - 1ull))] = (int)n;
}

// ------------------------------------------------------------------ one gt of one sample: dynamic k, its k matches
constexpr int CAP = 2048;                                       // entries of a selection buffer; a round appends at most WG
constexpr int BUF_BYTES = 8 * (CAP + CAP / 8 + 8);
constexpr int SEL_OFF_VS = 0;
constexpr int SEL_OFF_I = SEL_OFF_VS + (int)sizeof(VertexScratch<NT>);
constexpr int SEL_OFF_C = SEL_OFF_I + BUF_BYTES;
constexpr int QCAP = 2 * WG;                                    // priors queued for clipping; drained once a round more would not fit
constexpr int SEL_OFF_WL = SEL_OFF_C + BUF_BYTES;               // int [QCAP]
constexpr int SEL_OFF_THR = SEL_OFF_WL + QCAP * 4;               // u64 [2]: the K-th best entry of either buffer so far
constexpr int SEL_OFF_CTL = SEL_OFF_THR + 16;                   // int [4]: entries in either buffer, queue length, k
constexpr int SEL_OFF_GT = SEL_OFF_CTL + 16;                    // GtCtx: the workgroup's gt in every form its pairs consume
// kept in LDS and read where used (uniform addresses: broadcasts): held in registers through the kernel, these 35 floats spill
struct GtCtx {
  float gr[7];
  float pad;
  GtC gk;
  Lite gl;
  OBox Bx;
};
constexpr int SEL_LDS = SEL_OFF_GT + (((int)sizeof(GtCtx) + 15) & ~15);
static_assert(SEL_OFF_I % 16 == 0 && SEL_OFF_C % 16 == 0 && SEL_OFF_THR % 16 == 0, "LDS carve offsets");
static_assert(SEL_LDS <= 160 * 1024 && CAP >= 2 * WG, "LDS of a CU; a round must fit behind a cut buffer");

__device__ __forceinline__ void push(unsigned long long* buf, int* cnt, unsigned long long thr, unsigned long long e) {
  if (e > thr) buf[ldssort::PH(atomicAdd(cnt, 1))] = e;
}

// sort the buffer, keep its Kc largest entries and remember the Kc-th as the bar to beat (block uniform; ends on a barrier)
__device__ __forceinline__ void cut(unsigned long long* buf, int* cnt, unsigned long long* thr, int Kc) {
  const int n = *cnt;
  __syncthreads();
  ldssort::bitonic_desc(buf, n);
  if (threadIdx.x == 0) {
    *cnt = n < Kc ? n : Kc;
    *thr = n >= Kc ? buf[ldssort::PH(Kc - 1)] : 0ull;
  }
  __syncthreads();
}

__global__ __launch_bounds__(WG) void select_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  VertexScratch<NT>& vs = *reinterpret_cast<VertexScratch<NT>*>(lds + SEL_OFF_VS);
  unsigned long long* bufI = reinterpret_cast<unsigned long long*>(lds + SEL_OFF_I);
  unsigned long long* bufC = reinterpret_cast<unsigned long long*>(lds + SEL_OFF_C);
  int* wl = reinterpret_cast<int*>(lds + SEL_OFF_WL);
  unsigned long long* thr = reinterpret_cast<unsigned long long*>(lds + SEL_OFF_THR);
  int* ctl = reinterpret_cast<int*>(lds + SEL_OFF_CTL);
  const int tid = threadIdx.x;
  const int g = blockIdx.x, b = blockIdx.y;
  const int K = a.prm.K;
  long long p0, pn, g0, gn_all;
  segment_of(a.pcnt, b, a.P, p0, pn);
  segment_of(a.gcnt, b, a.G, g0, gn_all);
  const int gn = (int)(gn_all < a.G_cap ? gn_all : a.G_cap);
  int32_t* mp = a.match_prior + ((long long)b * a.G_cap + g) * K;
  float* mi = a.match_iou + ((long long)b * a.G_cap + g) * K;
  const int V = g < gn ? (int)clamp_count(a.cand_cnt[b], pn) : 0;
  if (V == 0) {                                                  // block uniform: no such gt, or nothing to take
    if (tid < K) {
      mp[tid] = -1;
      mi[tid] = 0.0f;
    }
    return;
  }
  const int Kc = K < V ? K : V;
  GtCtx& gx = *reinterpret_cast<GtCtx*>(lds + SEL_OFF_GT);
  const float* gr = gx.gr;
  const GtC& gk = gx.gk;
  const OBox& Bx = gx.Bx;
  const Lite& gl = gx.gl;
  const int64_t label = a.glabel[g0 + g];
  const int32_t* cand = a.cand + p0;
  if (tid == 0) {
    load7(a.gt + (g0 + g) * 7, gx.gr);
    gx.gk = gt_constants(gx.gr);
    bev_obox(gx.gr, gx.Bx);
    lite_of(gx.gr, gx.gl);
    ctl[0] = ctl[1] = ctl[2] = 0;
    thr[0] = thr[1] = 0ull;
  }
  __syncthreads();
  for (int base = 0; base < V; base += WG) {                     // block-uniform trip count
    const bool fullC = ctl[1] + WG > CAP;
    __syncthreads();                                             // every thread has read the counts before any thread moves them
    if (fullC) cut(bufC, &ctl[1], &thr[1], Kc);
    const unsigned long long tC = thr[1];
    const int i = base + tid;
    if (i < V) {
      const int n = cand[i];
      if (n >= 0 && n < pn) {
        float pr[7];
        load7(a.boxes + (p0 + n) * 7, pr);
        Lite pa;
        lite_of(pr, pa);
        if (may_overlap(pa, gl)) wl[atomicAdd(&ctl[2], 1)] = n;
        else push(bufC, &ctl[1], tC, cost_entry(cost_at(a, p0, n, gk, label, 0.0f), (unsigned)n));   // IoU exactly 0
      }
    }
    __syncthreads();
    // the queued pairs wait until they fill the clipping lanes several times over, or for the last round: a gt's neighbours arrive
    // a few per round, and NT lanes clipping a handful of pairs cost a round as much as clipping NT of them
    const int q = ctl[2];
    if (q + WG <= QCAP && base + WG < V) continue;               // block uniform
    for (int off = 0; off < q; off += WG) {                      // at most WG entries per buffer between two cuts
      const bool roomI = ctl[0] + WG <= CAP, roomC = ctl[1] + WG <= CAP;
      __syncthreads();                                           // as above
      if (!roomI) cut(bufI, &ctl[0], &thr[0], Kc);
      if (!roomC) cut(bufC, &ctl[1], &thr[1], Kc);
      const unsigned long long uI = thr[0], uC = thr[1];
      const int end = off + WG < q ? off + WG : q;
      if (tid < NT) {
        for (int j = off + tid; j < end; j += NT) {
          const int n = wl[j];
          float pr[7];
          load7(a.boxes + (p0 + n) * 7, pr);
          OBox A;
          bev_obox(pr, A);
          const float u = clean_iou(iou3d<NT>(pr, A, gr, Bx, vs, tid));
          if (u > 0.0f) push(bufI, &ctl[0], uI, iou_entry(u, (unsigned)n));
          push(bufC, &ctl[1], uC, cost_entry(cost_at(a, p0, n, gk, label, u), (unsigned)n));
        }
      }
      __syncthreads();
    }
    if (tid == 0) ctl[2] = 0;
    __syncthreads();
  }
  cut(bufI, &ctl[0], &thr[0], Kc);
  cut(bufC, &ctl[1], &thr[1], Kc);
  if (tid == 0) {
    float sum = 0.0f;
    for (int j = 0; j < ctl[0]; ++j) sum = sum + bits_f32((unsigned)(bufI[ldssort::PH(j)] >> 32));   // descending
    const int k = dynamic_k(sum, Kc);
    ctl[3] = k < ctl[1] ? k : ctl[1];
  }
  __syncthreads();
  const int k = ctl[3];
  if (tid < K) {                                                 // K <= 32 <= NT: the lane owns a column of the vertex scratch
    int n = -1;
    float u = 0.0f;
    if (tid < k) {
      n = (int)entry_prior(bufC[ldssort::PH(tid)]);
      float pr[7];
      load7(a.boxes + (p0 + n) * 7, pr);
      Lite pa;
      lite_of(pr, pa);
      if (may_overlap(pa, gl)) {
        OBox A;
        bev_obox(pr, A);
        u = clean_iou(iou3d<NT>(pr, A, gr, Bx, vs, tid));
      }
    }
    mp[tid] = n;
    mi[tid] = u;
  }
}

// ------------------------------------------------------------------ one sample: distinct priors, conflicts, outputs
constexpr int CB = 256;                                          // conflicted priors whose row minima are in LDS at a time
constexpr int RES_MIN_LDS = (int)sizeof(VertexScratch<NT>) + CB * 8 + 64;

__host__ __device__ inline int resolve_list_bytes(int matches) {
  int p = 8;
  while (p < matches) p <<= 1;
  return 8 * (p + p / 8 + 8);
}

__global__ __launch_bounds__(WG) void resolve_kernel(const Args a, int ctl_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int wave_cnt[WG / 64];
  unsigned long long* list = reinterpret_cast<unsigned long long*>(lds);                 // first the sort list ...
  VertexScratch<NT>& vs = *reinterpret_cast<VertexScratch<NT>*>(lds);                    // ... then the clipping scratch
  unsigned long long* mins = reinterpret_cast<unsigned long long*>(lds + sizeof(VertexScratch<NT>));
  int* ctl = reinterpret_cast<int*>(lds + ctl_off);                                      // [2] matches, conflicts
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int K = a.prm.K;
  const long long L = (long long)a.G_cap * K;
  long long p0, pn, g0, gn_all;
  segment_of(a.pcnt, b, a.P, p0, pn);
  segment_of(a.gcnt, b, a.G, g0, gn_all);
  const int gn = (int)(gn_all < a.G_cap ? gn_all : a.G_cap);
  const int32_t* mp = a.match_prior + (long long)b * L;
  const float* mi = a.match_iou + (long long)b * L;
  int32_t* conf = a.conflict + (long long)b * L;
  int64_t* pos_inds = a.pos_inds + (long long)b * L;
  int64_t* pos_gt = a.pos_gt_inds + (long long)b * L;
  if (tid == 0) ctl[0] = ctl[1] = 0;
  __syncthreads();
  const int S = gn * K;
  for (int s = tid; s < S; s += WG) {
    const int n = mp[s];
    if (n >= 0 && n < pn)
      list[ldssort::PH(atomicAdd(&ctl[0], 1))] = ((unsigned long long)(0xffffffffu - (unsigned)n) << 32) | (unsigned long long)(0xffffffffu - (unsigned)s);
  }
  __syncthreads();
  const int M = ctl[0];
  __syncthreads();
  ldssort::bitonic_desc(list, M);                               // descending entries: ascending prior, then ascending slot
  int run = 0;
  for (int base = 0; base < M; base += WG) {                    // block-uniform trip count
    const int i = base + tid;
    bool first = false, conflicted = false;
    int n = 0, s = 0;
    if (i < M) {
      const unsigned long long e = list[ldssort::PH(i)];
      const unsigned hi = (unsigned)(e >> 32);
      n = (int)(0xffffffffu - hi);
      s = (int)(0xffffffffu - (unsigned)e);
      first = i == 0 || (unsigned)(list[ldssort::PH(i - 1)] >> 32) != hi;
      conflicted = first && i + 1 < M && (unsigned)(list[ldssort::PH(i + 1)] >> 32) == hi;
    }
    const unsigned long long m = __ballot(first);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < WG / 64; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    __syncthreads();
    if (first) {
      const int rank = run + before + __popcll(m & ((1ull << lane) - 1ull));
      pos_inds[rank] = p0 + n;
      if (!conflicted) {
        const int g = s / K;
        a.gt_inds[p0 + n] = g + 1;
        a.labels[p0 + n] = a.glabel[g0 + g];
        a.max_overlaps[p0 + n] = mi[s];
        pos_gt[rank] = g0 + g;
      } else {
        const int c = atomicAdd(&ctl[1], 1);                    // at most M / 2 of them: 2 c + 1 < L
        conf[2 * c] = n;
        conf[2 * c + 1] = rank;
      }
    }
    run += total;
  }
  if (tid == 0) a.pos_cnt[b] = run;
  for (long long r = run + tid; r < L; r += WG) pos_inds[r] = pos_gt[r] = -1;
  __syncthreads();                                              // the sort list is dead: the vertex scratch takes its place
  const int nconf = ctl[1];
  for (int cb = 0; cb < nconf; cb += CB) {                      // block-uniform trip count
    const int nb = nconf - cb < CB ? nconf - cb : CB;
    if (tid < nb) mins[tid] = ~0ull;
    __syncthreads();
    if (tid < NT) {
      for (long long w = tid; w < (long long)nb * gn; w += NT) {
        const int c = (int)(w / gn), h = (int)(w - (long long)c * gn);
        const int n = conf[2 * (cb + c)];
        float pr[7], gr[7];
        load7(a.boxes + (p0 + n) * 7, pr);
        load7(a.gt + (g0 + h) * 7, gr);
        Lite pa, gl;
        lite_of(pr, pa);
        lite_of(gr, gl);
        float u = 0.0f;
        if (may_overlap(pa, gl)) {
          OBox A, Bx;
          bev_obox(pr, A);
          bev_obox(gr, Bx);
          u = clean_iou(iou3d<NT>(pr, A, gr, Bx, vs, tid));
        }
        const float cost = cost_at(a, p0, n, gt_constants(gr), a.glabel[g0 + h], u);
        atomicMin(&mins[c], ((unsigned long long)cost_key(cost) << 32) | (unsigned long long)(unsigned)h);
      }
    }
    __syncthreads();
    if (tid < nb) {                                             // nb <= CB == NT
      const int h = (int)(unsigned)mins[tid];
      const int n = conf[2 * (cb + tid)], rank = conf[2 * (cb + tid) + 1];
      float pr[7], gr[7];
      load7(a.boxes + (p0 + n) * 7, pr);
      load7(a.gt + (g0 + h) * 7, gr);
      Lite pa, gl;
      lite_of(pr, pa);
      lite_of(gr, gl);
      float u = 0.0f;
      if (may_overlap(pa, gl)) {
        OBox A, Bx;
        bev_obox(pr, A);
        bev_obox(gr, Bx);
        u = clean_iou(iou3d<NT>(pr, A, gr, Bx, vs, tid));
      }
      a.gt_inds[p0 + n] = h + 1;
      a.labels[p0 + n] = a.glabel[g0 + h];
      a.max_overlaps[p0 + n] = u;
      pos_gt[rank] = g0 + h;
    }
    __syncthreads();
  }
}

}  // namespace simota

using namespace simota;

extern "C" {

int gd3d_simota_assign(const float* pred_scores, const float* decoded_bboxes, const float* priors, int64_t prior_rows,
                       int64_t prior_stride, int32_t shared_priors, const int32_t* prior_batch_cnt, int64_t P, const float* gt_bboxes,
                       const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B, int32_t C, int32_t G_cap,
                       float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight, float match_init,
                       int64_t* gt_inds, int64_t* labels, float* max_overlaps, int32_t* pos_cnt, int64_t* pos_inds,
                       int64_t* pos_gt_inds, void* workspace, size_t workspace_bytes, void* stream) {
  Args a;
  const int rc = check_args(P, prior_rows, prior_stride, shared_priors, G, B, C, G_cap, center_radius, candidate_topk, iou_weight,
                            cls_weight, match_init, a.prm);
  if (rc != 0) return rc;
  if (prior_batch_cnt == nullptr || gt_batch_cnt == nullptr || pos_cnt == nullptr || workspace == nullptr) return GD3D_E_BADARG;
  if (P > 0 && (pred_scores == nullptr || decoded_bboxes == nullptr || gt_inds == nullptr || labels == nullptr || max_overlaps == nullptr))
    return GD3D_E_BADARG;
  if (prior_rows > 0 && priors == nullptr) return GD3D_E_BADARG;
  if (G > 0 && (gt_bboxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  const long long L = (long long)G_cap * candidate_topk;
  if (L > 0 && (pos_inds == nullptr || pos_gt_inds == nullptr)) return GD3D_E_BADARG;
  if (workspace_bytes < carve(a, workspace, P, B, G_cap, candidate_topk)) return GD3D_E_BADARG;
  const int res_list = resolve_list_bytes((int)L);
  const int res_ctl = res_list > RES_MIN_LDS - 64 ? res_list : RES_MIN_LDS - 64;
  const int res_lds = res_ctl + 64;
  static bool attr_set[64] = {};
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess) return GD3D_E_BADARG;
  if (devid < 0 || devid >= 64 || !attr_set[devid]) {
    hipError_t e = hipFuncSetAttribute((const void*)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SEL_LDS);
    if (e != hipSuccess) return (int)e;
    e = hipFuncSetAttribute((const void*)resolve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            resolve_list_bytes(MAX_MATCHES) + 64);
    if (e != hipSuccess) return (int)e;
    if (devid >= 0 && devid < 64) attr_set[devid] = true;
  }
  a.scores = pred_scores; a.boxes = decoded_bboxes; a.priors = priors; a.prior_rows = prior_rows; a.prior_stride = prior_stride;
  a.shared = shared_priors; a.pcnt = prior_batch_cnt; a.P = P; a.gt = gt_bboxes; a.glabel = gt_labels; a.gcnt = gt_batch_cnt;
  a.G = G; a.B = B; a.G_cap = G_cap; a.gt_inds = gt_inds; a.labels = labels; a.max_overlaps = max_overlaps; a.pos_cnt = pos_cnt;
  a.pos_inds = pos_inds; a.pos_gt_inds = pos_gt_inds;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(a.cand_cnt, 0, (size_t)B * 4, st);
  if (e != hipSuccess) return (int)e;
  if (P > 0) {
    hipLaunchKernelGGL(flag_kernel, dim3((unsigned)(P / WG + B + 1)), dim3(WG), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  if (G_cap > 0) {
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)G_cap, (unsigned)B), dim3(WG), SEL_LDS, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)B), dim3(WG), res_lds, st, a, res_ctl);
  return (int)hipGetLastError();
}

}  // extern "C"
