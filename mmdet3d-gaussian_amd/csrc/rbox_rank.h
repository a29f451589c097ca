// rbox_rank.h — NMS stages 0 and 1 (rbox.hip's head comment): rank_place_kernel, obox_prep_kernel; both can clear control words.
#pragma once
#include "rbox_nms_common.h"

namespace rbox {
// obox_prep_kernel's a.order (nullable): score order computed by the caller; box i of the NMS is boxes[order[i]] (saves the gather pass)
// `zero_words` (nullable; obox_prep_kernel, rank_place_kernel, zero_words_kernel): control words of the queued mask form, cleared here so that no separate fill sits in the stream
// (zero_n words PER GROUP; the first workgroup of group blockIdx.y clears that group's words)
__device__ __forceinline__ void zero_control_words(unsigned* zero_words, int zero_n) {
  if (zero_words != nullptr && blockIdx.x == 0)
    for (int k = threadIdx.x; k < zero_n; k += blockDim.x) zero_words[(size_t)blockIdx.y * zero_n + k] = 0u;
}

__global__ __launch_bounds__(256) void zero_words_kernel(unsigned* words, int per_group) { zero_control_words(words, per_group); }

__global__ __launch_bounds__(256) void obox_prep_kernel(const NmsArgs a, OBox* __restrict__ out, unsigned* zero_words, int zero_n) {
  zero_control_words(zero_words, zero_n);
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t src = a.order != nullptr ? (size_t)a.order[(size_t)g * a.cap + i] : (size_t)i;
  float b[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) b[k] = a.boxes[src * 5 + k];
  OBox o;
  obox_make(b, o);
  out[(size_t)g * a.cap + i] = o;
}

// Score order + prep without torch.sort, for up to RANK_MAX candidates (the heads cut to nms_pre before they call nms_gpu).
// Order = scores descending, ties by ascending index, NaN scores first: what torch.sort(descending=True, stable=True)
// yields.  Every box gets one UNIQUE 64-bit key — (order-preserving map of the float) << 32 | ~index — so its position
// in the order is simply the number of larger keys.  That count is embarrassingly parallel (a single-workgroup bitonic
// sort of 4096 keys is LDS-bandwidth-bound at ~50 us; rocPRIM's radix sort behind torch.sort takes 16-24 us + launches):
// rank_place_kernel below.
constexpr int RANK_MAX = 16384;


__device__ __forceinline__ unsigned long long score_key(float s, unsigned idx) {
  unsigned u = __float_as_uint(s);
  if (s != s) u = 0xfffffffeu;              // any NaN: greatest (+inf maps to 0xff800000); NOT 0xffffffff: rank_place forms u + 1
  else {
    if (u == 0x80000000u) u = 0u;           // -0.0 == +0.0 for the comparison torch.sort makes
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - idx);
}

// lt += #{keys of the lane's row of 16 that are < m}, two instructions per step: step T subtracts m from the key T places away
// in the row — row_ror:T as a DPP operand of v_sub_co_u32 (VOP2 takes DPP on gfx9, VOPC does not) — the borrow (key < m) lands in
// VCC and v_addc adds it.  Sixteen independent rotations of ONE register, no dependent chain, no wait states between the pairs
// (a VCC written by one VALU instruction may be the next one's carry-in).  The leading s_nop covers both DPP hazards (source
// VGPR written by the VALU instruction before: 2 wait states; EXEC written by a VALU instruction: 5) for whatever code the
// compiler puts in front of the block.  Measured on the chip before use (profiles/r06_nms_batched.txt): v_sub_co_u32_dpp
// computes dpp(src0) - src1 as written; v_subREV_co_u32_dpp does NOT compute src1 - dpp(src0): the rotation goes to the
// MINUEND there too (it gives dpp(src1) - src0), which pairs every key with the wrong box.
__device__ __forceinline__ void count_row_keys_below(unsigned ku, unsigned m, int& lt) {
  unsigned tmp;
  asm("s_nop 4\n"
      "v_sub_co_u32 %1, vcc, %2, %3\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:1 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:2 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:3 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:4 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:5 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:6 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:7 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:9 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:10 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:11 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:12 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:13 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:14 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      "v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:15 row_mask:0xf bank_mask:0xf\n v_addc_co_u32 %0, vcc, 0, %0, vcc\n"
      : "+v"(lt), "=&v"(tmp)
      : "v"(ku), "v"(m)
      : "vcc");
}

// rank_place_kernel: a 16-wave workgroup owns SIXTEEN boxes of a group and ALL of the group's keys — wave w counts, for the
// workgroup's boxes, the keys of the w-th sixteenth that are greater.  A wave is four DPP rows of 16 lanes: lane (row q, b) holds the
// workgroup's box b; of every 64 keys the wave loads (lane l builds key jb + l in registers) row q owns keys 16 q .. 16 q + 15 and
// rotates them through its lanes (v_mov_b32_dpp row_ror:1): sixteen steps show every box all 64 keys, one compare per lane and step.
// The four rows' counts meet by two lane exchanges, the sixteen waves' in LDS, and wave 0 places its boxes right away: order[r] = i
// and, for rotated NMS, the OBox record of box i in slot r (this IS the prep kernel, scattered).  No atomics, deterministic.
// (Until round 5 a workgroup owned 64 boxes, one per lane, the 64 keys broadcast by v_readlane: the same number of compare
// instructions, but n / 64 workgroups — 64 at n = 4096 — kept a quarter of the CUs busy; with n / 16 workgroups the kernel covers
// the chip: 14.9 -> 12.0 us averaged over n = 1000 / 4096 / 9000 (6.5 -> 5.2, 31.1 -> 26.4 at the ends).  Rounds 2-3 ran it as two launches — partial counts per 256-key slice in HBM, then a scatter kernel.)
// counts[g] (nullable) = min(#valid boxes of the group, n_keep): every workgroup sees all of the group's valid flags while it
// counts, so workgroup 0 WRITES the number — nothing is cleared and then added to (the round-3 form cleared counts with a memset
// that a captured hipGraph did not order reliably: profiles/r04_nms_queue_ab.txt).
// blockIdx.y = group.  Dense form: scores / valid are (G, n) rows; a box that is not `valid` in its group (nullable mask) gets
// key 0: below every real key, never placed.  Segmented form (seg != nullptr, (G+1) int32 on the device): group g owns the boxes
// [seg[g], seg[g+1]) of ONE flat score array and ranks only those — O(sum n_g^2) compares instead of the dense (G, G n) matrices;
// `n` is then the LARGEST group size (grid extent), indices inside a group are local.  gps > 0: every gps consecutive groups share
// one set of n boxes, set k at rows [k n, (k + 1) n) of the flat box array.
template <bool PREP>
__global__ __launch_bounds__(1024) void rank_place_kernel(const float* __restrict__ boxes, const float* __restrict__ scores_,
                                                          const unsigned char* __restrict__ valid_, const int* __restrict__ seg,
                                                          int n, int n_keep, long long* __restrict__ order_,
                                                          OBox* __restrict__ ob_, int* __restrict__ counts, int gps,
                                                          unsigned* zero_words, int zero_n) {
  __shared__ int spart[16][16];
  __shared__ int svalid[16];
  zero_control_words(zero_words, zero_n);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = (int)(blockDim.x >> 6);                               // waves per workgroup: 16; 4 in the masked dense form (below)
  const int g = blockIdx.y;
  const int sbase = seg != nullptr ? seg[g] : 0;                       // first score / box of the group in the flat arrays
  const int ng = seg != nullptr ? seg[g + 1] - sbase : n;
  if (ng <= 0) {                                                       // uniform: an empty group places nothing
    if (counts != nullptr && blockIdx.x == 0 && tid == 0) counts[g] = 0;
    return;
  }
  if ((int)blockIdx.x * 16 >= ng) return;                              // uniform: no box of this group in this workgroup
  const size_t grow = (size_t)g * n;
  const float* scores = seg != nullptr ? scores_ + sbase : scores_ + grow;
  const unsigned char* valid = (valid_ != nullptr && seg == nullptr) ? valid_ + grow : nullptr;
  const int i = blockIdx.x * 16 + (lane & 15);
  // dense form with a validity mask (multi-class NMS over shared boxes): a workgroup none of whose boxes takes part in this group
  // has nothing to place (workgroup 0 stays: it counts the group's valid boxes), and below a chunk of 64 keys without a valid one
  // is skipped — the work follows the group's own size, not the size of the shared box array
  if (valid != nullptr && blockIdx.x != 0 && __ballot(i < ng && valid[min(i, ng - 1)] != 0) == 0ull) return;   // uniform over the workgroup
  // The compares (round 6).  A key is (order-preserving 32-bit image u of the score, ~index): box i's rank = #{u_j > u_i} +
  // #{u_j == u_i, j < i}.  The workgroup's sixteen boxes lie in ONE chunk of 64 keys, C0; for every other chunk the index part is
  // decided by the chunk alone — keys of an EARLIER chunk count from u_j >= u_i, keys of a LATER chunk from u_j > u_i, i.e.
  // u_j >= u_i + 1 (images end at 0xfffffffe: nothing wraps) — so one 32-bit compare against a per-chunk uniform choice of
  // threshold m decides, counted as its complement: every lane sees 16 keys per chunk, #{u_j >= m} = 16 - #{u_j < m} (the 0 of
  // an unused key is below every m: real images start at 0x007fffff, the image of -inf).  v_sub + v_addc per 64 pairs where the
  // 64-bit keys cost a 64-bit compare, a select, an add and two dependent rotations: 2 against ~6 instructions and their wait
  // states per step.  Only chunk C0 compares whole keys.  (One class alone, 4096 keys: 7.4 -> 7.7 us, unchanged — 4.2 us of that
  // is the dispatch floor; the masked three-class form needed it together with fewer waves: profiles/r06_nms_batched.txt.)
  const int C0 = (int)(blockIdx.x * 16u) >> 6;
  const unsigned long long mine = i < ng ? score_key(scores[i], (unsigned)i) : ~0ull;
  const unsigned mu = (unsigned)(mine >> 32);
  int cnt = 0, nvalid = 0, lt = 0, n32 = 0;
  auto compare = [&](int c, bool use, float sc, int j) {
    if (c != C0) {   // uniform
      const unsigned ku = use ? (unsigned)(score_key(sc, 0u) >> 32) : 0u;
      const unsigned m = c < C0 ? mu : mu + 1u;
      count_row_keys_below(ku, m, lt);
      ++n32;
    } else {
      const unsigned long long kj = use ? score_key(sc, (unsigned)j) : 0ull;   // 0 is below every real key
      unsigned klo = (unsigned)kj, khi = (unsigned)(kj >> 32);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        cnt += (((unsigned long long)khi << 32) | klo) > mine ? 1 : 0;
        klo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)klo, 0x121, 0xf, 0xf, false);   // row_ror:1
        khi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)khi, 0x121, 0xf, 0xf, false);
      }
    }
  };
  if (valid == nullptr) {
    const int q = (((ng + nw - 1) / nw) + 63) & ~63;                     // keys per wave: a sixteenth, in whole chunks of 64
    const int b = wave * q, e = min(b + q, ng);
    for (int jb0 = b; jb0 < e; jb0 += 4 * 64) {   // four chunks' scores in flight together (a lane past the end re-reads the last key)
      float sc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) sc[u] = scores[min(jb0 + 64 * u + lane, ng - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jb = jb0 + 64 * u;
        if (jb >= e) break;   // (uniform)
        const int j = jb + lane;
        const bool use = j < e;
        nvalid += __popcll(__ballot(use));
        compare(jb >> 6, use, sc[u], j);
      }
    }
  } else {
    // Dense form with a validity mask: the group's valid keys are a SUBSET of the shared array (multi-class NMS: class c's 4096
    // candidates among 12 288 boxes).  Round 6 (profiles/r06_nms_batched.txt): 25.6 -> 16.9 us for 3 x 4096 of 12 288 —
    //  * the chunks are dealt INTERLEAVED (wave w: chunks w, w + nw, ...: any run of valid boxes spreads over all waves) and
    //    eight at a time, all sixteen loads independent: one memory round trip per eight chunks where the contiguous sixteenth
    //    per wave paid two per chunk (flag byte, then score) and left ten of sixteen waves without a valid key;
    //  * the launch uses FOUR waves per workgroup in this form: two thirds of the workgroups have no valid box of their group and
    //    leave after one byte load, but every wave of theirs costs dispatch (sweep: 128 threads 23.5 us, 256: 16.9, 512: 16.4,
    //    1024: 22.8; without the 32-bit compares below the busy workgroups were VALU-bound and four waves gained nothing);
    //  * a chunk without a valid key is skipped.
    constexpr int RU = 8;
    const int nchunk = (ng + 63) >> 6;
    for (int c0 = wave; c0 < nchunk; c0 += nw * RU) {
      // sixteen independent loads (eight flag bytes, eight scores; a lane past the end re-reads the group's last key): ONE memory
      // round trip per eight chunks — a score load that waits for its flag serialises the chunks (measured: 0.7 us per chunk)
      unsigned char fb[RU];
      float sc[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int j = min(((c0 + nw * u) << 6) + lane, ng - 1);
        fb[u] = valid[j];
        sc[u] = scores[j];
      }
      bool use[RU];
      unsigned long long usem[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        use[u] = ((c0 + nw * u) << 6) + lane < ng && fb[u] != 0;
        usem[u] = __ballot(use[u]);
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        nvalid += __popcll(usem[u]);
        if (usem[u] == 0ull) continue;   // (uniform)
        compare(c0 + nw * u, use[u], sc[u], ((c0 + nw * u) << 6) + lane);
      }
    }
  }
  cnt += 16 * n32 - lt;         // chunks compared through the 32-bit images: 16 keys each per lane, less those below the threshold
  cnt += __shfl_xor(cnt, 16);   // the four rows hold the same boxes
  cnt += __shfl_xor(cnt, 32);
  if (lane < 16) spart[wave][lane] = cnt;
  if (lane == 0) svalid[wave] = nvalid;
  __syncthreads();
  if (wave != 0) return;
  if (counts != nullptr && blockIdx.x == 0 && lane == 0) {
    int total = 0;
    for (int w = 0; w < nw; ++w) total += svalid[w];
    counts[g] = min(total, n_keep);
  }
  if (lane < 16 && i < ng && (valid == nullptr || valid[i] != 0)) {
    int r = 0;
    for (int w = 0; w < nw; ++w) r += spart[w][lane];
    if (r < n_keep) {
      const int bbase = seg != nullptr ? sbase : (gps > 0 ? (g / gps) * n : 0);
      order_[(size_t)g * n_keep + r] = (long long)(bbase + i);
      if (PREP) {
        float bx[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) bx[k] = boxes[(size_t)(bbase + i) * 5 + k];
        OBox o;
        obox_make(bx, o);
        ob_[(size_t)g * n_keep + r] = o;
      }
    }
  }
}
}  // namespace rbox
