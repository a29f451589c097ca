// rbox_scan.h — NMS stage 3 (rbox.hip's head comment), the greedy scan: classic, list, and the two-level form's propagate kernel.
#pragma once
#include <type_traits>
#include "rbox_nms_common.h"

namespace rbox {
// wave-wide OR on the DPP network (row_shr 1/2/4/8 inside each row of 16, row_bcast 15 / 31 across rows; lane 63 holds
// the result): replaces up to 64 same-address ds_or_b64, which the LDS serialises.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned int dpp_or(unsigned int v) {
  return v | (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
__device__ __forceinline__ unsigned int wave_or_u32(unsigned int v) {
  v = dpp_or<0x111, 0xf>(v);
  v = dpp_or<0x112, 0xf>(v);
  v = dpp_or<0x114, 0xf>(v);
  v = dpp_or<0x118, 0xf>(v);
  v = dpp_or<0x142, 0xa>(v);
  v = dpp_or<0x143, 0xc>(v);
  return (unsigned int)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
  // the two halves interleaved: every DPP step has to wait for the VALU result before it (two wait states); with two independent
  // chains one half's step fills the other's wait
  unsigned int lo = (unsigned int)v, hi = (unsigned int)(v >> 32);
  lo = dpp_or<0x111, 0xf>(lo); hi = dpp_or<0x111, 0xf>(hi);
  lo = dpp_or<0x112, 0xf>(lo); hi = dpp_or<0x112, 0xf>(hi);
  lo = dpp_or<0x114, 0xf>(lo); hi = dpp_or<0x114, 0xf>(hi);
  lo = dpp_or<0x118, 0xf>(lo); hi = dpp_or<0x118, 0xf>(hi);
  lo = dpp_or<0x142, 0xa>(lo); hi = dpp_or<0x142, 0xa>(hi);
  lo = dpp_or<0x143, 0xc>(lo); hi = dpp_or<0x143, 0xc>(hi);
  return ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)hi, 63) << 32) |
         (unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)lo, 63);
}
// ---- greedy scan: one workgroup, phase-shifted waves, one LDS-only barrier per 64-box block ("interval") -------------
// Measured with a cycle-stamp build (profiles/r05_nms_scan_stamps.txt): a global-memory round trip from this CU is ~2700 cycles,
// a resolved block ~1200.  So no wave may load and use a value inside one interval:
//   wave 0 (resolver) reads what the NEXT block waits for — colm[64t+l] and the first "urgent" word mask[64t+l][t+1] — from an
//     LDS ring that other waves filled one interval earlier.  It solves the block wave-parallel (kept = alive; kept' = alive &
//     ~ballot(col & kept) until stable: the unique solution of the triangular system the greedy order defines), publishes the
//     kept word and the compacted lane list, and carries the OR of the kept lanes' first urgent word to the next block in
//     registers (a full DPP reduction; round 5).
//   field waves (3, one per phase) fetch the resolver's inputs for block t0+3 (five fields per box), and in the interval in which
//     their loads fly run the SCRIBE step of block t0: kept ids to `keep`, urgent words 2 and 3 OR-ed into remv[t0+2], remv[t0+3],
//     the running count (round 5: until then all of that sat on the resolver's critical path).
//   waves 1..12 (3 groups x SCAN_GW row waves, group j phase-shifted by j intervals) run super-iterations of three intervals:
//     interval t0      ISSUE  : loads of the mask rows kept in block t0-1 (words >= t0+3; the group's waves split the rows);
//     interval t0+1    nothing (the loads are in flight across two barriers; straight-line code inside ONE loop
//                               iteration, so the compiler waits for them only at their first use);
//     interval t0+2    CONSUME: OR the rows into remv (ds_or_b64).
//   Block b's rows therefore reach remv[w >= b+4] during interval b+3, one barrier before block b+4 is resolved; words
//   b+1..b+3 are covered by the urgent words.  Every wave executes exactly cb barriers.
//   What bounds it (profiles/r05_nms_pmc.txt): a wave issues one instruction per ~10 cycles here (4 waves per SIMD, dependent
//   scalar/vector chains), and an interval lasts as long as its longest instruction stream: the row waves' ISSUE (~90
//   instructions for 4 rows), then the resolver (~60) and the CONSUME (~50).
// History: one scalar readlane step per kept box + load->use inside the interval: 1.2-3.8 us per block.
constexpr int SCAN_GW = 4;                          // row waves per propagate group
constexpr int SCAN_U = 16;                          // rows in flight per row wave: SCAN_GW x SCAN_U = 64 = every box of a block
constexpr int SCAN_T = 64 * (1 + 3 * SCAN_GW + 3);  // 1024 threads: resolver, 3 x 4 row waves, 3 field waves
constexpr int SCAN_NU = 3;                      // urgent words per box
constexpr int SCAN_RING = 4;

__device__ __forceinline__ unsigned int lds_offset(const void* p) {   // byte offset of a __shared__ object (ds_* address operand)
  return (unsigned int)(unsigned long long)(const __attribute__((address_space(3))) void*)p;
}

__device__ __forceinline__ void lds_barrier() {  // orders LDS only: global loads stay in flight across it
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  // (the builtin returns a signed int: go through unsigned before widening)
  return ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
}

constexpr int SCAN_SB = 64;         // blocks per super-block (4096 boxes): rows inside it fit the one-chunk scan variant

// U rows x CH 64-word chunks in flight per propagate lane (registers: 2*U*CH VGPRs); rows / chunks beyond that are OR-ed
// in synchronously during the issue interval (correct, slower; only very dense keeps or n > 64*(64*CH+4)).
template <int U, int CH>
__device__ __forceinline__ void nms_scan_body(const NmsArgs& a, const unsigned long long* __restrict__ mask_,
                                              const unsigned long long* __restrict__ colm_,
                                              long long* __restrict__ keep_, long long* __restrict__ num_keep,
                                              const ScanWindow& win) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long remv[];  // cbs words
  __shared__ unsigned long long skept[4];
  __shared__ int scount;        // boxes kept before the block the next scribe step handles (handed from field wave to field wave)
  __shared__ int klist[4][64];  // lane indices of the boxes kept in a block, compacted (k-th kept box -> lane)
  __shared__ unsigned long long rin[SCAN_RING][2 + SCAN_NU][64];  // [slot][col, urgent 1..3, id][lane]
  const int g = blockIdx.x;  // one workgroup per group
  const int n = group_n(a, g);
  const int cb_all = (n + 63) >> 6;
  const bool windowed = win.gremv != nullptr;
  const int c_begin = windowed ? win.c_begin : 0;
  const int cb = windowed ? min(win.c_end, cb_all) : cb_all;   // every "< cb" below means "inside this launch's range"
  const size_t cbs = (size_t)a.cbs;
  unsigned long long* gremv = windowed ? win.gremv + (size_t)g * cbs : nullptr;
  unsigned long long* gkept = windowed ? win.gkept + (size_t)g * cbs : nullptr;
  if (windowed && c_begin >= cb_all) {                          // uniform: this group ends before the super-block
    // an EMPTY group (cb_all == 0) never reaches a resolver: the first launch records its count here, as the
    // single-level scan does (callers allocate num_keep uninitialised)
    if (c_begin == 0 && threadIdx.x == 0) num_keep[g] = 0;
    return;
  }
  const long long* order = a.order != nullptr ? a.order + (size_t)g * a.cap : nullptr;
  const unsigned long long* mask = mask_ + (size_t)g * a.cap * cbs;
  const unsigned long long* colm = colm_ + (size_t)g * a.cap;
  long long* keep = keep_ + (size_t)g * a.cap;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int w = c_begin + tid; w < cb; w += SCAN_T) remv[w] = (windowed && c_begin > 0) ? gremv[w] : 0ull;
  if (windowed && c_begin == 0)   // the first super-block opens the global removed-set for everything right of it
    for (int w = cb + tid; w < cb_all; w += SCAN_T) gremv[w] = 0ull;
  if (tid < 4) skept[tid] = 0ull;
  // (windowed: the running count travels from launch to launch in the workspace word gcount[g]; num_keep[g] is written ONCE, by
  //  the launch that resolves the group's last block — a caller may point num_keep at pinned host memory and poll it)
  if (tid == 0) scount = (windowed && c_begin > 0) ? (int)win.gcount[g] : 0;
  lds_barrier();
  const int NB = cb - c_begin;  // intervals = barriers every wave executes in the main phase

  // resolver inputs of block B for this lane (0 where the box or the word does not exist)
  // field f of block B for this lane: 0 = column word, 1..3 = urgent words mask[i][B+f], 4 = box id.  (Contiguous
  // copies of the urgent words were tried: +7 us in the mask kernel at n = 4096, nothing gained here.)
  auto load_field = [&](int B, int f) -> unsigned long long {
    const int i = B * 64 + lane;
    const bool ok = B < cb && i < n;
    if (f == 0) return ok ? colm[i] : 0ull;
    if (f <= SCAN_NU) return (ok && B + f < cb) ? mask[(size_t)i * cbs + B + f] : 0ull;
    return (unsigned long long)((ok && order != nullptr) ? order[i] : (long long)i);
  };

  if (wave == 0) {
    // ---------------------------------------------------------------- resolver
    for (int B = c_begin; B < c_begin + 3; ++B) {  // the first three blocks: nobody runs ahead of them
#pragma unroll
      for (int f = 0; f < 2 + SCAN_NU; ++f) rin[B & (SCAN_RING - 1)][f][lane] = load_field(B, f);
    }
    // Round 5: the resolver keeps ONLY what the next block waits for.  Per block: the column word and the FIRST urgent word from
    // the ring, remv[c] from LDS, the fixed point, the kept word + compacted lane list published for the row waves, and the OR
    // of the kept lanes' first urgent word carried to the next block IN REGISTERS (a full DPP reduction: no LDS atomic and no
    // LDS round trip between two blocks).  Everything else a kept block owes — the kept ids to `keep`, the urgent words 2 and 3
    // into remv[c+2], remv[c+3], the running count — is done ONE INTERVAL LATER by the field wave that idles in that interval
    // (`scribe` below): off the critical path.  Until then the resolver's own stream was the scan's critical path at clustered
    // scenes (stamps, profiles/r05_nms_pmc.txt: lds 180 | solve 176 | ids + urgent ORs + lists 580 | barrier 116 of 1052 cycles).
    unsigned long long carry = 0ull;   // kept boxes of the previous block -> removed lanes of this one
    for (int c = c_begin; c < cb; ++c) {
      const int slot = c & (SCAN_RING - 1);
      const unsigned long long col = rin[slot][0][lane];
      unsigned long long urg1 = rin[slot][1][lane];
      const unsigned int clo = (unsigned int)col, chi = (unsigned int)(col >> 32);
      unsigned long long cur = uniform_u64(remv[c]) | carry;
      const int nvalid = min(64, n - c * 64);
      if (nvalid < 64) cur |= ~0ull << nvalid;
      const unsigned long long alive = ~cur;
      unsigned long long kept = alive;
      for (;;) {  // <= 65 rounds; the fixed point is the greedy keep set of the block
        const bool sup = ((clo & (unsigned int)kept) | (chi & (unsigned int)(kept >> 32))) != 0u;
        const unsigned long long nk = alive & ~__ballot(sup);
        if (nk == kept) break;
        kept = nk;
      }
      const bool mine = (kept >> lane) & 1ull;
      if (mine) klist[c & 3][__builtin_popcountll(kept & ((1ull << lane) - 1ull))] = lane;
      if (lane == 0) skept[c & 3] = kept;
      urg1 = mine ? urg1 : 0ull;
      carry = (c + 1 < cb) ? wave_or_u64(urg1) : 0ull;   // (uniform bound)
      lds_barrier();
    }
    if (NB == 0 && lane == 0) num_keep[g] = 0;   // an empty group: no block, no scribe step (a windowed launch returned above)
  } else {
    // ---------------------------------------------------------------- propagate / loader groups
    // Round 4: the resolver's inputs (five fields per box of block t + 3) are fetched by three FIELD waves of their own, one
    // per phase; the nine row waves only spread kept rows.  Until then rank 0 / 1 / 2 of a group also loaded two / two / one
    // field, and the group's issue interval (~250 dependent instructions at the 5-6 cycles a lone wave pays each) was as long
    // as the whole interval — the scan's critical stream together with the resolver (profiles/r04_nms_pmc.txt).
    const bool field_wave = wave > 3 * SCAN_GW;
    const int grp = field_wave ? wave - 1 - 3 * SCAN_GW : (wave - 1) / SCAN_GW;
    const int rank = field_wave ? 0 : (wave - 1) - grp * SCAN_GW;
    const int lead = min(grp, NB);
    const int S = (NB - lead) / 3;
    const int trail = NB - lead - 3 * S;
    for (int q = 0; q < lead; ++q) lds_barrier();
    if (field_wave) {
      // scribe: what block c owes beyond the resolver's critical path (see there), run by a field wave during the interval AFTER
      // block c was resolved — the one of its three intervals in which it used to wait for its loads.  The ring still holds the
      // block's fields (slot c & 3 is rewritten three intervals later), skept / klist are the resolver's, the count of boxes
      // kept so far travels from scribe to scribe through `scount`.
      auto scribe = [&](int c) {
        const int slot = c & (SCAN_RING - 1);
        const unsigned long long kept = uniform_u64(skept[c & 3]);
        unsigned long long urg[SCAN_NU - 1];
#pragma unroll
        for (int k = 0; k < SCAN_NU - 1; ++k) urg[k] = rin[slot][2 + k][lane];
        const long long id = (long long)rin[slot][1 + SCAN_NU][lane];
        const int count = __builtin_amdgcn_readfirstlane(scount);
        const bool mine = (kept >> lane) & 1ull;
        if (mine)  // with `order` the kept indices come out already mapped to the caller's box numbering
          keep[count + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = id;
        // the kept lanes' urgent words 2.. : OR-reduced inside every QUAD of lanes on the DPP network, then lanes 3, 7, ... 63 OR
        // their quad's totals into remv[c+2..] with ds_or_b64 (16 same-address LDS atomics per word; written out because an
        // atomicOr() here is rewritten into a readlane loop over the active lanes plus a scalar round trip)
#pragma unroll
        for (int k = 0; k < SCAN_NU - 1; ++k) urg[k] = mine ? urg[k] : 0ull;
        {
          unsigned int h[2 * (SCAN_NU - 1)];
#pragma unroll
          for (int k = 0; k < SCAN_NU - 1; ++k) {
            h[2 * k] = (unsigned int)urg[k];
            h[2 * k + 1] = (unsigned int)(urg[k] >> 32);
          }
#pragma unroll
          for (int k = 0; k < 2 * (SCAN_NU - 1); ++k) h[k] = dpp_or<0x111, 0xf>(h[k]);   // row_shr:1
#pragma unroll
          for (int k = 0; k < 2 * (SCAN_NU - 1); ++k) h[k] = dpp_or<0x112, 0xf>(h[k]);   // row_shr:2 -> lane 4q+3 holds quad q
#pragma unroll
          for (int k = 0; k < SCAN_NU - 1; ++k) urg[k] = ((unsigned long long)h[2 * k + 1] << 32) | h[2 * k];
        }
        if ((lane & 3) == 3) {
#pragma unroll
          for (int k = 0; k < SCAN_NU - 1; ++k)
            if (c + 2 + k < cb)   // (uniform bound)
              asm volatile("ds_or_b64 %0, %1" ::"v"(lds_offset(&remv[c + 2 + k])), "v"(urg[k]) : "memory");
        }
        if (lane == 0) {
          const int total = count + __builtin_popcountll(kept);
          scount = total;
          if (windowed) gkept[c] = kept;
          if (c == cb - 1) {
            if (windowed) win.gcount[g] = total;
            if (cb == cb_all) num_keep[g] = total;
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the ds_or_b64 above are inline asm: the compiler does not count them
      };
      for (int s2 = 0; s2 < S; ++s2) {
        const int t0 = c_begin + grp + 3 * s2;
        // ---- interval t0: issue the loads of block t0 + 3's inputs (constant field ids: a run-time id cost ~430 cycles per field)
        unsigned long long in[2 + SCAN_NU];
#pragma unroll
        for (int f = 0; f < 2 + SCAN_NU; ++f) in[f] = load_field(t0 + 3, f);
        lds_barrier();
        // ---- interval t0+1: the loads fly; block t0 was resolved in the interval before: its scribe step
        scribe(t0);
        lds_barrier();
        // ---- interval t0+2: into the ring (first USE of the loaded registers pinned here, see the row waves)
#pragma unroll
        for (int f = 0; f < 2 + SCAN_NU; ++f) asm volatile("" : "+v"(in[f]));
        if (t0 + 3 < cb) {
          const int slot = (t0 + 3) & (SCAN_RING - 1);
#pragma unroll
          for (int f = 0; f < 2 + SCAN_NU; ++f) rin[slot][f][lane] = in[f];
        }
        lds_barrier();
      }
      // the trailing intervals of this wave (no block left to fetch): interval tq = lead + 3 S + q; its scribe step falls on q == 1
      const int tq = c_begin + lead + 3 * S;
      for (int q = 0; q < trail; ++q) {
        if (q == 1) scribe(tq);
        lds_barrier();
      }
      // the LAST block was resolved in the last interval: its scribe step comes after the last barrier, from the field wave
      // whose turn it would be (block cb - 1 belongs to the phase of group (NB - 1) % 3)
      if (NB > 0 && grp == (NB - 1) % 3) scribe(cb - 1);
      return;
    }

    for (int s2 = 0; s2 < S; ++s2) {
      const int t0 = c_begin + grp + 3 * s2;
      // ---- interval t0: issue
      const int bk = t0 - 1;             // block whose kept rows this group spreads
      const int first = t0 + SCAN_NU;    // = bk + 1 + SCAN_NU: first word not covered by the urgent words
      // both LDS reads of the interval issued together, unconditionally (one round trip instead of two back to back: the kept
      // word used to be read under the bounds test and waited for before the lane list was even requested; ~120 of the issue
      // interval's ~650 cycles).  bk & 3 is a valid slot even for bk = c_begin - 1; its stale content is masked right below.
      // (written out: left to the compiler the first read is waited for — its value feeds scalar code — before the second is issued)
      unsigned long long kbv;
      int myl;
      asm volatile("ds_read_b64 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(kbv), "=&v"(myl)
                   : "v"(lds_offset(&skept[bk & 3])), "v"(lds_offset(&klist[bk & 3][(rank + SCAN_GW * lane) & 63]))
                   : "memory");
      unsigned long long kb = uniform_u64(kbv);
      if (!(bk >= c_begin && first < cb)) kb = 0ull;   // (uniform)
      // this wave's share: every SCAN_GW-th kept box, read from the compacted list the resolver left in LDS: lane u
      // fetches the row of slot u, the slots then cost a v_readlane + multiply + load each (a lone wave pays ~5 cycles
      // per instruction: walking the kept bits with ffbl / and / compare cost more than the memory round trip)
      const int cnt = __builtin_popcountll(kb);
      const int m = cnt > rank ? (cnt - rank + SCAN_GW - 1) / SCAN_GW : 0;  // rows of this wave (uniform)
      // (the lane-list read above is unconditional: a lane beyond m reads a stale or foreign slot that no readlane below ever
      //  selects; predicating the read on lane < m made it wait for the kept word's own LDS round trip first)
      const unsigned long long* blk = mask + (size_t)(max(bk, c_begin) * 64) * cbs;
      // Loads are unconditional per lane: the word index is clamped into the row (w < cb is the same for every row of a
      // chunk, so the surplus lanes are masked ONCE, at consume time) — a per-row lane predicate cost ~100 cycles per
      // row in exec-mask handling.  (Leaving the registers of absent row pairs unwritten and guarding their use at consume time
      // was tried in round 4: the compiler then copies every loaded value at the end of its conditional block — a use right
      // behind the load, one memory round trip per pair: 500 cycles each.  The zero fill below is the cheap form.)
      unsigned long long v[U][CH];
      unsigned int wcl[CH];
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) wcl[ch] = (unsigned int)min(first + ch * 64 + lane, cb - 1);
      static_assert(U % 2 == 0 && U * SCAN_GW >= 64, "rows are issued in pairs; a group's waves cover a whole block");
      const int mlast = max(m - 1, 0);
      const unsigned int myrow = (unsigned int)myl * (unsigned int)cbs;   // word offset of this lane's row inside the block (< 64 * 1024)
#pragma unroll
      for (int u = 0; u < U; u += 2) {  // pairs: half the uniform branches; an odd tail re-loads its last row (OR is idempotent).
        // (Fours were tried in round 5: n = 4096 clustered 52.4 -> 51.6 us, but the dense scenes lose more — 64.4 -> 65.6 us,
        //  n = 9000 147.0 -> 149.9 us: three clamped row indices per group instead of one per pair.)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) v[u][ch] = v[u + 1][ch] = 0ull;
        if (u < m) {  // uniform
          // row base as a UNIFORM pointer (scalar registers) + the lane's word as the vector offset: one readlane, one 64-bit
          // shift-add and the load per row (the row offset is multiplied out once per lane above, not once per row on the scalar
          // unit; adding it to the lane's word first made the whole address vector arithmetic: three VALU instructions per row)
          const unsigned long long* const r0 = blk + (unsigned int)__builtin_amdgcn_readlane((int)myrow, u);
          const unsigned long long* const r1 = blk + (unsigned int)__builtin_amdgcn_readlane((int)myrow, min(u + 1, mlast));
#pragma unroll
          for (int ch = 0; ch < CH; ++ch) {
            v[u][ch] = r0[wcl[ch]];
            v[u + 1][ch] = r1[wcl[ch]];
          }
        }
      }
      if (m > U || (m > 0 && first + 64 * CH < cb)) {  // overflow: finish it now, synchronously (rare)
        for (int w0 = first; w0 < cb; w0 += 64) {
          const int w = w0 + lane;
          unsigned long long acc = 0ull;
          for (int u = (w0 - first) < 64 * CH ? U : 0; u < m; ++u) {
            const unsigned int off = (unsigned int)__builtin_amdgcn_readlane((int)myrow, u);
            if (w < cb) acc |= blk[off + (unsigned int)w];
          }
          if (acc) atomicOr(&remv[w], acc);
        }
      }
      lds_barrier();
      // ---- interval t0+1: the loads fly
      lds_barrier();
      // ---- interval t0+2: consume.  The empty asm pins the first USE of every loaded register here: without it the
      // scheduler hoists the (pure VALU) OR tree above the two barriers and has to wait for the loads before them.
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) asm volatile("" : "+v"(v[u][ch]));
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        unsigned long long acc = 0ull;
#pragma unroll
        for (int u = 0; u < U; ++u) acc |= v[u][ch];
        const int w = first + ch * 64 + lane;
        if (w < cb && acc) atomicOr(&remv[w], acc);  // ds_or_b64: waves merge into the same words
      }
      lds_barrier();
    }
    for (int q = 0; q < trail; ++q) lds_barrier();
  }
}

// the classic scan as a kernel of its own (single-level, or one super-block of the two-level form)
template <int U, int CH>
__global__ __launch_bounds__(SCAN_T) void nms_scan_kernel(const NmsArgs a, const unsigned long long* __restrict__ mask_,
                                                          const unsigned long long* __restrict__ colm_,
                                                          long long* __restrict__ keep_, long long* __restrict__ num_keep,
                                                          const ScanWindow win) {
  nms_scan_body<U, CH>(a, mask_, colm_, keep_, num_keep, win);
}

// ---- LIST scan (round 5): the greedy scan on per-box VICTIM LISTS and one state BYTE per box in LDS ----------------------------------
// The classic scan above keeps the removed-set as bit words and PUSHES whole 512-byte mask rows of every kept box through twelve row
// waves; its interval is an instruction stream of ~90 (row waves) / ~60 (resolver) instructions, and a wave issues one instruction
// per ~8 cycles.  Here the clip kernel, which finds every pair (i < j, IoU > thr) anyway, also appends j to box i's near or far
// VICTIM LIST when j lies in a later 64-block (in-block pairs stay in colm), and the scan is:
//   state byte of box j (stb[j], LDS): 0 alive so far | 0x01 a kept earlier box suppresses it | after its block was resolved:
//                                      0x80 kept, 0x02 not kept;
//   block c, resolver wave:  alive = (stb == 0) per lane -> in-block fixed point over colm (skipped when no box of the block has an
//                            in-block candidate) -> kept; own byte := 0x80 / 0x02; kept lanes write 0x01 to their NEAR victims
//                            (blocks c + 1 .. c + LIST_K) — the LDS addresses of those bytes sit in a ring that helper waves filled
//                            long before, four per instruction pair;
//   helper wave of block c:  after the block is resolved, writes 0x01 to the FAR victims (blocks > c + LIST_K) of its kept boxes and
//                            sets fdone[c]; the resolver looks at fdone[c - LIST_K - 1] before it reads block c's bytes.
// What bounds it is the RESOLVER's instruction stream (~30 instructions per block on the usual path, one LDS round trip — its own
// state bytes — on the dependent chain), so everything that can be prepared is prepared by the helpers.  The resolver works in
// groups of four blocks, the body instantiated four times with the slot offsets as instruction offsets, and with two register sets
// (block c + 2's fields are fetched while block c is worked on).  No barrier in the loop: the workgroup synchronises through LDS
// words (one CU's LDS executes every wave's accesses in issue order, so "data, then flag" by the writer and "flag, then data" by the
// reader is enough; compiler fences keep the statements in that order):
//   rflag[slot] = (ring generation + 1) << 8 | (some column word non-zero) << 7 | near chunks (0..4),
//                 written by a helper AFTER the slot's fields; re-read by the resolver only if the block is not there yet;
//   stb[64 t]     polled by helper waves (s_sleep) for "block t resolved";   fdone[]  as above.
// Twelve helper waves (those that do not share the resolver's SIMD: waves w, w + 4, w + 8, w + 12 sit on one SIMD — HW_ID), wave g
// serving blocks t = g, g + 12, ...: issue the loads of block t's far list (as many uint4 as the block's longest far list needs: the
// counts were loaded one iteration earlier) and of block t + 16's near list / column word / id, wait for block t, far victims,
// fdone, count the kept boxes since its last block (the running count is the helper's own business), put block t + 16 into the
// ring slot block t just vacated (same wave, same iteration: no other ordering needed), write block t's kept ids.  The prologue
// fills the ring with all sixteen waves in one memory round trip.  Every polling loop is bounded (a bug must not hang the GPU): the
// scan is then marked failed and num_keep = -1.
// Two things this kernel is sensitive to, both measured (profiles/r05_nms_pmc.txt): (a) CODE SIZE — every launch starts with a cold
// instruction cache; a first build (resolver unrolled over all 16 slots, list loops unrolled: 61 KB) spent 2000-4000 cycles per
// block in its first pass; (b) the BYTES the helpers load — with one 128-byte list per box loaded twice per block the resolver ran at
// half speed although it never waited for a helper: hence near / far lists split by the clip kernel and far loads sized by count.
// Same greedy decisions by construction.  A full list or an overflowed block pair sets *lfail in the clip kernel: the workgroup then
// runs the CLASSIC scan instead (same launch: no second kernel).
// History (n = 9000, thr 0.7, scan kernels only): classic two-level ~100 us; pull formulation (suppressor lists, kept bits gathered)
// 66.8 us, 44.4 us once its field waves no longer kept loaded fields in SCRATCH memory (a select between two uint4 objects), 23.5 us
// with kept bytes, no barrier and an unrolled resolver — for thresholds >= 0.5 only; this push formulation serves every threshold.
constexpr int LIST_RING = 16;
constexpr int LIST_HW = 12;
constexpr int LIST_SPIN_MAX = 1 << 22;
constexpr int LIST_POLL_SLEEP = 2;

// volatile accesses that stay LDS instructions (a volatile access through a generic pointer becomes a flat_load / flat_store with an
// immediate wait)
typedef __attribute__((address_space(3))) unsigned int lds_u32;
typedef __attribute__((address_space(3))) unsigned char lds_u8;
__device__ __forceinline__ unsigned int lds_peek(const unsigned int* p) { return *(const volatile lds_u32*)p; }
__device__ __forceinline__ void lds_poke(unsigned int* p, unsigned int v) { *(volatile lds_u32*)p = v; }
// the byte at an LDS ADDRESS held in a register (ds_write_b8 vaddr, v: no base to add — the instruction's 16-bit offset field cannot
// reach an array the compiler placed beyond 64 KB)
__device__ __forceinline__ void lds_mark_at(unsigned int addr) { *(lds_u8*)(size_t)addr = 1; }
#define COMPILER_FENCE() asm volatile("" ::: "memory")
__device__ __forceinline__ int wave_max_i32(int m) {   // uniform result
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x111, 0xf, 0xf, true));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x112, 0xf, 0xf, true));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x114, 0xf, 0xf, true));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x118, 0xf, 0xf, true));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x142, 0xa, 0xf, false));
  m = max(m, __builtin_amdgcn_update_dpp(0, m, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(m, 63);
}

struct RingFields {      // what a ring slot is made of, as loaded
  uint4 n0, n1;          // the near list: sixteen 16-bit ids
  uint2 cnt;             // near / far count
  unsigned long long col;
  long long id;
};

// returns false — before anything was written — when the clip kernel's failure word says that the lists are unusable
__device__ __forceinline__ bool nms_list_body(const NmsArgs& a, const unsigned long long* __restrict__ colm_,
                                              const unsigned short* __restrict__ lists_, const unsigned* __restrict__ lcnt_,
                                              unsigned lblock,
                                              long long* __restrict__ keep_, long long* __restrict__ num_keep_) {
  constexpr int SB = (int)LIST_MAX_N + 384;
  __shared__ __attribute__((aligned(16))) unsigned char stb[SB];   // state byte per box; [LIST_DUMMY + 4 lane] are scratch
  __shared__ unsigned int rent[LIST_RING][LIST_NEAR][64];    // [slot][k][lane]: LDS address of the state byte of the lane's k-th near victim
  __shared__ unsigned long long rcol[LIST_RING][64], rid[LIST_RING][64];
  __shared__ unsigned int rflag[LIST_RING];
  __shared__ unsigned int fdone[256 + LIST_K + 1 + 7];       // [b + LIST_K + 1] != 0: the far victims of block b's kept boxes are marked
  __shared__ unsigned int failed;                            // a polling loop gave up: the result is void (num_keep = -1)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x;  // one workgroup per group
  const int n = group_n(a, g);
  const int cb = (n + 63) >> 6;
  const long long* order = a.order != nullptr ? a.order + (size_t)g * a.cap : nullptr;
  const unsigned long long* const colm = colm_ + (size_t)g * a.cap;
  const unsigned short* const lists = lists_ + (size_t)g * a.cap * (LIST_NEAR + LIST_FAR);
  const unsigned* const lcnt = lcnt_ + (size_t)g * lblock;   // the group's counters, then (last 64 words of the block) its failure word
  const unsigned* const lfail = lcnt + (lblock - 64u);
  long long* const keep = keep_ + (size_t)g * a.cap;
  long long* const num_keep = num_keep_ + g;
  const unsigned short* const flists = lists + (size_t)a.cap * LIST_NEAR;
  const uint2* const cnt2 = reinterpret_cast<const uint2*>(lcnt);
  const unsigned int sb0 = (unsigned int)(size_t)(lds_u8*)stb;   // LDS address of stb[0]: the ring holds ADDRESSES of state bytes
  const unsigned int mydummy = (unsigned int)LIST_DUMMY + 4u * (unsigned int)lane;   // (same-address byte writes of many lanes would be serialised)
  for (int w = tid; w < SB / 4; w += SCAN_T) reinterpret_cast<unsigned int*>(stb)[w] = 0u;
  if (tid < LIST_RING) rflag[tid] = 0u;
  if (tid < 256 + LIST_K + 1) fdone[tid] = tid <= LIST_K ? 1u : 0u;   // (nothing to wait for before block LIST_K + 1)
  if (tid == 0) failed = 0u;
  // The resolver works in groups of four blocks: blocks cb .. cbp - 1 are PADDING, entered into the ring like real ones; the state
  // bytes of everything past box n - 1 start as "suppressed".
  const int cbp = (cb + 3) & ~3;

  // ---- helper-side pieces.  Nothing may touch a loaded value before its consumer — not even a select: a use makes the compiler wait
  // for the load where the use stands (rows are read from a clamped index and masked where they are consumed).
  auto load_ring = [&](int B) -> RingFields {
    RingFields f;
    const int j = min(B * 64 + lane, n - 1);   // n >= 1 here
    const uint4* const l4 = reinterpret_cast<const uint4*>(lists + (size_t)j * LIST_NEAR);
    f.n0 = l4[0];
    f.n1 = l4[1];
    f.cnt = cnt2[j];
    f.col = colm[j];
    f.id = order != nullptr ? order[j] : (long long)j;
    return f;
  };
  auto store_ring = [&](int B, const RingFields f) {   // whole wave; (B < cbp is the caller's business)
    const int slot = B & (LIST_RING - 1);
    const bool ok = B * 64 + lane < n;
    const int cnt = ok ? (int)min(f.cnt.x, (unsigned)LIST_NEAR) : 0;
    unsigned int* const row0 = &rent[slot][0][lane];
    const unsigned int dummy = sb0 + mydummy;
    const int chunks = (wave_max_i32(cnt) + 3) >> 2;        // rows the resolver will look at
    auto put = [&](int k, unsigned int e) { row0[k * 64] = k < cnt ? sb0 + e : dummy; };
    auto put8 = [&](int k, const uint4 q) {
      put(k + 0, q.x & 0xffffu); put(k + 1, q.x >> 16); put(k + 2, q.y & 0xffffu); put(k + 3, q.y >> 16);
      put(k + 4, q.z & 0xffffu); put(k + 5, q.z >> 16); put(k + 6, q.w & 0xffffu); put(k + 7, q.w >> 16);
    };
    if (chunks > 0) put8(0, f.n0);
    if (chunks > 2) put8(8, f.n1);
    const unsigned long long col = ok ? f.col : 0ull;
    rcol[slot][lane] = col;
    rid[slot][lane] = (unsigned long long)f.id;
    const unsigned int hascol = __ballot(col != 0ull) != 0ull ? 0x80u : 0u;
    COMPILER_FENCE();                            // the flag goes last
    if (lane == 63) lds_poke(&rflag[slot], ((unsigned int)((B >> 4) + 1) << 8) | hascol | (unsigned int)chunks);
  };

  // prologue: sixteen waves, sixteen blocks, ONE memory round trip — the failure word travels with the first blocks' fields
  // (checked before them it is a round trip of its own; measured: no difference in the kernel's time, kept for the shorter chain)
  const unsigned int fail = __hip_atomic_load(lfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  RingFields f0 = {};
  if (wave < cbp) f0 = load_ring(wave);
  lds_barrier();                                 // (the zero fill above, before anything else is written)
  if (fail != 0u) return false;                  // uniform over the workgroup
  for (int j = n + tid; j < cbp * 64; j += SCAN_T) stb[j] = 1;   // boxes past the end: suppressed from the start
  if (wave < cbp) store_ring(wave, f0);
  lds_barrier();                                 // the only barriers of this scan
  if (cb == 0) {
    if (tid == 0) num_keep[0] = 0;
    return true;
  }

  if (wave == 0) {
    // ---------------------------------------------------------------- resolver
    const unsigned int* const rl = &rent[0][0][lane];
    const unsigned long long* const rc = &rcol[0][lane];
    struct Near { unsigned int x, y, z, w; };
    // entries 4 chunk .. 4 chunk + 3 of the lane's near list in the slot at `r` (rows 256 bytes apart)
    auto ring4 = [&](const unsigned int* r, int chunk) -> Near { return Near{r[chunk * 256], r[chunk * 256 + 64], r[chunk * 256 + 128], r[chunk * 256 + 192]}; };
    auto mark4 = [&](const Near& e) { lds_mark_at(e.x); lds_mark_at(e.y); lds_mark_at(e.z); lds_mark_at(e.w); };
    constexpr int SLOT_DW = LIST_NEAR * 64;   // dwords per ring slot
    // two register sets, blocks of even / odd index: block c's fields are fetched while block c - 1 waits for its state bytes, so
    // that neither the flag nor the entries are waited for
    unsigned long long colA = rc[0], colB = 0ull;
    Near l0A = ring4(rl, 0), l1A = ring4(rl, 1), l0B = {}, l1B = {};
    unsigned int nflagA = rflag[0], nflagB = 0u;         // (block 0 is in the ring since the prologue; set B is fetched during block 0)
    unsigned int fdA = 1u, fdB = 1u;                     // (block 0 waits for nobody)
    for (int c0 = 0; c0 < cbp; c0 += 4) {
      unsigned char* const kw = stb + c0 * 64 + lane;
      const unsigned int* const fdp = fdone + c0;
      const int s0 = c0 & (LIST_RING - 1), s4 = (c0 + 4) & (LIST_RING - 1);   // slots of blocks c0 and c0 + 4
      // ring addresses of the group's own slots and of the next group's (blocks c0 + 2 .. c0 + 5 are fetched here): computed once
      // per group, so that every access of a block is base register + instruction offset
      const unsigned int* const rl0 = rl + s0 * SLOT_DW;
      const unsigned int* const rl4 = rl + s4 * SLOT_DW;
      const unsigned long long* const rc0 = rc + s0 * 64;
      const unsigned long long* const rc4 = rc + s4 * 64;
      const unsigned int* const rf0 = rflag + s0;
      const unsigned int* const rf4 = rflag + s4;
      const unsigned int gen1 = (unsigned int)(c0 >> 4) + 1u;   // what the flag of every block of this group carries
      auto block = [&](auto U) {
        constexpr int u = decltype(U)::value;
        const unsigned int* const crl = rl0 + u * SLOT_DW;          // this block's slot
        // the slot fetched in this block: block c + 1
        const unsigned int* const frl = u < 3 ? rl0 + (u + 1) * SLOT_DW : rl4;
        const unsigned long long* const frc = u < 3 ? rc0 + (u + 1) * 64 : rc4;
        const unsigned int* const frf = u < 3 ? rf0 + (u + 1) : rf4;
        Near& l0 = (u & 1) ? l0B : l0A;
        Near& l1 = (u & 1) ? l1B : l1A;
        unsigned long long& col = (u & 1) ? colB : colA;
        unsigned int& nflag = (u & 1) ? nflagB : nflagA;
        unsigned int& fd = (u & 1) ? fdB : fdA;
        // 1. nothing of block c may be read before the far victims of block c - LIST_K - 1 are marked (flag fetched a block ago)
        if (__builtin_expect(__builtin_amdgcn_readfirstlane((int)fd) == 0, 0)) {
          bool got = false;
          for (int spins = 0; spins < LIST_SPIN_MAX && lds_peek(&failed) == 0u; ++spins) {
            __builtin_amdgcn_s_sleep(1);
            if (__builtin_amdgcn_readfirstlane((int)lds_peek(&fdp[u])) != 0) {
              got = true;
              break;
            }
          }
          if (!got) lds_poke(&failed, 1u);
        }
        COMPILER_FENCE();
        // 2. the block's state bytes: THE round trip of the block.  Everything that does not depend on it is issued in its shadow:
        //    block c + 1's fields into the other register set (its last user, block c - 1, is done), this block's ring flag check
        const unsigned char state = kw[u * 64];
        COMPILER_FENCE();
        {
          Near& l0n = (u & 1) ? l0A : l0B;
          Near& l1n = (u & 1) ? l1A : l1B;
          unsigned long long& coln = (u & 1) ? colA : colB;
          unsigned int& nflagn = (u & 1) ? nflagA : nflagB;
          unsigned int& fdn = (u & 1) ? fdA : fdB;
          nflagn = lds_peek(frf);          // flag first, then the fields it vouches for
          COMPILER_FENCE();
          l0n = ring4(frl, 0);
          l1n = ring4(frl, 1);
          coln = frc[0];
          fdn = lds_peek(&fdp[u + 1]);
          COMPILER_FENCE();
        }
        unsigned int flag = (unsigned int)__builtin_amdgcn_readfirstlane((int)nflag);
        if (__builtin_expect((flag >> 8) != gen1, 0)) {
          // the block is not in the ring yet (never in steady state): re-read flag and fields.  Gives up after LIST_SPIN_MAX polls,
          // marks the scan failed and goes on with a harmless flag; once failed, no more waiting.
          flag = gen1 << 8;
          bool got = false;
          for (int spins = 0; spins < LIST_SPIN_MAX && lds_peek(&failed) == 0u; ++spins) {
            __builtin_amdgcn_s_sleep(1);
            COMPILER_FENCE();
            const unsigned int fl = (unsigned int)__builtin_amdgcn_readfirstlane((int)lds_peek(rf0 + u));
            COMPILER_FENCE();
            l0 = ring4(crl, 0);
            l1 = ring4(crl, 1);
            col = rc0[u * 64];
            if ((fl >> 8) == gen1) {
              flag = fl;
              got = true;
              break;
            }
          }
          if (!got) lds_poke(&failed, 1u);
        }
        unsigned long long kept = __ballot(state == 0);   // nobody kept so far suppresses the lane's box
        if (__builtin_expect((flag & 0x80u) != 0u, 0)) {   // some box of the block has an earlier box of the block on its column word
          const unsigned long long alive = kept;
          const unsigned int clo = (unsigned int)col, chi = (unsigned int)(col >> 32);
          if (__ballot(((clo & (unsigned int)alive) | (chi & (unsigned int)(alive >> 32))) != 0u) != 0ull) {
            for (;;) {  // <= 65 rounds; the fixed point is the greedy keep set of the block
              const bool sup = ((clo & (unsigned int)kept) | (chi & (unsigned int)(kept >> 32))) != 0u;
              const unsigned long long nk = alive & ~__ballot(sup);
              if (nk == kept) break;
              kept = nk;
            }
          }
        }
        const bool mine = __builtin_amdgcn_inverse_ballot_w64(kept);
        // near victims first (read back by THIS wave for later blocks — LDS runs a wave's accesses in order), the block's own state
        // bytes LAST: they are what the helper waves poll, and a helper that sees the block resolved will refill this block's ring
        // slot — from which entries 8..15 (rare) are still being read here
        if ((flag & 7u) != 0u && mine) {
          mark4(l0);
          if ((flag & 6u) != 0u) {         // more than one 4-entry chunk (the count is 0..4)
            mark4(l1);
            if ((flag & 7u) > 2u) {
              mark4(ring4(crl, 2));
              if ((flag & 7u) > 3u) mark4(ring4(crl, 3));
            }
          }
        }
        COMPILER_FENCE();
        kw[u * 64] = mine ? 0x80 : 0x02;
        COMPILER_FENCE();
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
      block(std::integral_constant<int, 2>{});
      block(std::integral_constant<int, 3>{});
    }
    if (lds_peek(&failed) != 0u && lane == 0) num_keep[0] = -1;
    return true;
  }
  // ------------------------------------------------------------------ helper waves: every wave that is not on the resolver's SIMD
  if ((wave & 3) == 0) return true;
  const int hw = wave - 1 - (wave >> 2);
  int base = 0;                                   // kept boxes before block t
  auto kept_word = [&](int blk) -> unsigned long long { return __ballot(stb[blk * 64 + lane] == 0x80); };
  unsigned int fcnt_next = hw < cb ? cnt2[min(hw * 64 + lane, n - 1)].y : 0u;   // far count of this wave's next block, one iteration ahead
  for (int t = hw; t < cb; t += LIST_HW) {
    const bool more = t + LIST_RING < cbp;
    // block t's far lists: as many uint4 as its longest one needs (the counts were loaded an iteration ago; lanes past the end have
    // a clamped index and are never kept)
    const int fcnt = (int)min(fcnt_next, (unsigned)LIST_FAR);
    const int nq = (wave_max_i32(fcnt) + 7) >> 3;
    uint4 q[LIST_FAR / 8];
    {
      const uint4* const l4 = reinterpret_cast<const uint4*>(flists + (size_t)min(t * 64 + lane, n - 1) * LIST_FAR);
#pragma unroll
      for (int k = 0; k < LIST_FAR / 8; ++k) q[k] = k < nq ? l4[k] : make_uint4(0u, 0u, 0u, 0u);
    }
    RingFields fr = {};                           // block t + 16's fields (ring), in flight while the resolver works up to t
    if (more) fr = load_ring(t + LIST_RING);
    if (t + LIST_HW < cb) fcnt_next = cnt2[min((t + LIST_HW) * 64 + lane, n - 1)].y;
    int spins = 0;
    while ((__builtin_amdgcn_readfirstlane((int)*(const volatile lds_u8*)(size_t)(sb0 + (unsigned int)t * 64u)) & 0x82) == 0) {
      if (++spins > LIST_SPIN_MAX) {   // a helper gives up: the scan is void — say so (nobody may be left to notice otherwise:
        lds_poke(&failed, 1u);         // the blocks after this one have no waiter) and report it in the count
        if (lane == 0) num_keep[0] = -1;
        return true;
      }
      __builtin_amdgcn_s_sleep(LIST_POLL_SLEEP);
    }
    COMPILER_FENCE();
    const unsigned long long kept = kept_word(t);
    const bool mine = (kept >> lane) & 1ull;
    {   // far victims of the kept boxes: due before the resolver reaches block t + LIST_K + 1.  ROLLED, the list rotating through
        // q[0] (register arrays cannot be indexed): code size matters here (see the header)
      if (mine) {
#pragma unroll 1
        for (int k = 0; k < nq; ++k) {
          const uint4 v = q[0];
          const int kb = k * 8;
          auto mark = [&](int i, unsigned int e) { stb[kb + i < fcnt ? e : mydummy] = 1; };
          mark(0, v.x & 0xffffu); mark(1, v.x >> 16); mark(2, v.y & 0xffffu); mark(3, v.y >> 16);
          mark(4, v.z & 0xffffu); mark(5, v.z >> 16); mark(6, v.w & 0xffffu); mark(7, v.w >> 16);
#pragma unroll
          for (int r = 0; r + 1 < LIST_FAR / 8; ++r) q[r] = q[r + 1];
        }
      }
      COMPILER_FENCE();
      if (lane == 0) lds_poke(&fdone[t + LIST_K + 1], 1u);
      COMPILER_FENCE();
    }
    // scribe step of block t; its global store goes last (loads and stores share one in-order counter)
    // the kept boxes of the blocks since this wave's last one (all resolved before t).  Straight-line — eleven reads in flight at once,
    // a clamped index and a masked count for the first iteration: as a loop it was eleven LDS round trips in a row (1400-1900 cycles,
    // the longest phase of a helper and most of the kernel's tail after the resolver's last block)
#pragma unroll
    for (int i = 1; i < LIST_HW; ++i) {
      const int cntb = __builtin_popcountll(kept_word(max(t - i, 0)));
      base += t - i >= 0 ? cntb : 0;
    }
    const long long id = (long long)rid[t & (LIST_RING - 1)][lane];
    if (more) {
      COMPILER_FENCE();                           // (the id above is read before the slot is overwritten)
      asm volatile("" : "+v"(fr.col), "+v"(fr.id));   // first use of the loaded fields pinned here
      store_ring(t + LIST_RING, fr);
      COMPILER_FENCE();
    }
    if (mine) keep[base + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = id;
    base += __builtin_popcountll(kept);
    if (t == cb - 1 && lane == 0 && lds_peek(&failed) == 0u) num_keep[0] = base;
  }
  return true;
}

// ONE launch for a call that may take the list scan: the failure word the clip kernel left decides (uniform) between the list scan
// (thirteen waves; the others leave after the prologue) and the classic single-level scan — beyond two chunks per row its <.., 2> form ORs the
// rest in synchronously: correct, slower than the two-level form, and only ever run as a fallback here.
template <int CH>
__global__ __launch_bounds__(SCAN_T) void nms_list_or_scan_kernel(const NmsArgs a, const unsigned long long* __restrict__ mask,
                                                                  const unsigned long long* __restrict__ colm,
                                                                  const unsigned short* __restrict__ lists,
                                                                  const unsigned* __restrict__ lcnt, unsigned lblock,
                                                                  long long* __restrict__ keep, long long* __restrict__ num_keep,
                                                                  const ScanWindow win) {
  if (!nms_list_body(a, colm, lists, lcnt, lblock, keep, num_keep)) nms_scan_body<SCAN_U, CH>(a, mask, colm, keep, num_keep, win);
}

// Second level of the two-level scan: after super-block [c_begin, c_end) has been resolved, every box it KEPT suppresses
// boxes further right; those mask rows are OR-ed into the global removed-set by the whole chip instead of by the one scan
// workgroup.  One wave per (64-box row block of the super-block, 64-word chunk right of it): lane = word, the wave walks
// the kept boxes of its block (independent 512-byte row loads), one atomicOr (integer: deterministic) per word.
__global__ __launch_bounds__(256) void nms_propagate_kernel(const NmsArgs a, const unsigned long long* __restrict__ mask_,
                                                            const ScanWindow win, int wchunks) {
  const int g = blockIdx.y;
  const int n = group_n(a, g);
  const int cb = (n + 63) >> 6;
  const int c_end = win.c_end;
  if (c_end >= cb) return;                                     // nothing right of the super-block in this group
  const size_t cbs = (size_t)a.cbs;
  const int rb = win.c_begin + (int)(blockIdx.x / wchunks), wc = (int)(blockIdx.x % wchunks);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = c_end + wc * 64 + lane;
  if (c_end + wc * 64 >= cb) return;                           // uniform
  const unsigned long long kept = win.gkept[(size_t)g * cbs + rb];   // uniform
  // the four waves of the workgroup share the block's kept rows round-robin (k-th kept row -> wave k % 4)
  unsigned long long mine = 0ull;
  int k = 0;
  for (unsigned long long t = kept; t != 0ull; t &= t - 1ull, ++k)
    if ((k & 3) == wave) mine |= t & (~t + 1ull);
  if (mine == 0ull) return;
  const unsigned long long* rows = mask_ + ((size_t)g * a.cap + (size_t)rb * 64) * cbs;
  const unsigned int wcl = (unsigned int)min(w, cb - 1);
  unsigned long long acc = 0ull;
  while (mine != 0ull) {   // four independent 512-byte row loads per round trip (a duplicate row is harmless: OR)
    int idx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      idx[u] = mine != 0ull ? __builtin_ctzll(mine) : idx[u > 0 ? u - 1 : 0];
      mine &= mine - (mine != 0ull ? 1ull : 0ull);
    }
    const unsigned long long v0 = rows[(size_t)idx[0] * cbs + wcl], v1 = rows[(size_t)idx[1] * cbs + wcl];
    const unsigned long long v2 = rows[(size_t)idx[2] * cbs + wcl], v3 = rows[(size_t)idx[3] * cbs + wcl];
    acc |= (v0 | v1) | (v2 | v3);
  }
  if (w < cb && acc != 0ull) atomicOr(&win.gremv[(size_t)g * cbs + w], acc);
}
}  // namespace rbox
