// gd3d_loss.hip — fused forward+gradient kernel of the Gaussian-distance losses for gfx950, its second-stage kernels
// and their C-ABI entry points (include/gd3d.h).  The head-level kernels are in gd3d_anchor_head.hip and
// gd3d_center_head.hip; gd3d_loss_common.h holds what the three share.
//
// Data layout in HBM: pred / target / grad_* are (N,7) fp32 row-major (28-byte rows, exactly what
// the reference's bbox coders hand to GDLoss.forward, gaussian_distance_loss.py:280-310);
// loss / row_weight are (N,) fp32.
//
// Kernel shape (HBM-bound: 88 algorithmic bytes per pair, ~300 VALU ops per pair):
//   * one workgroup = 256 threads = one tile of 256 pairs = 7168 contiguous bytes per tensor
//     = exactly 7 wave-wide 1-KiB LDS-DMA pieces (global_load_lds_dwordx4): 14 pieces bring the
//     pred and target tiles into LDS with no VGPR round trip and fully coalesced 16-B lanes;
//   * thread i then reads row i (7 dwords at stride 7: coprime with the 32 banks, conflict-free),
//     does all the 2x2 algebra in registers, and writes its 7 gradient dwords back into ITS OWN
//     LDS row (no barrier needed for that hand-back);
//   * after one barrier the tile leaves as 448 coalesced 16-B stores; the per-pair loss as one
//     coalesced dword store; the tile's loss sum goes wave-shuffle -> LDS -> one fp32 partial per
//     block, and a second tiny kernel adds the partials in a fixed order in fp64 (deterministic,
//     no float atomics).  Finishing the sum INSIDE this kernel (sc1-stored partial, drained, agent-scope arrival
//     ticket per 64-tile group, last arriver adds) was built and measured in round 2: 516 us per 3-loss step against
//     421 us with the separate launch (profiles/r02_ticket_ab.txt) — the drain + ticket round trip keeps one wave of
//     every workgroup resident ~30 % longer; removed.
//   * tiles that are partial (the last one) or whose base pointers are not 16-B aligned take a
//     guarded scalar load/store path around the same compute code.
#include <hip/hip_ext.h>

#include <mutex>
#include <unordered_map>

#include "gd3d_loss_common.h"

namespace gd3d {

constexpr int TILE = 256;            // pairs (= threads) per workgroup; multiples of 256 give whole 1-KiB DMA pieces.
                                     // r01 A/B inside bench.py under rocprofv3: 512 halves the partials (reduce stage
                                     // 6.9 -> 4.9 us) and is neutral for the fused kernel once it is below ~300 VALU/pair,
                                     // but gave only +0.5 % step throughput with ~1 us longer event-bracketed kernels
                                     // (noise level); 1024 is 4 % slower.  256 ships.
constexpr int TILE_F = TILE * 7;     // floats per tensor tile (1792)
constexpr int TILE_V4 = TILE_F / 4;  // 16-byte vectors per tensor tile (448)
constexpr int NPIECE = TILE_F / 256; // 1-KiB LDS-DMA pieces per tensor tile (7)
constexpr int NWAVE = TILE / 64;     // waves per workgroup (4)

typedef __attribute__((address_space(3))) void lds_ptr_t;
typedef const __attribute__((address_space(1))) void gbl_cptr_t;

// LDS-DMA loads of pred (and of the optional (N,7) weights) with the nt cache policy: those bytes are read exactly once
// (measured r01, 10 M pairs: nt loads + nt stores 129 us vs 151 us plain; a persistent double-buffered grid-stride variant
// was 143-160 us and was dropped)
constexpr int DMA_AUX = 2;
// The TARGET is read with the default policy instead: a training step evaluates several losses against the same target
// back to back (GDLoss.forward(pred_k, target)), and default-policy lines stay in the 256 MiB Infinity Cache for the next
// launch while nt lines do not.  The launcher walks every launch on the same target opposite to the one before, so the rows
// read last are read again first (loss_launch).  tools/target_reuse_probe.hip, profiles/r07_target_reuse_probe.txt: three
// 2-read-1-write passes over a shared 280 MB buffer, us per pass after the first: nt 131, default 99-102 in alternating
// order (116 ascending); the first pass from clean caches 137 vs 134 with nt.  sc0 / sc1 behave as the default policy,
// sc0 nt / sc1 nt as nt.
constexpr int DMA_AUX_TARGET = 0;
// Occupancy cap.  The fused launch requests AT LEAST this much dynamic LDS, i.e. floor(160 KiB / bytes) workgroups per CU
// instead of the 8 that its own 14.4 KiB would admit: fewer tiles in flight per CU stream better (the kernel's data path
// without its math: 8 WG/CU 131.0 us, 6: 130.2, 5: 126.7, 4: 126.8, 3: 162; flat copy 127.5), but fewer waves hide less
// VALU latency, so the best cap depends on the loss.  Measured per loss at FIXED buffer placement
// (profiles/r02_lds_fixed_placement.txt; 10 M pairs, us per launch, good / bad placement):
//   WG/CU   gwd3d (217 VALU/pair)   kld3d (270)      bd3d (296)
//     8     134.1 / 137.6           134.2 / 139.5    134.5 / 139.1
//     7     133.1 / 137.1           131.2 / 138.8    133.0 / 138.3
//     6     131.7 / 136.4           129.6 / 138.0    130.1 / 137.6
//     5     131.4 / 134.7           135.8 / 137.6    140.0 / 140.9
//     4     132.2 / 134.6           136.0 / 136.8    139.9 / 140.3
// A launch that re-reads the target the previous launch read (loss_launch: Geometry::reuse) is NOT capped: with part of
// its bytes served by the Infinity Cache the math is what is left to hide, and 8 workgroups per CU hide it best
// (profiles/r07_target_reuse_ab.txt, bench step, us per fused launch: capped as below 130.7-133.7, 7 per CU 115.6-116.9,
// 8 per CU 117.2-117.4; a launch on a target nobody read just before keeps the cap: uncapped it took 135.5 against 133.0).
constexpr int MIN_LDS = 27300;         // 6 workgroups per CU
constexpr int MIN_LDS_GWD = 32768;     // 5
constexpr int MIN_LDS_W7 = 32768;      // 5, launches with (N,7) weights (any loss)
constexpr int MIN_LDS_KLD = MIN_LDS;
constexpr int MIN_LDS_BD = MIN_LDS;

typedef float v4f __attribute__((ext_vector_type(4)));

GD_DEV void store_v4(float* dst, const float* src_lds, int idx) {
  const v4f v = reinterpret_cast<const v4f*>(src_lds)[idx];
  __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(dst) + idx);   // written once, never re-read by this kernel
}

// 14 LDS-DMA pieces of 1 KiB bring one 256-pair tile of pred and target into LDS; wave w issues pieces w, w+4, w+8, w+12.
// The two tiles are adjacent in LDS (st = sp + TILE_F = sp + 7 pieces), so piece j of the 14 lands at sp + j * 256 and only
// its SOURCE and its cache policy depend on which tensor it belongs to.  Rounds 0 and 2-3 are pred-only / target-only at
// compile time; round 1 (pieces 4-7) is the only one that mixes them and takes one wave-uniform branch.  (Written as a loop
// over both tensors with per-piece if / else-if, the compiler built a tree of ~60 scalar compares and branches in front of
// the first load: issue slots on every workgroup's critical path, profiles/r02_pmc_issue_mix_by_cap.txt.)
// (an optional third tile, the (256,7) weights, sits behind the wave sums and keeps its own loop)
GD_DEV void issue_tile_dma(const float* gpred, const float* gtarget, float* sp, float* st, int wave, int lane,
                           const float* gw7, float* sw7) {
  static_assert(TILE_F == NPIECE * 256, "pred and target tiles must be whole pieces for the adjacent-piece addressing");
  (void)st;
  const float* const t_shifted = gtarget - NPIECE * 256;   // so that piece j >= NPIECE reads target piece j - NPIECE
#pragma unroll
  for (int k = 0; k * NWAVE < 2 * NPIECE; ++k) {
    const int j = wave + k * NWAVE;  // wave-uniform
    const float* const p_src = gpred + j * 256 + lane * 4;
    const float* const t_src = t_shifted + j * 256 + lane * 4;
    lds_ptr_t* const dst = (lds_ptr_t*)(sp + j * 256);
    if ((k + 1) * NWAVE <= NPIECE) {                // whole round in pred
      __builtin_amdgcn_global_load_lds((gbl_cptr_t*)p_src, dst, 16, 0, DMA_AUX);
    } else if (k * NWAVE >= NPIECE) {               // whole round in target; only the last round needs the runtime test
      if ((k + 1) * NWAVE <= 2 * NPIECE || j < 2 * NPIECE)
        __builtin_amdgcn_global_load_lds((gbl_cptr_t*)t_src, dst, 16, 0, DMA_AUX_TARGET);
    } else if (j < NPIECE) {                        // the mixed round: a wave-uniform branch
      __builtin_amdgcn_global_load_lds((gbl_cptr_t*)p_src, dst, 16, 0, DMA_AUX);
    } else {
      __builtin_amdgcn_global_load_lds((gbl_cptr_t*)t_src, dst, 16, 0, DMA_AUX_TARGET);
    }
  }
  if (gw7 != nullptr) {
#pragma unroll
    for (int k = 0; k * NWAVE < NPIECE; ++k) {
      const int j = wave + k * NWAVE;
      if ((k + 1) * NWAVE <= NPIECE || j < NPIECE)
        __builtin_amdgcn_global_load_lds((gbl_cptr_t*)(gw7 + j * 256 + lane * 4), (lds_ptr_t*)(sw7 + j * 256), 16, 0, DMA_AUX);
    }
  }
}

struct LossArgs {
  const float* pred;
  const float* target;
  const float* w;    // nullable: (N,) row weights
  const float* w7;   // nullable: (N,7) weights, row mean taken in the kernel (GDLoss.forward :295-296)
  float* loss;       // nullable
  float* gp;         // nullable
  float* gt;         // nullable (only read when the kernel is instantiated with GT)
  float* partials;   // nullable
  // GDLoss.forward's early-out when no weight entry is > 0 (gaussian_distance_loss.py:290-292), resolved on the device:
  // with wsel the block also leaves sum(pred * weight7) in partials[nbp + b] and "any weight > 0" in partials[2 nbp + b]
  int wsel;
  long long nbp;     // partial-array stride (number of tiles rounded up to 4)
  // single-launch form for small problems (<= FIN_MAX_TILES tiles): the workgroup whose arrival ticket comes last adds
  // the partials itself (fixed order, fp64) and writes the result — no reduce launch.  fin: device int32, 0 at launch,
  // left 0; fin_out: the loss sum; fin_any: the any-positive flag of a selecting call (nullable).
  int* fin;
  float* fin_out;
  int* fin_any;
  long long n;
  float scale, alpha, ia2, tau;
  float c0, c1, c2;
  int vec_ok;        // all (N,7) pointers 16-byte aligned
  int rev;           // tile order: workgroup b takes tile nb - 1 - b (chosen by loss_launch; results do not depend on it)
  // bbox-coder decode fused into the prologue (include/gd3d.h gd3d_prologue)
  int pro;
  int norm_bbox;
  const float* aux;
  float osf, vs0, vs1, pc0, pc1;
};

GD_DEV void decode_center(const float (&enc)[7], float loc0, float loc1, const LossArgs& a, float (&dec)[7],
                          DecodeJac& J) {
  dec[0] = (enc[0] + loc0) * a.osf * a.vs0 + a.pc0;
  dec[1] = (enc[1] + loc1) * a.osf * a.vs1 + a.pc1;
  dec[2] = enc[2];
#pragma unroll
  for (int k = 3; k < 6; ++k) {
    dec[k] = a.norm_bbox ? expf(enc[k]) : enc[k];
    J.j[k] = a.norm_bbox ? dec[k] : 1.0f;
  }
  dec[6] = enc[6];
  J.j[0] = a.osf * a.vs0; J.j[1] = a.osf * a.vs1; J.j[2] = 1.0f; J.j[6] = 1.0f;
}

// PLAIN: the launcher has checked that none of the options is in use (no weights, no selection, no prologue, no per-pair
// loss output, no single-launch finish); folding them to constants here removes their uniform tests and the kernarg loads
// behind them from every wave's issue stream (profiles/r02_pmc_issue_mix_by_cap.txt: issue slots are what the streaming
// launch has too many of).  Same code otherwise.
template <int LOSS, int FUN, bool FLAG, bool GT, bool PLAIN = false>
__global__ __launch_bounds__(TILE) void fused_kernel(const LossArgs a_in) {
  LossArgs a = a_in;
  if (PLAIN) {
    a.w = nullptr;
    a.w7 = nullptr;
    a.wsel = 0;
    a.pro = GD3D_PRO_NONE;
    a.aux = nullptr;
    a.loss = nullptr;
    a.fin = nullptr;
    a.fin_out = nullptr;
    a.fin_any = nullptr;
  }
  // dynamic LDS (16-byte aligned base, every carve offset a multiple of 16): two tiles + 32 floats of per-wave sums
  // (loss | pred*weight | any weight > 0), plus a third tile only when (N,7) weights are given, so that the common
  // launch keeps 8 workgroups per CU
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const sp = smem;
  float* const st = smem + TILE_F;
  float* const swave = smem + 2 * TILE_F;
  float* const sw7 = smem + 2 * TILE_F + 32;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: scalar branches below
  // every per-tile index (rows, partial sums) follows the tile, not the workgroup: the order changes no result
  const unsigned tile = a.rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const long long base = (long long)tile * TILE;
  const long long rows_left = a.n - base;
  const bool full = rows_left >= TILE;
  const bool fast = full && a.vec_ok;  // workgroup-uniform
  const bool valid = tid < rows_left;
  const float* gpred = a.pred + base * 7;
  const float* gtarget = a.target + base * 7;

  float wi = 1.0f;
  if (a.w != nullptr && valid) wi = a.w[base + tid];

  const float* gw7 = a.w7 != nullptr ? a.w7 + base * 7 : nullptr;
  if (fast) {
    issue_tile_dma(gpred, gtarget, sp, st, wave, lane, gw7, sw7);
  } else {
    const long long fl = (rows_left < TILE ? rows_left : TILE) * 7;
    for (int i = tid; i < TILE_F; i += TILE) {
      sp[i] = i < fl ? gpred[i] : 1.0f;
      st[i] = i < fl ? gtarget[i] : 1.0f;
      if (gw7 != nullptr) sw7[i] = i < fl ? gw7[i] : 0.0f;
    }
  }
  __syncthreads();  // s_waitcnt vmcnt(0) + barrier: every wave's pieces have landed

  if (a.w7 != nullptr) {  // weight.mean(dim=-1): sum of the 7 entries in index order, then / 7
    float sum = sw7[tid * 7];
#pragma unroll
    for (int k = 1; k < 7; ++k) sum += sw7[tid * 7 + k];
    wi = sum / 7.0f;
  }

  float pv[7], tv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    pv[k] = sp[tid * 7 + k];
    tv[k] = st[tid * 7 + k];
  }
  const float c[3] = {a.c0, a.c1, a.c2};
  const float f = a.scale * wi;
  float g1[7], g2[7];
  DecodeJac Jp, Jt;
  if (a.pro != GD3D_PRO_NONE) {  // workgroup-uniform; head-level calls are small (P <~ 1e4), aux is read directly
    if (a.pro == GD3D_PRO_ANCHOR_DELTA) {
      float an[7], dp[7], dt[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) an[k] = valid ? a.aux[(base + tid) * 7 + k] : 1.0f;
      decode_anchor(pv, an, dp, Jp);
      decode_anchor(tv, an, dt, Jt);
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        pv[k] = dp[k];
        tv[k] = dt[k];
      }
    } else {
      float dp[7];
      const float l0 = valid ? a.aux[(base + tid) * 2] : 0.0f, l1 = valid ? a.aux[(base + tid) * 2 + 1] : 0.0f;
      decode_center(pv, l0, l1, a, dp, Jp);
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        pv[k] = dp[k];
        Jt.j[k] = 1.0f;
      }
    }
  }
  float alt = 0.0f;      // wsel: this row's share of (pred * weight).sum() (ref :292; pred = the DECODED row)
  bool anyp = false;     //       and of torch.any(weight > 0) (ref :290; a NaN weight is not > 0)
  if (a.wsel && valid) { // uniform && per-thread
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float wk = sw7[tid * 7 + k];
      anyp |= wk > 0.0f;
      alt = fmaf(pv[k], wk, alt);
    }
  }
  const float L = pair_loss<LOSS, FUN, FLAG, GT>(pv, tv, c, a.alpha, a.ia2, a.tau, f, g1, g2);
  const float fl = valid ? f * L : 0.0f;
  if (a.pro != GD3D_PRO_NONE) {
    encode_grad(g1, Jp, a.pro == GD3D_PRO_ANCHOR_DELTA);
    if (GT) encode_grad(g2, Jt, a.pro == GD3D_PRO_ANCHOR_DELTA);
  }

  if (a.loss != nullptr && valid) a.loss[base + tid] = fl;

  if (a.gp != nullptr) {
#pragma unroll
    for (int k = 0; k < 7; ++k) sp[tid * 7 + k] = g1[k];  // own row: no hazard with other threads
  }
  if (GT) {
#pragma unroll
    for (int k = 0; k < 7; ++k) st[tid * 7 + k] = g2[k];
  }

  float bsum = 0.0f;
  if (a.partials != nullptr) {
    const float ws = wave_sum(fl);  // uniform (readlane 63)
    if (lane == 0) swave[wave] = ws;
    if (a.wsel) {                   // uniform
      const float wa = wave_sum(alt);
      const bool any_w = __builtin_amdgcn_ballot_w64(anyp) != 0ull;
      if (lane == 0) {
        swave[NWAVE + wave] = wa;
        swave[2 * NWAVE + wave] = any_w ? 1.0f : 0.0f;
      }
    }
  }
  __syncthreads();
  if (a.partials != nullptr && tid == 0) {
#pragma unroll
    for (int w4 = 0; w4 < NWAVE; w4 += 4) bsum += (swave[w4] + swave[w4 + 1]) + (swave[w4 + 2] + swave[w4 + 3]);
    float asum = 0.0f, fany = 0.0f;
    if (a.wsel) {
#pragma unroll
      for (int w4 = 0; w4 < NWAVE; ++w4) {
        asum += swave[NWAVE + w4];
        fany += swave[2 * NWAVE + w4];
      }
    }
    if (a.fin == nullptr) {
      a.partials[tile] = bsum;
      if (a.wsel) {
        a.partials[a.nbp + tile] = asum;
        a.partials[2 * a.nbp + tile] = fany;   // > 0: some weight of this tile is > 0
      }
    } else {   // handed to the last workgroup: write-through (sc1) stores, see the finish below
      __hip_atomic_store(a.partials + tile, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.wsel) {
        __hip_atomic_store(a.partials + a.nbp + tile, asum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.partials + 2 * a.nbp + tile, fany, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  if (fast) {
    if (a.gp != nullptr) {
      store_v4(a.gp + base * 7, sp, tid);
      if (tid < TILE_V4 - TILE) store_v4(a.gp + base * 7, sp, tid + TILE);  // 7/4 vectors per thread
    }
    if (GT) {
      store_v4(a.gt + base * 7, st, tid);
      if (tid < TILE_V4 - TILE) store_v4(a.gt + base * 7, st, tid + TILE);
    }
  } else {
    const long long fl7 = (rows_left < TILE ? rows_left : TILE) * 7;
    if (a.gp != nullptr)
      for (int i = tid; i < fl7; i += TILE) a.gp[base * 7 + i] = sp[i];
    if (GT)
      for (int i = tid; i < fl7; i += TILE) a.gt[base * 7 + i] = st[i];
  }

  // Single-launch finish (small grids only; the same hand-off cost 20 % in the streaming regime and is not used there,
  // profiles/r02_ticket_ab.txt).  Form: MI355X_MICROARCH.md, valid forms, row 1 — every handed-off word was stored sc1 by
  // lane 0 of its workgroup; that wave drains vmcnt, then takes an agent-scope ticket; the wave whose add returned last
  // loads the words with sc1 loads, one per lane, and adds them in lane order in fp64.  The ticket returns to 0.
  if (a.fin != nullptr && wave == 0) {   // uniform
    const int nb = (int)gridDim.x;       // <= 64: one partial per lane
    int t = 0;
    if (lane == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      t = __hip_atomic_fetch_add(a.fin, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    t = __builtin_amdgcn_readfirstlane(t);
    if (t == nb - 1) {
      double v[3] = {0.0, 0.0, 0.0};
      const int terms = a.wsel ? 3 : 1;
      for (int k = 0; k < terms; ++k) {
        if (lane < nb)
          v[k] = (double)__hip_atomic_load(a.partials + (long long)k * a.nbp + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
      }
      if (lane == 0) {
        const bool any = !a.wsel || v[2] > 0.0;
        *a.fin_out = (float)(any ? v[0] : v[1]);
        if (a.fin_any != nullptr) *a.fin_any = any ? 1 : 0;
        __hip_atomic_store(a.fin, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// ---- several losses on one target in one launch (gd3d_loss_fused_multi) -----------------------------------------------------
// A training step evaluates K losses against ONE target.  K single launches read that target K times (from HBM, or at
// about a third of that cost from the Infinity Cache when the launches follow each other: DMA_AUX_TARGET above); this kernel
// brings each target tile into LDS once, next to K prediction tiles, and evaluates the K losses on it: (1 + 2 K) x 28 bytes per
// row instead of 3 K x 28.  Unweighted, prologue-free, no target gradient; per loss the SAME pair_loss instance on the same
// operands in the same order as fused_kernel, the same per-wave and per-tile sums: bit-identical losses and gradients.
struct MultiArgs {
  const float* target;
  const float* pred[MULTI_MAX];
  float* gp[MULTI_MAX];         // nullable
  float* partials[MULTI_MAX];   // one partial array per loss (workspace rows of ws_nbp(n) floats)
  long long n;
  float scale[MULTI_MAX], alpha[MULTI_MAX], ia2[MULTI_MAX], tau[MULTI_MAX];
  float c[MULTI_MAX][3];
  int vec_ok;                   // target and every pred / gp pointer 16-byte aligned
};

// (K + 1) x NPIECE pieces of 1 KiB: the K pred tiles, then the target tile, adjacent in LDS (piece j lands at smem + j * 256).
// Wave w issues pieces w, w + 4, ...; a round of four pieces lies in one tensor or straddles ONE tensor boundary (4 < NPIECE),
// which is known at compile time: one wave-uniform branch in a straddling round, none otherwise (see issue_tile_dma).
template <int K>
GD_DEV void issue_multi_dma(const MultiArgs& a, long long off, float* smem, int wave, int lane) {
  constexpr int NP = (K + 1) * NPIECE;
#pragma unroll
  for (int k = 0; k * NWAVE < NP; ++k) {
    const int j = wave + k * NWAVE;   // wave-uniform
    const int t_lo = (k * NWAVE) / NPIECE;                                            // compile time after unrolling
    const int t_hi = (k * NWAVE + NWAVE - 1) / NPIECE < K ? (k * NWAVE + NWAVE - 1) / NPIECE : K;
    lds_ptr_t* const dst = (lds_ptr_t*)(smem + j * 256);
    // source of piece j when it belongs to tensor t: base_t + (j - t * NPIECE) * 256 floats
    const float* const lo_src = (t_lo < K ? a.pred[t_lo < K ? t_lo : 0] : a.target) + off + (j - t_lo * NPIECE) * 256 + lane * 4;
    const float* const hi_src = (t_hi < K ? a.pred[t_hi < K ? t_hi : 0] : a.target) + off + (j - t_hi * NPIECE) * 256 + lane * 4;
    const bool last_round = (k + 1) * NWAVE > NP;
    if (last_round && j >= NP) continue;   // uniform; only the last round can run past the last piece
    if (t_lo == t_hi || j < t_hi * NPIECE) {
      if (t_lo < K) __builtin_amdgcn_global_load_lds((gbl_cptr_t*)lo_src, dst, 16, 0, DMA_AUX);
      else __builtin_amdgcn_global_load_lds((gbl_cptr_t*)lo_src, dst, 16, 0, DMA_AUX_TARGET);
    } else {
      if (t_hi < K) __builtin_amdgcn_global_load_lds((gbl_cptr_t*)hi_src, dst, 16, 0, DMA_AUX);
      else __builtin_amdgcn_global_load_lds((gbl_cptr_t*)hi_src, dst, 16, 0, DMA_AUX_TARGET);
    }
  }
}

// loss k of the tuple on this thread's row: gradient into the row's own place in pred k's LDS tile, wave sum into swave
template <int LOSS, int KI>
GD_DEV void multi_eval(const MultiArgs& a, float* sp, const float (&tv_in)[7], float* swave, int tid, int lane, int wave,
                       bool valid) {
  float pv[7], tv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    pv[k] = sp[tid * 7 + k];
    tv[k] = tv_in[k];
    // each loss sees the target row as values of its own: nothing of one loss's arithmetic is shared with another's, so every
    // loss is contracted and rounded exactly as in its single-loss kernel
    asm volatile("" : "+v"(tv[k]));
  }
  const float c[3] = {a.c[KI][0], a.c[KI][1], a.c[KI][2]};
  const float f = a.scale[KI];
  float g1[7], g2[7];
  const float L = pair_loss<LOSS, MULTI_FUN, MULTI_FLAG, false>(pv, tv, c, a.alpha[KI], a.ia2[KI], a.tau[KI], f, g1, g2);
  const float fl = valid ? f * L : 0.0f;
#pragma unroll
  for (int k = 0; k < 7; ++k) sp[tid * 7 + k] = g1[k];   // own row: no hazard with other threads
  const float ws = wave_sum(fl);   // uniform (readlane 63)
  if (lane == 0) swave[KI * NWAVE + wave] = ws;
}

template <int L0, int L1, int L2>
__global__ __launch_bounds__(TILE) void fused_multi_kernel(const MultiArgs a) {
  constexpr int K = L2 < 0 ? 2 : 3;
  // dynamic LDS: K pred tiles | target tile | 32 floats of per-wave sums (K x NWAVE used)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const st = smem + K * TILE_F;
  float* const swave = smem + (K + 1) * TILE_F;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned tile = blockIdx.x;
  const long long base = (long long)tile * TILE;
  const long long rows_left = a.n - base;
  const bool fast = rows_left >= TILE && a.vec_ok;   // workgroup-uniform
  const bool valid = tid < rows_left;
  const long long fl7 = (rows_left < TILE ? rows_left : TILE) * 7;

  if (fast) {
    issue_multi_dma<K>(a, base * 7, smem, wave, lane);
  } else {
    for (int i = tid; i < TILE_F; i += TILE) {
#pragma unroll
      for (int k = 0; k < K; ++k) smem[k * TILE_F + i] = i < fl7 ? a.pred[k][base * 7 + i] : 1.0f;
      st[i] = i < fl7 ? a.target[base * 7 + i] : 1.0f;
    }
  }
  __syncthreads();  // s_waitcnt vmcnt(0) + barrier: every wave's pieces have landed

  float tv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) tv[k] = st[tid * 7 + k];
  multi_eval<L0, 0>(a, smem, tv, swave, tid, lane, wave, valid);
  multi_eval<L1, 1>(a, smem + TILE_F, tv, swave, tid, lane, wave, valid);
  if constexpr (K == 3) multi_eval<L2, 2>(a, smem + 2 * TILE_F, tv, swave, tid, lane, wave, valid);
  __syncthreads();

  static_assert(NWAVE == 4, "the tile sum below adds four wave sums");
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (tid == k) {   // thread k finishes loss k's tile sum, in fused_kernel's order
      float bsum = 0.0f;
      const float* const s4 = swave + k * NWAVE;
      bsum += (s4[0] + s4[1]) + (s4[2] + s4[3]);
      a.partials[k][tile] = bsum;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float* const gp = a.gp[k];
    if (gp == nullptr) continue;   // uniform
    const float* const sp = smem + k * TILE_F;
    if (fast) {
      store_v4(gp + base * 7, sp, tid);
      if (tid < TILE_V4 - TILE) store_v4(gp + base * 7, sp, tid + TILE);  // 7/4 vectors per thread
    } else {
      for (int i = tid; i < fl7; i += TILE) gp[base * 7 + i] = sp[i];
    }
  }
}

// Dynamic-LDS request of the multi-loss launch = its occupancy: floor(160 KiB / bytes) workgroups per CU.  Its own need is
// (K + 1) tiles + 128 bytes: 28 800 bytes at K = 3 (5 per CU at most), 21 632 at K = 2 (7 per CU).  Swept at K = 3 on
// gwd3d + kld3d + bd3d, 10 M rows, us per launch pair (fused + second stage) in back-to-back loops, three single launches with
// their second stages beside it in the same process (profiles/r20_multi_loss_probe.txt):
//   5 per CU 312.2-316.7 (singles 368.5-369.7)   4 per CU 321.2-324.2 (370.8-371.9)   3 per CU 368.2-369.5 (371.6-372.1)
// and at K = 2 on gwd3d + kld3d / kld3d + bd3d (two single launches with their second stages: 243.8-245.5 on every line):
//   7 per CU 209.6-211.8 / 206.5-209.9   6 per CU 211.5-213.8 / 214.1-216.2   5 per CU 222.1-223.1 / 234.2-236.8
//   4 per CU 221.0-221.7 / 236.7-237.2
// So neither launch is capped: the request is what the tiles need, and the single launches' caps (MIN_LDS) are not inherited.
constexpr int MULTI_LDS_K3 = 28800;   // 5 workgroups per CU
constexpr int MULTI_LDS_K2 = 21632;   // 7

// Clears (or fills) small or large device buffers from a KERNEL.  Not hipMemsetAsync: inside a captured hipGraph a memset node was
// found not to be reliably ordered against the kernels around it on this ROCm (profiles/r04_nms_queue_ab.txt) —
// rule of this library: no memset nodes in paths a caller may capture.
__global__ __launch_bounds__(256) void fill_words_kernel(unsigned* __restrict__ p, long long nwords, unsigned value) {
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if ((((uintptr_t)p) & 15) == 0) {
    uint4* p4 = reinterpret_cast<uint4*>(p);
    const long long nv = nwords >> 2;
    const uint4 v4 = make_uint4(value, value, value, value);
    for (long long k = i; k < nv; k += stride) p4[k] = v4;
    for (long long k = (nv << 2) + i; k < nwords; k += stride) p[k] = value;
    return;
  }
  for (; i < nwords; i += stride) p[i] = value;
}
int fill_words(void* p, size_t bytes, unsigned value, hipStream_t s) {   // bytes: a multiple of 4
  const long long nwords = (long long)(bytes / 4);
  if (nwords == 0) return 0;
  long long blocks = (nwords / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (unsigned*)p, nwords, value);
  return (int)hipGetLastError();
}

// second stage: fixed-order fp64 sum of the per-block partials -> one fp32.  One workgroup; the kernel is pure latency
// (39 K floats at 10 M pairs): every thread issues ALL its 16-byte loads of a 48 K-partial round before the first add
// (one memory round trip at 10 M pairs), then one barrier: thread t of wave 0 adds 16 consecutive per-thread sums from
// LDS and the wave finishes with 6 shuffle steps.  Deterministic (fixed order), independent of the launch geometry.
GD_DEV void reduce_partials_body(const float* __restrict__ partials, long long nb, float* __restrict__ out, double* sd) {
  constexpr int RU = 12;
  const int tid = threadIdx.x;
  const long long nv = nb >> 2;  // whole float4s (the workspace is 16-byte aligned)
  const float4* p4 = reinterpret_cast<const float4*>(partials);
  double acc = 0.0;
  for (long long i0 = 0; i0 < nv; i0 += 1024 * RU) {
    float4 v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const long long i = i0 + (long long)u * 1024 + tid;
      v[u] = i < nv ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) acc += ((double)v[u].x + (double)v[u].y) + ((double)v[u].z + (double)v[u].w);
  }
  const long long tail = (nv << 2) + tid;
  if (tail < nb) acc += (double)partials[tail];
  sd[tid] = acc;
  __syncthreads();
  if (tid < 64) {
    double s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s2 += sd[tid * 16 + k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s2 += __shfl_down(s2, off, 64);
    if (tid == 0) *out = (float)s2;
  }
}
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float* __restrict__ partials, long long nb,
                                                               float* __restrict__ out) {
  __shared__ double sd[1024];
  reduce_partials_body(partials, nb, out, sd);
}
// the same sum for the K losses of gd3d_loss_fused_multi in ONE launch: workgroup k adds row k of the workspace
struct ReduceMultiArgs {
  float* out[MULTI_MAX];
};
__global__ __launch_bounds__(1024) void reduce_partials_multi_kernel(const float* __restrict__ partials, long long nb,
                                                                     long long nbp, const ReduceMultiArgs o) {
  __shared__ double sd[1024];
  float* out = o.out[0];
  if (blockIdx.x == 1) out = o.out[1];
  if (blockIdx.x == 2) out = o.out[2];
  reduce_partials_body(partials + (long long)blockIdx.x * nbp, nb, out, sd);
}
int reduce_partials(const float* partials, long long nb, float* out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(1024), 0, s, partials, nb, out);
  return (int)hipGetLastError();
}

// grad[i,:] *= g  (scalar g: the whole grid exits after one scalar load when g == 1)
__global__ __launch_bounds__(1024) void scale_rows_kernel(float* __restrict__ grad, const float* __restrict__ g,
                                                         int per_row, long long nflt) {
  float gs = 1.0f;
  if (!per_row) {
    gs = g[0];
    if (gs == 1.0f) return;  // uniform across the grid
  }
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (!per_row && (((uintptr_t)grad & 15) == 0)) {
    v4f* g4 = reinterpret_cast<v4f*>(grad);
    const long long nv = nflt >> 2;
    for (long long i = i0; i < nv; i += stride) g4[i] = g4[i] * gs;
    for (long long i = (nv << 2) + i0; i < nflt; i += stride) grad[i] *= gs;
    return;
  }
  for (long long i = i0; i < nflt; i += stride) grad[i] *= per_row ? g[i / 7] : gs;
}

// The same second stage for a weighted call that must honour GDLoss.forward's early-out (ref :290-292) without a host
// sync: besides the loss partials the fused kernel left sum(pred * weight) and "some weight > 0" per tile.  One launch
// adds all three in a fixed order and SELECTS on the device:
//   *out = any weight > 0 ? scale * sum_i w_i L_i : sum(pred * weight)          *any_pos = that predicate (for backward)
__global__ __launch_bounds__(1024) void reduce_select_kernel(const float* __restrict__ partials, long long nb, long long nbp,
                                                             float* __restrict__ out, int* __restrict__ any_pos) {
  __shared__ double sd[3][1024];
  const int tid = threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  for (long long i = tid; i < nb; i += 1024) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += (double)partials[k * nbp + i];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) sd[k][tid] = acc[k];
  __syncthreads();
  if (tid < 64) {
    double s3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double s2 = 0.0;
      for (int j = 0; j < 16; ++j) s2 += sd[k][tid * 16 + j];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s2 += __shfl_down(s2, off, 64);
      s3[k] = s2;
    }
    if (tid == 0) {
      const bool any = s3[2] > 0.0;
      *out = (float)(any ? s3[0] : s3[1]);
      if (any_pos != nullptr) *any_pos = any ? 1 : 0;
    }
  }
}

// Autograd backward of a reduced call (replaces scale_rows_kernel there):
//   any weight > 0 (or no selection):  grad *= g            (the whole grid leaves after two scalar loads when g == 1)
//   otherwise (ref :290-292 took `(pred * weight).sum()`):  grad_pred = g * d(sum(dec(pred) * weight7)) / d pred,
//                                                           grad_target = 0
// One thread per row on the rare path; it is not a bandwidth path.
struct FinishArgs {
  float* gp;             // (n,7) nullable
  float* gt;             // (n,7) nullable
  const float* g;        // device scalar: upstream gradient
  const int* any_pos;    // device flag written by reduce_select_kernel; nullptr = no selection
  const float* w7;       // (n,7) weights      (selection only)
  const float* pred;     // (n,7) encoded rows (selection with a prologue only)
  const float* aux;
  long long n;
  int pro, norm_bbox;
  float osf, vs0, vs1;
};

constexpr int FINISH_T = 256;   // one wave per SIMD and CU on a 256-workgroup grid: the common case is the g == 1 early exit, whose cost
constexpr int FINISH_U = 8;     // is the dispatch of the grid's waves (4096 waves: 4.4 us, 1024 waves: see profiles/r03); a real
                                // scaling pass keeps FINISH_U 16-byte loads in flight per lane instead (32 KiB per CU)
__global__ __launch_bounds__(FINISH_T) void grad_finish_kernel(const FinishArgs a) {
  const float gs = a.g[0];
  const bool normal = a.any_pos == nullptr || a.any_pos[0] != 0;
  if (normal && gs == 1.0f) return;  // uniform across the grid
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nflt = a.n * 7;
  if (normal) {
    for (int which = 0; which < 2; ++which) {
      float* grad = which == 0 ? a.gp : a.gt;
      if (grad == nullptr) continue;
      if (((uintptr_t)grad & 15) == 0) {
        v4f* g4 = reinterpret_cast<v4f*>(grad);
        const long long nv = nflt >> 2;
        for (long long i = i0; i < nv; i += FINISH_U * stride) {
          v4f v[FINISH_U];
#pragma unroll
          for (int u = 0; u < FINISH_U; ++u)
            if (i + u * stride < nv) v[u] = g4[i + u * stride];
#pragma unroll
          for (int u = 0; u < FINISH_U; ++u)
            if (i + u * stride < nv) g4[i + u * stride] = v[u] * gs;
        }
        for (long long i = (nv << 2) + i0; i < nflt; i += stride) grad[i] *= gs;
      } else {
        for (long long i = i0; i < nflt; i += stride) grad[i] *= gs;
      }
    }
    return;
  }
  for (long long i = i0; i < a.n; i += stride) {
    float w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = a.w7[i * 7 + k];
    if (a.pro == GD3D_PRO_ANCHOR_DELTA) {
      float enc[7], an[7], dec[7];
      DecodeJac J;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        enc[k] = a.pred[i * 7 + k];
        an[k] = a.aux[i * 7 + k];
      }
      decode_anchor(enc, an, dec, J);
      encode_grad(w, J, true);
    } else if (a.pro == GD3D_PRO_CENTER) {
      w[0] *= a.osf * a.vs0;
      w[1] *= a.osf * a.vs1;
      if (a.norm_bbox) {
#pragma unroll
        for (int k = 3; k < 6; ++k) w[k] *= expf(a.pred[i * 7 + k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (a.gp != nullptr) a.gp[i * 7 + k] = gs * w[k];
      if (a.gt != nullptr) a.gt[i * 7 + k] = 0.0f;
    }
  }
}

// HBM ceiling probe for the access mix of the fused kernel: c = a + b over float4 vectors, nontemporal loads and
// stores, one vector per thread, full grid of 64-THREAD workgroups — the fastest and the most repeatable of the shapes
// a stand-alone probe measured (126.1-129 us over five processes for 3 x 280 MB; 256-thread workgroups: 126.8-133).
// bench.py runs it on the fused kernel's OWN three buffers right after the timed region, so that
// `roofline.copy_ceiling_GBps` is the ceiling of that box and of that buffer placement.
constexpr int PROBE_T = 64;
__global__ __launch_bounds__(PROBE_T) void probe_add_kernel(const v4f* __restrict__ x, const v4f* __restrict__ y,
                                                            v4f* __restrict__ z, long long nv) {
  const long long i = (long long)blockIdx.x * PROBE_T + threadIdx.x;
  if (i < nv) {
    const v4f p = __builtin_nontemporal_load(x + i);
    const v4f q = __builtin_nontemporal_load(y + i);
    __builtin_nontemporal_store(p + q, z + i);
  }
}

struct Geometry {
  unsigned tgrid;  // one workgroup per 256-pair tile
  // profiling only (gd3d_loss_fused_timed): events bound to THIS dispatch, see launch_one
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  bool reuse = false;  // the previous fused launch on this stream read the same target: no occupancy cap (MIN_LDS above)
};

template <int LOSS, int FUN, bool FLAG, bool GT>
static void launch_one(const Geometry& g, hipStream_t s, const LossArgs& a) {
  size_t lds = (size_t)(2 * TILE_F + 32 + (a.w7 != nullptr ? TILE_F : 0)) * sizeof(float);
  constexpr int min_lds = LOSS == GD3D_GWD3D ? MIN_LDS_GWD : (LOSS == GD3D_KLD3D ? MIN_LDS_KLD :
                          (LOSS == GD3D_BD3D ? MIN_LDS_BD : MIN_LDS));
  if (!g.reuse && lds < (size_t)min_lds) lds = (size_t)min_lds;   // occupancy cap (see MIN_LDS above)
  // with (N,7) weights a workgroup keeps three tiles in flight: 5 per CU for every loss (10 M pairs, fixed placement,
  // 7/6/5/4/3 per CU: kld3d 185.5/185.4/179.8/180.9/202.7 us, bd3d 185.8/184.7/178.0/177.9/204.9, gwd3d 185.0/185.2/182.3/182.7/201.4)
  if (a.w7 != nullptr && lds < (size_t)MIN_LDS_W7) lds = (size_t)MIN_LDS_W7;
  // The option-free instantiation, for calls that use none of the options — built and used for gwd3d only, without a
  // target gradient.  Same buffers, 4 sets, us per 10 M pairs against the general instantiation
  // (profiles/r02_plain_and_dma_issue_ab.txt): gwd3d -2.5 -0.7 -1.8 -0.5 (issue units per wave 424 -> 340), but kld3d
  // +1.0 +1.5 +1.2 +1.0 and bd3d +0.9 +0.7 +1.1 +1.9 at their cap of 6 workgroups per CU although their streams shrink
  // as well (483 -> 415, 519 -> 433): with less to issue they keep more bytes in flight, which is what the cap exists to
  // limit, and at 5 per CU they lose more than they gain on a fast box (133.0 vs 130.3 us).  gwd3d is the slowest of
  // the three on fast boxes, i.e. the kernel roofline.frac is computed from.
  constexpr bool HAS_PLAIN = LOSS == GD3D_GWD3D;
  const bool plain = HAS_PLAIN && !GT && a.w == nullptr && a.w7 == nullptr && !a.wsel && a.pro == GD3D_PRO_NONE &&
                     a.loss == nullptr && a.fin == nullptr;
  if (g.ev_start != nullptr || g.ev_stop != nullptr) {
    // hipExtLaunchKernel binds the two events to the begin / end timestamps of this dispatch packet itself: no marker
    // packets enter the stream, and hipEventElapsedTime(start, stop) is the kernel's execution time as rocprofv3 reports
    // it (events recorded AROUND a launch add the ~3 us of two barrier packets to every bracket).
    if (plain)
      hipExtLaunchKernelGGL((fused_kernel<LOSS, FUN, FLAG, false, HAS_PLAIN>), dim3(g.tgrid), dim3(TILE),
                            (std::uint32_t)lds, s, g.ev_start, g.ev_stop, 0u, a);
    else
      hipExtLaunchKernelGGL((fused_kernel<LOSS, FUN, FLAG, GT>), dim3(g.tgrid), dim3(TILE), (std::uint32_t)lds, s,
                            g.ev_start, g.ev_stop, 0u, a);
    return;
  }
  if (plain)
    hipLaunchKernelGGL((fused_kernel<LOSS, FUN, FLAG, false, HAS_PLAIN>), dim3(g.tgrid), dim3(TILE), lds, s, a);
  else
    hipLaunchKernelGGL((fused_kernel<LOSS, FUN, FLAG, GT>), dim3(g.tgrid), dim3(TILE), lds, s, a);
}

}  // namespace gd3d

using namespace gd3d;

extern "C" {

// workspace layout (all offsets multiples of 16 bytes), nb = tiles of 256 rows, nbp = nb rounded up to 4, ng = 64-tile groups:
//   float  partials[3][nbp]   loss | sum(pred * weight7) | any weight > 0   (rows 1, 2 only for gd3d_loss_fused_select)
static inline int64_t ws_nbp(int64_t n) { return (((n + 255) / 256) + 3) & ~(int64_t)3; }

size_t gd3d_loss_workspace_bytes(int64_t n) {
  if (n <= 0) return 64;
  return (size_t)(12 * ws_nbp(n) + 16);
}

int gd3d_loss_fused(const gd3d_params* p, const float* pred, const float* target, const float* row_weight,
                    int64_t n, float scale, float* loss, float* loss_sum, float* grad_pred, float* grad_target,
                    void* workspace, void* stream) {
  return gd3d_loss_fused_w7(p, pred, target, row_weight, nullptr, n, scale, loss, loss_sum, grad_pred, grad_target,
                            workspace, stream);
}

int gd3d_loss_fused_w7(const gd3d_params* p, const float* pred, const float* target, const float* row_weight,
                       const float* weight7, int64_t n, float scale, float* loss, float* loss_sum, float* grad_pred,
                       float* grad_target, void* workspace, void* stream) {
  return gd3d_loss_fused_decoded(p, nullptr, pred, target, row_weight, weight7, n, scale, loss, loss_sum, grad_pred,
                                 grad_target, workspace, stream);
}

static int loss_launch(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                       const float* row_weight, const float* weight7, int64_t n, float scale, float* loss,
                       float* loss_sum, float* grad_pred, float* grad_target, void* workspace, void* stream,
                       void* start_event, void* stop_event, int32_t* any_positive, bool select, int32_t* ticket = nullptr);

int gd3d_loss_fused_decoded(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                            const float* row_weight, const float* weight7, int64_t n, float scale, float* loss,
                            float* loss_sum, float* grad_pred, float* grad_target, void* workspace, void* stream) {
  return loss_launch(p, pro, pred, target, row_weight, weight7, n, scale, loss, loss_sum, grad_pred, grad_target,
                     workspace, stream, nullptr, nullptr, nullptr, false);
}

int gd3d_loss_fused_timed(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                          const float* row_weight, const float* weight7, int64_t n, float scale, float* loss,
                          float* loss_sum, float* grad_pred, float* grad_target, void* workspace, void* stream,
                          void* start_event, void* stop_event) {
  return loss_launch(p, pro, pred, target, row_weight, weight7, n, scale, loss, loss_sum, grad_pred, grad_target,
                     workspace, stream, start_event, stop_event, nullptr, false);
}

int gd3d_loss_fused_select(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                           const float* weight7, int64_t n, float scale, float* loss_sum, int32_t* any_positive,
                           float* grad_pred, float* grad_target, void* workspace, void* stream, void* start_event,
                           void* stop_event) {
  if ((n > 0 && weight7 == nullptr) || loss_sum == nullptr || any_positive == nullptr || workspace == nullptr)
    return GD3D_E_BADARG;   // (an empty weight array has no address)
  return loss_launch(p, pro, pred, target, nullptr, weight7, n, scale, nullptr, loss_sum, grad_pred, grad_target,
                     workspace, stream, start_event, stop_event, any_positive, true);
}

int gd3d_loss_fused_one_launch(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                               const float* row_weight, const float* weight7, int64_t n, float scale, float* loss_sum,
                               int32_t* any_positive, float* grad_pred, float* grad_target, void* workspace,
                               int32_t* ticket, void* stream) {
  if (loss_sum == nullptr || workspace == nullptr || ticket == nullptr || n > gd3d_one_launch_max_n()) return GD3D_E_BADARG;
  if (any_positive != nullptr && (row_weight != nullptr || (n > 0 && weight7 == nullptr))) return GD3D_E_BADARG;
  return loss_launch(p, pro, pred, target, row_weight, weight7, n, scale, nullptr, loss_sum, grad_pred, grad_target,
                     workspace, stream, nullptr, nullptr, any_positive, any_positive != nullptr, ticket);
}

int64_t gd3d_one_launch_max_n(void) { return 64 * (int64_t)TILE; }

// Tile order of the fused launch.  Callers evaluate several losses against ONE target back to back (the benchmark step:
// gwd3d, kld3d, bd3d); a launch on the same target and n as the previous fused launch of its stream walks the tiles
// opposite to it, so that it starts on the target rows that launch read last, which are still in the Infinity Cache
// (DMA_AUX_TARGET), and runs without the occupancy cap (MIN_LDS).  Any other launch ascends, capped.  One record per stream; calls may come from several threads.  Under graph
// capture the order is fixed at capture time: a graph of an odd number of such launches, replayed back to back, starts
// each replay in the direction its previous replay started in, and its first launch loses the reuse.
static bool next_tile_order_reversed(hipStream_t s, const float* target, int64_t n, bool* reuse) {
  struct Last {
    const float* target;
    int64_t n;
    bool rev;
  };
  static std::mutex mu;
  static std::unordered_map<hipStream_t, Last> last;
  std::lock_guard<std::mutex> lock(mu);
  auto it = last.find(s);
  *reuse = it != last.end() && it->second.target == target && it->second.n == n;
  const bool rev = *reuse && !it->second.rev;
  if (it == last.end() && last.size() >= 256) last.clear();   // stream handles of destroyed streams: keep the table small
  last[s] = Last{target, n, rev};
  return rev;
}

static int loss_launch(const gd3d_params* p, const gd3d_prologue* pro, const float* pred, const float* target,
                       const float* row_weight, const float* weight7, int64_t n, float scale, float* loss,
                       float* loss_sum, float* grad_pred, float* grad_target, void* workspace, void* stream,
                       void* start_event, void* stop_event, int32_t* any_positive, bool select, int32_t* ticket) {
  if (row_weight != nullptr && weight7 != nullptr) return GD3D_E_BADARG;
  if (pro != nullptr && pro->kind != GD3D_PRO_NONE) {
    if (pro->kind != GD3D_PRO_ANCHOR_DELTA && pro->kind != GD3D_PRO_CENTER) return GD3D_E_BADARG;
    if (n > 0 && pro->aux == nullptr) return GD3D_E_BADARG;
  }
  if (p == nullptr || n < 0) return GD3D_E_BADARG;
  if (n > 0 && (pred == nullptr || target == nullptr)) return GD3D_E_BADARG;
  if (check_instance(p->loss_type, p->fun) != 0) return GD3D_E_BADARG;
  if (loss_sum != nullptr && workspace == nullptr) return GD3D_E_BADARG;
  if (workspace != nullptr && ((uintptr_t)workspace & 15) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = (n + TILE - 1) / TILE;
  if (nb > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (n == 0) {
    // no rows: sum 0; torch.any() of an empty weight is False, so a selecting call takes the early-out, whose value is 0 too
    if (any_positive != nullptr) {
      const int e0 = fill_words(any_positive, sizeof(int32_t), 0u, s);
      if (e0 != 0) return e0;
    }
    if (loss_sum != nullptr) return fill_words(loss_sum, sizeof(float), 0u, s);
    return 0;
  }
  if (loss_sum == nullptr && loss == nullptr && grad_pred == nullptr && grad_target == nullptr && workspace == nullptr)
    return 0;  // nothing requested
  LossArgs a;
  a.wsel = select ? 1 : 0;
  a.nbp = ws_nbp(n);
  a.fin = (int*)ticket;
  a.fin_out = loss_sum;
  a.fin_any = (int*)any_positive;

  a.pred = pred;
  a.target = target;
  a.w = row_weight;
  a.w7 = weight7;
  a.loss = loss;
  a.gp = grad_pred;
  a.gt = grad_target;
  a.partials = (float*)workspace;  // per-workgroup partial sums are produced whenever a workspace is given
  a.n = n;
  a.scale = scale;
  a.alpha = p->alpha;
  a.ia2 = gd3d_inv_alpha2(p->alpha);
  a.tau = p->tau;
  a.c0 = p->center_offset[0];
  a.c1 = p->center_offset[1];
  a.c2 = p->center_offset[2];
  a.pro = (pro != nullptr) ? pro->kind : GD3D_PRO_NONE;
  a.norm_bbox = (pro != nullptr) ? pro->norm_bbox : 0;
  a.aux = (pro != nullptr) ? pro->aux : nullptr;
  a.osf = (pro != nullptr) ? pro->out_size_factor : 1.0f;
  a.vs0 = (pro != nullptr) ? pro->voxel_size[0] : 1.0f;
  a.vs1 = (pro != nullptr) ? pro->voxel_size[1] : 1.0f;
  a.pc0 = (pro != nullptr) ? pro->pc_range[0] : 0.0f;
  a.pc1 = (pro != nullptr) ? pro->pc_range[1] : 0.0f;
  const uintptr_t bits = (uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad_pred | (uintptr_t)grad_target |
                         (uintptr_t)weight7;
  a.vec_ok = (bits & 15) == 0;
  bool reuse = false;
  a.rev = next_tile_order_reversed(s, target, n, &reuse) ? 1 : 0;
  const bool gt = grad_target != nullptr;
  Geometry grid;
  grid.tgrid = (unsigned)nb;
  grid.ev_start = (hipEvent_t)start_event;
  grid.ev_stop = (hipEvent_t)stop_event;
  grid.reuse = reuse;
  const hipError_t e = with_instance(p->loss_type, p->fun, p->flag != 0, [&](auto inst) {
    using I = decltype(inst);
    if (gt) launch_one<I::loss, I::fun, I::flag, true>(grid, s, a);
    else launch_one<I::loss, I::fun, I::flag, false>(grid, s, a);
    return hipGetLastError();
  });
  if (e != hipSuccess) return (int)e;
  if (ticket != nullptr) return 0;   // the last workgroup of the fused kernel wrote the result
  if (select) {
    hipLaunchKernelGGL(reduce_select_kernel, dim3(1), dim3(1024), 0, s, (const float*)workspace, (long long)nb,
                       (long long)ws_nbp(n), loss_sum, (int*)any_positive);
    return (int)hipGetLastError();
  }
  if (loss_sum != nullptr) return gd3d_loss_reduce(workspace, n, loss_sum, stream);
  return 0;
}

int gd3d_grad_finish(float* grad_pred, float* grad_target, const float* g, int64_t n, const int32_t* any_positive,
                     const float* weight7, const float* pred, const gd3d_prologue* pro, void* stream) {
  if (n < 0 || g == nullptr) return GD3D_E_BADARG;
  if (n == 0 || (grad_pred == nullptr && grad_target == nullptr)) return 0;
  FinishArgs a;
  a.gp = grad_pred;
  a.gt = grad_target;
  a.g = g;
  a.any_pos = (const int*)any_positive;
  a.w7 = weight7;
  a.pred = pred;
  a.n = n;
  a.pro = (pro != nullptr) ? pro->kind : GD3D_PRO_NONE;
  a.norm_bbox = (pro != nullptr) ? pro->norm_bbox : 0;
  a.aux = (pro != nullptr) ? pro->aux : nullptr;
  a.osf = (pro != nullptr) ? pro->out_size_factor : 1.0f;
  a.vs0 = (pro != nullptr) ? pro->voxel_size[0] : 1.0f;
  a.vs1 = (pro != nullptr) ? pro->voxel_size[1] : 1.0f;
  if (any_positive != nullptr) {
    if (weight7 == nullptr) return GD3D_E_BADARG;
    if (a.pro != GD3D_PRO_NONE && pred == nullptr) return GD3D_E_BADARG;
    if (a.pro == GD3D_PRO_ANCHOR_DELTA && a.aux == nullptr) return GD3D_E_BADARG;
  }
  // few waves: the common case is the g == 1 early exit, whose cost is the dispatch itself
  long long blocks = ((long long)n * 7 + 4 * FINISH_T - 1) / (4 * FINISH_T);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)blocks), dim3(FINISH_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int gd3d_probe_stream(const float* x, const float* y, float* z, int64_t n_floats, void* stream, void* start_event,
                      void* stop_event) {
  if (n_floats < 0 || (n_floats & 3) != 0) return GD3D_E_BADARG;
  if (n_floats == 0) return 0;
  if (x == nullptr || y == nullptr || z == nullptr) return GD3D_E_BADARG;
  if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)z) & 15) != 0) return GD3D_E_BADARG;
  const long long nv = n_floats >> 2;
  const long long nb = (nv + PROBE_T - 1) / PROBE_T;
  if (nb > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  hipExtLaunchKernelGGL(probe_add_kernel, dim3((unsigned)nb), dim3(PROBE_T), 0u, (hipStream_t)stream, (hipEvent_t)start_event,
                        (hipEvent_t)stop_event, 0u, (const v4f*)x, (const v4f*)y, (v4f*)z, nv);
  return (int)hipGetLastError();
}

int gd3d_loss_reduce(const void* workspace, int64_t n, float* loss_sum, void* stream) {
  if (n < 0 || loss_sum == nullptr) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return fill_words(loss_sum, sizeof(float), 0u, s);
  if (workspace == nullptr) return GD3D_E_BADARG;
  const long long nparts = (n + TILE - 1) / TILE;
  return reduce_partials((const float*)workspace, nparts, loss_sum, s);
}

size_t gd3d_loss_fused_multi_workspace_bytes(int32_t count, int64_t n) {
  if (n <= 0 || count <= 0) return 64;
  return (size_t)(4 * (int64_t)count * ws_nbp(n) + 16);
}

int gd3d_loss_fused_multi_eligible(const gd3d_params* p) {
  return p != nullptr && multi_marked(p->loss_type, p->fun, p->flag != 0) ? 1 : 0;
}

int gd3d_loss_fused_multi(int32_t count, const gd3d_params* params, const float* const* preds, const float* target,
                          int64_t n, const float* scales, float* const* loss_sums, float* const* grad_preds,
                          void* workspace, void* stream) {
  if (count < 2 || count > MULTI_MAX || params == nullptr || preds == nullptr || scales == nullptr || loss_sums == nullptr ||
      n < 0)
    return GD3D_E_BADARG;
  for (int k = 0; k < count; ++k) {
    if (!gd3d_loss_fused_multi_eligible(&params[k]) || loss_sums[k] == nullptr) return GD3D_E_BADARG;
    if (n > 0 && preds[k] == nullptr) return GD3D_E_BADARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    for (int k = 0; k < count; ++k) {
      const int e0 = fill_words(loss_sums[k], sizeof(float), 0u, s);
      if (e0 != 0) return e0;
    }
    return 0;
  }
  if (target == nullptr || workspace == nullptr || ((uintptr_t)workspace & 15) != 0) return GD3D_E_BADARG;
  const int64_t nb = (n + TILE - 1) / TILE;
  if (nb > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  // the kernels exist for non-decreasing loss types: slot j of the launch is the caller's loss order[j] (stable)
  int order[MULTI_MAX] = {0, 1, 2};
  for (int i = 1; i < count; ++i)
    for (int j = i; j > 0 && params[order[j]].loss_type < params[order[j - 1]].loss_type; --j) {
      const int t = order[j];
      order[j] = order[j - 1];
      order[j - 1] = t;
    }
  const long long nbp = ws_nbp(n);
  MultiArgs a = {};
  ReduceMultiArgs r = {};
  uintptr_t bits = (uintptr_t)target;
  int lt[MULTI_MAX] = {-1, -1, -1};
  for (int j = 0; j < count; ++j) {
    const int k = order[j];
    const gd3d_params& p = params[k];
    lt[j] = p.loss_type;
    a.pred[j] = preds[k];
    a.gp[j] = grad_preds != nullptr ? grad_preds[k] : nullptr;
    a.partials[j] = (float*)workspace + j * nbp;
    a.scale[j] = scales[k];
    a.alpha[j] = p.alpha;
    a.ia2[j] = gd3d_inv_alpha2(p.alpha);
    a.tau[j] = p.tau;
    for (int q = 0; q < 3; ++q) a.c[j][q] = p.center_offset[q];
    r.out[j] = loss_sums[k];
    bits |= (uintptr_t)a.pred[j] | (uintptr_t)a.gp[j];
  }
  a.target = target;
  a.n = n;
  a.vec_ok = (bits & 15) == 0;
  // this launch walks the tiles upwards once and leaves the end of the target in the Infinity Cache at best: the next
  // single launch on this stream starts without reuse (ascending, capped)
  bool reuse = false;
  next_tile_order_reversed(s, nullptr, -1, &reuse);
  const hipError_t e = with_multi_tuple(lt[0], lt[1], lt[2], [&](auto tup) {
    using T = decltype(tup);
    constexpr int K = T::count;
    size_t lds = (size_t)((K + 1) * TILE_F + 32) * sizeof(float);
    constexpr size_t min_lds = K == 3 ? MULTI_LDS_K3 : MULTI_LDS_K2;
    if (lds < min_lds) lds = min_lds;
    hipLaunchKernelGGL((fused_multi_kernel<T::l0, T::l1, T::l2>), dim3((unsigned)nb), dim3(TILE), lds, s, a);
    return hipGetLastError();
  });
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(reduce_partials_multi_kernel, dim3((unsigned)count), dim3(1024), 0, s, (const float*)workspace,
                     (long long)nb, nbp, r);
  return (int)hipGetLastError();
}

int gd3d_prof_event_create(void** event) {
  if (event == nullptr) return GD3D_E_BADARG;
  hipEvent_t e = nullptr;
  const hipError_t rc = hipEventCreate(&e);
  *event = (void*)e;
  return (int)rc;
}

int gd3d_prof_event_destroy(void* event) {
  if (event == nullptr) return 0;
  return (int)hipEventDestroy((hipEvent_t)event);
}

int gd3d_prof_event_elapsed_ms(void* start_event, void* stop_event, float* ms) {
  if (start_event == nullptr || stop_event == nullptr || ms == nullptr) return GD3D_E_BADARG;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

int gd3d_scale_rows(float* grad, const float* g, int per_row, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (grad == nullptr || g == nullptr))) return GD3D_E_BADARG;
  if (n == 0) return 0;
  const long long nflt = (long long)n * 7;
  // grid-stride with FEW, LARGE workgroups: the common case is the g == 1 early exit, whose cost is the dispatch of the
  // workgroups (1024 x 256 threads: 4.5 us; 256 x 1024 threads: the same 262 144 lanes for a real scaling pass)
  long long blocks = (nflt + 1023) / 1024;
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, grad, g, per_row,
                     nflt);
  return (int)hipGetLastError();
}

int gd3d_abi_version(const char** arch) {
  if (arch != nullptr) *arch = "gfx950";
  return GD3D_ABI_VERSION;
}

}  // extern "C"
