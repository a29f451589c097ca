// target_reuse_probe.hip — does a buffer that three back-to-back streaming passes all read stay in the Infinity Cache?
//
// The benchmark step runs three fused loss launches that read the SAME target array (280 MB at 10 M pairs) beside their own
// pred (read) and grad (written) arrays.  This probe reproduces that access shape without the loss math: pass k computes
// C_k = A_k + B over 256-row tiles of 28-byte rows, A_k and B brought into LDS by LDS-DMA (global_load_lds_dwordx4, 14
// 1-KiB pieces per tile, as the fused kernel's issue_tile_dma does), C_k leaving as 16-byte stores.  What varies:
//   * the cache policy of the B (shared) loads: aux bits of global_load_lds (sc0 = 1, nt = 2, sc1 = 16);
//   * the policy of the A loads and C stores: nt (the fused kernel's) or default;
//   * tile order: ascending in every pass, or alternating (pass 2 descends, so it starts on the rows pass 1 read last);
//   * the size of B (A_k and C_k are the same size).
// Before each triple of passes a 1 GiB scratch buffer is read (and, by default, written) with default-policy accesses, so pass 1 starts
// from caches that hold none of the probe's buffers.  Each pass is timed by an event pair bound to its own dispatch.
//
// Output: one JSON line per (size, variant, order) with the per-pass median over the repetitions, in microseconds.
// Usage: target_reuse_probe [reps=7] [sizes in MB, comma separated = 150,280,400] [flush: dirty (default) | clean]
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(x)                                                                                    \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) {                                                                         \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
      std::exit(2);                                                                                 \
    }                                                                                               \
  } while (0)

constexpr int TILE = 256, TILE_F = TILE * 7, NPIECE = TILE_F / 256, NWAVE = TILE / 64, TILE_V4 = TILE_F / 4;
constexpr int LDS_BYTES = 27300;   // the fused kernel's occupancy cap for kld3d / bd3d: 6 workgroups per CU

typedef __attribute__((address_space(3))) void lds_ptr_t;
typedef const __attribute__((address_space(1))) void gbl_cptr_t;
typedef float v4f __attribute__((ext_vector_type(4)));

// BPOL: aux of the B loads; ACNT: A loads and C stores nontemporal (else default policy).  n is a multiple of TILE.
template <int BPOL, bool ACNT>
__global__ __launch_bounds__(TILE) void pass_kernel(const float* a, const float* b, float* c, int rev) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const sa = smem;
  float* const sb = smem + TILE_F;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long tile = rev ? (long long)gridDim.x - 1 - blockIdx.x : (long long)blockIdx.x;
  const long long off = tile * TILE_F;
  // pieces 0..6 are A's, 7..13 B's; wave w issues w, w+4, w+8, w+12: only round k = 1 mixes the two tensors
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = wave + k * NWAVE;
    if (j < NPIECE) {
      __builtin_amdgcn_global_load_lds((gbl_cptr_t*)(a + off + j * 256 + lane * 4), (lds_ptr_t*)(sa + j * 256), 16, 0,
                                       ACNT ? 2 : 0);
    } else if (j < 2 * NPIECE) {
      const int jb = j - NPIECE;
      __builtin_amdgcn_global_load_lds((gbl_cptr_t*)(b + off + jb * 256 + lane * 4), (lds_ptr_t*)(sb + jb * 256), 16, 0,
                                       BPOL);
    }
  }
  __syncthreads();
  v4f* const dst = reinterpret_cast<v4f*>(c + off);
  const v4f* const va = reinterpret_cast<const v4f*>(sa);
  const v4f* const vb = reinterpret_cast<const v4f*>(sb);
  for (int i = tid; i < TILE_V4; i += TILE) {
    const v4f v = va[i] + vb[i];
    if (ACNT)
      __builtin_nontemporal_store(v, dst + i);
    else
      dst[i] = v;
  }
}

// default-policy read (+ write) of a scratch buffer: evicts the probe's buffers from L2 and the Infinity Cache.  With
// write = 0 the caches are left holding clean lines, with write = 1 dirty ones, which a later allocating load must write
// back to HBM before it can take their place.
__global__ __launch_bounds__(256) void flush_kernel(v4f* x, long long nv, int write) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const v4f v = x[i];
    if (write || v.x == 12345.f) x[i] = v + (v4f){1.f, 1.f, 1.f, 1.f};   // the buffer holds zeros: read-only when write == 0
  }
}

typedef void (*kfn)(const float*, const float*, float*, int);
struct Variant {
  const char* name;
  int bpol;
  bool acnt;
  kfn k;
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  const size_t m = v.size() / 2;
  return v.size() % 2 ? v[m] : 0.5 * (v[m - 1] + v[m]);
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 7;
  std::vector<double> sizes_mb;
  {
    std::string s = argc > 2 ? argv[2] : "150,280,400";
    size_t p = 0;
    while (p < s.size()) {
      size_t q = s.find(',', p);
      if (q == std::string::npos) q = s.size();
      sizes_mb.push_back(std::atof(s.substr(p, q - p).c_str()));
      p = q + 1;
    }
  }
  const int dirty = !(argc > 3 && std::strcmp(argv[3], "clean") == 0);
  const Variant variants[] = {
      {"B nt", 2, true, pass_kernel<2, true>},          // the fused kernel today
      {"B default", 0, true, pass_kernel<0, true>},
      {"B sc0", 1, true, pass_kernel<1, true>},
      {"B sc1", 16, true, pass_kernel<16, true>},
      {"B sc0 sc1", 17, true, pass_kernel<17, true>},
      {"B sc0 nt", 3, true, pass_kernel<3, true>},
      {"B sc1 nt", 18, true, pass_kernel<18, true>},
      {"B default, A/C default", 0, false, pass_kernel<0, false>},
      {"B nt, A/C default", 2, false, pass_kernel<2, false>},
  };
  const int nvar = sizeof(variants) / sizeof(variants[0]);
  for (const Variant& v : variants)
    CHECK(hipFuncSetAttribute((const void*)v.k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));

  hipStream_t s;
  CHECK(hipStreamCreate(&s));
  hipEvent_t ev[6];
  for (auto& e : ev) CHECK(hipEventCreate(&e));
  const long long flush_nv = (1LL << 30) / 16;
  v4f* flush;
  CHECK(hipMalloc(&flush, flush_nv * 16));
  CHECK(hipMemset(flush, 0, flush_nv * 16));

  for (double mb : sizes_mb) {
    const long long tiles = (long long)(mb * 1e6 / (TILE * 28.0) + 0.5);
    const long long n = tiles * TILE;
    const size_t bytes = (size_t)n * 28;
    // one allocation for the seven arrays, as bench.py's arena keeps its inputs in one (placement: DESIGN.md §5.3)
    float* arena;
    CHECK(hipMalloc(&arena, 7 * bytes));
    CHECK(hipMemset(arena, 0, 7 * bytes));
    float* B = arena;
    float* A[3] = {arena + n * 7, arena + 2 * n * 7, arena + 3 * n * 7};
    float* C[3] = {arena + 4 * n * 7, arena + 5 * n * 7, arena + 6 * n * 7};
    // t[variant][order][pass][rep]
    std::vector<double> t((size_t)nvar * 2 * 3 * reps);
    auto at = [&](int v, int o, int p, int r) -> double& { return t[(((size_t)v * 2 + o) * 3 + p) * reps + r]; };
    for (int r = 0; r < reps; ++r) {
      for (int v = 0; v < nvar; ++v) {
        for (int o = 0; o < 2; ++o) {
          hipLaunchKernelGGL(flush_kernel, dim3((unsigned)((flush_nv + 255) / 256)), dim3(256), 0, s, flush, flush_nv, dirty);
          for (int p = 0; p < 3; ++p) {
            const int rev = o == 1 ? (p & 1) : 0;
            hipExtLaunchKernelGGL(variants[v].k, dim3((unsigned)tiles), dim3(TILE), (std::uint32_t)LDS_BYTES, s,
                                  ev[2 * p], ev[2 * p + 1], 0u, (const float*)A[p], (const float*)B, C[p], rev);
          }
          CHECK(hipGetLastError());
          CHECK(hipStreamSynchronize(s));
          for (int p = 0; p < 3; ++p) {
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, ev[2 * p], ev[2 * p + 1]));
            at(v, o, p, r) = 1e3 * ms;
          }
        }
      }
    }
    for (int v = 0; v < nvar; ++v)
      for (int o = 0; o < 2; ++o) {
        double med[3];
        for (int p = 0; p < 3; ++p) {
          std::vector<double> x(reps);
          for (int r = 0; r < reps; ++r) x[r] = at(v, o, p, r);
          med[p] = median(x);
        }
        std::printf("{\"flush\": \"%s\", \"B_MB\": %.1f, \"n\": %lld, \"variant\": \"%s\", \"order\": \"%s\", \"pass_us\": [%.1f, %.1f, %.1f], "
                    "\"speedup_2\": %.3f, \"speedup_3\": %.3f}\n",
                    dirty ? "dirty" : "clean", bytes / 1e6, n, variants[v].name, o ? "alternating" : "ascending", med[0], med[1], med[2],
                    med[0] / med[1], med[0] / med[2]);
      }
    std::fflush(stdout);
    CHECK(hipFree(arena));
  }
  CHECK(hipFree(flush));
  return 0;
}
