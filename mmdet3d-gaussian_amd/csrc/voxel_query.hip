// voxel_query.hip — voxel query and the fused voxel query-and-group for gfx950 (include/gd3d.h, gd3d_vsa_voxel_*):
// a query looks only at the cells of a (2 rz + 1) x (2 ry + 1) x (2 rx + 1) window around its own cell.  Replaces the reference's
// ops/vsa/src/voxel_query_gpu.cu:10-89 (voxel_query_kernel_stack), which reads a dense (B, Z, Y, X) table of rows; here the cells are
// looked up in a sorted list of 64-bit keys (sparse_conv::in_key, device_sort.h's stable radix sort, sparse_conv::lower_bound), and the
// table form stays for callers who hold one.
//
// Shapes:
//   query / group : one wave per query, QW queries per workgroup, no block-wide barrier; the idx row is staged per wave in LDS and a
//                   wave stops as soon as it holds nsample members.
//     dense table : a lane takes one window cell per step (64 cells a step): one table load, one xyz row load, the test; a ballot and
//                   a lane prefix count give every member its slot — window order by construction.
//     sorted keys : a lane takes one window ROW (dz, dy) per step: the row's cells x - rx .. x + rx, clipped to [0, X), are consecutive
//                   keys, so ONE lower_bound finds the run's first entry and the lane walks on while skey <= the run's last key (an
//                   entry whose key equals its predecessor's is a duplicate cell: the stable sort put the lowest row first).  A wave
//                   prefix sum of the lanes' member counts gives every lane its slot base: rows ascending, then x ascending, is window
//                   order.  The lane remembers the outcome of its first 64 entries in a bit mask and walks the run a second time to
//                   write its slots.
//                   The gather that follows is csrc/vsa_gather.h's, shared with csrc/vsa.hip.
//   index         : key kernel -> device_sort.h's sort_pairs (stable, key_bits of the sentinel) straight into skey / srow.
//   table         : fill with -1, then an unsigned atomicMin per row: -1 is the largest unsigned value, the lowest row wins.
//   coords        : a thread per query row.
// Compiled with -ffp-contract=off: every membership and every cell replays bit for bit in csrc/voxel_query_cpu.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd3d.h"
#include "device_sort.h"
#include "gd3d_fill.h"
#include "gd3d_workspace.h"
#include "voxel_query_common.h"
#include "vsa_gather.h"

namespace voxel_query {

struct QueryArgs {
  const float* xyz;
  const float* new_xyz;
  const int32_t* new_coords;
  const long long* skey;
  const int32_t* srow;
  const int32_t* table;
  const float* feats;
  Geo g;
  Window w;
  long long N, M;
  int C, nsample, c_xyz;   // c_xyz: 3 when the xyz channels are written, else 0
  int cc;                  // feature channels per pass through the transpose buffer
  unsigned magic_ns;
  float radius2;
  float* out;
  int32_t* idx;
  int32_t* cnt;
  uint8_t* mask;
};

template <bool DENSE, bool GROUP>
__global__ __launch_bounds__(QW * 64) void query_kernel(const QueryArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long m = (long long)blockIdx.x * QW + w;
  if (m >= a.M) return;   // no block-wide barrier below
  const int nsample = a.nsample;
  int* const lidx = reinterpret_cast<int*>(lds_f) + w * nsample;
  float* const xp = reinterpret_cast<float*>(reinterpret_cast<int*>(lds_f) + QW * nsample) + w * vsa::XP;
  const float q[3] = {a.new_xyz[m * 3 + 0], a.new_xyz[m * 3 + 1], a.new_xyz[m * 3 + 2]};
  const int b = a.new_coords[m * 4 + 0], cz = a.new_coords[m * 4 + 1], cy = a.new_coords[m * 4 + 2], cx = a.new_coords[m * 4 + 3];
  int found = 0;
  if (b >= 0 && b < a.g.B) {   // wave-uniform
    if (DENSE) {
      for (int j0 = 0; j0 < a.w.cells; j0 += 64) {
        const int j = j0 + lane;
        bool member = false;
        int row = 0;
        long long key = 0;
        if (j < a.w.cells && window_cell(a.g, a.w, b, cz, cy, cx, j, &key)) {
          row = a.table[key];
          if (row >= 0 && row < a.N) member = is_member(q, a.xyz + (long long)row * 3, a.radius2);   // a caller's table may hold garbage
        }
        const unsigned long long bal = __ballot(member);
        if (bal != 0ull) {
          const int slot = found + __popcll(bal & ((1ull << lane) - 1ull));
          if (member && slot < nsample) lidx[slot] = row;
          found += __popcll(bal);
          if (found >= nsample) {   // early stop: later cells cannot change idx, cnt or the mask
            found = nsample;
            break;
          }
        }
      }
    } else {
      for (int j0 = 0; j0 < a.w.rows; j0 += 64) {
        const int j = j0 + lane;
        long long at = 0, k0 = 0, k1 = -1;
        int members = 0;
        unsigned long long bits = 0ull;   // outcome of the run's first 64 entries
        const bool live = j < a.w.rows && window_row(a.g, a.w, b, cz, cy, cx, j, &k0, &k1);
        if (live) {
          at = sparse_conv::lower_bound(a.skey, a.N, k0);
          long long prev = -1;
          for (long long e = at; e < a.N; ++e) {
            const long long key = a.skey[e];
            if (key > k1) break;
            if (key == prev) continue;
            prev = key;
            const int row = a.srow[e];
            if (row >= 0 && row < a.N && is_member(q, a.xyz + (long long)row * 3, a.radius2)) {
              if (e - at < 64) bits |= 1ull << (e - at);
              ++members;
            }
          }
        }
        int incl = members;   // inclusive wave prefix sum
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int t = __shfl_up(incl, d);
          if (lane >= d) incl += t;
        }
        const int total = __shfl(incl, 63);
        if (total != 0) {
          int slot = found + incl - members;
          if (members > 0 && slot < nsample) {
            long long prev = -1;
            for (long long e = at; e < a.N; ++e) {
              const long long key = a.skey[e];
              if (key > k1) break;
              if (key == prev) continue;
              prev = key;
              const int row = a.srow[e];
              const bool member = e - at < 64 ? ((bits >> (e - at)) & 1ull) != 0ull
                                              : (row >= 0 && row < a.N && is_member(q, a.xyz + (long long)row * 3, a.radius2));
              if (member) {
                lidx[slot] = row;
                if (++slot >= nsample) break;
              }
            }
          }
          found += total;
          if (found >= nsample) {
            found = nsample;
            break;
          }
        }
      }
    }
  }
  vsa::write_query<true, GROUP>(a, m, 0LL, lidx, xp, found, q[0], q[1], q[2], lane);   // rows are global: p0 = 0
}

__global__ __launch_bounds__(BLOCK) void key_kernel(const void* __restrict__ coors, int is64, long long n, const Geo g,
                                                    long long* __restrict__ keys, int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  keys[i] = row_key(coors, is64, i, g);
  vals[i] = (int)i;
}

__global__ __launch_bounds__(BLOCK) void table_kernel(const void* __restrict__ coors, int is64, long long n, const Geo g,
                                                      int32_t* __restrict__ table) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const long long key = row_key(coors, is64, i, g);
  if (key < g.in_sent) atomicMin(reinterpret_cast<unsigned*>(table) + key, (unsigned)i);   // -1 is the largest unsigned value
}

struct CoordsArgs {
  float vsl[3], lo[3];
};

__global__ __launch_bounds__(BLOCK) void coords_kernel(const float* __restrict__ new_xyz, const int32_t* __restrict__ qcnt, int B,
                                                       long long M, const CoordsArgs c, int32_t* __restrict__ out) {
  const long long m = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (m >= M) return;
  const float p[3] = {new_xyz[m * 3 + 0], new_xyz[m * 3 + 1], new_xyz[m * 3 + 2]};
  int32_t r[4];
  query_coords(p, sample_of_row(qcnt, B, M, m), c.vsl, c.lo, r);
  for (int k = 0; k < 4; ++k) out[m * 4 + k] = r[k];
}

static unsigned blocks_of(long long n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }   // n <= 2^31 - 1

// the workspace of gd3d_vsa_voxel_index; its size is the same carve at address 0
struct IndexWork {
  long long* key_in;
  int* val_in;
  char* sort_tmp;
  size_t sort_bytes = 0, bytes = 0;
  hipError_t err;
  IndexWork(void* workspace, int64_t n) {
    err = gd3d::sort_pairs_temp_bytes((size_t)n, sort_bytes);
    if (err != hipSuccess) return;
    gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
    key_in = c.take<long long>((size_t)n);
    val_in = c.take<int>((size_t)n);
    sort_tmp = c.take<char>(sort_bytes);
    bytes = c.bytes();
  }
};

// Dynamic LDS of a query launch: the waves' idx rows (16 * nsample B) and, when grouping, their transpose buffers (17408 B):
// at most 33792 B, below the default limit.
template <bool GROUP>
constexpr size_t query_lds_bytes(int nsample) {
  return ((size_t)QW * nsample + (GROUP ? (size_t)QW * vsa::XP : 0)) * 4;
}
static_assert(query_lds_bytes<true>(vsa::MAX_NSAMPLE) <= 65536, "no raised dynamic-LDS limit");

template <bool DENSE, bool GROUP>
static int launch_query(const QueryArgs& a, hipStream_t s) {
  const long long blocks = (a.M + QW - 1) / QW;
  hipLaunchKernelGGL((query_kernel<DENSE, GROUP>), dim3((unsigned)blocks), dim3(QW * 64), query_lds_bytes<GROUP>(a.nsample), s, a);
  return (int)hipGetLastError();
}

}  // namespace voxel_query

using namespace voxel_query;

extern "C" {

size_t gd3d_vsa_voxel_index_workspace_bytes(int64_t N) {
  if (N <= 0 || N > 0x7fffffffLL) return 256;
  const IndexWork w(nullptr, N);
  return w.err == hipSuccess ? w.bytes : 0;
}

int gd3d_vsa_voxel_index(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                         void* workspace, int64_t* skey, int32_t* srow, void* stream) {
  Geo g;
  const int rc = make_grid(N, B, Z, Y, X, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || skey == nullptr || srow == nullptr || workspace == nullptr || ((uintptr_t)workspace & 255) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const IndexWork w(workspace, N);
  if (w.err != hipSuccess) return (int)w.err;
  hipLaunchKernelGGL(key_kernel, dim3(blocks_of(N)), dim3(BLOCK), 0, s, coors, coors_is_int64 ? 1 : 0, (long long)N, g, w.key_in, w.val_in);
  const hipError_t he = gd3d::sort_pairs(w.sort_tmp, w.sort_bytes, w.key_in, reinterpret_cast<long long*>(skey), w.val_in, srow, (size_t)N,
                                         (unsigned)gd3d::key_bits(g.in_sent), s);
  return he != hipSuccess ? (int)he : (int)hipGetLastError();
}

int gd3d_vsa_voxel_table(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                         int32_t* table, void* stream) {
  Geo g;
  const int rc = make_grid(N, B, Z, Y, X, &g);
  if (rc != 0) return rc;
  if (g.in_sent == 0) return 0;
  if (table == nullptr || (N > 0 && coors == nullptr)) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int e = gd3d::fill_words(table, (size_t)g.in_sent * 4, 0xffffffffu, s);
  if (e != 0 || N == 0) return e;
  hipLaunchKernelGGL(table_kernel, dim3(blocks_of(N)), dim3(BLOCK), 0, s, coors, coors_is_int64 ? 1 : 0, (long long)N, g, table);
  return (int)hipGetLastError();
}

int gd3d_vsa_voxel_coords(const float* new_xyz, const int32_t* new_xyz_batch_cnt, int32_t B, int64_t M, const float* cell_size,
                          const float* range_min, int32_t* new_coords, void* stream) {
  if (B < 0 || M < 0 || cell_size == nullptr || range_min == nullptr) return GD3D_E_BADARG;
  if (M > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  CoordsArgs c;
  for (int k = 0; k < 3; ++k) {
    if (!(cell_size[k] > 0.0f) || !(range_min[k] == range_min[k])) return GD3D_E_BADARG;
    c.vsl[k] = cell_size[k];
    c.lo[k] = range_min[k];
  }
  if (M == 0) return 0;
  if (new_xyz == nullptr || new_coords == nullptr || (B > 0 && new_xyz_batch_cnt == nullptr)) return GD3D_E_BADARG;
  hipLaunchKernelGGL(coords_kernel, dim3(blocks_of(M)), dim3(BLOCK), 0, (hipStream_t)stream, new_xyz, new_xyz_batch_cnt, (int)B, (long long)M, c,
                     new_coords);
  return (int)hipGetLastError();
}

int gd3d_vsa_voxel_query(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey, const int32_t* srow,
                         const int32_t* table, int32_t B, int32_t Z, int32_t Y, int32_t X, int64_t N, int64_t M, const int32_t* max_range,
                         float radius, int32_t nsample, int32_t* idx, int32_t* cnt, uint8_t* empty_mask, void* stream) {
  return gd3d_vsa_voxel_query_and_group(xyz, new_xyz, new_coords, skey, srow, table, nullptr, B, Z, Y, X, N, M, 0, max_range, radius, nsample,
                                        0, nullptr, idx, cnt, empty_mask, stream);
}

int gd3d_vsa_voxel_query_and_group(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                                   const int32_t* srow, const int32_t* table, const float* features, int32_t B, int32_t Z, int32_t Y,
                                   int32_t X, int64_t N, int64_t M, int32_t C, const int32_t* max_range, float radius, int32_t nsample,
                                   int32_t use_xyz, float* out, int32_t* idx, int32_t* cnt, uint8_t* empty_mask, void* stream) {
  QueryArgs a;
  bool run;
  const int rc = check_query(xyz, new_xyz, new_coords, skey, srow, table, features, B, Z, Y, X, N, M, C, max_range, nsample, use_xyz, out, idx,
                             &a.g, &a.w, &run);
  if (rc != 0 || !run) return rc;
  const bool group = out != nullptr;
  a.xyz = xyz; a.new_xyz = new_xyz; a.new_coords = new_coords; a.skey = reinterpret_cast<const long long*>(skey); a.srow = srow;
  a.table = table; a.feats = features;
  a.N = N; a.M = M; a.C = group ? C : 0; a.nsample = nsample; a.c_xyz = (group && use_xyz) ? 3 : 0;
  a.cc = vsa::channels_per_pass(C, nsample);
  a.magic_ns = vsa::magic_of(nsample);
  a.radius2 = radius * radius;
  a.out = out; a.idx = idx; a.cnt = cnt; a.mask = empty_mask;
  hipStream_t s = (hipStream_t)stream;
  if (table != nullptr) return group ? launch_query<true, true>(a, s) : launch_query<true, false>(a, s);
  return group ? launch_query<false, true>(a, s) : launch_query<false, false>(a, s);
}

}  // extern "C"
