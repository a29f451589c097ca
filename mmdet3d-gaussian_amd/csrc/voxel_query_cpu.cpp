// voxel_query_cpu.cpp — the `_cpu` twins of the voxel query entry points (include/gd3d.h, gd3d_vsa_voxel_*_cpu): plain loops over the
// window in its stated order, with the arithmetic of csrc/voxel_query_common.h (both units compiled with -ffp-contract=off), so skey,
// srow, the table, the coords, idx, cnt, the mask and the grouped block are bit-identical to the kernels'.  Host memory in and out, no
// stream, no HIP call.  Queries are split over `nthreads` std::threads.
#include "voxel_query_common.h"

#include "host_threads.h"

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

using gd3d_host::parallel_ranges;
using namespace voxel_query;

namespace {

// the cell's row in either look-up form (the LOWEST row of the cell), or -1
int32_t row_at(const long long* skey, const int32_t* srow, const int32_t* table, long long n, long long key) {
  return table != nullptr ? table[key] : sparse_conv::find_row(skey, srow, n, key);
}

}  // namespace

extern "C" {

int gd3d_vsa_voxel_index_cpu(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                             void* workspace, int64_t* skey, int32_t* srow) {
  (void)workspace;
  Geo g;
  const int rc = make_grid(N, B, Z, Y, X, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || skey == nullptr || srow == nullptr) return GD3D_E_BADARG;
  try {
    std::vector<long long> key((size_t)N);
    for (int64_t i = 0; i < N; ++i) key[i] = row_key(coors, coors_is_int64 ? 1 : 0, i, g);
    std::iota(srow, srow + N, 0);
    std::stable_sort(srow, srow + N, [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    for (int64_t i = 0; i < N; ++i) skey[i] = key[srow[i]];
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
  return 0;
}

int gd3d_vsa_voxel_table_cpu(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                             int32_t* table) {
  Geo g;
  const int rc = make_grid(N, B, Z, Y, X, &g);
  if (rc != 0) return rc;
  if (g.in_sent == 0) return 0;
  if (table == nullptr || (N > 0 && coors == nullptr)) return GD3D_E_BADARG;
  for (long long k = 0; k < g.in_sent; ++k) table[k] = -1;
  for (int64_t i = N - 1; i >= 0; --i) {   // descending: the lowest row is written last
    const long long key = row_key(coors, coors_is_int64 ? 1 : 0, i, g);
    if (key < g.in_sent) table[key] = (int32_t)i;
  }
  return 0;
}

int gd3d_vsa_voxel_coords_cpu(const float* new_xyz, const int32_t* new_xyz_batch_cnt, int32_t B, int64_t M, const float* cell_size,
                              const float* range_min, int32_t* new_coords) {
  if (B < 0 || M < 0 || cell_size == nullptr || range_min == nullptr) return GD3D_E_BADARG;
  if (M > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  for (int k = 0; k < 3; ++k)
    if (!(cell_size[k] > 0.0f) || !(range_min[k] == range_min[k])) return GD3D_E_BADARG;
  if (M == 0) return 0;
  if (new_xyz == nullptr || new_coords == nullptr || (B > 0 && new_xyz_batch_cnt == nullptr)) return GD3D_E_BADARG;
  for (int64_t m = 0; m < M; ++m)
    query_coords(new_xyz + m * 3, sample_of_row(new_xyz_batch_cnt, B, M, m), cell_size, range_min, new_coords + m * 4);
  return 0;
}

int gd3d_vsa_voxel_query_and_group_cpu(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                                       const int32_t* srow, const int32_t* table, const float* features, int32_t B, int32_t Z, int32_t Y,
                                       int32_t X, int64_t N, int64_t M, int32_t C, const int32_t* max_range, float radius, int32_t nsample,
                                       int32_t use_xyz, float* out, int32_t* idx, int32_t* cnt, uint8_t* empty_mask, int32_t nthreads) {
  Geo g;
  Window w;
  bool run;
  const int rc = check_query(xyz, new_xyz, new_coords, skey, srow, table, features, B, Z, Y, X, N, M, C, max_range, nsample, use_xyz, out, idx,
                             &g, &w, &run);
  if (rc != 0 || !run) return rc;
  const bool group = out != nullptr;
  const float radius2 = radius * radius;
  const int c_xyz = (group && use_xyz) ? 3 : 0;
  const int ct = c_xyz + (group ? C : 0);
  const long long* sk = reinterpret_cast<const long long*>(skey);
  const int team = gd3d_host::team_size(nthreads, M, 64, 256);
  const bool ok = parallel_ranges(M, team, [&](int64_t m0, int64_t m1) {
    for (int64_t m = m0; m < m1; ++m) {
      const float* q = new_xyz + m * 3;
      const int32_t* c = new_coords + m * 4;
      int32_t* row = idx + m * nsample;
      int found = 0;
      if (c[0] >= 0 && c[0] < g.B) {
        for (int j = 0; j < w.cells && found < nsample; ++j) {
          long long key = 0;
          if (!window_cell(g, w, c[0], c[1], c[2], c[3], j, &key)) continue;
          const int32_t i = row_at(sk, srow, table, N, key);
          if (i < 0 || i >= N) continue;
          if (is_member(q, xyz + (long long)i * 3, radius2)) row[found++] = i;
        }
      }
      const int32_t first = found > 0 ? row[0] : 0;
      for (int s = found; s < nsample; ++s) row[s] = first;
      if (cnt != nullptr) cnt[m] = found;
      if (empty_mask != nullptr) empty_mask[m] = found == 0 ? 1 : 0;
      if (!group) continue;
      float* o = out + m * ct * nsample;
      if (found == 0) {
        for (long long e = 0; e < (long long)ct * nsample; ++e) o[e] = 0.0f;
        continue;
      }
      for (int k = 0; k < c_xyz; ++k)
        for (int s = 0; s < nsample; ++s) o[k * nsample + s] = xyz[(long long)row[s] * 3 + k] - q[k];
      for (int ch = 0; ch < C; ++ch)
        for (int s = 0; s < nsample; ++s) o[(long long)(c_xyz + ch) * nsample + s] = features[(long long)row[s] * C + ch];
    }
  });
  return ok ? 0 : GD3D_E_HOST;
}

int gd3d_vsa_voxel_query_cpu(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey, const int32_t* srow,
                             const int32_t* table, int32_t B, int32_t Z, int32_t Y, int32_t X, int64_t N, int64_t M,
                             const int32_t* max_range, float radius, int32_t nsample, int32_t* idx, int32_t* cnt, uint8_t* empty_mask,
                             int32_t nthreads) {
  return gd3d_vsa_voxel_query_and_group_cpu(xyz, new_xyz, new_coords, skey, srow, table, nullptr, B, Z, Y, X, N, M, 0, max_range, radius,
                                            nsample, 0, nullptr, idx, cnt, empty_mask, nthreads);
}

}  // extern "C"
