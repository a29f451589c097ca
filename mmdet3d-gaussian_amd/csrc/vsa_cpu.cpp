// vsa_cpu.cpp — the `_cpu` twins of the voxel-set-abstraction entry points (include/gd3d.h, gd3d_vsa_*_cpu): plain loops over
// the same fp32 operation sequence as csrc/vsa.hip (csrc/vsa_common.h, both compiled with -ffp-contract=off), so idx, cnt, the
// empty-ball mask and the FPS picks are bit-identical to the kernels', and the grouped outputs (copies and one subtraction) too.
// Host memory in and out, no stream, no HIP call.  Queries / samples are split over `nthreads` std::threads.
#include "vsa_common.h"

#include "../../include/gd3d.h"
#include "host_threads.h"

#include <vector>

using gd3d_host::parallel_ranges;
using namespace vsa;

namespace {

// members of query m's ball into idx_row (first nsample, ascending, tail = first member, empty = zeros); returns the count
int scan_ball(const float* xyz, long long p0, int np, const float* c, float radius2, int nsample, int32_t* idx_row) {
  int found = 0;
  for (int k = 0; k < np && found < nsample; ++k) {
    const float* p = xyz + (p0 + k) * 3;
    if (dist2(c[0], c[1], c[2], p[0], p[1], p[2]) < radius2) idx_row[found++] = k;
  }
  const int first = found > 0 ? idx_row[0] : 0;
  for (int s = found; s < nsample; ++s) idx_row[s] = first;
  return found;
}

int query_and_group(const float* xyz, const int32_t* xyz_cnt, const float* new_xyz, const int32_t* new_cnt, const float* features,
                    int32_t B, int64_t N, int64_t M, int32_t C, float radius, int32_t nsample, int32_t use_xyz, float* out,
                    int32_t* idx, int32_t* cnt, uint8_t* mask, int32_t nthreads) {
  if (B < 0 || N < 0 || M < 0 || C < 0 || nsample <= 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE) return GD3D_E_TOOLARGE;
  if (M == 0) return 0;
  if (new_xyz == nullptr || idx == nullptr || (B > 0 && (xyz_cnt == nullptr || new_cnt == nullptr))) return GD3D_E_BADARG;
  if (N > 0 && xyz == nullptr) return GD3D_E_BADARG;
  if (C > 0 && features == nullptr && N > 0) return GD3D_E_BADARG;
  const bool group = out != nullptr;
  if (group && !use_xyz && C == 0) return GD3D_E_BADARG;
  if ((long long)((use_xyz ? 3 : 0) + C) * nsample > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  const float radius2 = radius * radius;
  const int c_xyz = (group && use_xyz) ? 3 : 0;
  const int ct = c_xyz + (group ? C : 0);
  const int team = gd3d_host::team_size(nthreads, M, 64, 256);
  const bool ok = parallel_ranges(M, team, [&](int64_t m0, int64_t m1) {
    for (int64_t m = m0; m < m1; ++m) {
      long long p0 = 0;
      int np = 0;
      if (!row_segment(xyz_cnt, new_cnt, B, N, M, m, p0, np)) np = 0;   // rows the counts do not cover: empty balls
      int32_t* row = idx + m * nsample;
      const float* c = new_xyz + m * 3;
      const int found = scan_ball(xyz, p0, np, c, radius2, nsample, row);
      if (cnt != nullptr) cnt[m] = found;
      if (mask != nullptr) mask[m] = found == 0 ? 1 : 0;
      if (!group) continue;
      float* o = out + m * ct * nsample;
      if (found == 0) {
        for (long long e = 0; e < (long long)ct * nsample; ++e) o[e] = 0.0f;
        continue;
      }
      for (int k = 0; k < c_xyz; ++k)
        for (int s = 0; s < nsample; ++s) o[k * nsample + s] = xyz[(p0 + row[s]) * 3 + k] - c[k];
      for (int ch = 0; ch < C; ++ch)
        for (int s = 0; s < nsample; ++s) o[(long long)(c_xyz + ch) * nsample + s] = features[(p0 + row[s]) * C + ch];
    }
  });
  return ok ? 0 : GD3D_E_HOST;
}

int group_backward(const float* grad_out, const int32_t* idx, const int32_t* cnt, const int32_t* idx_cnt, const int32_t* feat_cnt,
                   int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample, int32_t ct, int32_t c_off, float* grad_features) {
  if (B < 0 || N < 0 || M < 0 || C < 0 || nsample <= 0 || c_off < 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE) return GD3D_E_TOOLARGE;
  if (N == 0 || C == 0) return 0;
  if (grad_features == nullptr) return GD3D_E_BADARG;
  for (long long i = 0; i < (long long)N * C; ++i) grad_features[i] = 0.0f;
  if (M == 0 || B == 0) return 0;
  if (grad_out == nullptr || idx == nullptr || idx_cnt == nullptr || feat_cnt == nullptr) return GD3D_E_BADARG;
  for (int64_t m = 0; m < M; ++m) {
    long long p0 = 0;
    int np = 0;
    if (!row_segment(feat_cnt, idx_cnt, B, N, M, m, p0, np) || np <= 0) continue;
    if (cnt != nullptr && cnt[m] <= 0) continue;   // empty ball: no gradient
    const float* g = grad_out + (m * ct + c_off) * nsample;
    for (int s = 0; s < nsample; ++s) {   // the padded slots name the first member: the same destination either way
      float* row = grad_features + (p0 + clamp_index(idx[m * nsample + s], np)) * C;
      for (int ch = 0; ch < C; ++ch) row[ch] += g[(long long)ch * nsample + s];
    }
  }
  return 0;
}

// one sample: n points at P, picks into out[0 .. npoint) (n picks, then cyclic)
template <typename OutT>
void fps_sample(const float* P, int n, int npoint, OutT* out, std::vector<float>& t) {
  if (n <= 0) {
    for (int j = 0; j < npoint; ++j) out[j] = (OutT)0;
    return;
  }
  t.assign((size_t)n, FPS_FAR);
  const int picks = npoint < n ? npoint : n;
  int old = 0;
  if (npoint > 0) out[0] = (OutT)0;
  for (int p = 1; p < picks; ++p) {
    const float px = P[3 * old], py = P[3 * old + 1], pz = P[3 * old + 2];
    float best = -1.0f;
    int bi = 0;
    for (int k = 0; k < n; ++k) {   // ascending index and strict >: of equal distances the lowest index wins
      const float d = dist2(px, py, pz, P[3 * k], P[3 * k + 1], P[3 * k + 2]);
      const float tt = d < t[k] ? d : t[k];
      t[k] = tt;
      if (tt > best) {
        best = tt;
        bi = k;
      }
    }
    old = bi;
    out[p] = (OutT)bi;
  }
  for (int j = picks; j < npoint; ++j) out[j] = out[j - n];   // picks == n here
}

}  // namespace

extern "C" {

int gd3d_vsa_ball_query_cpu(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz, const int32_t* new_xyz_batch_cnt,
                            int32_t B, int64_t N, int64_t M, float radius, int32_t nsample, int32_t* idx, int32_t* cnt,
                            uint8_t* empty_mask, int32_t nthreads) {
  return query_and_group(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, nullptr, B, N, M, 0, radius, nsample, 0, nullptr, idx, cnt,
                         empty_mask, nthreads);
}

int gd3d_vsa_query_and_group_cpu(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                                 const int32_t* new_xyz_batch_cnt, const float* features, int32_t B, int64_t N, int64_t M,
                                 int32_t C, float radius, int32_t nsample, int32_t use_xyz, float* out, int32_t* idx, int32_t* cnt,
                                 uint8_t* empty_mask, int32_t nthreads) {
  return query_and_group(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, B, N, M, C, radius, nsample, use_xyz, out, idx,
                         cnt, empty_mask, nthreads);
}

int gd3d_vsa_group_cpu(const float* features, const int32_t* features_batch_cnt, const int32_t* idx, const int32_t* idx_batch_cnt,
                       int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample, float* out, int32_t nthreads) {
  if (B < 0 || N < 0 || M < 0 || C <= 0 || nsample <= 0) return GD3D_E_BADARG;
  if (nsample > MAX_NSAMPLE || (long long)C * nsample > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (M == 0) return 0;
  if (idx == nullptr || out == nullptr || (B > 0 && (features_batch_cnt == nullptr || idx_batch_cnt == nullptr))) return GD3D_E_BADARG;
  if (N > 0 && features == nullptr) return GD3D_E_BADARG;
  const int team = gd3d_host::team_size(nthreads, M, 256, 1024);
  const bool ok = parallel_ranges(M, team, [&](int64_t m0, int64_t m1) {
    for (int64_t m = m0; m < m1; ++m) {
      long long p0 = 0;
      int np = 0;
      if (!row_segment(features_batch_cnt, idx_batch_cnt, B, N, M, m, p0, np)) np = 0;
      float* o = out + m * C * nsample;
      for (int ch = 0; ch < C; ++ch)
        for (int s = 0; s < nsample; ++s)
          o[(long long)ch * nsample + s] = np > 0 ? features[(p0 + clamp_index(idx[m * nsample + s], np)) * C + ch] : 0.0f;
    }
  });
  return ok ? 0 : GD3D_E_HOST;
}

int gd3d_vsa_group_backward_cpu(const float* grad_out, const int32_t* idx, const int32_t* idx_batch_cnt,
                                const int32_t* features_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample,
                                float* grad_features) {
  return group_backward(grad_out, idx, nullptr, idx_batch_cnt, features_batch_cnt, B, N, M, C, nsample, C, 0, grad_features);
}

int gd3d_vsa_query_and_group_backward_cpu(const float* grad_out, const int32_t* idx, const int32_t* cnt,
                                          const int32_t* new_xyz_batch_cnt, const int32_t* xyz_batch_cnt, int32_t B, int64_t N,
                                          int64_t M, int32_t C, int32_t nsample, int32_t c_off, float* grad_features) {
  if (cnt == nullptr && M > 0 && N > 0 && C > 0) return GD3D_E_BADARG;
  return group_backward(grad_out, idx, cnt, new_xyz_batch_cnt, xyz_batch_cnt, B, N, M, C, nsample, c_off + C, c_off, grad_features);
}

int gd3d_vsa_fps_cpu(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* out, int32_t nthreads) {
  if (B < 0 || n < 0 || npoint < 0) return GD3D_E_BADARG;
  if (B == 0 || npoint == 0) return 0;
  if (out == nullptr || (n > 0 && xyz == nullptr)) return GD3D_E_BADARG;
  const bool ok = parallel_ranges(B, gd3d_host::team_size(nthreads, B, 1, 2), [&](int64_t b0, int64_t b1) {
    std::vector<float> t;
    for (int64_t b = b0; b < b1; ++b) fps_sample(xyz + b * n * 3, n, npoint, out + b * npoint, t);
  });
  return ok ? 0 : GD3D_E_HOST;
}

int gd3d_vsa_fps_stacked_cpu(const float* xyz, const int32_t* xyz_batch_cnt, int32_t B, int64_t N, int32_t npoint, int64_t* out,
                             int32_t nthreads) {
  if (B < 0 || N < 0 || npoint < 0) return GD3D_E_BADARG;
  if (B == 0 || npoint == 0) return 0;
  if (out == nullptr || xyz_batch_cnt == nullptr || (N > 0 && xyz == nullptr)) return GD3D_E_BADARG;
  std::vector<long long> start((size_t)B);
  std::vector<int> count((size_t)B);
  long long p0 = 0;
  for (int b = 0; b < B; ++b) {
    start[b] = p0;
    count[b] = (int)clamp_count(xyz_batch_cnt[b], N - p0);
    p0 += count[b];
  }
  const bool ok = parallel_ranges(B, gd3d_host::team_size(nthreads, B, 1, 2), [&](int64_t b0, int64_t b1) {
    std::vector<float> t;
    for (int64_t b = b0; b < b1; ++b) fps_sample(xyz + start[b] * 3, count[b], npoint, out + b * npoint, t);
  });
  return ok ? 0 : GD3D_E_HOST;
}

}  // extern "C"
