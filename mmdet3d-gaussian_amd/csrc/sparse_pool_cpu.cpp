// sparse_pool_cpu.cpp — the `_cpu` twins of csrc/sparse_pool.hip (include/gd3d.h, gd3d_sparse_max_pool_*) on the thread
// team of csrc/host_threads.h.  The same walk per element: the maximum kept as the element it was read as, a candidate winning when it
// is greater or a NaN; the gradient summed in ascending offset order in fp32 and rounded to nearest even once.  The same bits as the device.
#include "host_threads.h"
#include "sparse_pool_common.h"

using namespace sparse_pool;
using namespace sparse_elem;

namespace {

int team_for(int64_t units, int64_t min_per_thread) {
  const int t = gd3d_host::team_size(0, units, min_per_thread, 2 * min_per_thread);
  return t < 16 ? t : 16;
}

template <typename E>
bool pool(const void* features, const int32_t* nbr, long long limit, int64_t N, int64_t R, int32_t K, int32_t C, void* out) {
  typedef typename E::T T;
  const T* x = (const T*)features;
  T* y = (T*)out;
  return gd3d_host::parallel_ranges(R, team_for(R, 1024), [&](int64_t r0, int64_t r1) {
    for (int64_t row = r0; row < r1; ++row)
      for (int c = 0; c < C; ++c) {
        T best = (T)0;
        float top = 0.0f;
        bool any = false;
        if (row < limit)
          for (int j = 0; j < K; ++j) {
            const int32_t i = nbr[row * K + j];
            if (i < 0 || i >= N) continue;
            const T cur = x[(int64_t)i * C + c];
            const float v = E::widen(cur);
            if (!any || v > top || v != v) { best = cur; top = v; }
            any = true;
          }
        y[row * C + c] = best;
      }
  });
}

template <typename E>
bool unpool(const void* grad_out, const void* features, const void* out, const int32_t* nbr_t, int64_t N, int64_t R, int32_t K, int32_t C,
            void* grad_features) {
  typedef typename E::T T;
  const T *x = (const T*)features, *y = (const T*)out, *gy = (const T*)grad_out;
  T* gx = (T*)grad_features;
  return gd3d_host::parallel_ranges(N, team_for(N, 1024), [&](int64_t r0, int64_t r1) {
    for (int64_t row = r0; row < r1; ++row)
      for (int c = 0; c < C; ++c) {
        float acc = 0.0f;
        for (int j = 0; j < K; ++j) {
          const int32_t o = nbr_t[row * K + j];
          if (o < 0 || o >= R) continue;
          if (E::widen(x[row * C + c]) == E::widen(y[(int64_t)o * C + c])) acc = acc + E::widen(gy[(int64_t)o * C + c]);
        }
        gx[row * C + c] = E::narrow(acc);
      }
  });
}

}  // namespace

extern "C" {

int gd3d_sparse_max_pool_forward_cpu(const void* features, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                     int32_t C, int32_t dtype, void* out) {
  const int rc = check_dims(N, R, K, C, dtype);
  if (rc != 0) return rc;
  if (R == 0) return 0;
  if (nbr == nullptr || out == nullptr || (N > 0 && features == nullptr)) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(features, es) || misaligned(out, es) || misaligned(nbr, 4) || misaligned(num, 8)) return GD3D_E_BADARG;
  const long long limit = row_limit((const long long*)num, R);
  return with_elem(dtype, [&](auto e) { return pool<decltype(e)>(features, nbr, limit, N, R, K, C, out); }) ? 0 : GD3D_E_HOST;
}

int gd3d_sparse_max_pool_backward_cpu(const void* grad_out, const void* features, const void* out, const int32_t* nbr_t, int64_t N,
                                      int64_t R, int32_t K, int32_t C, int32_t dtype, void* grad_features) {
  const int rc = check_dims(N, R, K, C, dtype);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (nbr_t == nullptr || grad_features == nullptr || features == nullptr || (R > 0 && (grad_out == nullptr || out == nullptr))) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(grad_out, es) || misaligned(features, es) || misaligned(out, es) || misaligned(grad_features, es) || misaligned(nbr_t, 4))
    return GD3D_E_BADARG;
  return with_elem(dtype, [&](auto e) { return unpool<decltype(e)>(grad_out, features, out, nbr_t, N, R, K, C, grad_features); }) ? 0 : GD3D_E_HOST;
}

}  // extern "C"
