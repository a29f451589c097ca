// sparse_bn_cpu.cpp — the `_cpu` twins of csrc/sparse_bn.hip (include/gd3d.h, gd3d_sparse_bn_*) on the thread team
// of csrc/host_threads.h.  The same definition and the same fp32 sequence per element (fmaf included; 16-bit operands widened, one
// rounding to nearest even); the sums are taken per tile of csrc/sparse_bn_common.h's cut in fp64 — two passes, the mean and then the
// centred squares — and rounded to fp32 once: another order than the device's, the values agree to the tests' bound, not to the bit.
#include <cmath>
#include <new>
#include <vector>

#include "host_threads.h"
#include "sparse_bn_common.h"

using namespace sparse_bn;
using namespace sparse_elem;

namespace {

inline float get(const void* p, int64_t i, int32_t dtype) {
  return with_elem(dtype, [&](auto e) { return decltype(e)::widen(((const typename decltype(e)::T*)p)[i]); });
}

inline void put(void* p, int64_t i, int32_t dtype, float v) {
  with_elem(dtype, [&](auto e) { ((typename decltype(e)::T*)p)[i] = decltype(e)::narrow(v); });
}

struct Dims {
  int64_t R;
  int32_t C, B, D, H, W;
};

inline bool live_row(const int32_t* coors, int64_t row, const Dims& d) {
  const int32_t* c = coors + 4 * row;
  return c[0] >= 0 && c[0] < d.B && c[1] >= 0 && c[1] < d.D && c[2] >= 0 && c[2] < d.H && c[3] >= 0 && c[3] < d.W;
}

int team_for(int64_t units, int64_t min_per_thread) {
  const int t = gd3d_host::team_size(0, units, min_per_thread, 2 * min_per_thread);
  return t < 16 ? t : 16;
}

// per channel, over the live rows: out[c] = sum term(row, c) in fp64, a partial per tile, the tiles added in ascending order;
// returns the live rows (-1: a worker failed)
template <typename F>
int64_t live_sums(const int32_t* coors, const Dims& d, std::vector<double>* out, F&& term) {
  int64_t tiles, chunk;
  cut_rows(d.R, &tiles, &chunk);
  std::vector<double> part((size_t)tiles * (size_t)d.C, 0.0);
  std::vector<int64_t> cnt((size_t)tiles, 0);
  const bool ok = gd3d_host::parallel_ranges(tiles, team_for(tiles, 4), [&](int64_t t0, int64_t t1) {
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t r1 = (t + 1) * chunk < d.R ? (t + 1) * chunk : d.R;
      for (int64_t row = t * chunk; row < r1; ++row) {
        if (!live_row(coors, row, d)) continue;
        ++cnt[(size_t)t];
        for (int c = 0; c < d.C; ++c) part[(size_t)t * d.C + c] += term(row, c);
      }
    }
  });
  if (!ok) return -1;
  out->assign((size_t)d.C, 0.0);
  int64_t n = 0;
  for (int64_t t = 0; t < tiles; ++t) {
    n += cnt[(size_t)t];
    for (int c = 0; c < d.C; ++c) (*out)[(size_t)c] += part[(size_t)t * d.C + c];
  }
  return n;
}

// y = fmaf(x - sub, mul, add); xhat = (x - sub) * istd: csrc/sparse_bn.hip's channel_constants
struct Constants {
  std::vector<float> sub, mul, add, istd;
};

Constants constants_of(int32_t C, int32_t training, float eps, const float* gamma, const float* beta, const float* mean, const float* istd) {
  Constants k;
  k.sub.resize((size_t)C); k.mul.resize((size_t)C); k.add.resize((size_t)C); k.istd.resize((size_t)C);
  for (int c = 0; c < C; ++c) {
    const float g = gamma != nullptr ? gamma[c] : 1.0f, b = beta != nullptr ? beta[c] : 0.0f;
    if (training) {
      k.istd[c] = istd[c];
      k.sub[c] = mean[c];
      k.mul[c] = istd[c] * g;
      k.add[c] = b;
    } else {
      const float root = std::sqrt(istd[c] + eps);
      k.istd[c] = 1.0f / root;
      k.sub[c] = 0.0f;
      k.mul[c] = g / root;
      k.add[c] = std::fmaf(-mean[c], k.mul[c], b);
    }
  }
  return k;
}

}  // namespace

extern "C" {

int gd3d_sparse_bn_forward_cpu(const void* features, const int32_t* coors, const void* residual, const float* weight, const float* bias,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t R, int32_t C, int32_t B,
                               int32_t D, int32_t H, int32_t W, int32_t training, float momentum, float eps, int32_t act, int32_t dtype,
                               void* workspace, void* out, float* save_mean, float* save_invstd) {
  (void)workspace;
  const int rc = check_dims(R, C, B, D, H, W, act, dtype);
  if (rc != 0) return rc;
  if (training ? (save_mean == nullptr || save_invstd == nullptr) : (running_mean == nullptr || running_var == nullptr)) return GD3D_E_BADARG;
  if (R > 0 && (features == nullptr || coors == nullptr || out == nullptr)) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(features, es) || misaligned(residual, es) || misaligned(out, es) || misaligned(coors, 4)) return GD3D_E_BADARG;
  if (R > 0 && residual != nullptr && sparse_conv::ranges_overlap(residual, out, es * (size_t)R * (size_t)C)) return GD3D_E_BADARG;
  const Dims d = {R, C, B, D, H, W};
  try {
    if (training) {
      std::vector<double> sum, m2;
      const int64_t n = live_sums(coors, d, &sum, [&](int64_t row, int c) { return (double)get(features, row * C + c, dtype); });
      if (n < 0) return GD3D_E_HOST;
      std::vector<double> mean((size_t)C, 0.0);
      for (int c = 0; c < C; ++c) mean[(size_t)c] = n > 0 ? sum[(size_t)c] / (double)n : 0.0;
      if (live_sums(coors, d, &m2, [&](int64_t row, int c) {
            const double v = (double)get(features, row * C + c, dtype) - mean[(size_t)c];
            return v * v;
          }) < 0)
        return GD3D_E_HOST;
      for (int c = 0; c < C; ++c) {
        const float var = n > 0 ? (float)(m2[(size_t)c] / (double)n) : 0.0f;
        save_mean[c] = (float)mean[(size_t)c];
        save_invstd[c] = 1.0f / std::sqrt(var + eps);
        if (n >= 2) {
          const float fn = (float)n;
          if (running_mean != nullptr) running_mean[c] = std::fmaf(momentum, save_mean[c], (1.0f - momentum) * running_mean[c]);
          if (running_var != nullptr) running_var[c] = std::fmaf(momentum, var * (fn / (fn - 1.0f)), (1.0f - momentum) * running_var[c]);
        }
      }
      if (n >= 2 && num_batches_tracked != nullptr) *num_batches_tracked += 1;
    }
    if (R == 0) return 0;
    const Constants k = constants_of(C, training, eps, weight, bias, training ? save_mean : running_mean, training ? save_invstd : running_var);
    const bool relu = act == GD3D_ACT_RELU;
    const bool ok = gd3d_host::parallel_ranges(R, team_for(R, 2048), [&](int64_t r0, int64_t r1) {
      for (int64_t row = r0; row < r1; ++row) {
        const bool live = live_row(coors, row, d);
        for (int c = 0; c < C; ++c) {
          float t = 0.0f;
          if (live) {
            t = std::fmaf(get(features, row * C + c, dtype) - k.sub[c], k.mul[c], k.add[c]);
            if (residual != nullptr) t = t + get(residual, row * C + c, dtype);
            t = relu && t < 0.0f ? 0.0f : t;
          }
          put(out, row * C + c, dtype, t);
        }
      }
    });
    return ok ? 0 : GD3D_E_HOST;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_bn_backward_cpu(const void* grad_out, const void* features, const void* out, const int32_t* coors, const float* weight,
                                const float* mean, const float* invstd_or_var, int64_t R, int32_t C, int32_t B, int32_t D, int32_t H,
                                int32_t W, int32_t training, float eps, int32_t act, int32_t dtype, void* workspace, void* grad_features,
                                void* grad_residual, float* grad_weight, float* grad_bias) {
  (void)workspace;
  const int rc = check_dims(R, C, B, D, H, W, act, dtype);
  if (rc != 0) return rc;
  if (mean == nullptr || invstd_or_var == nullptr) return GD3D_E_BADARG;
  const bool relu = act == GD3D_ACT_RELU;
  if (R > 0 && (grad_out == nullptr || features == nullptr || coors == nullptr || grad_features == nullptr || (relu && out == nullptr)))
    return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(grad_out, es) || misaligned(features, es) || misaligned(out, es) || misaligned(grad_features, es) || misaligned(grad_residual, es) ||
      misaligned(coors, 4))
    return GD3D_E_BADARG;
  const Dims d = {R, C, B, D, H, W};
  try {
    Constants k = constants_of(C, training, eps, weight, nullptr, mean, invstd_or_var);
    if (!training)
      for (int c = 0; c < C; ++c) k.sub[c] = mean[c];                   // xhat of a frozen BatchNorm: (x - running_mean) * invstd
    auto g_at = [&](int64_t row, int c) {
      const float g = get(grad_out, row * C + c, dtype);
      return relu && !(get(out, row * C + c, dtype) > 0.0f) ? 0.0f : g;
    };
    auto xhat_at = [&](int64_t row, int c) { return (get(features, row * C + c, dtype) - k.sub[c]) * k.istd[c]; };
    std::vector<float> mg((size_t)C, 0.0f), mgx((size_t)C, 0.0f);
    if (training || grad_weight != nullptr || grad_bias != nullptr) {
      std::vector<double> sg, sgx;
      const int64_t n = live_sums(coors, d, &sg, [&](int64_t row, int c) { return (double)g_at(row, c); });
      if (n < 0 || live_sums(coors, d, &sgx, [&](int64_t row, int c) { return (double)g_at(row, c) * (double)xhat_at(row, c); }) < 0)
        return GD3D_E_HOST;
      for (int c = 0; c < C; ++c) {
        if (grad_bias != nullptr) grad_bias[c] = (float)sg[(size_t)c];
        if (grad_weight != nullptr) grad_weight[c] = (float)sgx[(size_t)c];
        mg[(size_t)c] = n > 0 ? (float)sg[(size_t)c] / (float)n : 0.0f;
        mgx[(size_t)c] = n > 0 ? (float)sgx[(size_t)c] / (float)n : 0.0f;
      }
    }
    if (R == 0) return 0;
    const bool ok = gd3d_host::parallel_ranges(R, team_for(R, 2048), [&](int64_t r0, int64_t r1) {
      for (int64_t row = r0; row < r1; ++row) {
        const bool live = live_row(coors, row, d);
        for (int c = 0; c < C; ++c) {
          float g = 0.0f, o = 0.0f;
          if (live) {
            g = g_at(row, c);
            o = training ? k.mul[c] * std::fmaf(-xhat_at(row, c), mgx[(size_t)c], g - mg[(size_t)c]) : g * k.mul[c];
          }
          put(grad_features, row * C + c, dtype, o);
          if (grad_residual != nullptr) put(grad_residual, row * C + c, dtype, g);
        }
      }
    });
    return ok ? 0 : GD3D_E_HOST;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

}  // extern "C"
