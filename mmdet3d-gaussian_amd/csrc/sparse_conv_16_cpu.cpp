// sparse_conv_16_cpu.cpp — the `_cpu` twins of csrc/sparse_conv_16.hip (include/gd3d.h, gd3d_sparse_conv_*_16): the
// 16-bit operands widened to fp32 (exact), the fp32 twins of csrc/sparse_conv_cpu.cpp on them, and ONE rounding to nearest even of
// every 16-bit output.  Another summation order than the device's matrix cores: the values agree to the tests' bound, not to the bit.
// fp16 goes through _Float16 (F16C at x86-64-v3); bf16 is the upper half of an fp32, rounded by explicit bit operations.
#include <cstring>
#include <new>
#include <vector>

#include "sparse_conv_common.h"

using namespace sparse_conv;

namespace {

using sparse_elem::BF16;
using sparse_elem::F16;

std::vector<float> widen(const void* p, int64_t n, int32_t dtype) {
  std::vector<float> out((size_t)(p == nullptr || n < 0 ? 0 : n));
  const uint16_t* s = (const uint16_t*)p;
  if (dtype == GD3D_DTYPE_F16)
    for (size_t i = 0; i < out.size(); ++i) out[i] = F16::widen(s[i]);
  else
    for (size_t i = 0; i < out.size(); ++i) out[i] = BF16::widen(s[i]);
  return out;
}

void narrow(const std::vector<float>& v, int32_t dtype, void* p) {
  uint16_t* d = (uint16_t*)p;
  if (dtype == GD3D_DTYPE_F16)
    for (size_t i = 0; i < v.size(); ++i) d[i] = F16::narrow(v[i]);
  else
    for (size_t i = 0; i < v.size(); ++i) d[i] = BF16::narrow(v[i]);
}

}  // namespace

extern "C" {

int gd3d_sparse_conv_forward_16_cpu(const void* features, const void* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                    int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* out) {
  bool run;
  const int rc = check_gemm_call(2, dtype, R, N, K, Cin, Cout, true, features, weight, nbr, nullptr, out, &run);
  if (rc != 0 || !run) return rc;
  try {
    const std::vector<float> x = widen(features, N * Cin, dtype), w = widen(weight, (int64_t)K * Cin * Cout, dtype);
    std::vector<float> o((size_t)(R * Cout));
    const int e = gd3d_sparse_conv_forward_cpu(N > 0 ? x.data() : nullptr, w.data(), bias, nbr, num, N, R, K, Cin, Cout, o.data());
    if (e != 0) return e;
    narrow(o, dtype, out);
    return 0;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_conv_forward_fused_16_cpu(const void* features, const void* weight, const float* scale, const float* shift,
                                          const void* residual, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                          int32_t Cin, int32_t Cout, int32_t act, int32_t dtype, void* out) {
  bool run;
  const int rc = check_gemm_call(2, dtype, R, N, K, Cin, Cout, act_ok(act), features, weight, nbr, residual, out, &run);
  if (rc != 0 || !run) return rc;
  try {
    const std::vector<float> x = widen(features, N * Cin, dtype), w = widen(weight, (int64_t)K * Cin * Cout, dtype);
    const std::vector<float> res = widen(residual, R * Cout, dtype);
    std::vector<float> o((size_t)(R * Cout));                    // the fp32 twin's sequence on the widened operands, then the one rounding
    const int e = gd3d_sparse_conv_forward_fused_cpu(N > 0 ? x.data() : nullptr, w.data(), scale, shift, residual != nullptr ? res.data() : nullptr,
                                                     nbr, num, N, R, K, Cin, Cout, act, o.data());
    if (e != 0) return e;
    narrow(o, dtype, out);
    return 0;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_conv_backward_input_16_cpu(const void* grad_out, const void* weight, const int32_t* table, int32_t flip, int64_t N,
                                           int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* grad_features) {
  bool run;
  const int rc = check_gemm_call(2, dtype, N, R, K, Cin, Cout, !flip || N == R, grad_out, weight, table, nullptr, grad_features, &run);
  if (rc != 0 || !run) return rc;
  try {
    const std::vector<float> gy = widen(grad_out, R * Cout, dtype), w = widen(weight, (int64_t)K * Cin * Cout, dtype);
    std::vector<float> gx((size_t)(N * Cin));
    const int e = gd3d_sparse_conv_backward_input_cpu(R > 0 ? gy.data() : nullptr, w.data(), table, flip, N, R, K, Cin, Cout, gx.data());
    if (e != 0) return e;
    narrow(gx, dtype, grad_features);
    return 0;
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_conv_backward_weight_16_cpu(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num,
                                            int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                            float* grad_weight, float* grad_bias) {
  // not check_wgrad_call: this twin refuses an odd pointer BEFORE it looks for an empty call, and the shared order would change that code
  const int rc = check_channels(K, Cin, Cout);
  if (rc != 0) return rc;
  if (!elem_ok(2, dtype) || N < 0 || R < 0 || grad_weight == nullptr) return GD3D_E_BADARG;
  if (N > 0x7fffffffLL || R > 0x7fffffffLL || R * K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (misaligned(features, 2) || misaligned(grad_out, 2)) return GD3D_E_BADARG;
  try {
    const bool empty = R == 0 || N == 0;
    const std::vector<float> x = widen(features, empty ? 0 : N * Cin, dtype), gy = widen(grad_out, empty ? 0 : R * Cout, dtype);
    return gd3d_sparse_conv_backward_weight_cpu(empty || features == nullptr ? nullptr : x.data(), empty || grad_out == nullptr ? nullptr : gy.data(),
                                                nbr, num, N, R, K, Cin, Cout, workspace, grad_weight, grad_bias);
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_to_dense_16_cpu(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                int32_t W, void* dense) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (dense == nullptr || misaligned(dense, 2)) return GD3D_E_BADARG;
  const long long plane = (long long)D * H * W;
  uint16_t* d = (uint16_t*)dense;
  std::memset(d, 0, sizeof(uint16_t) * (size_t)g.in_sent * (size_t)C);
  if (N == 0) return 0;
  if (features == nullptr || coors == nullptr || misaligned(features, 2)) return GD3D_E_BADARG;
  const uint16_t* f = (const uint16_t*)features;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    if (!row_active(c, g)) continue;
    const long long cell = ((long long)c[1] * H + c[2]) * W + c[3];
    for (int ch = 0; ch < C; ++ch) d[((long long)c[0] * C + ch) * plane + cell] = f[i * C + ch];
  }
  return 0;
}

int gd3d_sparse_to_dense_backward_16_cpu(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D,
                                         int32_t H, int32_t W, void* grad_features) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || grad_features == nullptr || (B > 0 && grad_dense == nullptr)) return GD3D_E_BADARG;
  if (misaligned(grad_dense, 2) || misaligned(grad_features, 2)) return GD3D_E_BADARG;
  const long long plane = (long long)D * H * W;
  const uint16_t* s = (const uint16_t*)grad_dense;
  uint16_t* gx = (uint16_t*)grad_features;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    const bool in = row_active(c, g);
    const long long cell = in ? ((long long)c[1] * H + c[2]) * W + c[3] : 0;
    for (int ch = 0; ch < C; ++ch) gx[i * C + ch] = in ? s[((long long)c[0] * C + ch) * plane + cell] : (uint16_t)0;
  }
  return 0;
}

}  // extern "C"
