// sparse_conv_cpu.cpp — the `_cpu` twins of csrc/sparse_conv.hip (include/gd3d.h, gd3d_sparse_conv_*): the same
// contracts on HOST memory on the calling thread.  The index build is the kernels' own sequence — keys, a stable sort, look-ups by lower
// bound through csrc/sparse_conv_common.h — so every table is bit-identical to the device's; the values are plain gather / multiply-add
// loops in offset-then-channel order (the device's tiles fix another order: values agree to rounding, not to the bit).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "sparse_conv_common.h"

using namespace sparse_conv;

namespace {

bool row_live(const int32_t* nb, int K, int64_t n_src) {
  for (int j = 0; j < K; ++j)
    if (nb[j] >= 0 && nb[j] < n_src) return true;
  return false;
}

int index_build(const int32_t* coors, int64_t N, const Geo& g, int64_t max_out, int32_t* out_coors, int32_t* nbr, int32_t* nbr_t,
                int64_t* num, int32_t* out_batch_cnt) {
  const int K = g.K;
  std::vector<long long> key(N), skey(N);
  std::vector<int32_t> srow(N);
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    key[i] = row_active(c, g) ? in_key(g, c[0], c[1], c[2], c[3]) : g.in_sent;
    srow[i] = (int32_t)i;
  }
  std::stable_sort(srow.begin(), srow.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
  for (int64_t i = 0; i < N; ++i) skey[i] = key[srow[i]];
  const long long cells = g.B > 0 ? g.in_sent / g.B : 0, ocells = g.B > 0 ? g.out_sent / g.B : 0;
  if (g.subm) {
    for (int64_t o = 0; o < N; ++o) {
      const int32_t* c = coors + o * 4;
      std::memcpy(out_coors + o * 4, c, 4 * sizeof(int32_t));
      const bool act = row_active(c, g);
      const int oc[3] = {c[1], c[2], c[3]};
      for (int j = 0; j < K; ++j) {
        int off[3], in[3];
        int32_t v = -1;
        split_offset(g, j, off);
        if (act && input_of(g, oc, off, in)) v = find_row(skey.data(), srow.data(), N, in_key(g, c[0], in[0], in[1], in[2]));
        nbr[o * K + j] = v;
      }
    }
    num[0] = num[1] = N;
    for (int b = 0; b < g.B; ++b)
      out_batch_cnt[b] = (int32_t)(lower_bound(skey.data(), N, (long long)(b + 1) * cells) - lower_bound(skey.data(), N, (long long)b * cells));
    return 0;
  }
  std::vector<long long> ukey;
  ukey.reserve((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    if (!row_active(c, g)) continue;
    const int in[3] = {c[1], c[2], c[3]};
    for (int j = 0; j < K; ++j) {
      int off[3], o[3];
      split_offset(g, j, off);
      if (output_of(g, in, off, o)) ukey.push_back(out_key(g, c[0], o[0], o[1], o[2]));
    }
  }
  std::sort(ukey.begin(), ukey.end());
  ukey.erase(std::unique(ukey.begin(), ukey.end()), ukey.end());
  const long long total = (long long)ukey.size(), kept = total < max_out ? total : max_out;
  num[0] = kept; num[1] = total;
  for (int b = 0; b < g.B; ++b)
    out_batch_cnt[b] = (int32_t)(lower_bound(ukey.data(), kept, (long long)(b + 1) * ocells) - lower_bound(ukey.data(), kept, (long long)b * ocells));
  for (int64_t r = 0; r < max_out; ++r) {
    int32_t c[4] = {-1, -1, -1, -1};
    if (r < kept) decode_out(g, ukey[r], c);
    std::memcpy(out_coors + r * 4, c, 4 * sizeof(int32_t));
    const int oc[3] = {c[1], c[2], c[3]};
    for (int j = 0; j < K; ++j) {
      int off[3], in[3];
      int32_t v = -1;
      split_offset(g, j, off);
      if (r < kept && input_of(g, oc, off, in)) v = find_row(skey.data(), srow.data(), N, in_key(g, c[0], in[0], in[1], in[2]));
      nbr[r * K + j] = v;
    }
  }
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    const bool mine = row_active(c, g) && find_row(skey.data(), srow.data(), N, in_key(g, c[0], c[1], c[2], c[3])) == (int32_t)i;
    const int in[3] = {c[1], c[2], c[3]};
    for (int j = 0; j < K; ++j) {
      int off[3], o[3];
      int32_t v = -1;
      split_offset(g, j, off);
      if (mine && output_of(g, in, off, o)) {
        const long long k = out_key(g, c[0], o[0], o[1], o[2]);
        const long long at = lower_bound(ukey.data(), kept, k);
        if (at < kept && ukey[at] == k) v = (int32_t)at;
      }
      nbr_t[i * K + j] = v;
    }
  }
  return 0;
}

// out (rows, Co) = sum over offsets of src[table] . W[j] (TRANS: . W[j]^T)
void gemm(const float* src, const float* W, const float* bias, const int32_t* table, long long limit, int64_t n_src, int64_t rows, int K,
          int Cr, int Co, bool trans, bool flip, float* out) {
  for (int64_t r = 0; r < rows; ++r) {
    float* o = out + r * Co;
    for (int c = 0; c < Co; ++c) o[c] = 0.0f;
    if (r >= limit) continue;
    bool live = false;
    for (int j = 0; j < K; ++j) {
      const int32_t v = table[r * K + (flip ? K - 1 - j : j)];
      if (v < 0 || v >= n_src) continue;
      live = true;
      const float* x = src + (int64_t)v * Cr;
      const float* Wj = W + (int64_t)j * Cr * Co;
      for (int k = 0; k < Cr; ++k)
        for (int c = 0; c < Co; ++c) o[c] = __builtin_fmaf(x[k], trans ? Wj[(int64_t)c * Cr + k] : Wj[(int64_t)k * Co + c], o[c]);
    }
    if (live && bias != nullptr)
      for (int c = 0; c < Co; ++c) o[c] += bias[c];
  }
}

}  // namespace

extern "C" {

int gd3d_sparse_conv_index_cpu(const int32_t* coors, int64_t N, int32_t B, const int32_t* spatial_shape, const int32_t* kernel_size,
                               const int32_t* stride, const int32_t* padding, int32_t subm, int64_t max_out, void* workspace,
                               int32_t* out_coors, int32_t* nbr, int32_t* nbr_t, int64_t* num, int32_t* out_batch_cnt) {
  (void)workspace;
  Geo g;
  const int rc = make_geo(N, B, spatial_shape, kernel_size, stride, padding, subm, &g);
  if (rc != 0) return rc;
  if (num == nullptr || (B > 0 && out_batch_cnt == nullptr) || max_out < 0) return GD3D_E_BADARG;
  const int64_t R = subm ? N : max_out;
  if (R > 0x7fffffffLL || R * g.K > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (R > 0 && (out_coors == nullptr || nbr == nullptr)) return GD3D_E_BADARG;
  if (N > 0 && (coors == nullptr || (!subm && nbr_t == nullptr))) return GD3D_E_BADARG;
  try {
    return index_build(coors, N, g, max_out, out_coors, nbr, nbr_t, num, out_batch_cnt);
  } catch (const std::bad_alloc&) {
    return GD3D_E_HOST;
  }
}

int gd3d_sparse_conv_forward_cpu(const float* features, const float* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                 int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* out) {
  bool run;
  const int rc = check_gemm_call(4, 0, R, N, K, Cin, Cout, true, features, weight, nbr, nullptr, out, &run);
  if (rc != 0 || !run) return rc;
  gemm(features, weight, bias, nbr, row_limit((const long long*)num, R), N, R, K, Cin, Cout, false, false, out);
  return 0;
}

int gd3d_sparse_conv_forward_fused_cpu(const float* features, const float* weight, const float* scale, const float* shift,
                                       const float* residual, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                       int32_t Cin, int32_t Cout, int32_t act, float* out) {
  bool run;
  const int rc = check_gemm_call(4, 0, R, N, K, Cin, Cout, act_ok(act), features, weight, nbr, residual, out, &run);
  if (rc != 0 || !run) return rc;
  const long long limit = row_limit((const long long*)num, R);
  gemm(features, weight, nullptr, nbr, limit, N, R, K, Cin, Cout, false, false, out);
  for (int64_t r = 0; r < limit; ++r) {                          // the rows past the limit and the rows without a neighbour stay zero
    if (!row_live(nbr + r * K, K, N)) continue;
    float* o = out + r * Cout;
    for (int c = 0; c < Cout; ++c) {
      const float sh = shift != nullptr ? shift[c] : 0.0f;
      float t = scale != nullptr ? __builtin_fmaf(o[c], scale[c], sh) : o[c] + sh;
      if (residual != nullptr) t = t + residual[r * Cout + c];
      if (act == GD3D_ACT_RELU) t = t < 0.0f ? 0.0f : t;
      o[c] = t;
    }
  }
  return 0;
}

int gd3d_sparse_conv_backward_input_cpu(const float* grad_out, const float* weight, const int32_t* table, int32_t flip, int64_t N,
                                        int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* grad_features) {
  bool run;
  const int rc = check_gemm_call(4, 0, N, R, K, Cin, Cout, !flip || N == R, grad_out, weight, table, nullptr, grad_features, &run);
  if (rc != 0 || !run) return rc;
  gemm(grad_out, weight, nullptr, table, N, R, N, K, Cout, Cin, true, flip != 0, grad_features);
  return 0;
}

int gd3d_sparse_conv_backward_weight_cpu(const float* features, const float* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                         int64_t R, int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight,
                                         float* grad_bias) {
  bool run;
  const int rc = check_wgrad_call(4, 0, N, R, K, Cin, Cout, features, grad_out, nbr, workspace, false, grad_weight, &run);
  if (rc != 0) return rc;
  const int64_t cc = (int64_t)Cin * Cout;
  for (int64_t i = 0; i < K * cc; ++i) grad_weight[i] = 0.0f;
  if (grad_bias != nullptr)
    for (int c = 0; c < Cout; ++c) grad_bias[c] = 0.0f;
  if (!run) return 0;                                            // no pair: the gradients are zeros
  const long long limit = row_limit((const long long*)num, R);
  for (int64_t r = 0; r < limit; ++r) {
    const float* gy = grad_out + r * Cout;
    if (grad_bias != nullptr && row_live(nbr + r * K, K, N))
      for (int c = 0; c < Cout; ++c) grad_bias[c] += gy[c];
    for (int j = 0; j < K; ++j) {
      const int32_t v = nbr[r * K + j];
      if (v < 0 || v >= N) continue;
      const float* x = features + (int64_t)v * Cin;
      float* gw = grad_weight + j * cc;
      for (int k = 0; k < Cin; ++k)
        for (int c = 0; c < Cout; ++c) gw[(int64_t)k * Cout + c] = __builtin_fmaf(x[k], gy[c], gw[(int64_t)k * Cout + c]);
    }
  }
  return 0;
}

int gd3d_sparse_to_dense_cpu(const float* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                             int32_t W, float* dense) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  if (dense == nullptr) return GD3D_E_BADARG;
  const long long plane = (long long)D * H * W;
  std::memset(dense, 0, sizeof(float) * (size_t)g.in_sent * (size_t)C);
  if (N == 0) return 0;
  if (features == nullptr || coors == nullptr) return GD3D_E_BADARG;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    if (!row_active(c, g)) continue;
    const long long cell = ((long long)c[1] * H + c[2]) * W + c[3];
    for (int ch = 0; ch < C; ++ch) dense[((long long)c[0] * C + ch) * plane + cell] = features[i * C + ch];
  }
  return 0;
}

int gd3d_sparse_to_dense_backward_cpu(const float* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D,
                                      int32_t H, int32_t W, float* grad_features) {
  Geo g;
  const int rc = dense_geo(N, C, B, D, H, W, &g);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  if (coors == nullptr || grad_features == nullptr || (B > 0 && grad_dense == nullptr)) return GD3D_E_BADARG;
  const long long plane = (long long)D * H * W;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t* c = coors + i * 4;
    const bool in = row_active(c, g);
    const long long cell = in ? ((long long)c[1] * H + c[2]) * W + c[3] : 0;
    for (int ch = 0; ch < C; ++ch) grad_features[i * C + ch] = in ? grad_dense[((long long)c[0] * C + ch) * plane + cell] : 0.0f;
  }
  return 0;
}

}  // extern "C"
