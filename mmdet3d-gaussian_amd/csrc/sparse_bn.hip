// sparse_bn.hip — batch normalisation over the LIVE rows of a sparse tensor, with a basic block's residual add and ReLU in the same
// pass, forward and backward, training and eval, fp32 / fp16 / bf16, for gfx950 (include/gd3d.h, gd3d_sparse_bn_*).
//
//   stats_kernel    a workgroup per row tile (csrc/sparse_bn_common.h, cut_rows): the tile's live-row count and, per channel, its mean
//                   m_t, then (a second sweep over the tile, which the first left in the cache) the centred sum r_t = sum(x - m_t) and
//                   M2_t = sum (x - m_t)^2.  Never E[x^2] - E[x]^2.  A lane owns a fixed channel group and every rows-th row; the
//                   lanes of a group are summed by a fixed tree in LDS.
//   finish_kernel   a wave per channel: the tiles' partials merged in ascending tile order (a lane takes every 64th tile, the lanes
//                   are folded by a fixed tree): n, the mean M = sum n_t m_t / n, then Chan's formula about M with the cross term kept,
//                   S = sum (M2_t + n_t d_t^2 + 2 d_t r_t), d_t = m_t - M, and the corrected two-pass step R = sum (n_t d_t + r_t),
//                   mean = M + R / n, M2 = S - R^2 / n.  It writes mean and invstd, and the running statistics and the batch counter
//                   when n >= 2.
//   norm_kernel     y = act((x - mean) * (invstd * gamma) + beta + residual) on live rows, 0 on dead rows (a select); in eval the
//                   same launch alone with scale and shift formed from the running statistics.
//   bstats_kernel / bfinish_kernel / bnorm_kernel: the backward in the same three stages: per-tile sum g and sum g * xhat, their merge
//                   (grad_bias, grad_weight), and grad_x, grad_residual.
// No atomics; the order of every sum depends on (R, C) and the element size alone: the same bits on every run and under graph replay,
// whatever the dead rows hold.  -ffp-contract=off: every fused multiply-add below is an explicit fmaf.
#include <hip/hip_runtime.h>

#include "sparse_bn_common.h"

using namespace sparse_bn;
using namespace sparse_elem;

namespace {

struct Args {
  const void *x, *res, *gy, *y;          // features, residual, grad_out, the saved output (the ReLU's mask)
  void *out, *gx, *gres;
  const int32_t* coors;
  const float *gamma, *beta, *mean, *istd;   // istd: invstd (training) or the running variance (eval)
  float *rmean, *rvar, *smean, *sistd, *ggamma, *gbeta;
  long long* nbt;
  float* ws;
  long long R, chunk;
  int C, B, D, H, W, tiles, groups, rows, half;   // half: the first step of the LDS tree over `rows` lanes
  int training, relu;
  float momentum, eps;
  unsigned wide;                          // bit per operand: its base is 16-byte aligned
};

enum { W_X = 1, W_RES = 2, W_OUT = 4, W_GY = 8, W_Y = 16, W_GX = 32, W_GRES = 64, W_COORS = 128 };

__device__ __forceinline__ bool live_row(const int32_t* coors, long long row, const Args& a) {
  int4 c;
  if (a.wide & W_COORS) c = *reinterpret_cast<const int4*>(coors + 4 * row);       // one 16-byte load
  else c = make_int4(coors[4 * row], coors[4 * row + 1], coors[4 * row + 2], coors[4 * row + 3]);
  return c.x >= 0 && c.x < a.B && c.y >= 0 && c.y < a.D && c.z >= 0 && c.z < a.H && c.w >= 0 && c.w < a.W;
}

// acc[v] summed over the lanes of one channel group (lanes tid, tid + groups, ...) by a fixed tree; every lane gets the group's total
template <int V>
__device__ __forceinline__ void fold(float (*red)[BLOCK], float* acc, int tid, int g, int rr, const Args& a) {
  __syncthreads();                                                      // the previous fold's totals have been read
#pragma unroll
  for (int v = 0; v < V; ++v) red[v][tid] = acc[v];
  __syncthreads();
  for (int s = a.half; s > 0; s >>= 1) {
    if (rr < s && rr + s < a.rows) {
#pragma unroll
      for (int v = 0; v < V; ++v) red[v][tid] = red[v][tid] + red[v][tid + s * a.groups];
    }
    __syncthreads();
  }
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = red[v][g];
}

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void stats_kernel(Args a) {
  __shared__ float red[V][BLOCK];
  const int tid = threadIdx.x, rr = tid / a.groups;
  const bool on = rr < a.rows;
  const int g = on ? tid % a.groups : 0;
  const typename E::T* x = (const typename E::T*)a.x;
  const long long r0 = (long long)blockIdx.x * a.chunk, r1 = r0 + a.chunk < a.R ? r0 + a.chunk : a.R;
  const bool wide = a.wide & W_X;
  float sum[V], cnt[1] = {0.0f}, xv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) sum[v] = 0.0f;
  if (on)
    for (long long row = r0 + rr; row < r1; row += a.rows) {
      if (!live_row(a.coors, row, a)) continue;
      load<E, V>(x, row * a.C + g * V, wide, xv);
      cnt[0] += 1.0f;                                                   // at most chunk / rows <= 2^23: exact
#pragma unroll
      for (int v = 0; v < V; ++v) sum[v] = sum[v] + xv[v];
    }
  fold<1>(red, cnt, tid, g, rr, a);
  fold<V>(red, sum, tid, g, rr, a);
  const float n = cnt[0];
  float m[V], r[V], m2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    m[v] = n > 0.0f ? sum[v] / n : 0.0f;
    r[v] = 0.0f;
    m2[v] = 0.0f;
  }
  if (on)
    for (long long row = r0 + rr; row < r1; row += a.rows) {
      if (!live_row(a.coors, row, a)) continue;
      load<E, V>(x, row * a.C + g * V, wide, xv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float d = xv[v] - m[v];
        r[v] = r[v] + d;
        m2[v] = fmaf(d, d, m2[v]);
      }
    }
  fold<V>(red, r, tid, g, rr, a);
  fold<V>(red, m2, tid, g, rr, a);
  if (on && rr == 0) {
    const Space sp = space_of(a.C);
    const long long at = (long long)blockIdx.x * a.C + g * V;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      a.ws[sp.plane[0] + at + v] = m[v];
      a.ws[sp.plane[1] + at + v] = r[v];
      a.ws[sp.plane[2] + at + v] = m2[v];
    }
    if (g == 0) a.ws[sp.cnt + blockIdx.x] = n;
  }
}

// v summed over the 64 lanes of a wave by a fixed tree; lane 0's total handed to every lane
__device__ __forceinline__ float wave_total(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
  return __shfl(v, 0, 64);
}

__global__ __launch_bounds__(BLOCK) void finish_kernel(Args a) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= a.C) return;                                                 // a whole wave: no barrier below
  const Space sp = space_of(a.C);
  const float *cnt = a.ws + sp.cnt, *pm = a.ws + sp.plane[0], *pr = a.ws + sp.plane[1], *p2 = a.ws + sp.plane[2];
  float n = 0.0f, w = 0.0f;
  for (int t = lane; t < a.tiles; t += 64) {
    n = n + cnt[t];                                                     // whole numbers below 2^31 rows; exact up to 2^24, rounded above
    w = fmaf(cnt[t], pm[(long long)t * a.C + c], w);
  }
  n = wave_total(n);
  const float M = n > 0.0f ? wave_total(w) / n : 0.0f;
  float S = 0.0f, Rr = 0.0f;
  for (int t = lane; t < a.tiles; t += 64) {
    const float nt = cnt[t], d = pm[(long long)t * a.C + c] - M, r = pr[(long long)t * a.C + c];
    Rr = Rr + fmaf(nt, d, r);
    S = S + (p2[(long long)t * a.C + c] + fmaf(nt * d, d, 2.0f * d * r));
  }
  S = wave_total(S);
  Rr = wave_total(Rr);
  if (lane != 0) return;
  float mean = 0.0f, var = 0.0f;
  if (n > 0.0f) {
    mean = M + Rr / n;
    const float m2 = S - Rr * Rr / n;
    var = (m2 > 0.0f || m2 != m2) ? m2 / n : 0.0f;                      // a NaN passes
  }
  a.smean[c] = mean;
  a.sistd[c] = 1.0f / sqrtf(var + a.eps);
  if (c == 0) a.ws[sp.total] = n;
  if (n >= 2.0f) {
    if (a.rmean != nullptr) a.rmean[c] = fmaf(a.momentum, mean, (1.0f - a.momentum) * a.rmean[c]);
    if (a.rvar != nullptr) a.rvar[c] = fmaf(a.momentum, var * (n / (n - 1.0f)), (1.0f - a.momentum) * a.rvar[c]);
    if (c == 0 && a.nbt != nullptr) *a.nbt = *a.nbt + 1;
  }
}

// the per-channel constants of the normalising kernels: y = fmaf(x - sub, mul, add); xhat = (x - sub) * istd
template <int V>
__device__ __forceinline__ void channel_constants(const Args& a, int c0, float* sub, float* mul, float* add, float* istd) {
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = c0 + v;
    const float gamma = a.gamma != nullptr ? a.gamma[c] : 1.0f, beta = a.beta != nullptr ? a.beta[c] : 0.0f;
    if (a.training) {
      istd[v] = a.istd[c];
      sub[v] = a.mean[c];
      mul[v] = istd[v] * gamma;
      add[v] = beta;
    } else {                                                            // scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale
      const float root = sqrtf(a.istd[c] + a.eps);
      istd[v] = 1.0f / root;
      sub[v] = 0.0f;
      mul[v] = gamma / root;
      add[v] = fmaf(-a.mean[c], mul[v], beta);
    }
  }
}

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void norm_kernel(Args a) {
  const int tid = threadIdx.x, rr = tid / a.groups, g = tid % a.groups;
  if (rr >= a.rows) return;
  const typename E::T *x = (const typename E::T*)a.x, *res = (const typename E::T*)a.res;
  typename E::T* out = (typename E::T*)a.out;
  float sub[V], mul[V], add[V], istd[V], xv[V], rv[V], yv[V];
  channel_constants<V>(a, g * V, sub, mul, add, istd);
  for (long long row = (long long)blockIdx.x * a.rows + rr; row < a.R; row += (long long)gridDim.x * a.rows) {
    const long long at = row * a.C + g * V;
    const bool live = live_row(a.coors, row, a);
#pragma unroll
    for (int v = 0; v < V; ++v) yv[v] = 0.0f;
    if (live) {
      load<E, V>(x, at, a.wide & W_X, xv);
      if (res != nullptr) load<E, V>(res, at, a.wide & W_RES, rv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float t = fmaf(xv[v] - sub[v], mul[v], add[v]);
        if (res != nullptr) t = t + rv[v];
        yv[v] = a.relu && t < 0.0f ? 0.0f : t;                          // a NaN passes, as torch.relu
      }
    }
    store<E, V>(out, at, a.wide & W_OUT, yv);
  }
}

// g = grad_out where the row is live and the ReLU let the output through, else 0
template <typename E, int V>
__device__ __forceinline__ void masked_grad(const Args& a, long long at, float* g) {
  load<E, V>((const typename E::T*)a.gy, at, a.wide & W_GY, g);
  if (a.relu) {
    float y[V];
    load<E, V>((const typename E::T*)a.y, at, a.wide & W_Y, y);
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] = y[v] > 0.0f ? g[v] : 0.0f;
  }
}

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void bstats_kernel(Args a) {
  __shared__ float red[V][BLOCK];
  const int tid = threadIdx.x, rr = tid / a.groups;
  const bool on = rr < a.rows;
  const int g = on ? tid % a.groups : 0;
  const long long r0 = (long long)blockIdx.x * a.chunk, r1 = r0 + a.chunk < a.R ? r0 + a.chunk : a.R;
  float sub[V], mul[V], add[V], istd[V], sg[V], sgx[V], gv[V], xv[V], cnt[1] = {0.0f};
  channel_constants<V>(a, g * V, sub, mul, add, istd);
  if (!a.training) {
#pragma unroll
    for (int v = 0; v < V; ++v) sub[v] = a.mean[g * V + v];             // xhat of a frozen BatchNorm: (x - running_mean) * invstd
  }
#pragma unroll
  for (int v = 0; v < V; ++v) sg[v] = sgx[v] = 0.0f;
  if (on)
    for (long long row = r0 + rr; row < r1; row += a.rows) {
      if (!live_row(a.coors, row, a)) continue;
      const long long at = row * a.C + g * V;
      masked_grad<E, V>(a, at, gv);
      load<E, V>((const typename E::T*)a.x, at, a.wide & W_X, xv);
      cnt[0] += 1.0f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        sg[v] = sg[v] + gv[v];
        sgx[v] = fmaf(gv[v], (xv[v] - sub[v]) * istd[v], sgx[v]);
      }
    }
  fold<1>(red, cnt, tid, g, rr, a);
  fold<V>(red, sg, tid, g, rr, a);
  fold<V>(red, sgx, tid, g, rr, a);
  if (on && rr == 0) {
    const Space sp = space_of(a.C);
    const long long at = (long long)blockIdx.x * a.C + g * V;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      a.ws[sp.plane[0] + at + v] = sg[v];
      a.ws[sp.plane[1] + at + v] = sgx[v];
    }
    if (g == 0) a.ws[sp.cnt + blockIdx.x] = cnt[0];
  }
}

__global__ __launch_bounds__(BLOCK) void bfinish_kernel(Args a) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= a.C) return;
  const Space sp = space_of(a.C);
  const float *cnt = a.ws + sp.cnt, *pg = a.ws + sp.plane[0], *pgx = a.ws + sp.plane[1];
  float n = 0.0f, sg = 0.0f, sgx = 0.0f;
  for (int t = lane; t < a.tiles; t += 64) {
    n = n + cnt[t];
    sg = sg + pg[(long long)t * a.C + c];
    sgx = sgx + pgx[(long long)t * a.C + c];
  }
  n = wave_total(n);
  sg = wave_total(sg);
  sgx = wave_total(sgx);
  if (lane != 0) return;
  if (a.gbeta != nullptr) a.gbeta[c] = sg;
  if (a.ggamma != nullptr) a.ggamma[c] = sgx;
  a.ws[sp.merged + c] = n > 0.0f ? sg / n : 0.0f;
  a.ws[sp.merged + a.C + c] = n > 0.0f ? sgx / n : 0.0f;
}

template <typename E, int V>
__global__ __launch_bounds__(BLOCK) void bnorm_kernel(Args a) {
  const int tid = threadIdx.x, rr = tid / a.groups, g = tid % a.groups;
  if (rr >= a.rows) return;
  typename E::T *gx = (typename E::T*)a.gx, *gres = (typename E::T*)a.gres;
  float sub[V], mul[V], add[V], istd[V], mg[V], mgx[V], gv[V], xv[V], ov[V];
  channel_constants<V>(a, g * V, sub, mul, add, istd);
  if (a.training) {
    const Space sp = space_of(a.C);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      mg[v] = a.ws[sp.merged + g * V + v];
      mgx[v] = a.ws[sp.merged + a.C + g * V + v];
    }
  }
  for (long long row = (long long)blockIdx.x * a.rows + rr; row < a.R; row += (long long)gridDim.x * a.rows) {
    const long long at = row * a.C + g * V;
    const bool live = live_row(a.coors, row, a);
#pragma unroll
    for (int v = 0; v < V; ++v) gv[v] = ov[v] = 0.0f;
    if (live) {
      masked_grad<E, V>(a, at, gv);
      if (a.training) {                                                 // grad_x = gamma * invstd * (g - sum g / n - xhat * sum (g xhat) / n)
        load<E, V>((const typename E::T*)a.x, at, a.wide & W_X, xv);
#pragma unroll
        for (int v = 0; v < V; ++v) ov[v] = mul[v] * fmaf(-((xv[v] - sub[v]) * istd[v]), mgx[v], gv[v] - mg[v]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) ov[v] = gv[v] * mul[v];
      }
    }
    store<E, V>(gx, at, a.wide & W_GX, ov);
    if (gres != nullptr) store<E, V>(gres, at, a.wide & W_GRES, gv);
  }
}

int first_step(int rows) {
  int s = 1;
  while (s < rows) s <<= 1;
  return s >> 1;
}

void lay_out(Args* a, int64_t R, int32_t C, int32_t dtype) {
  const Lanes l = lanes_of(C, dtype, BLOCK);
  int64_t tiles, chunk;
  cut_rows(R, &tiles, &chunk);
  a->R = R; a->C = C; a->chunk = chunk; a->tiles = (int)tiles;
  a->groups = l.groups; a->rows = l.rows; a->half = first_step(l.rows);
}

unsigned sweep_blocks(const Args& a) {
  const long long b = (a.R + a.rows - 1) / a.rows;
  return (unsigned)(b < 2048 ? b : 2048);
}

template <typename E>
int launch_forward(const Args& a, bool vec, hipStream_t s) {
  constexpr int V = E::WIDE;
  if (a.training) {
    if (vec) hipLaunchKernelGGL((stats_kernel<E, V>), dim3((unsigned)a.tiles), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((stats_kernel<E, 1>), dim3((unsigned)a.tiles), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(BLOCK), 0, s, a);
  }
  if (vec) hipLaunchKernelGGL((norm_kernel<E, V>), dim3(sweep_blocks(a)), dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL((norm_kernel<E, 1>), dim3(sweep_blocks(a)), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

template <typename E>
int launch_backward(const Args& a, bool vec, bool sums, hipStream_t s) {
  constexpr int V = E::WIDE;
  if (sums) {
    if (vec) hipLaunchKernelGGL((bstats_kernel<E, V>), dim3((unsigned)a.tiles), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((bstats_kernel<E, 1>), dim3((unsigned)a.tiles), dim3(BLOCK), 0, s, a);
    hipLaunchKernelGGL(bfinish_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(BLOCK), 0, s, a);
  }
  if (vec) hipLaunchKernelGGL((bnorm_kernel<E, V>), dim3(sweep_blocks(a)), dim3(BLOCK), 0, s, a);
  else hipLaunchKernelGGL((bnorm_kernel<E, 1>), dim3(sweep_blocks(a)), dim3(BLOCK), 0, s, a);
  return (int)hipGetLastError();
}

__global__ void fill_kernel(float* p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

extern "C" {

size_t gd3d_sparse_bn_workspace_bytes(int64_t R, int32_t C) {
  if (R < 0 || C < 1 || C > MAX_C) return 0;
  return (space_of(C).words * sizeof(float) + 255) / 256 * 256;
}

int gd3d_sparse_bn_forward(const void* features, const int32_t* coors, const void* residual, const float* weight, const float* bias,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t R, int32_t C, int32_t B, int32_t D,
                           int32_t H, int32_t W, int32_t training, float momentum, float eps, int32_t act, int32_t dtype, void* workspace,
                           void* out, float* save_mean, float* save_invstd, void* stream) {
  const int rc = check_dims(R, C, B, D, H, W, act, dtype);
  if (rc != 0) return rc;
  if (training ? (save_mean == nullptr || save_invstd == nullptr || workspace == nullptr) : (running_mean == nullptr || running_var == nullptr))
    return GD3D_E_BADARG;
  if (R > 0 && (features == nullptr || coors == nullptr || out == nullptr)) return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(features, es) || misaligned(residual, es) || misaligned(out, es) || misaligned(coors, 4) || misaligned(workspace, 4))
    return GD3D_E_BADARG;
  if (R > 0 && residual != nullptr && sparse_conv::ranges_overlap(residual, out, es * (size_t)R * (size_t)C)) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  Args a = {};
  lay_out(&a, R, C, dtype);
  a.x = features; a.res = residual; a.out = out; a.coors = coors; a.gamma = weight; a.beta = bias;
  a.rmean = running_mean; a.rvar = running_var; a.nbt = (long long*)num_batches_tracked; a.smean = save_mean; a.sistd = save_invstd;
  a.mean = training ? save_mean : running_mean;
  a.istd = training ? save_invstd : running_var;
  a.ws = (float*)workspace;
  a.B = B; a.D = D; a.H = H; a.W = W; a.training = training ? 1 : 0; a.relu = act == GD3D_ACT_RELU; a.momentum = momentum; a.eps = eps;
  a.wide = wide_bit(features, W_X) | wide_bit(residual, W_RES) | wide_bit(out, W_OUT) | wide_bit(coors, W_COORS);
  if (R == 0) {                                                         // no row: the statistics of nothing, no running update
    if (training) {
      hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, save_mean, (int)C, 0.0f);
      hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, save_invstd, (int)C, 1.0f / sqrtf(eps));
    }
    return (int)hipGetLastError();
  }
  const bool vec = lanes_of(C, dtype, BLOCK).vec > 1;
  return with_elem(dtype, [&](auto e) { return launch_forward<decltype(e)>(a, vec, s); });
}

int gd3d_sparse_bn_backward(const void* grad_out, const void* features, const void* out, const int32_t* coors, const float* weight,
                            const float* mean, const float* invstd_or_var, int64_t R, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                            int32_t training, float eps, int32_t act, int32_t dtype, void* workspace, void* grad_features, void* grad_residual,
                            float* grad_weight, float* grad_bias, void* stream) {
  const int rc = check_dims(R, C, B, D, H, W, act, dtype);
  if (rc != 0) return rc;
  if (mean == nullptr || invstd_or_var == nullptr || workspace == nullptr) return GD3D_E_BADARG;
  if (R > 0 && (grad_out == nullptr || features == nullptr || coors == nullptr || grad_features == nullptr || (act == GD3D_ACT_RELU && out == nullptr)))
    return GD3D_E_BADARG;
  const size_t es = elem_size(dtype);
  if (misaligned(grad_out, es) || misaligned(features, es) || misaligned(out, es) || misaligned(grad_features, es) || misaligned(grad_residual, es) ||
      misaligned(coors, 4) || misaligned(workspace, 4))
    return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  Args a = {};
  lay_out(&a, R, C, dtype);
  a.gy = grad_out; a.x = features; a.y = out; a.coors = coors; a.gamma = weight; a.mean = mean; a.istd = invstd_or_var;
  a.gx = grad_features; a.gres = grad_residual; a.ggamma = grad_weight; a.gbeta = grad_bias; a.ws = (float*)workspace;
  a.B = B; a.D = D; a.H = H; a.W = W; a.training = training ? 1 : 0; a.relu = act == GD3D_ACT_RELU; a.eps = eps;
  a.wide = wide_bit(grad_out, W_GY) | wide_bit(features, W_X) | wide_bit(out, W_Y) | wide_bit(grad_features, W_GX) | wide_bit(grad_residual, W_GRES) | wide_bit(coors, W_COORS);
  if (R == 0) {
    if (grad_weight != nullptr) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, grad_weight, (int)C, 0.0f);
    if (grad_bias != nullptr) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, grad_bias, (int)C, 0.0f);
    return (int)hipGetLastError();
  }
  const bool vec = lanes_of(C, dtype, BLOCK).vec > 1, sums = training || grad_weight != nullptr || grad_bias != nullptr;
  return with_elem(dtype, [&](auto e) { return launch_backward<decltype(e)>(a, vec, sums, s); });
}

}  // extern "C"
