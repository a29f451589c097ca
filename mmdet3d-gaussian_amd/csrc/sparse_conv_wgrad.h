// sparse_conv_wgrad.h — what the two stage-one forms of the sparse convolution's weight gradient share (csrc/sparse_conv_wgrad.hip: the
// fp32 FMA form for fp32, fp16 and bf16 operands; csrc/sparse_conv_wgrad_16.hip: the matrix-core form for fp16 / bf16; DESIGN.md §3.18,
// §3.19, §3.29): the launch arguments, the cut of the caller's workspace into the partial sums, and the launches that follow stage one.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gd3d_fill.h"
#include "gd3d_workspace.h"
#include "sparse_conv_common.h"

namespace sparse_conv {

struct WgradArgs {
  const void *X, *gY;       // (n_src, Cin) and (rows, Cout) of E::T
  const int32_t* nbr;
  const long long* num;
  long long n_src, rows, chunk, parts;
  int K, Cin, Cout, tiles_co;
  float *part_w, *part_b;   // (parts, K, Cin, Cout) and (parts, Cout)
  float *gW, *gb;           // gb nullable
};

// part_w and part_b out of the caller's workspace (256-byte aligned), for the a.parts and a.Cout set.  At address 0 it is the size function.
static size_t carve(WgradArgs& a, void* workspace, int64_t kcc) {
  gd3d::Carver c(workspace, gd3d::Carver::CALLER_ALIGNED);
  a.part_w = c.take<float>((size_t)a.parts * (size_t)kcc);
  a.part_b = c.take<float>((size_t)a.parts * (size_t)a.Cout);
  return c.bytes();
}

// everything of a checked call but the stage-one launch: the chunks of weight_parts, the workspace carved, the outputs
static void fill_args(WgradArgs& a, const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R,
                      int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight, float* grad_bias) {
  const int64_t kcc = (int64_t)K * Cin * Cout;
  a.X = features; a.gY = grad_out; a.nbr = nbr; a.num = (const long long*)num; a.n_src = N; a.rows = R;
  weight_parts(R, kcc, (int64_t*)&a.parts, (int64_t*)&a.chunk);
  a.K = K; a.Cin = Cin; a.Cout = Cout; a.tiles_co = 1;
  carve(a, workspace, kcc);
  a.gW = grad_weight; a.gb = grad_bias;
}

// the call without a pair (check_wgrad_call's *run = false): the gradients are zeros
static int zero_wgrad(int32_t K, int32_t Cin, int32_t Cout, float* grad_weight, float* grad_bias, hipStream_t s) {
  int e = gd3d::fill_words(grad_weight, sizeof(float) * (size_t)K * (size_t)Cin * (size_t)Cout, 0u, s);
  if (e == 0 && grad_bias != nullptr) e = gd3d::fill_words(grad_bias, sizeof(float) * (size_t)Cout, 0u, s);
  return e;
}

// what follows stage one, whichever form wrote part_w (csrc/sparse_conv_wgrad.hip): bias_kernel<E of dtype> where a.gb is given, then
// wfinish_kernel.  -> hipGetLastError()
int finish_wgrad(const WgradArgs& a, int32_t dtype, hipStream_t s);

}  // namespace sparse_conv
