// gd3d_loss_common.h — what the three GD-loss translation units (gd3d_loss.hip: the fused per-pair kernel and its second
// stage; gd3d_anchor_head.hip; gd3d_center_head.hip) share: the anchor decode and its chain rule, the wave sum, the head
// kernels' workgroup size, and the two launches that live in gd3d_loss.hip and are reached from the head units through
// plain functions (a __global__ kernel is defined in exactly one unit; nothing here is exported, see gd3d.map).
#pragma once
#include <hip/hip_runtime.h>

#include "gd3d_device.h"
#include "gd3d_fill.h"
#include "gd3d_instances.h"

namespace gd3d {

constexpr int HEAD_T = 256;          // threads per workgroup of the head-level kernels

// Decode the encoded rows in registers and remember what the chain rule needs.
//   ANCHOR_DELTA: j = (diag, diag, ha, w, l, h, 1) with the z/h cross term handled in encode_grad()
struct DecodeJac {
  float j[7];
};

GD_DEV void decode_anchor(const float (&enc)[7], const float (&an)[7], float (&dec)[7], DecodeJac& J) {
  const float diag = fsqrt(fmaf(an[4], an[4], an[3] * an[3]));
  const float w = expf(enc[3]) * an[3], l = expf(enc[4]) * an[4], h = expf(enc[5]) * an[5];
  dec[0] = fmaf(enc[0], diag, an[0]);
  dec[1] = fmaf(enc[1], diag, an[1]);
  dec[2] = fmaf(enc[2], an[5], an[2] + an[5] * 0.5f) - h * 0.5f;
  dec[3] = w;
  dec[4] = l;
  dec[5] = h;
  dec[6] = enc[6] + an[6];
  J.j[0] = diag; J.j[1] = diag; J.j[2] = an[5]; J.j[3] = w; J.j[4] = l; J.j[5] = h; J.j[6] = 1.0f;
}

// gradient wrt the decoded row -> gradient wrt the encoded row (in place)
GD_DEV void encode_grad(float (&g)[7], const DecodeJac& J, bool anchor_kind) {
  const float gz = g[2];
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] *= J.j[k];
  if (anchor_kind) g[5] = fmaf(-0.5f * gz, J.j[5], g[5]);  // z = ... - h/2 with h = exp(ht)*ha
}

// wave64 sum with DPP adds (no LDS crossbar): inclusive scan inside each 16-lane row (row_shr 1,2,4,8 with
// zero fill), then row_bcast:15 / row_bcast:31 carry the row totals; lane 63 holds the total.  Fixed order.
template <int CTRL, int ROW_MASK>
GD_DEV float dpp_add(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true);
  return v + __builtin_bit_cast(float, moved);
}
GD_DEV float wave_sum(float v) {
  v = dpp_add<0x111, 0xf>(v);  // row_shr:1
  v = dpp_add<0x112, 0xf>(v);  // row_shr:2
  v = dpp_add<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add<0x118, 0xf>(v);  // row_shr:8
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// defined in gd3d_loss.hip (fill_words: gd3d_fill.h)
int reduce_partials(const float* partials, long long nb, float* out, hipStream_t s);   // reduce_partials_kernel

}  // namespace gd3d
