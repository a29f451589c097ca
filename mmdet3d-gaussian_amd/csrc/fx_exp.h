// fx_exp.h — the exponential as ONE fixed sequence of fp32 operations, next to fx_logf (csrc/fx_log.h) and in its namespace: the
// argument is reduced by a multiple of ln 2 kept in two pieces, x = k ln 2 + r with |r| <= ln 2 / 2, exp(r) comes from the classic
// rational form r c / (2 - c) with a degree-2 polynomial c in r^2, and the scale by 2^k is an integer add on the bit pattern.
// No libm, no hardware v_exp, no fma.  A unit that includes it must be compiled with -ffp-contract=off (and the device's
// correctly rounded division): the same source then gives the same bits on gfx950 and on the host, which is what lets a decision
// that hangs on a sigmoid (csrc/rpn_proposal_common.h: `score > score_thr`) and the decoded box sizes replay in a `_cpu` twin.
// Measured against fp64 exp, correctly rounded, on 2^20 uniform arguments of the finite-result range [ln FLT_MIN, ln FLT_MAX],
// every integer multiple of ln 2 / 2 in that range with its 4 neighbours either side, and the 4096 values either side of 0
// (tests/test_cpu_rpn_proposal.py): worst error 0.880 ulp (documented bound 0.90: faithful); the host libm's expf on the same
// sample: 0.502 ulp.
#pragma once
#include "rbox_device.h"   // RB_DEV; under GD3D_HOST_TWIN the host's definitions of the function-space keywords

namespace rbox {

// exp(x): NaN for NaN; +inf for x > 88.7228317 (0x42b17217, the largest argument whose exponential is finite); +0 EXACTLY for
// x < -87.3365402 (0xc2aeac4f, the smallest argument whose exponential is a normal number): a subnormal result is never produced,
// so the bits do not depend on the denormal mode (a documented deviation from exp, at most 1.18e-38 absolute).
RB_DEV float fx_expf(float x) {
  const float LN2_HI = 6.9313812256e-01f, LN2_LO = 9.0580006145e-06f;   // ln 2 in two pieces: k * LN2_HI is exact for |k| < 2^9
  const float INV_LN2 = 1.4426950216e+00f;
  const float P1 = 1.6666625440e-01f, P2 = -2.7667332906e-03f;
  if (x != x) return x;
  if (x > 88.72283172607422f) return __builtin_inff();
  if (x < -87.33654022216797f) return 0.0f;
  const int k = (int)(INV_LN2 * x + (x < 0.0f ? -0.5f : 0.5f));          // truncation: |k| <= 128
  const float kf = (float)k;
  const float hi = x - kf * LN2_HI;
  const float lo = kf * LN2_LO;
  const float r = hi - lo;
  const float t = r * r;
  const float c = r - t * (P1 + t * P2);
  const float y = 1.0f + (hi - (lo - (r * c) / (2.0f - c)));            // in (0.70, 1.42)
  const unsigned yb = __builtin_bit_cast(unsigned, y);
  const int e = (int)((yb >> 23) & 255u) + k;                            // the result's biased exponent
  if (e <= 0) return 0.0f;                                               // rounding at the lower cut-off: still never a subnormal
  if (e >= 255) return __builtin_inff();
  return __builtin_bit_cast(float, yb + ((unsigned)k << 23));
}

}  // namespace rbox
