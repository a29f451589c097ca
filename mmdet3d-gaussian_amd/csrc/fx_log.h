// fx_log.h — the natural logarithm as ONE fixed sequence of fp32 operations, next to fx_sincosf / fx_atan2f of rbox_device.h and in
// their namespace: exponent extraction on the bit pattern, the classic s = f / (2 + f) reduction and a degree-4 even polynomial,
// no libm, no hardware v_log.  A unit that includes it must be compiled with -ffp-contract=off (and the device's correctly
// rounded division): the same source then gives the same bits on gfx950 and on the host, which is what lets a decision that
// hangs on a logarithm (csrc/simota_common.h: the SimOTA cost) replay in a `_cpu` twin.
// Measured against fp64 log, correctly rounded, on 2^20 log-uniform values of [1e-8, 2], every binade edge and the 4096 values
// next below 1 (tests/test_cpu_simota.py): worst error 0.795 ulp (documented bound 0.80); the host libm's logf on the same
// sample: 0.795 ulp.
#pragma once
#include "rbox_device.h"   // RB_DEV; under GD3D_HOST_TWIN the host's definitions of the function-space keywords

namespace rbox {

// log(x): NaN for NaN and for x < 0, -inf for +-0, +inf for +inf; subnormal x is scaled by 2^25 first (exact).
RB_DEV float fx_logf(float x) {
  const float LN2_HI = 6.9313812256e-01f, LN2_LO = 9.0580006145e-06f;   // ln 2 in two pieces: k * LN2_HI is exact for |k| < 2^9
  const float L1 = 0.66666662693f, L2 = 0.40000972152f, L3 = 0.28498786688f, L4 = 0.24279078841f;
  unsigned ix = __builtin_bit_cast(unsigned, x);
  int k = 0;
  if (ix < 0x00800000u || (ix >> 31)) {
    if ((ix << 1) == 0u) return -__builtin_inff();
    if (ix >> 31) return __builtin_nanf("");     // negative, or a NaN with the sign bit set
    k -= 25;
    x = x * 33554432.0f;
    ix = __builtin_bit_cast(unsigned, x);
  } else if (ix >= 0x7f800000u) {
    return x;                                    // +inf, NaN
  }
  // x = 2^k * m with m in [sqrt(2) / 2, sqrt(2))
  ix += 0x3f800000u - 0x3f3504f3u;
  k += (int)(ix >> 23) - 127;
  ix = (ix & 0x007fffffu) + 0x3f3504f3u;
  const float f = __builtin_bit_cast(float, ix) - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s;
  const float w = z * z;
  const float t1 = w * (L2 + w * L4);
  const float t2 = z * (L1 + w * L3);
  const float r = t2 + t1;
  const float hfsq = 0.5f * f * f;
  const float dk = (float)k;
  return s * (hfsq + r) + dk * LN2_LO - hfsq + f + dk * LN2_HI;
}

}  // namespace rbox
