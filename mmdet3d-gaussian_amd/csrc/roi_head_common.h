// roi_head_common.h — what csrc/roi_head.hip (gfx950 kernels) and csrc/roi_head_cpu.cpp (their `_cpu` twins) share: the per-row
// math of PVRCNNBboxHead's training slice (models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:140-351) as ONE sequence of fp32
// operations each — the label of a RoI, the regression target of a positive, and the three loss terms of a row with their
// gradients.  Both units are compiled with -ffp-contract=off.  The decisions (label branch, label >= 0, the flip and wrap of the
// target yaw) are comparisons of exactly rounded fp32 values (fmodf is exact), so they are the same bits on the device and on the
// host; sin / cos / exp / log come from each target's own math library, so the VALUES agree to a few ulp, not bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
#define RH_HD __device__ __forceinline__
#else
#define RH_HD inline
#endif

namespace roi_head {

constexpr int WG = 1024;            // threads of the one workgroup = rows of a chunk
constexpr int MAX_SAMPLES = 1024;   // samples whose segment starts the targets kernel keeps in LDS
constexpr long long MAX_ROWS = 1LL << 24;   // counts of rows are exact in fp32 up to here (the normalisers are fp32 sums of ones)

// the fp32 roundings of the doubles 2 pi, pi, pi / 2, 3 pi / 2 (what a Python float becomes next to an fp32 tensor)
constexpr float TWO_PI = (float)6.283185307179586;
constexpr float PI = (float)3.141592653589793;
constexpr float HALF_PI = (float)1.5707963267948966;
constexpr float THREE_HALF_PI = (float)4.71238898038469;

RH_HD void sin_cos(float a, float& s, float& c) {
#if defined(__HIPCC__) && !defined(GD3D_HOST_TWIN)
  sincosf(a, &s, &c);
#else
  s = sinf(a);
  c = cosf(a);
#endif
}

// Python's `a % (2 pi)` as torch.remainder evaluates it on fp32: the exact fmod, moved up by one period when negative
RH_HD float pymod(float a) {
  float m = fmodf(a, TWO_PI);
  if (m < 0.0f) m += TWO_PI;
  return m;
}

// :270-276   label = iou > pos ? 1 : (iou < neg ? 0 : iou * 2 - 0.5)
RH_HD float label_of(float iou, float pos_thr, float neg_thr) {
  if (iou > pos_thr) return 1.0f;
  if (iou < neg_thr) return 0.0f;
  return iou * 2.0f - 0.5f;
}

// the turn of (x, y) about z by the angle whose sine and cosine are (s, c): counter-clockwise (mmdet3d 1.0's
// rotation_3d_in_axis, axis 2), or its transpose (0.x) with `clockwise`
RH_HD void turn(float x, float y, float s, float c, int clockwise, float& ox, float& oy) {
  const float xc = x * c, ys = y * s, xs = x * s, yc = y * c;
  ox = clockwise ? xc + ys : xc - ys;
  oy = clockwise ? yc - xs : xs + yc;
}

// :285-310   the regression target of a positive: the gt in the RoI's canonical frame, its yaw folded into [-pi/2, pi/2],
// encoded by DeltaXYZWLHRBBoxCoder.encode against the anchor (0, 0, 0, roi dims, 0)
RH_HD void target_row(const float* roi, const float* gt, int clockwise, float* t) {
  const float ry = pymod(roi[6]);
  const float dx = gt[0] - roi[0], dy = gt[1] - roi[1], dz = gt[2] - roi[2];
  float s, c;
  sin_cos(ry, s, c);
  float x, y;
  turn(dx, dy, -s, c, clockwise, x, y);   // by -ry: sin(-ry) = -sin(ry) exactly
  float r = pymod(gt[6] - ry);
  if (r > HALF_PI && r < THREE_HALF_PI) r = pymod(r + PI);
  if (r > PI) r -= TWO_PI;
  r = r < -HALF_PI ? -HALF_PI : (r > HALF_PI ? HALF_PI : r);
  const float wa = roi[3], la = roi[4], ha = roi[5];
  const float wg = gt[3], lg = gt[4], hg = gt[5];
  const float za = 0.0f + ha / 2;
  const float zg = dz + hg / 2;
  const float diagonal = sqrtf(la * la + wa * wa);
  t[0] = (x - 0.0f) / diagonal;
  t[1] = (y - 0.0f) / diagonal;
  t[2] = (zg - za) / ha;
  t[3] = logf(wg / wa);
  t[4] = logf(lg / la);
  t[5] = logf(hg / ha);
  t[6] = r - 0.0f;
}

// sigmoid cross entropy of one logit x against the soft label z, weight w:  w (max(x, 0) - x z + log1p(exp(-|x|)));
// *grad = scale * w (sigmoid(x) - z)
RH_HD float cls_row(float x, float z, float w, float scale, float* grad) {
  const float ax = x < 0.0f ? -x : x;
  const float e = expf(-ax);
  const float loss = (x > 0.0f ? x : 0.0f) - x * z + log1pf(e);
  const float sig = x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
  *grad = scale * (w * (sig - z));
  return w * loss;
}

// smooth L1 of the 7 residuals p against the target t, weight w:  e = |p - t|;  w (e < beta ? 0.5 e e / beta : e - 0.5 beta);
// g[j] = scale * w * d/dp
RH_HD float smooth_l1_row(const float* p, const float* t, float w, float beta, float scale, float* g) {
  float loss = 0.0f;
  for (int j = 0; j < 7; ++j) {
    const float d = p[j] - t[j];
    const float e = d < 0.0f ? -d : d;
    const bool quad = e < beta;
    loss += quad ? 0.5f * e * e / beta : e - 0.5f * beta;
    const float dl = quad ? d / beta : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
    g[j] = scale * (w * dl);
  }
  return w * loss;
}

// :187-209 + :318-351   the corner loss of one positive: the residuals p decoded against the anchor (0, 0, 0, roi dims, roi yaw)
// (coder_roi_decode's sequence), the centre turned by the roi yaw and moved to the roi centre; the 8 corners of that box against
// those of the gt and of the gt turned by pi, the nearer of the two per corner, Huber(delta = 1), mean over the corners.
// g[0..7) = scale * d(mean) / dp, back through the decode.  Rules at the two points where the distance is not differentiable:
// a zero distance gives a zero gradient (as torch.norm's backward does); on an exact tie of the two distances the UNFLIPPED
// gt takes the whole gradient (torch.min's backward gives each branch half).
RH_HD float corner_row(const float* roi, const float* p, const float* gt, int clockwise, float scale, float* g) {
  const float wa = roi[3], la = roi[4], ha = roi[5], ra = roi[6];
  const float za = 0.0f + ha / 2;
  const float diagonal = sqrtf(la * la + wa * wa);
  const float xl = p[0] * diagonal + 0.0f;
  const float yl = p[1] * diagonal + 0.0f;
  float zg = p[2] * ha + za;
  const float lg = expf(p[4]) * la;
  const float wg = expf(p[3]) * wa;
  const float hg = expf(p[5]) * ha;
  const float rg = p[6] + ra;
  zg = zg - hg / 2;
  float sa, ca;
  sin_cos(ra, sa, ca);
  float xr, yr;
  turn(xl, yl, sa, ca, clockwise, xr, yr);
  const float cx = xr + roi[0], cy = yr + roi[1], cz = zg + roi[2];
  float sp, cp, sg, cg, sf, cf;
  sin_cos(rg, sp, cp);
  sin_cos(gt[6], sg, cg);
  sin_cos(gt[6] + PI, sf, cf);
  float loss = 0.0f;
  float gcx = 0.0f, gcy = 0.0f, gcz = 0.0f, gw = 0.0f, gl = 0.0f, gh = 0.0f, gyaw = 0.0f;
  for (int k = 0; k < 8; ++k) {
    const float nx = (k & 4) ? 0.5f : -0.5f, ny = (k & 2) ? 0.5f : -0.5f, nz = (k & 1) ? 1.0f : 0.0f;
    const float lx = wg * nx, ly = lg * ny, lz = hg * nz;
    float px, py;
    turn(lx, ly, sp, cp, clockwise, px, py);
    px += cx;
    py += cy;
    const float pz = lz + cz;
    const float ax = gt[3] * nx, ay = gt[4] * ny, az = gt[5] * nz;
    float qx, qy, fx, fy;
    turn(ax, ay, sg, cg, clockwise, qx, qy);
    turn(ax, ay, sf, cf, clockwise, fx, fy);
    const float qz = az + gt[2];
    const float d1x = px - (qx + gt[0]), d1y = py - (qy + gt[1]), dz = pz - qz;
    const float d2x = px - (fx + gt[0]), d2y = py - (fy + gt[1]);
    const float n1 = sqrtf(d1x * d1x + d1y * d1y + dz * dz);
    const float n2 = sqrtf(d2x * d2x + d2y * d2y + dz * dz);
    const bool first = n1 <= n2;
    const float dist = first ? n1 : n2;
    const float q = dist < 1.0f ? dist : 1.0f;
    loss += 0.5f * q * q + (dist - q);
    // d Huber / d dist = q;  d dist / d corner = (corner - gt corner) / dist
    const float coef = dist > 0.0f ? q / dist : 0.0f;
    const float gx = coef * (first ? d1x : d2x), gy = coef * (first ? d1y : d2y), gz = coef * dz;
    gcx += gx;
    gcy += gy;
    gcz += gz;
    // corner = centre + turn(l, yaw):  d/dl is the transposed turn of the gradient, d/dyaw the turn's derivative
    float tx, ty;
    turn(gx, gy, sp, cp, !clockwise, tx, ty);
    gw += nx * tx;
    gl += ny * ty;
    gh += nz * gz;
    gyaw += clockwise ? gx * (ly * cp - lx * sp) - gy * (lx * cp + ly * sp) : gy * (lx * cp - ly * sp) - gx * (lx * sp + ly * cp);
  }
  // centre = turn((xl, yl), roi yaw) + roi centre;  z = p2 ha + ha / 2 - hg / 2
  float gxl, gyl;
  turn(gcx, gcy, sa, ca, !clockwise, gxl, gyl);
  const float s8 = scale * 0.125f;
  g[0] = s8 * (gxl * diagonal);
  g[1] = s8 * (gyl * diagonal);
  g[2] = s8 * (gcz * ha);
  g[3] = s8 * (gw * wg);
  g[4] = s8 * (gl * lg);
  g[5] = s8 * ((gh - 0.5f * gcz) * hg);
  g[6] = s8 * gyaw;
  return loss * 0.125f;
}

RH_HD int clamp_count(int c, int room) {
  const int v = c < 0 ? 0 : c;
  return v < room ? v : room;
}

// the sample of row i among the segment starts s[0] <= s[1] <= .. <= s[B]: the b with s[b] <= i < s[b + 1], B for a row past s[B]
template <typename S>
RH_HD int sample_of(const S* s, int B, int i) {
  int lo = 0, hi = B;   // the first b in [0, B] with s[b + 1] > i  (s[B + 1] = +inf)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid + 1] > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

}  // namespace roi_head
