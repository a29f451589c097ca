// pib_cpu.cpp — the `_cpu` twins of the point-in-rotated-box entry points (include/gd3d.h, gd3d_pib_*_cpu,
// gd3d_roi_grid_points_cpu): plain loops over the same fp32 operation sequence as csrc/pib.hip (csrc/pib_common.h and the
// fixed-sequence sincos of csrc/rbox_device.h, both units compiled with -ffp-contract=off), so box_idx, the flags, the
// segmentation targets and the grid points are bit-identical to the kernels'.
// Host memory in and out, no stream, no HIP call.  Points / RoIs are split over `nthreads` std::threads.
#define GD3D_HOST_TWIN 1
#include "pib_common.h"

#include "../../include/gd3d.h"
#include "host_threads.h"

#include <cstring>
#include <vector>

using gd3d_host::parallel_ranges;
using namespace pib;

namespace {

// the samples' clamped segments: start[b] .. start[b + 1]; rows from start[B] on belong to no sample
std::vector<long long> segment_starts(const int32_t* pcnt, int B, long long N) {
  std::vector<long long> start((size_t)B + 1, 0);
  for (int b = 0; b < B; ++b) start[b + 1] = start[b] + clamp_count(pcnt[b], N - start[b]);
  return start;
}

// per sample: its tested boxes' constants (and the enlarged ones)
struct SampleBoxes {
  std::vector<BoxC> box, big;
};

std::vector<SampleBoxes> sample_boxes(const float* boxes, const int32_t* box_cnt, int B, int T, bool enlarged, float w) {
  std::vector<SampleBoxes> out((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int tb = boxes_of(box_cnt, b, T);
    out[b].box.resize((size_t)tb);
    if (enlarged) out[b].big.resize((size_t)tb);
    for (int t = 0; t < tb; ++t) {
      const float* q = boxes + ((long long)b * T + t) * 7;
      out[b].box[t] = box_constants(q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
      if (enlarged) out[b].big[t] = box_constants_enlarged(q[0], q[1], q[2], q[3], q[4], q[5], q[6], w);
    }
  }
  return out;
}

int first_hit(const std::vector<BoxC>& k, const float* p) {
  for (size_t t = 0; t < k.size(); ++t)
    if (contains(k[t], p[0], p[1], p[2])) return (int)t;
  return -1;
}

int first_box(const float* points, const int32_t* pcnt, const float* boxes, const int64_t* labels, const int32_t* box_cnt, int32_t B,
              int64_t N, int32_t T, bool mask, float extra_width, int32_t num_classes, int64_t* seg, int32_t* box_idx,
              int32_t nthreads) {
  bool ok = true;
  try {
    const std::vector<long long> start = segment_starts(pcnt, B, N);
    const std::vector<SampleBoxes> sb = sample_boxes(boxes, box_cnt, B, T, mask, extra_width);
    ok = parallel_ranges(N, gd3d_host::team_size(nthreads, N, 256, 1024), [&](int64_t n0, int64_t n1) {
      int b = 0;
      for (int64_t n = n0; n < n1; ++n) {
        while (b < B && n >= start[b + 1]) ++b;
        int hit = -1, ehit = -1;
        if (b < B) {
          hit = first_hit(sb[b].box, points + n * 3);
          if (mask) ehit = first_hit(sb[b].big, points + n * 3);
        }
        if (mask) {
          int64_t s = hit >= 0 ? labels[(long long)b * T + hit] : (int64_t)num_classes;
          if ((hit >= 0) != (ehit >= 0)) s = -1;
          seg[n] = s;
        }
        if (box_idx != nullptr) box_idx[n] = hit;
      }
    });
  } catch (...) {
    ok = false;
  }
  return ok ? 0 : GD3D_E_HOST;
}

}  // namespace

extern "C" {

int gd3d_pib_part_cpu(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt, int32_t B,
                      int64_t N, int32_t T, int32_t* box_idx, int32_t nthreads) {
  if (B < 0 || N < 0 || T < 0) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || box_idx == nullptr || (B > 0 && pts_batch_cnt == nullptr) || (B > 0 && T > 0 && boxes == nullptr)) return GD3D_E_BADARG;
  return first_box(points, pts_batch_cnt, boxes, nullptr, box_cnt, B, N, T, false, 0.0f, 0, nullptr, box_idx, nthreads);
}

int gd3d_pib_mask_targets_cpu(const float* points, const int32_t* pts_batch_cnt, const float* gt_boxes, const int64_t* gt_labels,
                              const int32_t* box_cnt, int32_t B, int64_t N, int32_t T, float extra_width, int32_t num_classes,
                              int64_t* seg_targets, int32_t* box_idx, int32_t nthreads) {
  if (B < 0 || N < 0 || T < 0) return GD3D_E_BADARG;
  if (N == 0) return 0;
  if (points == nullptr || seg_targets == nullptr || (B > 0 && pts_batch_cnt == nullptr)) return GD3D_E_BADARG;
  if (B > 0 && T > 0 && (gt_boxes == nullptr || gt_labels == nullptr)) return GD3D_E_BADARG;
  return first_box(points, pts_batch_cnt, gt_boxes, gt_labels, box_cnt, B, N, T, true, extra_width, num_classes, seg_targets, box_idx,
                   nthreads);
}

int gd3d_pib_all_cpu(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt, int32_t B,
                     int64_t N, int32_t T, void* flags, int32_t elem_size, int32_t nthreads) {
  if (B < 0 || N < 0 || T < 0 || (elem_size != 1 && elem_size != 4)) return GD3D_E_BADARG;
  if (N == 0 || T == 0) return 0;
  if (points == nullptr || flags == nullptr || (B > 0 && (pts_batch_cnt == nullptr || boxes == nullptr))) return GD3D_E_BADARG;
  bool ok = true;
  try {
    const std::vector<long long> start = segment_starts(pts_batch_cnt, B, N);
    const std::vector<SampleBoxes> sb = sample_boxes(boxes, box_cnt, B, T, false, 0.0f);
    ok = parallel_ranges(N, gd3d_host::team_size(nthreads, N, 64, 256), [&](int64_t n0, int64_t n1) {
      int b = 0;
      for (int64_t n = n0; n < n1; ++n) {
        while (b < B && n >= start[b + 1]) ++b;
        const float* p = points + n * 3;
        const int tb = b < B ? (int)sb[b].box.size() : 0;
        for (int t = 0; t < T; ++t) {
          const int f = t < tb && contains(sb[b].box[t], p[0], p[1], p[2]) ? 1 : 0;
          if (elem_size == 4)
            static_cast<int32_t*>(flags)[n * T + t] = f;
          else
            static_cast<uint8_t*>(flags)[n * T + t] = (uint8_t)f;
        }
      }
    });
  } catch (...) {
    ok = false;
  }
  return ok ? 0 : GD3D_E_HOST;
}

int gd3d_roi_grid_points_cpu(const float* rois, int32_t roi_stride, int32_t first_col, int64_t R, int32_t G, int32_t clockwise,
                             float* out, int32_t nthreads) {
  if (R < 0 || roi_stride < 7 || first_col < 0 || first_col + 7 > roi_stride || G < 1 || G > MAX_GRID) return GD3D_E_BADARG;
  if (R == 0) return 0;
  if (rois == nullptr || out == nullptr) return GD3D_E_BADARG;
  const int cw = clockwise != 0;
  const float g = (float)G;
  const bool ok = parallel_ranges(R, gd3d_host::team_size(nthreads, R, 64, 256), [&](int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r) {
      const RoiC k = roi_constants(rois + r * roi_stride + first_col);
      float* o = out + r * 3 * G * G * G;
      for (int i = 0; i < G; ++i)
        for (int j = 0; j < G; ++j)
          for (int kk = 0; kk < G; ++kk)
            for (int comp = 0; comp < 3; ++comp) *o++ = grid_coord(k, i, j, kk, g, cw, comp);
    }
  });
  return ok ? 0 : GD3D_E_HOST;
}

}  // extern "C"
