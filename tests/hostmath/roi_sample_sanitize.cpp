// roi_sample_sanitize.cpp — a stand-alone driver (its own main) for the `_cpu` twins of the RoI assign-and-sample stage
// (mmdet3d-gaussian_amd/csrc/roi_sample_cpu.cpp), meant to be compiled TOGETHER with that file under -fsanitize=address,undefined
// and run as a program on a CPU-only machine (tests/test_cpu_pvrcnn_sample.py does so): nothing here is loaded into Python, nothing
// touches a GPU.  It reads one case as flat text (counts, thresholds, then every operand; fp32 values as their bit patterns), runs
// gd3d_roi_iou3d_cpu per sample and gd3d_roi_assign_sample_cpu on the batch into EXACTLY sized heap buffers — so a write past any
// output is a report — and prints a checksum per integer output for the test to compare with the restatement's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <vector>

#include "../../include/gd3d.h"

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }   // no slack behind the last element

template <typename T>
static std::unique_ptr<T[]> read_ints(std::istream& in, size_t n) {
  auto p = exact<T>(n);
  for (size_t i = 0; i < n; ++i) {
    long long v;
    in >> v;
    p[i] = (T)v;
  }
  return p;
}

static std::unique_ptr<float[]> read_bits(std::istream& in, size_t n) {
  auto p = exact<float>(n);
  for (size_t i = 0; i < n; ++i) {
    unsigned long long v;
    in >> v;
    const uint32_t b = (uint32_t)v;
    std::memcpy(&p[i], &b, 4);
  }
  return p;
}

template <typename T>
static std::unique_ptr<T[]> read_reals(std::istream& in, size_t n) {
  auto p = exact<T>(n);
  for (size_t i = 0; i < n; ++i) {
    double v;
    in >> v;
    p[i] = (T)v;
  }
  return p;
}

template <typename T>
static long long checksum(const T* v, size_t n) {
  long long s = 0;
  for (size_t i = 0; i < n; ++i) s += ((long long)v[i] + 2) * (long long)(i % 1009 + 1);
  return s;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  long long B, N, G, C, num, npos, K;
  in >> B >> N >> G >> C >> num >> npos >> K;
  if (!in || B < 1) return 2;
  auto pcnt = read_ints<int32_t>(in, (size_t)B), gcnt = read_ints<int32_t>(in, (size_t)B);
  auto pos = read_reals<float>(in, (size_t)C), neg = read_reals<float>(in, (size_t)C), low = read_reals<float>(in, (size_t)C);
  auto flags = read_ints<int32_t>(in, (size_t)C);
  auto fracs = read_reals<double>(in, (size_t)K);
  auto thrs = read_reals<float>(in, (size_t)K);
  auto props = read_bits(in, (size_t)N * 7);
  auto plab = read_ints<int64_t>(in, (size_t)N);
  auto gts = read_bits(in, (size_t)G * 7);
  auto glab = read_ints<int64_t>(in, (size_t)G);
  auto keys = read_bits(in, (size_t)N);
  auto fill = read_bits(in, (size_t)(B * num));
  if (!in) return 2;

  long long iou_bits = 0, p0 = 0, g0 = 0;
  for (long long b = 0; b < B; ++b) {
    const size_t n = (size_t)pcnt[b], g = (size_t)gcnt[b];
    auto iou = exact<float>(n * g);
    if (gd3d_roi_iou3d_cpu(props.get() + p0 * 7, (int64_t)n, gts.get() + g0 * 7, (int64_t)g, iou.get()) != 0) return 1;
    for (size_t i = 0; i < n * g; ++i) {
      int32_t bits;
      std::memcpy(&bits, &iou[i], 4);
      iou_bits += bits;
    }
    p0 += (long long)n;
    g0 += (long long)g;
  }

  const size_t R = (size_t)(B * num), Q = (size_t)(B * npos);
  auto rois = exact<float>(R * 8), ious = exact<float>(R), pb = exact<float>(Q * 7), pg = exact<float>(Q * 7), mo = exact<float>((size_t)N);
  auto inds = exact<int64_t>(R), pgi = exact<int64_t>(Q), gi = exact<int64_t>((size_t)N), labels = exact<int64_t>((size_t)N);
  auto pc = exact<int32_t>((size_t)B), rc = exact<int32_t>((size_t)B), stage = exact<int32_t>((size_t)(B * (2 + num)));
  for (int round = 0; round < 2; ++round) {   // the second round with counts that overrun the rows: clamped, nothing beyond the buffers
    if (round == 1) {
      pcnt[B - 1] += 1000;
      gcnt[B - 1] += 1000;
    }
    const int rcode = gd3d_roi_assign_sample_cpu(props.get(), plab.get(), pcnt.get(), N, gts.get(), glab.get(), gcnt.get(), G, (int32_t)B, keys.get(),
                                                 fill.get(), (int32_t)C, pos.get(), neg.get(), low.get(), flags.get(), (int32_t)num, (int32_t)npos,
                                                 (int32_t)K, fracs.get(), thrs.get(), rois.get(), ious.get(), inds.get(), pb.get(), pg.get(),
                                                 pgi.get(), pc.get(), rc.get(), gi.get(), mo.get(), labels.get(), stage.get());
    if (rcode != 0) {
      std::printf("status rc=%d\n", rcode);
      return 1;
    }
    if (round == 0) {
      std::printf("inds %lld\npos_assigned_gt_inds %lld\npos_batch_cnt %lld\nroi_batch_cnt %lld\ngt_inds %lld\nlabels %lld\niou_bits %lld\n",
                  checksum(inds.get(), R), checksum(pgi.get(), Q), checksum(pc.get(), (size_t)B), checksum(rc.get(), (size_t)B),
                  checksum(gi.get(), (size_t)N), checksum(labels.get(), (size_t)N), iou_bits);
    }
  }
  std::printf("status OK\n");
  return 0;
}
