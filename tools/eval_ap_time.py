#!/usr/bin/env python3
"""Times the flexible mAP's accumulate stage (mmdet3d_gaussian_amd.ap_accumulate, csrc/eval_ap.hip) and the whole evaluator.

`ap_accumulate` at 8 M rows, K = 12, T = 2 and at 32 M rows, K = 12, T = 10, device events around each call after a warm-up, against
  (a) a torch-op STAND-IN written here, on the same GPU — what a user has without the kernels: a stable sort on (group, -score), then
      per group and threshold a masked cumsum, the flipped cummax and a masked fp64 sum.  The two are timed in alternation;
  (b) the reference's literal numpy lines with mmdet's Python loop over every detection, on this host's CPU, at 1 M rows, one group
      and one threshold;
  (c) the bytes each phase must move over the copy rate measured in this process.
Then the whole evaluator on a synthetic KITTI-val-like set (3 769 frames, 3 classes, about 50 detections and 10 ground truths per
frame), on device tensors and on CPU tensors: wall time and launches per frame.  Report only.

    python tools/eval_ap_time.py [--out FILE] [--reps 7] [--frames 3769]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/eval_ap_time.py --profile-run     (a run of its own)
    python tools/eval_ap_time.py --kernel-stats DIR [--out FILE]      appends the per-phase kernel times of that run
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet3d_gaussian_amd as amd  # noqa: E402

SHAPES = ((8 << 20, 12, 2), (32 << 20, 12, 10))
PROFILE_CALLS = 4     # ap_accumulate calls of a --profile-run
PHASES = (('eval_ap::key_kernel(', 'keys'), ('rocprim', 'sort (rocPRIM)'), ('eval_ap::gather_kernel(', 'gather + tile counts'), ('eval_ap::carry_sum_kernel(', 'count carries'),
          ('eval_ap::max_kernel(', 'tile maxima'), ('eval_ap::carry_max_kernel(', 'envelope carries'), ('eval_ap::sum_kernel(', 'envelope + limb sums'),
          ('eval_ap::finish_kernel(', 'finish'))


def records(n, K, T, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    group = torch.randint(0, K, (n,), generator=g, device='cuda', dtype=torch.int32)
    score = torch.rand(n, generator=g, device='cuda')
    bits = lambda p: sum(((torch.rand(n, generator=g, device='cuda') < p).to(torch.int32) << t) for t in range(T))  # noqa: E731
    return group, score, bits(0.4), bits(0.85), torch.randint(1, max(2, n // K), (K,), generator=g, device='cuda')


def standin(group, score, tp, msk, num_gt, T):
    """torch ops only: the same numbers up to the order of the fp64 sum (ties broken by row order, as the kernels do)"""
    K = num_gt.numel()
    o1 = torch.sort(score, descending=True, stable=True).indices
    order = o1[torch.sort(group[o1], stable=True).indices]
    g, tp, msk = group[order], tp[order], msk[order]
    counts = torch.bincount(g.long(), minlength=K).tolist()
    ap = torch.zeros((K, T), dtype=torch.float64, device=group.device)
    at = 0
    for k in range(K):
        sl = slice(at, at + counts[k])
        at += counts[k]
        den = num_gt[k].double().clamp(min=1e-7)
        for t in range(T):
            m = ((msk[sl] >> t) & 1).bool()
            h = (((tp[sl] >> t) & 1).bool() & m)[m]
            c = torch.cumsum(h, 0)
            p = c.double() / torch.arange(1, c.numel() + 1, device=c.device, dtype=torch.float64)
            e = torch.cummax(p.flip(0), 0).values.flip(0)
            ap[k, t] = (e * h).sum() / den
    return ap


def literal_numpy(num_gt, score, tp, msk):
    """mean_ap_flexible.py:133-141 and mmdet's average_precision(mode='area') for one threshold, loop and all"""
    rank = score.argsort()[::-1]
    tpcumsum = tp[rank][msk[rank]].cumsum()
    recall = tpcumsum / max(num_gt, 1e-7)
    precision = tpcumsum / np.arange(1, len(tpcumsum) + 1)
    mrec = np.hstack((0.0, recall, 1.0))
    mpre = np.hstack((0.0, precision, 0.0))
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def copy_rate():
    """bytes read + written per second of a device copy of 1 GiB"""
    src = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = min(event_ms(lambda: dst.copy_(src)) for _ in range(5))
    return 2 * src.numel() / (ms * 1e-3)


def phase_bytes(n, K, T):
    """what each phase reads + writes, from the shapes (the sort: rocPRIM's radix passes of 8 bits over 32 + bits(K) key bits)"""
    passes = -(-(32 + int(K).bit_length()) // 8)
    tiles = -(-n // 1024)
    return (('keys', n * (4 + 4) + n * (8 + 4)), ('sort (rocPRIM)', passes * 2 * n * 12), ('gather + tile counts', n * 12 + n * 8 + n * 12),
            ('tile maxima', n * 12 + tiles * T * 16), ('envelope + limb sums', n * 12 + tiles * T * (16 + 32)))


def synthetic_dataset(frames, seed=0):
    rng = np.random.default_rng(seed)
    det_results, annotations = [], []
    for _ in range(frames):
        G = int(rng.integers(5, 16))
        gt = np.concatenate([rng.uniform(-60, 60, (G, 2)), rng.uniform(-1.5, 0.5, (G, 1)), rng.uniform(1.2, 4.5, (G, 3)),
                             rng.uniform(-3.1, 3.1, (G, 1))], 1).astype(np.float32)
        labels = rng.integers(0, 3, G)
        annotations.append(dict(gt_bboxes=gt, gt_labels=labels, gt_attrs=dict(ignore=rng.uniform(0, 1, G) < 0.1)))
        frame = []
        for c in range(3):
            hit = gt[labels == c].copy()
            hit[:, :2] += rng.normal(0, 0.2, (len(hit), 2))
            fp = np.concatenate([rng.uniform(-60, 60, (14, 2)), rng.uniform(-1.5, 0.5, (14, 1)), rng.uniform(1.2, 4.5, (14, 3)),
                                 rng.uniform(-3.1, 3.1, (14, 1))], 1)
            boxes = np.concatenate([hit, fp]).astype(np.float32)
            frame.append(np.concatenate([boxes, rng.uniform(0, 1, (len(boxes), 1)).astype(np.float32)], 1))
        det_results.append(frame)
    return det_results, annotations


def count_launches(fn):
    """device kernels launched by fn, from torch's profiler (a run of its own, after the timed ones)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def kernel_stats(directory, say):
    rows = []
    for p in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        rows += list(csv.DictReader(open(p)))
    say(f'kernel time per phase (rocprofv3 --kernel-trace --stats, a run of its own: {SHAPES[1][0]} rows, K = {SHAPES[1][1]}, T = {SHAPES[1][2]})')
    for needle, label in PHASES:
        hit = [r for r in rows if needle in r['Name']]
        if hit:
            calls = sum(int(r['Calls']) for r in hit)
            total = sum(float(r['AverageNs']) * int(r['Calls']) for r in hit)
            say(f'  {label:24s} {len(hit):2d} kernel(s), {calls:5d} launches, {total / PROFILE_CALLS / 1e3:12.1f} us per ap_accumulate call')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            with open(args.out, 'a' if args.kernel_stats else 'w') as f:
                f.write('\n'.join(lines) + '\n')

    if args.kernel_stats:
        kernel_stats(args.kernel_stats, say)
        return finish()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    if args.profile_run:
        cols = records(*SHAPES[1])
        for _ in range(PROFILE_CALLS):
            amd.ap_accumulate(*cols, SHAPES[1][2])
        torch.cuda.synchronize()
        return

    say(f'flexible mAP, accumulate stage on {torch.cuda.get_device_name(0)}; device events, {args.reps} alternating repeats after warm-up')
    rate = copy_rate()
    say(f'device copy of 1 GiB: {rate / 1e12:.2f} TB/s read + written')
    for n, K, T in SHAPES:
        cols = records(n, K, T)
        native = lambda: amd.ap_accumulate(*cols, T)   # noqa: E731
        torch_way = lambda: standin(*cols, T)          # noqa: E731
        got, want = native()[2], torch_way()
        rel = ((got - want).abs() / want.abs().clamp(min=1e-300)).max().item()
        for _ in range(2):
            native()
            torch_way()
        torch.cuda.synchronize()
        tn, ts = [], []
        for _ in range(args.reps):
            tn.append(event_ms(native))
            ts.append(event_ms(torch_way))
        say(f'{n} rows, K = {K}, T = {T}:')
        say(f'  ap_accumulate       median {statistics.median(tn):9.3f} ms  (min {min(tn):.3f}, max {max(tn):.3f})')
        say(f'  torch-op stand-in   median {statistics.median(ts):9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f});  '
            f'stand-in / native = {statistics.median(ts) / statistics.median(tn):.2f};  largest relative difference of ap {rel:.1e}')
        total = 0
        for label, b in phase_bytes(n, K, T):
            total += b
            say(f'    bytes of {label:22s} {b / 1e6:10.1f} MB = {b / rate * 1e3:8.3f} ms at the copy rate')
        say(f'    all phases {total / 1e6:10.1f} MB = {total / rate * 1e3:8.3f} ms at the copy rate')
        del cols
        torch.cuda.empty_cache()
    # the literal loop on this host's CPU
    rng = np.random.default_rng(0)
    n = 1 << 20
    score, tp, msk = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n) < 0.4, rng.uniform(0, 1, n) < 0.85
    t0 = time.perf_counter()
    literal_numpy(n // 3, score, tp, msk)
    say(f'literal numpy lines with mmdet\'s loop, {n} rows, one group, one threshold, this host\'s CPU: {time.perf_counter() - t0:.2f} s')

    # the whole evaluator: bound by launches in its per-frame stage
    det, anno = synthetic_dataset(args.frames)
    kw = dict(match_thrs=[0.5, 0.7], breakdowns=[dict(type='RangeBreakdown', ranges={'0-30m': (0, 30), '30-50m': (30, 50), '50m+': (50, 1e9)})],
              classes=['Car', 'Pedestrian', 'Cyclist'], logger='silent')
    say(f'whole evaluator, {args.frames} frames x 3 classes, {sum(len(d) for f in det for d in f) / args.frames:.1f} detections and '
        f'{sum(len(a["gt_labels"]) for a in anno) / args.frames:.1f} ground truths per frame, 4 breakdown rows, 2 thresholds (report only):')
    for device in ('cuda', 'cpu'):
        torch.set_num_threads(16)
        tens = [[torch.from_numpy(d).to(device) for d in f] for f in det]
        amd.eval_map_flexible(tens[:50], anno[:50], **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        report = amd.eval_map_flexible(tens, anno, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        extra = ''
        if device == 'cuda':
            per = count_launches(lambda: amd.eval_map_flexible(tens[:64], anno[:64], **kw)) / 64
            extra = f', {per:.0f} kernel launches per frame (the per-frame stage is bound by launches, not by bytes)'
        say(f'  {device:4s} tensors{" (16 threads)" if device == "cpu" else ""}: {wall:7.2f} s wall, {wall / args.frames * 1e3:.2f} ms per frame, '
            f'map {float(report["map"]):.4f}{extra}')
    finish()


if __name__ == '__main__':
    main()
