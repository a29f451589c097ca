#!/usr/bin/env python3
"""Times the flexible mAP evaluator's per-frame stage, one frame at a time (frame_batch=0, `_frame_records`) against batches of frames
through `frames_records` (csrc/eval_frames.hip), in ONE process, on the synthetic KITTI-val-like set of tools/eval_ap_time.py
(3 769 frames, 3 classes, about 52 detections and 10 ground truths per frame, 4 breakdown rows, 2 thresholds; generated from a seed).

`statistics_eval` wall time ending in a device synchronise, on device tensors and on CPU tensors with 16 threads; frame_batch 0, 64,
512 and all frames in alternation, `--reps` repeats after a warm-up, the median with the spread of the repeats beside it.  The results
of every frame_batch are compared with frame_batch=0's.  Report only.

    python tools/eval_frames_time.py [--out FILE] [--reps 5] [--frames 3769]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/eval_frames_time.py --profile-run FRAME_BATCH
    python tools/eval_frames_time.py --kernel-stats DIR --label TEXT [--out FILE]     appends the launches per frame of that run
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet3d_gaussian_amd as amd  # noqa: E402
from eval_ap_time import synthetic_dataset  # noqa: E402

PROFILE_FRAMES = 512
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
RANGES = {'0-30m': (0, 30), '30-50m': (30, 50), '50m+': (50, 1e9)}


def evaluator():
    return amd.FlexibleStatisticsEval(CLASSES, [0.5, 0.7], [dict(type='RangeBreakdown', ranges=RANGES)], dict(type='LidarIOU3D'),
                                      dict(type='MatcherCoCo'), [], 0)


def timed(fse, tens, anno, frame_batch):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fse.statistics_eval(tens, anno, frame_batch=frame_batch)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1]['num_det'] == y[1]['num_det'] and x[1]['num_gt'] == y[1]['num_gt'] and
                                    float(x[1]['recall']) == float(y[1]['recall']) and float(x[1]['mAP']) == float(y[1]['mAP']) for x, y in zip(a, b))


def kernel_stats(directory, label, say):
    rows = []
    for p in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        rows += list(csv.DictReader(open(p)))
    calls = sum(int(r['Calls']) for r in rows)
    ours = sum(int(r['Calls']) for r in rows if 'eval_frames::' in r['Name'])
    say(f'launches (rocprofv3 --kernel-trace --stats, a run of its own: {PROFILE_FRAMES} frames, device tensors), {label}: {calls} kernel '
        f'launches = {calls / PROFILE_FRAMES:.1f} per frame, of which eval_frames kernels {ours}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--profile-run', type=int, default=None, metavar='FRAME_BATCH')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--label', default='')
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
        kernel_stats(args.kernel_stats, args.label, say)
        return finish()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    torch.set_num_threads(16)
    fse = evaluator()
    if args.profile_run is not None:
        det, anno = synthetic_dataset(PROFILE_FRAMES)
        tens = [[torch.from_numpy(d).cuda() for d in f] for f in det]
        fse.statistics_eval(tens, anno, frame_batch=args.profile_run)
        torch.cuda.synchronize()
        return
    det, anno = synthetic_dataset(args.frames)
    batches = (0, 64, 512, args.frames)
    say(f'flexible mAP evaluator, per-frame stage: frame_batch=0 (one frame at a time) against batches of frames, {torch.cuda.get_device_name(0)}')
    say(f'{args.frames} frames x 3 classes, {sum(len(d) for f in det for d in f) / args.frames:.1f} detections and '
        f'{sum(len(a["gt_labels"]) for a in anno) / args.frames:.1f} ground truths per frame, 4 breakdown rows, 2 thresholds, LidarIOU3D;')
    say(f'statistics_eval wall time ending in a device synchronise, one process, {args.reps} alternating repeats after a warm-up: median (min .. max)')
    medians = {}
    for device in ('cuda', 'cpu'):
        tens = [[torch.from_numpy(d).to(device) for d in f] for f in det]
        want = None
        for fb in batches:       # warm-up, and the results of every batch size against frame_batch=0
            _, res = timed(fse, tens[:600], anno[:600], fb)
            want = res if want is None else want
            assert same(res, want), f'frame_batch={fb} differs from frame_batch=0 on {device}'
        times = {fb: [] for fb in batches}
        for _ in range(args.reps):
            for fb in batches:
                times[fb].append(timed(fse, tens, anno, fb)[0])
        for fb in batches:
            t = times[fb]
            medians[device, fb] = statistics.median(t)
            say(f'  {device:4s} tensors{" (16 threads)" if device == "cpu" else "             "} frame_batch={fb:<5d} {statistics.median(t):7.3f} s '
                f'({min(t):.3f} .. {max(t):.3f}), {statistics.median(t) / args.frames * 1e3:6.3f} ms per frame')
        del tens
    say('results of every frame_batch equal frame_batch=0 bit for bit (checked on the first 600 frames, both devices)')
    best = min(batches[1:], key=lambda fb: medians['cuda', fb])
    say(f'device, frame_batch={best}: {medians["cuda", 0] / medians["cuda", best]:.2f}x the device path of frame_batch=0, '
        f'{medians["cpu", 0] / medians["cuda", best]:.2f}x the CPU-tensor per-frame run')
    finish()


if __name__ == '__main__':
    main()
