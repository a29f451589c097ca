#!/usr/bin/env python3
"""Times the point-in-box ops (mmdet3d_gaussian_amd.points_in_boxes, csrc/pib.hip) at the shapes their users in the reference have:
  part, mask_targets : PV-RCNN's keypoints, 8 samples x 2048 against 8 x 64 GT boxes (pointwise_mask_head.py:62-92);
  all (bool, int32)  : SimOTA's 219 024 BEV priors against 64 GT boxes made infinitely tall (sim_ota_3d_assigner.py:158-182);
  roi_grid_points    : 8 x 128 RoIs at grid size 6 (batch_roigrid_extractor.py:56-71).
One process, device events around `reps` back-to-back calls after a warm-up.

Each op is compared with a plain-torch formulation of the same op on the same GPU — what a user has without these kernels (the
third-party CUDA ops have no ROCm build): a broadcast (N, T) evaluation of the membership test, argmax for `part`, the reference's
per-sample loop for the mask targets, and the reference's nonzero / repeat / rotate chain for the grid points.  `all` is also
compared with its bytes floor, N * T * sizeof(element) written at the copy rate measured in this process.
    python tools/pib_time.py [--out FILE] [--reps 50]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet3d_gaussian_amd as amd  # noqa: E402
from vsa_time import timed  # noqa: E402

B, KEYPOINTS, GT, PRIORS, ROIS, GRID, CLASSES = 8, 2048, 64, 219024, 128, 6, 3


def torch_inside(p, boxes):
    """p (N, 3), boxes (T, 7) -> (N, T) bool"""
    hz = boxes[:, 5] * 0.5
    in_z = (p[:, None, 2] - (boxes[:, 2] + hz)[None]).abs() <= hz[None]
    c, s = torch.cos(-boxes[:, 6]), torch.sin(-boxes[:, 6])
    sx, sy = p[:, None, 0] - boxes[None, :, 0], p[:, None, 1] - boxes[None, :, 1]
    lx = sx * c[None] - sy * s[None]
    ly = sx * s[None] + sy * c[None]
    return in_z & (lx.abs() < boxes[None, :, 3] * 0.5) & (ly.abs() < boxes[None, :, 4] * 0.5)


def torch_part(p, boxes):
    m = torch_inside(p, boxes)
    return torch.where(m.any(1), m.int().argmax(1), -1)


def torch_mask_targets(xyz, n_per, boxes, labels, w):
    out = []
    for b in range(B):
        p = xyz[b * n_per:(b + 1) * n_per]
        big = boxes[b].clone()
        big[:, 3:6] += 2 * w
        big[:, 2] -= w
        i, e = torch_part(p, boxes[b]), torch_part(p, big)
        seg = torch.nn.functional.pad(labels[b], (1, 0), value=CLASSES)[i + 1]
        seg[(i >= 0) ^ (e >= 0)] = -1
        out.append(seg)
    return torch.cat(out)


def torch_grid_points(rois, g):
    """the reference's chain: nonzero of a ones grid, repeat, scale by the RoI size, shift, rotate about z, move"""
    r = rois.shape[0]
    idx = torch.ones((g, g, g), device=rois.device).nonzero().repeat(r, 1, 1).float()
    size = rois[:, 3:6]
    pts = (idx + 0.5) / g * size[:, None, :] - size[:, None, :] / 2
    pts[..., 2] += size[:, None, 2] / 2
    c, s = torch.cos(rois[:, 6])[:, None], torch.sin(rois[:, 6])[:, None]
    x = pts[..., 0] * c - pts[..., 1] * s
    y = pts[..., 0] * s + pts[..., 1] * c
    return torch.stack((x, y, pts[..., 2]), -1) + rois[:, None, :3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pib_time.py measures on the GPU: no device found')
    gen = torch.Generator(device='cuda').manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rand(*shape, lo=0.0, hi=1.0):
        return torch.rand(*shape, generator=gen, device='cuda') * (hi - lo) + lo

    say(f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; us per call, mean of {args.reps} back-to-back calls')
    big = torch.empty(512 << 20, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(big)
    copy_us = timed(lambda: dst.copy_(big), 10)
    rate = 2 * big.numel() / (copy_us * 1e-6)
    say(f'# copy rate (512 MiB read + 512 MiB written): {rate / 1e12:.2f} TB/s')
    del big, dst

    def gt_boxes(b, t):   # KITTI-like scene: x 0..70, y -40..40
        return torch.cat([rand(b, t, 1, lo=0, hi=70), rand(b, t, 1, lo=-40, hi=40), rand(b, t, 1, lo=-2.5, hi=-0.5),
                          rand(b, t, 1, lo=1.5, hi=4.5), rand(b, t, 1, lo=0.6, hi=2.0), rand(b, t, 1, lo=1.4, hi=2.0),
                          rand(b, t, 1, lo=-3.14, hi=3.14)], 2).contiguous()

    say(f'\n## keypoints: {B} x {KEYPOINTS} points against {B} x {GT} GT boxes (a third of the keypoints drawn inside a box)')
    boxes = gt_boxes(B, GT)
    labels = torch.randint(0, CLASSES, (B, GT), generator=gen, device='cuda')
    xyz = torch.cat([rand(B * KEYPOINTS, 1, lo=0, hi=70), rand(B * KEYPOINTS, 1, lo=-40, hi=40), rand(B * KEYPOINTS, 1, lo=-3, hi=1)], 1)
    pick = torch.randint(0, GT, (B, KEYPOINTS // 3), generator=gen, device='cuda')
    for b in range(B):
        xyz[b * KEYPOINTS:b * KEYPOINTS + KEYPOINTS // 3] = boxes[b, pick[b], :3] + rand(KEYPOINTS // 3, 3, lo=-0.3, hi=0.3) + \
            torch.tensor([0, 0, 0.8], device='cuda')
    xyz = xyz.contiguous()
    pc = torch.full((B,), KEYPOINTS, dtype=torch.int32, device='cuda')
    us = timed(lambda: amd.points_in_boxes_part_stacked(xyz, pc, boxes), args.reps)
    t_us = timed(lambda: [torch_part(xyz[b * KEYPOINTS:(b + 1) * KEYPOINTS], boxes[b]) for b in range(B)], args.reps)
    got = amd.points_in_boxes_part_stacked(xyz, pc, boxes)
    ref = torch.cat([torch_part(xyz[b * KEYPOINTS:(b + 1) * KEYPOINTS], boxes[b]) for b in range(B)])
    say(f'part                   {us:10.1f} us   plain torch (per-sample broadcast) {t_us:10.1f} us   x{t_us / us:.1f}'
        f'   ({int((got >= 0).sum())} of {got.numel()} points in a box; {int((got != ref).sum())} differ from the torch formulation)')
    us = timed(lambda: amd.pointwise_mask_targets(xyz, pc, boxes, labels, 0.2, CLASSES), args.reps)
    t_us = timed(lambda: torch_mask_targets(xyz, KEYPOINTS, boxes, labels, 0.2), max(2, args.reps // 5))
    seg = amd.pointwise_mask_targets(xyz, pc, boxes, labels, 0.2, CLASSES)
    differ = int((seg != torch_mask_targets(xyz, KEYPOINTS, boxes, labels, 0.2)).sum())
    say(f'mask_targets           {us:10.1f} us   plain torch (reference chain)      {t_us:10.1f} us   x{t_us / us:.1f}'
        f'   ({int((seg == -1).sum())} ignore, {int((seg < CLASSES).sum() - (seg == -1).sum())} foreground; {differ} differ)')

    say(f'\n## SimOTA: {PRIORS} BEV priors against {GT} GT boxes with z = -1e8, dz = 2e8;  floor = N * T * sizeof(element) at the copy rate')
    tall = gt_boxes(1, GT)
    tall[..., 2], tall[..., 5] = -1e8, 2e8
    pri = torch.cat([rand(PRIORS, 1, lo=0, hi=70), rand(PRIORS, 1, lo=-40, hi=40), torch.zeros(PRIORS, 1, device='cuda')], 1).contiguous()
    pcnt = torch.full((1,), PRIORS, dtype=torch.int32, device='cuda')
    t_us = timed(lambda: torch_inside(pri, tall[0]), max(2, args.reps // 5))
    ref = torch_inside(pri, tall[0])
    for dtype, size in ((torch.bool, 1), (torch.int32, 4)):
        us = timed(lambda: amd.points_in_boxes_all_stacked(pri, pcnt, tall, dtype=dtype), args.reps)
        got = amd.points_in_boxes_all_stacked(pri, pcnt, tall, dtype=dtype)
        floor = PRIORS * GT * size / rate * 1e6      # the copy rate counts bytes read + written: the flags are bytes written
        say(f'all {str(dtype)[6:]:6}             {us:10.1f} us   plain torch (broadcast, bool)      {t_us:10.1f} us   x{t_us / us:.1f}'
            f'   floor {floor:6.1f} us = {floor / us:.0%} of the time   ({int((got.bool() != ref).sum())} of {got.numel()} flags differ)')

    say(f'\n## RoI grid points: {B} x {ROIS} RoIs, grid {GRID}')
    rois = gt_boxes(1, B * ROIS)[0]
    us = timed(lambda: amd.roi_grid_points(rois, GRID), args.reps)
    t_us = timed(lambda: torch_grid_points(rois, GRID), args.reps)
    err = float((amd.roi_grid_points(rois, GRID) - torch_grid_points(rois, GRID)).abs().max())
    out_bytes = B * ROIS * GRID ** 3 * 12
    say(f'roi_grid_points        {us:10.1f} us   plain torch (reference chain)      {t_us:10.1f} us   x{t_us / us:.1f}'
        f'   floor {out_bytes / rate * 1e6:5.1f} us   (max |difference| {err:.2e})')
    r8 = torch.cat([torch.arange(B, device='cuda').repeat_interleave(ROIS)[:, None].float(), rois], 1)
    us = timed(lambda: amd.roi_grid_queries(r8, B, GRID), args.reps)
    say(f'roi_grid_queries       {us:10.1f} us   (grid points + the device-side counts)')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
