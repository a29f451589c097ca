#!/usr/bin/env python3
"""Times `VoxelQueryAndGroup` (mmdet3d_gaussian_amd.voxel_query, csrc/voxel_query.hip) against the existing `QueryAndGroup` on the
SAME voxel centres and queries, at the shapes of the reference's PV-RCNN KITTI config
(configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:75-91,147-154): B = 4, the x2 / x4 / x8 levels of the 41 x 1600 x 1408 grid
with 8192 / 4096 / 2048 voxels per sample and their `voxel_sa_configs` (radius, nsample) pairs, queried by 4 x 2048 keypoints, and
4 x 27 648 RoI-grid queries on the x4 level (C = 64).  max_range = ceil(radius / (voxel_size * scale)) per axis.

Both look-up forms are timed.  The dense form's time includes its table (fill + build) — it must be refilled on every step; the sorted
form's index build is listed apart (one build serves every query of a level).  Outputs are NOT compared: the order (window order
against ascending index) and the equality rule (inclusive against strict) differ; tests/test_*_voxel_query.py hold the member sets to
each other.  One process; device events around `reps` back-to-back calls after a warm-up; `rounds` rounds that alternate the forms,
reported as the lowest-highest round mean.
    python tools/voxel_query_time.py [--out FILE] [--reps 100] [--rounds 3]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdet3d_gaussian_amd as amd  # noqa: E402

B, KEYPOINTS, ROI_QUERIES = 4, 2048, 128 * 216
VOXEL_SIZE, PC_RANGE, GRID = (0.05, 0.05, 0.1), (0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (41, 1600, 1408)
# name, scale, voxels per sample, C, ((radius, nsample), ...), queries per sample
LEVELS = (('x2', 2, 8192, 32, ((0.8, 16), (1.2, 32)), KEYPOINTS),
          ('x4', 4, 4096, 64, ((1.2, 16), (2.4, 32)), KEYPOINTS),
          ('x8', 8, 2048, 64, ((2.4, 16), (4.8, 32)), KEYPOINTS),
          ('roi_x4', 4, 4096, 64, ((1.2, 16), (2.4, 32)), ROI_QUERIES))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps       # us per call


def cloud(n, gen):
    """points as a KITTI sweep lies: x 0..70.4, y -40..40, z -3..1, denser near the sensor"""
    r = torch.rand(n, generator=gen, device='cuda') ** 1.5 * 70.4
    y = (torch.rand(n, generator=gen, device='cuda') * 2 - 1) * torch.clamp(r * 0.8, max=40.0)
    z = torch.rand(n, generator=gen, device='cuda') * 4 - 3
    return torch.stack((r, y, z), 1).contiguous()


def level_voxels(raw, scale, n_per, shape):
    """the first n_per occupied cells of every sample's sweep at this level -> coors (B * n_per, 4) int32 and their centres"""
    cell = [v * scale for v in VOXEL_SIZE]
    coors = []
    for b, pts in enumerate(raw):
        c = torch.stack([((pts[:, 2] - PC_RANGE[2]) / cell[2]).floor(), ((pts[:, 1] - PC_RANGE[1]) / cell[1]).floor(),
                         ((pts[:, 0] - PC_RANGE[0]) / cell[0]).floor()], 1).long()
        for a in range(3):
            c[:, a].clamp_(0, shape[a] - 1)
        c = torch.unique(c, dim=0)
        c = c[torch.randperm(c.size(0), device='cuda')[:n_per]]
        assert c.size(0) == n_per, (b, c.size(0), n_per)
        coors.append(torch.cat([torch.full((n_per, 1), b, device='cuda'), c], 1))
    coors = torch.cat(coors).to(torch.int32).contiguous()
    centres = torch.stack([(coors[:, 3] + 0.5) * cell[0] + PC_RANGE[0], (coors[:, 2] + 0.5) * cell[1] + PC_RANGE[1],
                           (coors[:, 1] + 0.5) * cell[2] + PC_RANGE[2]], 1).float().contiguous()
    return coors, centres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('voxel_query_time.py measures on the GPU: no device found')
    gen = torch.Generator(device='cuda').manual_seed(0)
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; B = {B}; us per call, mean of {args.reps} back-to-back calls, '
        f'lowest-highest of {args.rounds} alternating rounds')
    raw = [cloud(16384 * 8, gen) for _ in range(B)]
    flat = torch.cat([r[:16384] for r in raw]).contiguous()
    cnt_raw = torch.full((B,), 16384, dtype=torch.int32, device='cuda')
    picks = amd.furthest_point_sample_stacked(flat, cnt_raw, KEYPOINTS)
    keypoints = torch.cat([raw[b][:16384][picks[b]] for b in range(B)]).contiguous()
    say(f'{"level":8}{"N/sample":>9}{"M/sample":>9}{"C":>4}{"radius":>7}{"ns":>4}{"max_range":>12} | {"index":>7} | {"sorted fwd":>13}{"dense fwd+table":>17}'
        f'{"QueryAndGroup":>15} | {"QAG/sorted":>11}{"QAG/dense":>10} | {"empty":>6}{"full":>6}   (us)')
    for name, scale, n_per, c, pairs, m_per in LEVELS:
        shape = tuple(math.ceil(g / scale) for g in GRID)
        coors, centres = level_voxels(raw, scale, n_per, shape)
        if m_per == KEYPOINTS:
            qry = keypoints
        else:        # RoI grid points around the keypoints
            sel = torch.randint(0, KEYPOINTS, (B, m_per), generator=gen, device='cuda') + torch.arange(B, device='cuda')[:, None] * KEYPOINTS
            qry = (keypoints[sel.reshape(-1)] + torch.randn(B * m_per, 3, generator=gen, device='cuda') * 0.5).contiguous()
        pc = torch.full((B,), n_per, dtype=torch.int32, device='cuda')
        qc = torch.full((B,), m_per, dtype=torch.int32, device='cuda')
        feats = torch.randn(B * n_per, c, generator=gen, device='cuda')
        nc = amd.voxel_query_coords(qry, qc, VOXEL_SIZE, PC_RANGE, scale)
        index = amd.voxel_query_index(coors, shape, B)
        index_us = timed(lambda: amd.voxel_query_index(coors, shape, B), args.reps)
        for radius, ns in pairs:
            rng = tuple(math.ceil(radius / (VOXEL_SIZE[a] * scale) - 1e-9) for a in (2, 1, 0))
            vq = amd.VoxelQueryAndGroup(rng, radius, ns)
            qag = amd.QueryAndGroup(radius, ns)
            with torch.no_grad():
                forms = (lambda: vq(centres, qry, nc, index, feats),
                         lambda: vq(centres, qry, nc, amd.voxel_point_indices(coors, shape, B), feats),
                         lambda: qag(centres, pc, qry, qc, feats))
                us = [[timed(f, args.reps) for f in forms] for _ in range(args.rounds)]
                _, mask, cnt = amd.voxel_query(rng, radius, ns, centres, qry, nc, index, return_cnt=True)
            lo = [min(r[k] for r in us) for k in range(3)]
            hi = [max(r[k] for r in us) for k in range(3)]
            mean = [sum(r[k] for r in us) / len(us) for k in range(3)]
            span = lambda k: f'{lo[k]:.1f}-{hi[k]:.1f}'
            say(f'{name:8}{n_per:9d}{m_per:9d}{c:4d}{radius:7.1f}{ns:4d}{str(rng):>12} | {index_us:7.1f} | {span(0):>13}{span(1):>17}{span(2):>15} | '
                f'{mean[2] / mean[0]:10.2f}x{mean[2] / mean[1]:9.2f}x | {float(mask.float().mean()):6.2f}{float((cnt == ns).float().mean()):6.2f}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
