#!/usr/bin/env python3
"""The pillar encoders' point decoration on the GPU, us per call, each entry against the torch statements it replaces, in one process:

  point_voxel_stats   4 samples x 20 000 points, C = 4, 0.16 m pillars over KITTI's range, a `Scatter` built once outside the timing:
                        * the KITTI dv config's flags (cluster offset + centre offset) with the trailing column appended: 10 channels
                        * all six flags: 25 channels
                        * one skewed cloud: a quarter of the points moved into a single voxel (its one sub-wave walks 20 000 points)
  pillar_decorate     (16 000, 32, 4) with cluster + centre (KITTI hv: 10 channels) and (30 000, 20, 5) (nuScenes: 11 channels)

torch  = the reference's statements (voxel_encoders/utils.py:48-89 plus the cat of pillar_encoder.py:215-216; pillar_encoder.py:105-153)
         written out HERE over this package's own `Scatter` (reduce_mapback / mapback) and plain torch ops.  Checked against the op before
         it is timed: the stats bit for bit, the decoration to 1e-5 relative (torch's sum(1) chooses its own order).
The two sides are timed ALTERNATELY, in blocks of 10 calls: median and min of 100 hipEvent-timed calls per side after 20 warm-ups, host
glue included; the kernels one call launches come from torch.profiler, each duration the median over 5 profiled calls.
    python tests/perf/pillar_feat_time.py [--out profiles/r17_pillar_feat_time.txt]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402

WARM, ITERS, BLOCK = 20, 100, 10
B, N_PER = 4, 20000
KITTI = ((0.16, 0.16, 4.0), (0.0, -39.68, -3.0, 69.12, 39.68, 1.0))
NUS = ((0.2, 0.2, 8.0), (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0))
DV = dict(with_cluster_center=False, with_cluster_center_offset=True, with_covariance=False, with_voxel_center=False,
          with_voxel_point_count=False, with_voxel_center_offset=True)
ALL = {k: True for k in DV}


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternated(*sides):
    """-> [(median, min)] per side, the sides in alternating blocks"""
    for _ in range(WARM):
        for s in sides:
            s()
    torch.cuda.synchronize()
    t = [[] for _ in sides]
    for _ in range(ITERS // BLOCK):
        for i, s in enumerate(sides):
            t[i] += [one(s) for _ in range(BLOCK)]
    return [(round(statistics.median(x), 1), round(min(x), 1)) for x in t]


PROFILED = 5


def kernels(fn):
    """[(kernel name, device us)] of one call (memory copies not counted): the call is profiled PROFILED times, one call per profile, and
    each kernel's duration is the median over them (a single sample of a long kernel spreads by 20 %); the first profile's figures if
    the profiles do not list the same kernels; a string with the reason when the profiler is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(PROFILED):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            runs.append([(e.name, float(e.time_range.elapsed_us())) for e in prof.events()
                         if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()])
        if any([n for n, _ in r] != [n for n, _ in runs[0]] for r in runs):
            return runs[0]
        return [(n, statistics.median(r[i][1] for r in runs)) for i, (n, _) in enumerate(runs[0])]
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}'


def summary(k):
    if not isinstance(k, list):
        return dict(kernel_launches=k)
    return dict(kernel_launches=len(k), kernel_us=round(sum(d for _, d in k), 1))


def make_points(g):
    """a ground sheet seen from the origin: range 2 .. 68 m with density falling with range, +-45 degrees, z around -1.6 m"""
    out = []
    for _ in range(B):
        r = 2.0 + 66.0 * torch.rand(N_PER, generator=g) ** 2
        a = (torch.rand(N_PER, generator=g) - 0.5) * (math.pi / 2)
        z = -1.6 + 0.15 * torch.randn(N_PER, generator=g)
        out.append(torch.stack([r * torch.cos(a), r * torch.sin(a), z, torch.rand(N_PER, generator=g)], 1))
    return torch.cat(out, 0)


def stats_torch(features, sc, voxel_size, rng, flags):
    """the calculator's forward over our Scatter, then the cat with the trailing columns"""
    xyz = features[:, :3]
    parts = [xyz]
    if flags['with_cluster_center'] or flags['with_cluster_center_offset'] or flags['with_covariance']:
        centre = sc.reduce_mapback(xyz, 'mean')
        diff = xyz - centre
        if flags['with_cluster_center']:
            parts.append(centre)
        if flags['with_cluster_center_offset']:
            parts.append(diff)
        if flags['with_covariance']:
            parts.append(sc.reduce_mapback((diff[:, None, :] * diff[:, :, None]).reshape(-1, 9), 'mean'))
    if flags['with_voxel_center'] or flags['with_voxel_center_offset']:
        rows = sc.pts_coors
        cell = torch.stack([rows[:, -1 - k] * voxel_size[k] + (voxel_size[k] / 2 + rng[k]) for k in range(3)], dim=-1)
        if flags['with_voxel_center']:
            parts.append(cell)
        if flags['with_voxel_center_offset']:
            parts.append(xyz - cell)
    if flags['with_voxel_point_count']:
        parts.append(sc.mapback(sc.voxel_pts_counts.unsqueeze(-1)))
    return torch.cat([torch.cat(parts, dim=-1), features[:, 3:]], dim=-1)


def decorate_torch(features, num_points, coors, voxel_size, rng):
    """cluster offset, pillar-centre offset, cat, padding mask"""
    xyz = features[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / num_points.type_as(features).view(-1, 1, 1)
    centre = torch.zeros_like(xyz)
    for k in range(3):
        centre[:, :, k] = xyz[:, :, k] - (coors[:, 3 - k].to(features.dtype).unsqueeze(1) * voxel_size[k] + (voxel_size[k] / 2 + rng[k]))
    out = torch.cat([features, xyz - mean, centre], dim=-1)
    mask = num_points.unsqueeze(1) > torch.arange(features.size(1), device=features.device).unsqueeze(0)
    out *= mask.unsqueeze(-1).type_as(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_pillar_feat_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pillar_feat_time.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, warmups=WARM, timed_calls=ITERS, alternating_block=BLOCK,
                        torch_side='the reference\'s statements written out in this script over this package\'s Scatter')))
    vs, rng = KITTI
    points = make_points(torch.Generator().manual_seed(17)).to(dev)
    cnt = torch.full((B,), N_PER, dtype=torch.int32, device=dev)
    skewed = points.clone()
    quarter = torch.arange(N_PER, device=dev)                     # all of sample 0: one cell of one sample, a quarter of the batch
    skewed[quarter, :3] = torch.tensor([9.95, 0.03, -1.0], device=dev) + 0.1 * torch.rand((quarter.numel(), 3), device=dev)
    skewed[quarter, 3] = 0.5
    for name, pts, flags in (('KITTI dv config, 10 channels', points, DV), ('all six flags, 25 channels + 1', points, ALL),
                             ('skewed cloud, dv flags', skewed, DV), ('skewed cloud, all six flags', skewed, ALL)):
        sc = amd.Scatter(amd.dynamic_voxelize(pts, vs, rng, cnt))
        ours = lambda: amd.point_voxel_stats(pts, sc, vs, rng, append_features=True, **flags)          # noqa: E731
        theirs = lambda: stats_torch(pts, sc, vs, rng, flags)                                         # noqa: E731
        a, b = ours(), theirs()
        same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-5, equal_nan=True), 'the statements disagree with the op'
        (t_ours, t_theirs) = alternated(ours, theirs)
        k = kernels(ours)                                          # the summary and the listing below come from the same profiles
        say(json.dumps(dict(what=f'point_voxel_stats: {name}', points=pts.size(0), voxels=sc.voxel_coors.size(0), largest_voxel=int(sc.voxel_pts_counts.max()),
                            dropped=int((sc.pts_voxel_maps < 0).sum()), channels=a.size(1), bits_equal_to_the_statements=same,
                            ours=dict(us_median=t_ours[0], us_min=t_ours[1], **summary(k)),
                            torch_statements=dict(us_median=t_theirs[0], us_min=t_theirs[1], **summary(kernels(theirs))),
                            ratio_of_medians_statements_over_ours=round(t_theirs[0] / t_ours[0], 2))))
        if isinstance(k, list):
            say(json.dumps(dict(what=f'point_voxel_stats: {name}: kernels of one of our calls', kernels=[[n[:60], round(d, 1)] for n, d in k])))
    for name, (V, P, C), (vs, rng) in (('KITTI hv (16000, 32, 4)', (16000, 32, 4), KITTI), ('nuScenes (30000, 20, 5)', (30000, 20, 5), NUS)):
        g = torch.Generator().manual_seed(19)
        num = torch.randint(1, P + 1, (V,), generator=g).clamp(max=P).int()
        num[::3] = torch.randint(1, 4, (num[::3].numel(),), generator=g).int()                         # many pillars hold few points
        coors = torch.stack([torch.randint(0, 4, (V,), generator=g), torch.zeros(V, dtype=torch.int64), torch.randint(0, 400, (V,), generator=g),
                             torch.randint(0, 400, (V,), generator=g)], 1).int()
        lo, size = torch.tensor(rng[:3]), torch.tensor(vs)
        feats = torch.cat([(lo + (coors[:, [3, 2, 1]].float() + 0.5) * size)[:, None, :] + (torch.rand((V, P, 3), generator=g) - 0.5) * size,
                           torch.rand((V, P, C - 3), generator=g)], 2)
        feats = feats * (torch.arange(P)[None, :] < num[:, None])[:, :, None]                          # zero padding, as hard_voxelize leaves it
        feats, num, coors = feats.to(dev), num.to(dev), coors.to(dev)
        ours = lambda: amd.pillar_decorate(feats, num, coors, vs, rng, True, True, False)              # noqa: E731
        theirs = lambda: decorate_torch(feats, num, coors, vs, rng)                                   # noqa: E731
        a, b = ours(), theirs()
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-4), float((a - b).abs().max())
        (t_ours, t_theirs) = alternated(ours, theirs)
        say(json.dumps(dict(what=f'pillar_decorate: {name}', shape=[V, P, C], channels=a.size(2), filled_slots=int(num.sum()),
                            ours=dict(us_median=t_ours[0], us_min=t_ours[1], **summary(kernels(ours))),
                            torch_statements=dict(us_median=t_theirs[0], us_min=t_theirs[1], **summary(kernels(theirs))),
                            ratio_of_medians_statements_over_ours=round(t_theirs[0] / t_ours[0], 2))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
