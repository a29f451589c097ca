#!/usr/bin/env python3
"""Hard voxelization plus the mean voxel encoder (PVRCNN.voxelize + HardSimpleVFE, pv_rcnn.py:43-49, 66-86) on the GPU, us per call, at
two shapes: PV-RCNN's (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py: 4 samples x 20 000 points, C = 4, max_num_points 5,
max_voxels 16 000, voxel 0.05 x 0.05 x 0.1 over KITTI's range) and PointPillars' (the same points, 0.16 m pillars, max_num_points 32).
The points are synthetic: a ground sheet whose density falls with range, so that voxels near the sensor hold several points and far ones one.
ours   = amd.hard_voxelize(list of samples, with_mean=True): the whole batch in one call, with its one read-back of the total; also the
         static form (no read-back) and, for PV-RCNN, with_voxels=False (the mean without the (V, P, C) tensor).
torch  = a STAND-IN written here, NOT mmdet3d's op (which is CUDA-only and absent): per sample a key, torch.sort(stable), unique_consecutive,
         the rank of first appearance, masked scatters, then cat / pad and voxels.sum(1) / num_points — what a user could write with
         torch ops alone.  It is checked against the op before it is timed: voxels, coors and num_points exactly, the mean to 1e-6
         (torch's sum(1) chooses its own order).
The two sides are timed ALTERNATELY, in blocks of 10 calls: median and min of 100 hipEvent-timed calls per side after 20 warm-ups, host
glue included; the kernels one call launches and the sort's share of their time come from torch.profiler.  A last section times our
call on the same points under wider declared ranges, which changes nothing but the number of key bits handed to the radix sort.
    python tests/perf/pvrcnn_voxelize_time.py [--out profiles/r16_pvrcnn_voxelize_time.txt]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402

WARM, ITERS, BLOCK = 20, 100, 10
B, N_PER, C = 4, 20000, 4
SHAPES = (('pvrcnn', (0.05, 0.05, 0.1), (0.0, -40.0, -3.0, 70.4, 40.0, 1.0), 5, 16000),
          ('pointpillars', (0.16, 0.16, 4.0), (0.0, -39.68, -3.0, 69.12, 39.68, 1.0), 32, 16000))
SORT_WORDS = ('sort', 'radix', 'onesweep', 'histogram', 'merge')


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


def kernels(fn):
    """[(kernel name, device us)] of one call (memory copies not counted), or a string with the reason when the profiler is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [(e.name, float(e.time_range.elapsed_us())) for e in prof.events()
                if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}'


def summary(k):
    """launches, device us and the sort's share of them"""
    if not isinstance(k, list):
        return dict(kernel_launches=k)
    total = sum(d for _, d in k)
    sort = sum(d for n, d in k if any(w in n.lower() for w in SORT_WORDS))
    return dict(kernel_launches=len(k), kernel_us=round(total, 1), sort_kernel_us=round(sort, 1), sort_share=round(sort / total, 3) if total else None)


def make_points(g):
    """a ground sheet seen from the origin: range 2 .. 70 m with density falling with range, +-45 degrees, z around -1.6 m"""
    out = []
    for _ in range(B):
        r = 2.0 + 68.0 * torch.rand(N_PER, generator=g) ** 2
        a = (torch.rand(N_PER, generator=g) - 0.5) * (math.pi / 2)
        z = -1.6 + 0.15 * torch.randn(N_PER, generator=g)
        out.append(torch.stack([r * torch.cos(a), r * torch.sin(a), z, torch.rand(N_PER, generator=g)], 1))
    return out


def standin(points, voxel_size, rng, P, MV):
    """hard voxelization + mean with torch ops, sample by sample -> (voxels, coors, num_points, mean)"""
    dev = points[0].device
    vs, lo = torch.tensor(voxel_size, device=dev), torch.tensor(rng[:3], device=dev)
    gx, gy, gz = amd.voxelize.grid_size(voxel_size, rng)
    grid = torch.tensor([gx, gy, gz], device=dev, dtype=torch.float32)
    G = gx * gy * gz
    voxels, coors, nums = [], [], []
    for b, pts in enumerate(points):
        n = pts.size(0)
        f = torch.floor((pts[:, :3] - lo) / vs)
        kept = ((f >= 0) & (f < grid)).all(1)
        c = torch.where(kept[:, None], f, torch.zeros_like(f)).long()
        key = torch.where(kept, (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0], torch.full_like(c[:, 0], G))
        skey, order = torch.sort(key, stable=True)
        uniq, inv, counts = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
        starts = torch.cumsum(counts, 0) - counts
        slot = torch.arange(n, device=dev) - starts[inv]
        first = torch.where(uniq != G, order[starts], torch.full_like(starts, n))      # a cell's first point; the dropped bucket goes last
        rank = torch.empty_like(first)
        rank[torch.argsort(first)] = torch.arange(first.numel(), device=dev)
        cell_ok = (uniq != G) & (rank < MV)
        V = int(cell_ok.sum())                                                         # the stand-in's read-back
        ok = cell_ok[inv] & (slot < P)
        vox = torch.zeros((V, P, pts.size(1)), device=dev)
        vox[rank[inv][ok], slot[ok]] = pts[order[ok]]
        num = torch.zeros((V,), dtype=torch.int32, device=dev)
        num[rank[cell_ok]] = counts[cell_ok].clamp(max=P).int()
        zyx = torch.zeros((V, 3), dtype=torch.int32, device=dev)
        u = uniq[cell_ok]
        zyx[rank[cell_ok]] = torch.stack([u // (gx * gy), (u // gx) % gy, u % gx], 1).int()
        voxels.append(vox); nums.append(num); coors.append(F.pad(zyx, (1, 0), mode='constant', value=b))
    voxels, nums = torch.cat(voxels, 0), torch.cat(nums, 0)
    return voxels, torch.cat(coors, 0), nums, voxels.sum(1) / nums[:, None].float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_pvrcnn_voxelize_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pvrcnn_voxelize_time.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, samples=B, points_per_sample=N_PER, C=C, warmups=WARM,
                        timed_calls=ITERS, alternating_block=BLOCK, torch_side='a torch-op stand-in written in this script, not mmdet3d')))
    points = [p.to(dev) for p in make_points(torch.Generator().manual_seed(16))]
    for name, vs, rng, P, MV in SHAPES:
        ours = lambda: amd.hard_voxelize(points, vs, rng, P, MV, with_mean=True)                       # noqa: E731
        ours_static = lambda: amd.hard_voxelize(points, vs, rng, P, MV, with_mean=True, static=True)   # noqa: E731
        ours_lean = lambda: amd.hard_voxelize(points, vs, rng, P, MV, with_voxels=False, with_mean=True)   # noqa: E731
        theirs = lambda: standin(points, vs, rng, P, MV)                                               # noqa: E731
        a, b = ours(), theirs()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), 'the stand-in disagrees with the op'
        assert torch.allclose(a[4], b[3], rtol=1e-6, atol=1e-6), float((a[4] - b[3]).abs().max())
        say(json.dumps(dict(what=f'{name}: shape', voxel_size=vs, max_num_points=P, max_voxels=MV, voxels=a[0].size(0), voxels_per_sample=a[3].tolist(),
                            full_voxels=int((a[2] == P).sum()), points_kept=int(a[2].sum()), mean_bits_equal_to_stand_in=bool(torch.equal(a[4], b[3])))))
        del a, b
        sides = [ours, theirs, ours_static] + ([ours_lean] if name == 'pvrcnn' else [])
        times = alternated(*sides)
        labels = ['ours', 'torch_stand_in', 'ours_static_no_read_back', 'ours_mean_without_voxels']
        row = dict(what=f'{name}: hard voxelization + mean, us per call')
        for label, side, (med, mn) in zip(labels, sides, times):
            row[label] = dict(us_median=med, us_min=mn, **summary(kernels(side)))
        row['ratio_of_medians_stand_in_over_ours'] = round(times[1][0] / times[0][0], 2)
        say(json.dumps(row))
        k = kernels(ours)
        if isinstance(k, list):
            say(json.dumps(dict(what=f'{name}: kernels of one of our calls', kernels=[[n[:60], round(d, 1)] for n, d in k])))
    # the key bits handed to the radix sort: the same points and cells, a wider declared range (more cells along z, then along all axes)
    name, vs, rng, P, MV = SHAPES[0]
    lo, hi = torch.tensor(rng[:3], device=dev), torch.tensor(rng[3:], device=dev)
    inside = [p[((p[:, :3] >= lo) & (p[:, :3] < hi - 0.01)).all(1)] for p in points]      # a wider range must not let new points in
    want = amd.hard_voxelize(inside, vs, rng, P, MV, with_mean=True, static=True)
    rows = []
    for label, hi in (('as configured', rng[3:]), ('z axis 2^23 cells', (rng[3], rng[4], rng[2] + vs[2] * 2 ** 23)),
                      ('x, y 2^23 cells, z 2^13', (rng[0] + vs[0] * 2 ** 23, rng[1] + vs[1] * 2 ** 23, rng[2] + vs[2] * 2 ** 13))):
        wide = tuple(rng[:3]) + tuple(hi)
        gx, gy, gz = amd.voxelize.grid_size(vs, wide)
        bits = (B * gx * gy * gz).bit_length()
        call = lambda: amd.hard_voxelize(inside, vs, wide, P, MV, with_mean=True, static=True)         # noqa: E731
        assert all(torch.equal(x, y) for x, y in zip(call(), want)), 'the wider range changed the result'
        (med, mn), = alternated(call)
        rows.append(dict(declared_range=label, points=sum(p.size(0) for p in inside), key_bits=bits, us_median=med, us_min=mn, **summary(kernels(call))))
    say(json.dumps(dict(what='pvrcnn: our static call against the key bits of the sort (same points, same cells)', rows=rows)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
