#!/usr/bin/env python3
"""The multi-view pillar encoder's view ops on the GPU, us per call, each entry against the torch statements it replaces, in one process,
at the shipped config's shape (configs/_base_/models/pillarmvf_*_kitti.py): 4 samples x 20 000 points, C = 4, 64 feature channels, the
cartesian map 496 x 432 cells, the cylindrical map 100 x 1264.

  multi_view_voxelize   the config's two views ['cartesian', 'cylindrical'] from the per-sample list
  pillar_scatter        the pillars of each view onto its canvas, forward and forward + backward, contiguous NCHW and channels last
  view_sample           every point of the batch on each view's map, forward and forward + backward, in both layouts; the NCHW backward
                        in both of its forms (straight atomics; a channels-last workspace plus one transpose)

torch  = the reference's statements as tests/view_net_ref.py restates them (voxelize_view over the dynamic voxelizer written in torch,
         mmdet3d's PointPillarsScatter, the per-sample grid_sample loop with its torch.where host sync): what a user of the parent
         commit runs.  Each is checked against the op before it is timed.
The two sides are timed ALTERNATELY, in blocks of 10 calls: median and min of 100 hipEvent-timed calls per side after 20 warm-ups, host
glue included; the kernels one call launches come from torch.profiler, each duration the median over 5 profiled calls.
    python tests/perf/view_net_time.py [--out profiles/r18_view_net_time.txt]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
import view_net_ref as ref  # noqa: E402
from mmdet3d_gaussian_amd import view_net  # noqa: E402

WARM, ITERS, BLOCK = 20, 100, 10
B, N_PER, C_FEAT = 4, 20000, 64
VIEWS = ('cartesian', 'cylindrical')
ATOMIC_RATE = 1.3e12        # bytes per second of float atomic adds, chip-wide (the rate DESIGN.md §3.16 budgets with)


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
    """[(kernel name, device us)] of one call (memory copies not counted), each duration the median over PROFILED profiled calls; the
    first profile's figures if the profiles do not list the same kernels; a string with the reason when the profiler is unavailable"""
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
    return out


def entry(say, what, ours, theirs, extra=None):
    (t_ours, t_theirs) = alternated(ours, theirs)
    k = kernels(ours)
    say(json.dumps(dict(what=what, **(extra or {}), ours=dict(us_median=t_ours[0], us_min=t_ours[1], **summary(k)),
                        torch_statements=dict(us_median=t_theirs[0], us_min=t_theirs[1], **summary(kernels(theirs))),
                        ratio_of_medians_statements_over_ours=round(t_theirs[0] / t_ours[0], 2))))
    if isinstance(k, list):
        say(json.dumps(dict(what=f'{what}: kernels of one of our calls', kernels=[[n[:60], round(d, 1)] for n, d in k])))
    return t_ours[0], t_theirs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_view_net_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('view_net_time.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, warmups=WARM, timed_calls=ITERS, alternating_block=BLOCK,
                        torch_side='the reference\'s statements as tests/view_net_ref.py restates them')))
    sizes, ranges = [ref.GEOMETRY[v][0] for v in VIEWS], [ref.GEOMETRY[v][1] for v in VIEWS]
    shapes = [(math.ceil((r[4] - r[1]) / s[1]), math.ceil((r[3] - r[0]) / s[0])) for s, r in zip(sizes, ranges)]
    assert shapes == [(496, 432), (100, 1264)], shapes
    points = [p.to(dev) for p in make_points(torch.Generator().manual_seed(18))]
    voxelizers = [ref.dynamic_voxelizer(s, r) for s, r in zip(sizes, ranges)]

    ours = lambda: amd.multi_view_voxelize(points, VIEWS, sizes, ranges)                                          # noqa: E731
    theirs = lambda: [ref.voxelize_view(v, vox, points) for v, vox in zip(VIEWS, voxelizers)]                     # noqa: E731
    (mp, mc), want = ours(), theirs()
    for i in range(len(VIEWS)):
        assert torch.allclose(mp[i], want[i][0], rtol=1e-5, atol=1e-5)
        differ = int((mc[i] != want[i][1]).any(dim=1).sum())                  # a point within an ulp of a cell face may fall either side
        assert differ <= 8, differ
    entry(say, 'multi_view_voxelize: cartesian + cylindrical, per-sample list', ours, theirs, dict(points=B * N_PER, views=list(VIEWS)))

    g = torch.Generator().manual_seed(19)
    for i, view in enumerate(VIEWS):
        H, W = shapes[i]
        sc = amd.Scatter(mc[i])
        vcoors = sc.voxel_coors
        V = vcoors.size(0)
        feats = torch.randn(V, C_FEAT, generator=g).to(dev).requires_grad_(True)
        gcanvas = torch.randn(B, C_FEAT, H, W, generator=g).to(dev)
        theirs_f = lambda: ref.pillars_scatter(feats, vcoors, B, H, W)                                           # noqa: E731
        theirs_fb = lambda: torch.autograd.grad(ref.pillars_scatter(feats, vcoors, B, H, W), feats, gcanvas)      # noqa: E731
        for last in (False, True):
            gl = gcanvas.contiguous(memory_format=torch.channels_last) if last else gcanvas
            ours_f = lambda: amd.pillar_scatter(feats, vcoors, B, (H, W), channels_last=last)                     # noqa: E731
            ours_fb = lambda: torch.autograd.grad(amd.pillar_scatter(feats, vcoors, B, (H, W), channels_last=last), feats, gl)   # noqa: E731
            assert torch.equal(ours_f(), theirs_f()) and torch.equal(ours_fb()[0], theirs_fb()[0])
            tag = f'pillar_scatter: {view} canvas {H} x {W}, {"channels last" if last else "NCHW"}'
            extra = dict(voxels=V, channels=C_FEAT, canvas_MB=round(B * C_FEAT * H * W * 4 / 1e6, 1))
            entry(say, tag + ', forward', ours_f, theirs_f, extra)
            entry(say, tag + ', forward + backward', ours_fb, theirs_fb, extra)
        del gcanvas

        xyz = mp[i]
        vmap = torch.randn(B, C_FEAT, H, W, generator=g).to(dev).requires_grad_(True)
        gout = torch.randn(B * N_PER, C_FEAT, generator=g).to(dev)
        rng = ranges[i]
        ids = mc[i][:, 0].long()
        theirs_f = lambda: ref.single_view_sample(vmap, xyz[:, :3], ids, rng)                                    # noqa: E731
        theirs_fb = lambda: torch.autograd.grad(ref.single_view_sample(vmap, xyz[:, :3], ids, rng), vmap, gout)   # noqa: E731
        want_f, want_b = theirs_f().detach(), theirs_fb()[0]
        atomic_bytes = 4 * 4 * B * N_PER * C_FEAT
        floor_us = atomic_bytes / ATOMIC_RATE * 1e6
        for last in (False, True):
            ml = vmap.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) if last else vmap
            ours_f = lambda: amd.view_sample(ml, xyz[:, :3], mc[i], rng)                                          # noqa: E731
            ours_fb = lambda: torch.autograd.grad(amd.view_sample(ml, xyz[:, :3], mc[i], rng), ml, gout)          # noqa: E731
            diff = float((ours_f().detach() - want_f).abs().max())          # fp32 pixel coordinates up to 1264: an ulp there is 1e-4 of a cell
            assert diff < 2e-3, diff
            tag = f'view_sample: {view} map {H} x {W}, {"channels last" if last else "NCHW"}'
            extra = dict(points=B * N_PER, channels=C_FEAT, map_MB=round(B * C_FEAT * H * W * 4 / 1e6, 1), largest_difference_from_the_statements=diff)
            entry(say, tag + ', forward', ours_f, theirs_f, extra)
            for via in ((True, False) if not last else (None,)):
                if via is not None:
                    view_net.NCHW_BACKWARD_VIA_WORKSPACE = via
                assert torch.allclose(ours_fb()[0], want_b, rtol=1e-3, atol=1e-3)
                form = '' if via is None else (', sums in a channels-last workspace + transpose' if via else ', atomics straight into NCHW')
                extra_b = dict(extra, atomic_MB=round(atomic_bytes / 1e6, 1), atomic_floor_us=round(floor_us, 1))
                t, _ = entry(say, tag + ', forward + backward' + form, ours_fb, theirs_fb, extra_b)
                say(json.dumps(dict(what=tag + form + ': forward + backward over the atomic floor', times_the_floor=round(t / floor_us, 2))))
        del vmap, gout
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
