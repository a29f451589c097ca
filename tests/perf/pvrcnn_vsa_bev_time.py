#!/usr/bin/env python3
"""VoxelSetAbstraction's keypoint BEV interpolation (voxel_set_abstraction.py:153-177) and its voxel centres with their per-sample counts
(:179-193, :303-305) on the GPU, us per call, at the shipped config's shapes (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py):
B = 4 samples, a (4, 256, 200, 176) BEV map at stride 8, 2048 keypoints per sample, voxel 0.05 x 0.05 x 0.1, four sparse-conv levels at
strides 1, 2, 4, 8 (their row counts are stand-ins of a KITTI frame's order of magnitude: the config fixes the strides, not the counts).
ours   = bev_interpolate, forward alone and forward + backward with a resident upstream gradient, for the map in contiguous NCHW (what
         the reference's backbone produces) and in channels last; voxel_centers for the four levels
torch  = the reference's statements (tests/vsa_bev_ref.py: the grid ops, F.grid_sample, the permute; get_voxel_centers and the count loop)
         on the same device tensors in the same process: what a user runs without this package.
The two sides are timed ALTERNATELY, in blocks of 10 calls: median and min of 100 hipEvent-timed calls per side after 20 warm-ups, host
glue included, and the kernels one call launches (torch.profiler).
    python tests/perf/pvrcnn_vsa_bev_time.py [--out profiles/r15_pvrcnn_vsa_bev_time.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
import vsa_bev_ref as ref  # noqa: E402

WARM, ITERS, BLOCK = 20, 100, 10
B, C, H, W, M = 4, 256, 200, 176, 2048
VOXEL_SIZE = (0.05, 0.05, 0.1)
RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
ALIGN = 'half'
LEVELS = ((1, 64000), (2, 100000), (4, 60000), (8, 24000))       # (stride, rows over the batch)


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternated(ours, torch_side):
    """-> ((median, min) of ours, (median, min) of torch), the two sides in alternating blocks"""
    for _ in range(WARM):
        ours()
        torch_side()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(ITERS // BLOCK):
        a += [one(ours) for _ in range(BLOCK)]
        b += [one(torch_side) for _ in range(BLOCK)]
    return (round(statistics.median(a), 1), round(min(a), 1)), (round(statistics.median(b), 1), round(min(b), 1))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_pvrcnn_vsa_bev_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pvrcnn_vsa_bev_time.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, B=B, C=C, H=H, W=W, keypoints_per_sample=M,
                        warmups=WARM, timed_calls=ITERS, alternating_block=BLOCK)))
    count = lambda k: len(k) if isinstance(k, list) else k      # noqa: E731
    g = torch.Generator().manual_seed(15)
    kp = torch.stack([torch.rand(B, M, generator=g) * 70.4, torch.rand(B, M, generator=g) * 80 - 40, torch.rand(B, M, generator=g) * 4 - 3], dim=-1).to(dev)
    grad_out = torch.randn(B, M, C, generator=g).to(dev)
    base = torch.randn(B, C, H, W, generator=g)
    geo = (VOXEL_SIZE, RANGE, 8, ALIGN)
    not_faster = []
    for layout in ('nchw', 'channels_last'):
        bev = (base.to(dev).contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else base.to(dev)).requires_grad_(True)

        def ours_fwd():
            with torch.no_grad():
                return amd.bev_interpolate(kp, bev, *geo)

        def torch_fwd():
            with torch.no_grad():
                return ref.interpolate_from_bev_features(kp, bev, *geo)

        def ours_both():
            bev.grad = None
            amd.bev_interpolate(kp, bev, *geo).backward(grad_out)

        def torch_both():
            bev.grad = None
            ref.interpolate_from_bev_features(kp, bev, *geo).backward(grad_out)

        a, b = ours_fwd(), torch_fwd()
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), float((a - b).abs().max())
        ours_both()
        ga = bev.grad.clone()
        torch_both()
        assert torch.allclose(ga, bev.grad, rtol=1e-4, atol=1e-4), float((ga - bev.grad).abs().max())
        del ga, a, b
        for what, mine, theirs in (('forward', ours_fwd, torch_fwd), ('forward + backward', ours_both, torch_both)):
            (o_med, o_min), (t_med, t_min) = alternated(mine, theirs)
            ko, kt = kernels(mine), kernels(theirs)
            say(json.dumps(dict(what=f'bev_interpolate {what}, {layout}', ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=count(ko),
                                torch_restatement_us_median=t_med, torch_restatement_us_min=t_min, torch_restatement_kernel_launches=count(kt),
                                ratio_of_medians=round(t_med / o_med, 2))))
            if isinstance(ko, list):
                say(json.dumps(dict(what=f'kernels of one of our calls, {what}, {layout}', kernels=[[n[:60], round(d, 1)] for n, d in ko])))
            if isinstance(kt, list) and what != 'forward':
                say(json.dumps(dict(what=f'kernels of one torch call, {what}, {layout}', kernels=[[n[:60], round(d, 1)] for n, d in kt])))
            if o_med > t_med:
                not_faster.append((what, layout, o_med, t_med))
        bev.grad = None
        del bev
        torch.cuda.empty_cache()

    levels = []
    for scale, n in LEVELS:
        per = n // B
        dims = (int(round(4.0 / VOXEL_SIZE[2] / scale)) + 1, int(round(80.0 / VOXEL_SIZE[1] / scale)), int(round(70.4 / VOXEL_SIZE[0] / scale)))
        c = torch.stack([torch.arange(n) // per] + [torch.randint(0, d, (n,), generator=g) for d in dims], dim=1).int().to(dev)
        levels.append((scale, c))

    def ours_centres():
        return [amd.voxel_centers(c, VOXEL_SIZE, RANGE, scale, ALIGN, B) for scale, c in levels]

    def torch_centres():
        out = []
        for scale, c in levels:
            xyz = ref.get_voxel_centers(c, VOXEL_SIZE, RANGE, scale, ALIGN).contiguous()
            out.append((xyz, ref.count_loop(c, xyz, B)))
        return out

    for (xa, ca), (xb, cb) in zip(ours_centres(), torch_centres()):
        assert torch.equal(xa, xb) and torch.equal(ca, cb)
    (o_med, o_min), (t_med, t_min) = alternated(ours_centres, torch_centres)
    ko, kt = kernels(ours_centres), kernels(torch_centres)
    say(json.dumps(dict(what=f'voxel_centers, four levels, rows {[n for _, n in LEVELS]}', ours_us_median=o_med, ours_us_min=o_min,
                        ours_kernel_launches=count(ko), torch_restatement_us_median=t_med, torch_restatement_us_min=t_min,
                        torch_restatement_kernel_launches=count(kt), ratio_of_medians=round(t_med / o_med, 2))))
    if o_med > t_med:
        not_faster.append(('voxel_centers', '-', o_med, t_med))
    say(json.dumps(dict(not_faster_than_torch=not_faster)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
