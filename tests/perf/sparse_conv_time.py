#!/usr/bin/env python3
"""Sparse 3D convolution on the GPU, us per call, for one stage at PV-RCNN's level-1 shape: 4 x 16 000 voxels from `pvrcnn_voxelize` on
synthetic points (a dense ground patch and twelve wall faces per sample, so that voxels have neighbours as a LiDAR sweep's do), sparse_shape (41, 1600, 1408).
  index      : sparse_conv_index, submanifold k3 and strided k3 s2 p1 (the static form: nothing read back)
  subm 16->16: sparse_conv forward, and forward + backward (input, weight and bias gradients)
  s2   16->32: the strided layer, the same two
ours     = the HIP entry points through the Python wrappers (csrc/sparse_conv.hip)
stand-in = what a ROCm user can write today: per offset `index_select` -> `mm` -> `index_add_` in torch over OUR nbr table, the per-offset
           pair lists handed to it free (built outside the timed region).  A stand-in written in this script is NOT spconv: spconv has no
           ROCm build to measure.  Its backward is torch autograd through the same statements (index_add_'s float atomics).
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; kernel launches from torch.profiler.  The
forward's gathered bytes (valid pairs x Cin x 4) over its time are printed beside the copy rate a 512 MiB torch copy reaches in the same
process."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402

dev = torch.device('cuda:0')
B, MAX_VOXELS, BATCHES = 4, 16000, 5
SHAPE = (41, 1600, 1408)
VOXEL_LAYER = dict(max_num_points=5, point_cloud_range=[0, -40, -3, 70.4, 40, 1], voxel_size=[0.05, 0.05, 0.1], max_voxels=(MAX_VOXELS, 40000))


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return round(statistics.median(us), 1), round(min(us), 1)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
              and 'memset' not in e.name.lower()]
        dur = {}
        for e in ev:
            dur[e.name[:40]] = round(dur.get(e.name[:40], 0.0) + (getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)), 1)
        return len(ev), dur
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}', {}


def synthetic_points(rng):
    """one sample: a 5 m x 5 m ground patch (100 x 100 cells, two cell layers of z noise) and 12 wall faces of 2 m x 2 m (40 x 20 cells), 70 000 points
    in random order -> about 19 000 occupied voxels of 5 x 5 x 10 cm, of which hard voxelization keeps the first 16 000: surfaces, as a LiDAR sweep"""
    n = 70000
    cx0, cy0 = rng.uniform(10, 50), rng.uniform(-30, 25)
    ground = np.stack([cx0 + rng.uniform(0, 5, 40000), cy0 + rng.uniform(0, 5, 40000), rng.normal(-1.7, 0.03, 40000)], 1)
    walls = []
    for _ in range(12):
        cx, cy = cx0 + rng.uniform(0, 5), cy0 + rng.uniform(0, 3)
        m = (n - 40000) // 12
        walls.append(np.stack([cx + rng.uniform(-0.02, 0.02, m), cy + rng.uniform(0, 2, m), rng.uniform(-1.7, 0.3, m)], 1))
    xyz = np.concatenate([ground] + walls)
    xyz = xyz[rng.permutation(len(xyz))]
    return torch.from_numpy(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], 1).astype(np.float32))


def pair_lists(nbr):
    """per offset (output rows, input rows) with a valid neighbour: the table handed to the stand-in free"""
    out = []
    for j in range(nbr.size(1)):
        o = (nbr[:, j] >= 0).nonzero().squeeze(1)
        out.append((o, nbr[o, j].long()))
    return out


def standin(x, w, pairs, rows):
    out = x.new_zeros((rows, w.size(2)))
    for j, (o, i) in enumerate(pairs):
        if o.numel():
            out.index_add_(0, o, x.index_select(0, i) @ w[j])
    return out


def main():
    rng = np.random.default_rng(7)
    vox = amd.pvrcnn_voxelize([synthetic_points(rng).to(dev) for _ in range(B)], VOXEL_LAYER, True)
    coors = vox['coors']
    N = coors.size(0)
    big = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    other = torch.empty_like(big)
    c_med, _ = timed(lambda: other.copy_(big), 10)
    copy_tbs = round(2 * big.numel() / (c_med * 1e-6) / 1e12, 2)
    del big, other
    print(json.dumps(dict(what='setup', voxels=N, per_sample=[int(v) for v in torch.bincount(coors[:, 0].long(), minlength=B)], sparse_shape=SHAPE,
                          copy_rate_TBps_same_process=copy_tbs)), flush=True)

    sub = amd.sparse_conv_index(coors, SHAPE, B, 3, 1, 1, True)
    dyn = amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1, False)
    R2 = dyn.nbr.size(0)
    for what, fn in (('index build, submanifold k3', lambda: amd.sparse_conv_index(coors, SHAPE, B, 3, 1, 1, True)),
                     ('index build, strided k3 s2 p1, static form', lambda: amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1, False, max_out=R2))):
        med, low = timed(fn, 10)
        n, dur = launches(fn)
        print(json.dumps(dict(what=what, rows_in=N, rows_out=N if 'sub' in what else R2, ours_us_median=med, ours_us_min=low, ours_kernel_launches=n,
                              ours_kernels_device_us=dur)), flush=True)

    torch.manual_seed(0)
    for what, index, cin, cout in (('subm k3 16->16', sub, 16, 16), ('strided k3 s2 p1 16->32', dyn, 16, 32)):
        rows = index.nbr.size(0)
        x = torch.randn(N, cin, device=dev, requires_grad=True)
        w = (torch.randn(27, cin, cout, device=dev) / (27 * cin) ** 0.5).requires_grad_(True)
        b = torch.randn(cout, device=dev, requires_grad=True)
        gy = torch.randn(rows, cout, device=dev)
        pairs = pair_lists(index.nbr)
        valid = int((index.nbr >= 0).sum())

        def ours_fwd():
            with torch.no_grad():
                return amd.sparse_conv(x, w, b, index)

        def ours_fb():
            return torch.autograd.grad(amd.sparse_conv(x, w, b, index), (x, w, b), gy)

        def standin_fwd():
            with torch.no_grad():
                return standin(x, w, pairs, rows) + b

        def standin_fb():
            return torch.autograd.grad(standin(x, w, pairs, rows) + b, (x, w, b), gy)

        live = (index.nbr >= 0).any(1, keepdim=True)
        diff = float((ours_fwd() - standin_fwd() * live).abs().max())
        g_o, g_s = ours_fb(), standin_fb()
        gdiff = [float((a - c).abs().max()) for a, c in zip(g_o, g_s)]
        for tag, ours, other, calls in (('forward', ours_fwd, standin_fwd, 20), ('forward + backward', ours_fb, standin_fb, 10)):
            o_med, o_min = timed(ours, calls)
            s_med, s_min = timed(other, max(2, calls // 4))
            o_n, o_dur = launches(ours)
            s_n, _ = launches(other)
            rec = dict(what=f'{what}, {tag}', rows_in=N, rows_out=rows, valid_pairs=valid, pairs_per_row=round(valid / max(rows, 1), 2),
                       ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=o_n, ours_kernels_device_us=o_dur,
                       standin_us_median=s_med, standin_us_min=s_min, standin_kernel_launches=s_n, ratio_of_medians=round(s_med / o_med, 2),
                       ours_slower_than_standin=bool(o_med > s_med), max_abs_diff_forward=diff, max_abs_diff_grads=gdiff)
            if tag == 'forward':
                rec['gathered_MB'] = round(valid * cin * 4 / 1e6, 1)
                rec['gathered_TBps'] = round(valid * cin * 4 / (o_med * 1e-6) / 1e12, 3)
                rec['copy_rate_TBps_same_process'] = copy_tbs
            print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
