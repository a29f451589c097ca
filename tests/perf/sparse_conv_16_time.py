#!/usr/bin/env python3
"""fp16 / bf16 sparse 3D convolution on the GPU (csrc/sparse_conv_16.hip), us per call, at PV-RCNN's levels: 4 x 16 000 voxels from
`pvrcnn_voxelize` on the synthetic points of tests/perf/sparse_conv_time.py, sparse_shape (41, 1600, 1408).
  index       : sparse_conv_index, submanifold k3 and strided k3 s2 p1 (the static form) — the 16-bit path uses the same tables
  subm 16->16 : level 1
  s2   16->32 : level 1 -> 2, k3 s2 p1
  subm 64->64 : a submanifold layer over the rows the chained index gives for level 3 (two strided layers down)
Per shape and 16-bit type, forward and forward + backward (input, weight and bias gradients), three sides in the same process:
  new   = compute_dtype = the type, on 16-bit features and weights (bias fp32)
  (a)   = compute_dtype=None on the SAME 16-bit tensors: the cast - evaluate in fp32 - cast route
  (b)   = the fp32 layer on fp32 tensors
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; kernel launches from torch.profiler.  The
forward's gathered bytes (valid pairs x Cin x element size) over its time are printed beside the copy rate a 512 MiB torch copy reaches
in the same process."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
from sparse_conv_time import B, SHAPE, VOXEL_LAYER, launches, synthetic_points, timed  # noqa: E402

dev = torch.device('cuda:0')


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

    sub1 = amd.sparse_conv_index(coors, SHAPE, B, 3, 1, 1, True)
    down1 = amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1, False)
    down2 = amd.sparse_conv_index(down1.out_coors, down1.out_shape, B, 3, 2, 1, False)
    sub3 = amd.sparse_conv_index(down2.out_coors, down2.out_shape, B, 3, 1, 1, True)
    print(json.dumps(dict(what='setup', voxels=N, rows_level_2=down1.nbr.size(0), rows_level_3=down2.nbr.size(0), sparse_shape=SHAPE,
                          shape_level_3=list(down2.out_shape), copy_rate_TBps_same_process=copy_tbs)), flush=True)
    R2 = down1.nbr.size(0)
    for what, fn in (('index build, submanifold k3', lambda: amd.sparse_conv_index(coors, SHAPE, B, 3, 1, 1, True)),
                     ('index build, strided k3 s2 p1, static form', lambda: amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1, False, max_out=R2))):
        med, low = timed(fn, 10)
        print(json.dumps(dict(what=what, rows_in=N, rows_out=N if 'sub' in what else R2, us_median=med, us_min=low)), flush=True)

    torch.manual_seed(0)
    for what, index, cin, cout in (('subm k3 16->16, level 1', sub1, 16, 16), ('strided k3 s2 p1 16->32, level 1 -> 2', down1, 16, 32),
                                   ('subm k3 64->64, level 3', sub3, 64, 64)):
        rows, n_in = index.nbr.size(0), index.num_in
        valid = int((index.nbr >= 0).sum())
        x32 = torch.randn(n_in, cin, device=dev)
        w32 = torch.randn(27, cin, cout, device=dev) / (27 * cin) ** 0.5
        b = torch.randn(cout, device=dev, requires_grad=True)
        gy32 = torch.randn(rows, cout, device=dev)

        def sides(dtype):
            x, w, gy = (t.to(dtype).requires_grad_(r) for t, r in ((x32, True), (w32, True), (gy32, False)))
            xf, wf = x32.clone().requires_grad_(True), w32.clone().requires_grad_(True)
            return dict(new=(x, w, gy, dtype), a=(x, w, gy, None), b=(xf, wf, gy32, None))

        for kind, dtype in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
            runs = sides(dtype)

            def fwd(side):
                x, w, _, cd = runs[side]
                with torch.no_grad():
                    return amd.sparse_conv(x, w, b, index, compute_dtype=cd)

            def fb(side):
                x, w, gy, cd = runs[side]
                return torch.autograd.grad(amd.sparse_conv(x, w, b, index, compute_dtype=cd), (x, w, b), gy)

            diff = float((fwd('new').float() - fwd('b')).abs().max())
            for tag, fn, calls in (('forward', fwd, 20), ('forward + backward', fb, 10)):
                rec = dict(what=f'{what}, {kind}, {tag}', rows_in=n_in, rows_out=rows, valid_pairs=valid, pairs_per_row=round(valid / max(rows, 1), 2))
                for side in ('new', 'a', 'b'):
                    med, low = timed(lambda: fn(side), calls)
                    n, dur = launches(lambda: fn(side))
                    rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
                    if side == 'new':
                        rec['new_kernels_device_us'] = dur
                rec['a_over_new'] = round(rec['a_us_median'] / rec['new_us_median'], 2)
                rec['b_over_new'] = round(rec['b_us_median'] / rec['new_us_median'], 2)
                rec['new_beats_a_and_b'] = bool(rec['new_us_median'] < rec['a_us_median'] and rec['new_us_median'] < rec['b_us_median'])
                if tag == 'forward':
                    rec['max_abs_diff_new_vs_fp32'] = diff
                    rec['new_gathered_MB'] = round(valid * cin * 2 / 1e6, 1)
                    rec['new_gathered_TBps'] = round(valid * cin * 2 / (rec['new_us_median'] * 1e-6) / 1e12, 3)
                    rec['b_gathered_TBps'] = round(valid * cin * 4 / (rec['b_us_median'] * 1e-6) / 1e12, 3)
                    rec['copy_rate_TBps_same_process'] = copy_tbs
                print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
