#!/usr/bin/env python3
"""The sparse decoder on the GPU, us per call, on `sparse_conv_time.py`'s synthetic 4 x 16 000-voxel scene.

Pooling (`sparse_max_pool`, gd3d_sparse_max_pool_*): k3 s2 p1 and k2 s2 at 16 and 64 channels, fp32 and bf16, forward and forward +
backward, against a torch stand-in written here over OUR table (handed to it free, as int64 with its mask): gather (R, K, C), fill the
missing entries with -inf, `amax` over K — and against an in-process copy of the bytes the forward has to move (the valid neighbours'
pieces and the table read, the output written), with the gathered bytes per second.
Inverse layer (`sparse_inverse_conv`) over spconv2's table, 32 -> 16, against the forward layer's input-gradient launch on the same table
and operands of the same shape: the same kernel over the same table, so the two should agree.
Whole model: `SparseUNet` forward (eval, unfused and fused) and train step (forward + backward), launches and time, fp32 and bf16.
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; launches from torch.profiler."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
from mmdet3d_gaussian_amd.sparse_conv import _backward_entries  # noqa: E402
from sparse_conv_time import B, SHAPE, VOXEL_LAYER, launches, synthetic_points, timed  # noqa: E402

dev = torch.device('cuda:0')


def copy_us(nbytes):
    """an in-process device copy that moves `nbytes` in all (half read, half written), us"""
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), 50)[0]


def main():
    rng = np.random.default_rng(7)
    vox = amd.pvrcnn_voxelize([synthetic_points(rng).to(dev) for _ in range(B)], VOXEL_LAYER, True)
    coors, feats = vox['coors'], vox['voxel_features'].float().contiguous()
    N = coors.size(0)

    for geom, (k, s, p) in (('k3 s2 p1', (3, 2, 1)), ('k2 s2', (2, 2, 0))):
        index = amd.sparse_conv_index(coors, SHAPE, B, k, s, p)
        R, K = index.nbr.shape
        valid = int((index.nbr >= 0).sum())
        gather, missing = index.nbr.clamp(min=0).long(), (index.nbr < 0)[:, :, None]

        def standin(x):
            return x[gather].masked_fill(missing, float('-inf')).amax(1)
        for C in (16, 64):
            for kind, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
                torch.manual_seed(0)
                x = torch.randn(N, C, device=dev).to(dtype).requires_grad_(True)
                gy = torch.randn(R, C, device=dev).to(dtype)
                es = x.element_size()
                with torch.no_grad():
                    same = bool(torch.equal(amd.sparse_max_pool(x, index), standin(x)))
                moved = valid * C * es + R * K * 4 + R * C * es
                sides = {'forward': dict(ours=lambda: amd.sparse_max_pool(x, index), standin=lambda: standin(x)),
                         'forward + backward': dict(ours=lambda: torch.autograd.grad(amd.sparse_max_pool(x, index), x, gy),
                                                    standin=lambda: torch.autograd.grad(standin(x), x, gy))}
                for tag, pair in sides.items():
                    rec = dict(what=f'max pool {geom}, {N} -> {R} rows x {C}, {kind}, {tag}', forward_equals_standin=same)
                    for side in ('ours', 'standin'):
                        med, low = timed(pair[side], 50)
                        n, dur = launches(pair[side])
                        rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
                        rec[f'{side}_kernels_device_us_sum'] = round(sum(dur.values()), 1)
                    rec['standin_over_ours'] = round(rec['standin_us_median'] / rec['ours_us_median'], 2)
                    rec['ours_not_slower_than_standin'] = bool(rec['ours_us_median'] <= rec['standin_us_median'])
                    if tag == 'forward':
                        rec['forward_bytes_moved'] = moved
                        rec['copy_of_the_same_bytes_us'] = copy_us(moved)
                        rec['gathered_GB_per_s_by_kernel_time'] = round(valid * C * es / max(rec['ours_kernels_device_us_sum'], 1e-3) / 1e3, 1)
                    print(json.dumps(rec), flush=True)

    # the inverse layer over spconv2's table (k3 s2 p1 over the input voxels), 32 -> 16, beside the forward layer's input gradient
    index = amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1)
    R, K = index.nbr.shape
    for kind, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
        torch.manual_seed(1)
        t = dtype or torch.float32
        f = torch.randn(R, 32, device=dev).to(t)
        w_inv = (torch.randn(K, 32, 16, device=dev) / (K * 32) ** 0.5).to(t)       # the inverse layer's weight (K, Cin = 32, Cout = 16)
        w_fwd = w_inv.transpose(1, 2).contiguous()                                 # the 16 -> 32 forward layer whose input gradient is the same sum
        x = torch.zeros(N, 16, device=dev).to(t)
        inverse = lambda: amd.sparse_inverse_conv(f, w_inv, None, index, dtype)
        twin = lambda: _backward_entries(x, w_fwd, f, index.nbr, index.nbr_t, index.num, False, True, False, False, dtype)[0]
        with torch.no_grad():
            diff = float((inverse().float() - twin().float()).abs().max())
        rec = dict(what=f'inverse conv over spconv2\'s table, {R} -> {N} rows, 32 -> 16, {kind}', max_abs_diff_inverse_vs_input_gradient=diff)
        with torch.no_grad():
            for side, fn in (('inverse', inverse), ('input_gradient', twin)):
                med, low = timed(fn, 50)
                n, dur = launches(fn)
                rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
                rec[f'{side}_kernels_device_us_sum'] = round(sum(dur.values()), 1)
        rec['inverse_over_input_gradient'] = round(rec['inverse_us_median'] / rec['input_gradient_us_median'], 3)
        print(json.dumps(rec), flush=True)

    for kind, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
        torch.manual_seed(2)
        net = amd.SparseUNet(in_channels=feats.size(1), sparse_shape=list(SHAPE), compute_dtype=dtype).to(dev)
        rec = dict(what=f'SparseUNet, {kind}', voxels=N)
        params = list(net.parameters())

        def step():
            out = net(feats, coors, B)
            return torch.autograd.grad(out['seg_features'].float().sum() + out['spatial_features'].float().sum(), params)
        net.train()
        med, low = timed(step, 5)
        n, _ = launches(step)
        rec['train_step_us_median'], rec['train_step_us_min'], rec['train_step_kernel_launches'] = med, low, n
        fused = copy.deepcopy(net).eval().fuse()
        net.eval()
        with torch.no_grad():
            a, b = net(feats, coors, B)['seg_features'], fused(feats, coors, B)['seg_features']
            rec['max_abs_diff_fused_vs_unfused_seg_features'] = float((a.float() - b.float()).abs().max())
            for side, m in (('eval_forward_unfused', net), ('eval_forward_fused', fused)):
                fn = lambda m=m: m(feats, coors, B)
                med, low = timed(fn, 5)
                n, _ = launches(fn)
                rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
        rec['unfused_over_fused'] = round(rec['eval_forward_unfused_us_median'] / rec['eval_forward_fused_us_median'], 2)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
