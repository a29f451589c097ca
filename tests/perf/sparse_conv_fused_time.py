#!/usr/bin/env python3
"""The fused sparse convolution layer on the GPU (gd3d_sparse_conv_forward_fused[_16]), us per call, against the unfused
eval chain on the same tensors, at PV-RCNN's levels: 4 x 16 000 voxels from `pvrcnn_voxelize` on the synthetic points of
tests/perf/sparse_conv_time.py, sparse_shape (41, 1600, 1408) — the shapes of tests/perf/sparse_conv_16_time.py.
  subm 16->16 : level 1
  s2   16->32 : level 1 -> 2, k3 s2 p1
  subm 64->64 : a submanifold layer over the rows the chained index gives for level 3
Per shape, in fp32 and in bf16, inference (no_grad), all sides in the same process:
  layer       : fused  = sparse_conv(..., scale, shift, activation='relu')               one launch
                chain  = sparse_conv -> BatchNorm1d.eval() -> ReLU(inplace)              what `make_sparse_convmodule` runs
                plain  = sparse_conv alone
  block tail  : fused  = sparse_conv(..., scale, shift, residual, activation='relu')     one launch
                chain  = sparse_conv -> BatchNorm1d.eval() -> + identity -> ReLU(inplace) the second half of `SparseBasicBlock`
  expectation : fused <= chain, and fused <= plain + the time of reading one more (R, Cout) array at the copy probe's rate
and a whole `MlvlSparseEncoder.eval()` forward, fused (`.fuse()`) against unfused, with the kernel launches of both.
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; kernel launches from torch.profiler; the copy
probe is a 512 MiB torch copy in the same process."""
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
from sparse_conv_time import B, SHAPE, VOXEL_LAYER, launches, synthetic_points, timed  # noqa: E402

dev = torch.device('cuda:0')


def trained(bn):
    """running statistics and affine parameters a trained model would hold"""
    bn.running_mean.normal_(0, 0.1)
    bn.running_var.uniform_(0.5, 1.5)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.1)
    return bn


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
                          copy_rate_TBps_same_process=copy_tbs)), flush=True)

    torch.manual_seed(0)
    relu = torch.nn.ReLU(inplace=True)
    for what, index, cin, cout in (('subm k3 16->16, level 1', sub1, 16, 16), ('strided k3 s2 p1 16->32, level 1 -> 2', down1, 16, 32),
                                   ('subm k3 64->64, level 3', sub3, 64, 64)):
        rows, n_in = index.nbr.size(0), index.num_in
        x32 = torch.randn(n_in, cin, device=dev)
        w32 = torch.randn(27, cin, cout, device=dev) / (27 * cin) ** 0.5
        id32 = torch.randn(rows, cout, device=dev)
        bn = trained(torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(dev)).eval()
        layer = amd.FusedSparseConv(amd.SubMConv3d(cin, cout, 3, bias=False).to(dev), bn, 'relu')      # folds the BatchNorm: scale, shift
        scale, shift = layer.scale, layer.shift
        for kind, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
            x, w, identity = ((t if dtype is None else t.to(dtype)) for t in (x32, w32, id32))
            sides = {
                'layer': dict(fused=lambda: amd.sparse_conv(x, w, None, index, dtype, scale=scale, shift=shift, activation='relu'),
                              chain=lambda: relu(bn(amd.sparse_conv(x, w, None, index, dtype)))),
                'block tail': dict(fused=lambda: amd.sparse_conv(x, w, None, index, dtype, scale=scale, shift=shift, residual=identity, activation='relu'),
                                   chain=lambda: relu(bn(amd.sparse_conv(x, w, None, index, dtype)) + identity)),
            }
            plain = lambda: amd.sparse_conv(x, w, None, index, dtype)
            with torch.no_grad():
                p_med, p_min = timed(plain, 20)
                extra_us = rows * cout * x.element_size() / (copy_tbs * 1e12) * 1e6       # one more (R, Cout) array at the copy probe's rate
                for tag, pair in sides.items():
                    diff = float((pair['fused']().float() - pair['chain']().float()).abs().max())
                    rec = dict(what=f'{what}, {kind}, {tag}', rows_in=n_in, rows_out=rows, plain_us_median=p_med, plain_us_min=p_min)
                    for side in ('fused', 'chain'):
                        med, low = timed(pair[side], 20)
                        n, dur = launches(pair[side])
                        rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
                        if side == 'fused':
                            rec['fused_kernels_device_us'] = dur
                    rec['chain_over_fused'] = round(rec['chain_us_median'] / rec['fused_us_median'], 2)
                    rec['fused_not_slower_than_chain'] = bool(rec['fused_us_median'] <= rec['chain_us_median'])
                    budget = p_med + (extra_us if tag == 'block tail' else 0.0)
                    rec['plain_plus_one_more_array_us'] = round(budget, 1)
                    rec['fused_within_plain_plus_one_more_array'] = bool(rec['fused_us_median'] <= budget)
                    rec['max_abs_diff_fused_vs_chain'] = diff
                    rec['copy_rate_TBps_same_process'] = copy_tbs
                    print(json.dumps(rec), flush=True)

    feats = vox['voxel_features'].float().contiguous()                  # (V, 4): HardSimpleVFE's means
    for kind, dtype in (('fp32', None), ('bf16', torch.bfloat16)):
        torch.manual_seed(1)
        enc = amd.MlvlSparseEncoder(in_channels=feats.size(1), sparse_shape=list(SHAPE), compute_dtype=dtype).to(dev)
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                trained(m)
        enc.eval()
        fused = copy.deepcopy(enc).fuse()
        with torch.no_grad():
            a, b = enc(feats, coors, B)['spatial_features'], fused(feats, coors, B)['spatial_features']
            rec = dict(what=f'MlvlSparseEncoder.eval() forward, {kind}', voxels=N, spatial_features=list(a.shape),
                       max_abs_diff_fused_vs_chain=float((a.float() - b.float()).abs().max()), max_abs_chain=float(a.float().abs().max()))
            for side, net in (('fused', fused), ('chain', enc)):
                med, low = timed(lambda: net(feats, coors, B), 5)
                n, _ = launches(lambda: net(feats, coors, B))
                rec[f'{side}_us_median'], rec[f'{side}_us_min'], rec[f'{side}_kernel_launches'] = med, low, n
        rec['chain_over_fused'] = round(rec['chain_us_median'] / rec['fused_us_median'], 2)
        rec['fused_not_slower_than_chain'] = bool(rec['fused_us_median'] <= rec['chain_us_median'])
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
