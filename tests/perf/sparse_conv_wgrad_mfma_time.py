#!/usr/bin/env python3
"""The matrix-core weight gradient of the 16-bit sparse convolution (csrc/sparse_conv_wgrad_16.hip) against the FMA form
(csrc/sparse_conv_wgrad.hip on 16-bit operands), us, at the three shapes of tests/perf/sparse_conv_16_time.py on its voxel set
(4 x 16 000 voxels from `pvrcnn_voxelize`, sparse_shape (41, 1600, 1408)): subm k3 16->16, strided k3 s2 p1 16->32, subm k3 64->64 two
levels down; fp16 and bf16; both sides in the same process.
  (a) the C entries called directly on the same tensors and workspace: the whole entry (device events around back-to-back calls, the
      median of 5 batches after a warm-up) and STAGE ONE ALONE — the device time of `wgrad16_kernel` / `wgrad_kernel` from
      torch.profiler, the median over 10 calls.  The gathered bytes of stage one (valid pairs x (Cin + Cout) x 2) over its time are printed
      beside the rate a 512 MiB torch copy reaches in the same process.
  (b) `sparse_conv` forward + backward (input, weight and bias gradients) with weight_grad='mfma' and None.
  (c) one `MlvlSparseEncoder.train()` step in bf16, forward + backward, with `set_weight_grad('mfma')` and without."""
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
from mmdet3d_gaussian_amd import _lib  # noqa: E402
from sparse_conv_time import B, SHAPE, VOXEL_LAYER, launches, synthetic_points, timed  # noqa: E402

dev = torch.device('cuda:0')
ENTRIES = dict(mfma=('gd3d_sparse_conv_backward_weight_16_mfma', 'wgrad16_kernel'), fma=('gd3d_sparse_conv_backward_weight_16', 'wgrad_kernel'))


def kernel_us(fn, needle, calls=10):
    """the device time of the kernels whose name holds `needle`, per call of fn: the median over `calls` profiled calls"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    us = [getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0) for e in prof.events()
          if e.device_type == torch.autograd.DeviceType.CUDA and needle in e.name]
    assert len(us) == calls, (needle, len(us))
    return round(statistics.median(us), 1), round(min(us), 1)


def main():
    rng = np.random.default_rng(7)
    vox = amd.pvrcnn_voxelize([synthetic_points(rng).to(dev) for _ in range(B)], VOXEL_LAYER, True)
    coors = vox['coors']
    big = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    other = torch.empty_like(big)
    c_med, _ = timed(lambda: other.copy_(big), 10)
    copy_tbs = round(2 * big.numel() / (c_med * 1e-6) / 1e12, 2)
    del big, other
    sub1 = amd.sparse_conv_index(coors, SHAPE, B, 3, 1, 1, True)
    down1 = amd.sparse_conv_index(coors, SHAPE, B, 3, 2, 1, False)
    down2 = amd.sparse_conv_index(down1.out_coors, down1.out_shape, B, 3, 2, 1, False)
    sub3 = amd.sparse_conv_index(down2.out_coors, down2.out_shape, B, 3, 1, 1, True)
    print(json.dumps(dict(what='setup', voxels=coors.size(0), rows_level_2=down1.nbr.size(0), rows_level_3=down2.nbr.size(0), sparse_shape=SHAPE,
                          copy_rate_TBps_same_process=copy_tbs)), flush=True)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    for what, index, cin, cout in (('subm k3 16->16, level 1', sub1, 16, 16), ('strided k3 s2 p1 16->32, level 1 -> 2', down1, 16, 32),
                                   ('subm k3 64->64, level 3', sub3, 64, 64)):
        rows, n_in, K = index.nbr.size(0), index.num_in, index.nbr.size(1)
        valid = int((index.nbr >= 0).sum())
        padded = torch.cat([index.nbr, index.nbr.new_full(((-rows) % 32, K), -1)])
        steps = int((padded.view(-1, 32, K) >= 0).any(1).sum())                                    # 32-row steps that hold a pair, over the offsets
        x32 = torch.randn(n_in, cin, device=dev)
        w32 = torch.randn(K, cin, cout, device=dev) / (K * cin) ** 0.5
        b = torch.randn(cout, device=dev, requires_grad=True)
        gy32 = torch.randn(rows, cout, device=dev)
        work = torch.empty(lib.gd3d_sparse_conv_backward_weight_workspace_bytes(rows, K, cin, cout), dtype=torch.uint8, device=dev)
        gw, gb = torch.empty(K, cin, cout, device=dev), torch.empty(cout, device=dev)
        for kind, dtype, code in (('fp16', torch.float16, 1), ('bf16', torch.bfloat16, 2)):
            x16, g16, w16 = x32.to(dtype), gy32.to(dtype), w32.to(dtype)

            def entry(side):
                _lib.check(getattr(lib, ENTRIES[side][0])(x16.data_ptr(), g16.data_ptr(), index.nbr.data_ptr(), index.num.data_ptr(), n_in, rows, K, cin, cout,
                                                          code, work.data_ptr(), gw.data_ptr(), gb.data_ptr(), stream), ENTRIES[side][0])

            rec = dict(what=f'(a) {what}, {kind}, weight + bias gradient entry', rows_in=n_in, rows_out=rows, valid_pairs=valid,
                       pairs_per_row=round(valid / max(rows, 1), 2), steps_with_a_pair=steps, steps_in_all=-(-rows // 32) * K)
            got = {}
            for side in ('mfma', 'fma'):
                rec[f'{side}_entry_us_median'], rec[f'{side}_entry_us_min'] = timed(lambda: entry(side), 20)
                rec[f'{side}_stage_one_us_median'], rec[f'{side}_stage_one_us_min'] = kernel_us(lambda: entry(side), ENTRIES[side][1])
                got[side] = gw.clone()
            rec['max_abs_diff_mfma_vs_fma'] = float((got['mfma'] - got['fma']).abs().max())
            rec['fma_over_mfma_stage_one'] = round(rec['fma_stage_one_us_median'] / rec['mfma_stage_one_us_median'], 2)
            rec['fma_over_mfma_entry'] = round(rec['fma_entry_us_median'] / rec['mfma_entry_us_median'], 2)
            rec['mfma_stage_one_is_lower'] = bool(rec['mfma_stage_one_us_median'] < rec['fma_stage_one_us_median'])
            rec['stage_one_gathered_MB'] = round(valid * (cin + cout) * 2 / 1e6, 1)
            for side in ('mfma', 'fma'):
                rec[f'{side}_stage_one_gathered_TBps'] = round(valid * (cin + cout) * 2 / (rec[f'{side}_stage_one_us_median'] * 1e-6) / 1e12, 3)
            rec['copy_rate_TBps_same_process'] = copy_tbs
            print(json.dumps(rec), flush=True)

            x, w, gy = x16.clone().requires_grad_(True), w16.clone().requires_grad_(True), g16

            def fb(mode):
                return torch.autograd.grad(amd.sparse_conv(x, w, b, index, compute_dtype=dtype, weight_grad=mode), (x, w, b), gy)

            rec = dict(what=f'(b) {what}, {kind}, sparse_conv forward + backward', rows_in=n_in, rows_out=rows)
            for side, mode in (('mfma', 'mfma'), ('fma', None)):
                rec[f'{side}_us_median'], rec[f'{side}_us_min'] = timed(lambda: fb(mode), 10)
                rec[f'{side}_kernel_launches'], dur = launches(lambda: fb(mode))
                rec[f'{side}_kernels_device_us'] = dur
            rec['fma_over_mfma'] = round(rec['fma_us_median'] / rec['mfma_us_median'], 2)
            print(json.dumps(rec), flush=True)

    feats = vox['voxel_features'].float().contiguous()
    torch.manual_seed(1)
    enc = amd.MlvlSparseEncoder(in_channels=feats.size(1), sparse_shape=list(SHAPE), compute_dtype=torch.bfloat16).to(dev).train()
    on = copy.deepcopy(enc).set_weight_grad('mfma')
    rec = dict(what='(c) MlvlSparseEncoder.train() forward + backward, bf16', voxels=coors.size(0))
    for side, net in (('mfma', on), ('fma', enc)):
        params = [p for p in net.parameters()]

        def step(net=net, params=params):
            out = net(feats, coors, B)['spatial_features']
            return torch.autograd.grad(out.float().sum(), params)
        rec[f'{side}_us_median'], rec[f'{side}_us_min'] = timed(step, 5)
        rec[f'{side}_kernel_launches'], _ = launches(step)
    rec['fma_over_mfma'] = round(rec['fma_us_median'] / rec['mfma_us_median'], 2)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
