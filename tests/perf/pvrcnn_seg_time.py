#!/usr/bin/env python3
"""PV-RCNN's keypoint segmentation slice (pointwise_mask_head.py:124-144, pvrcnn_roi_head.py:211-212) on the GPU, us per step, at the
shipped config's shapes (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py): N = 4 x 2048 keypoints, C = 128 fused channels,
num_classes = 3, K = 1 (class agnostic, the config) and K = 3, focal gamma 2 / alpha 0.25 / reduction 'sum'.
A step = the seg loss, the reweighting, and the backward of `loss + out.sum()`.
ours       = pvrcnn_seg_loss + keypoint_reweight, `(loss + out.sum()).backward()`: our four launches plus what torch adds for the sum,
             the addition, the expanded upstream gradient made contiguous, the scale by the upstream gradient and the accumulation
ours_unit  = the same two calls, backward with `unit_grad` for the loss and a resident ones tensor for the features: our launches
             and the accumulation of the two gradients of seg_preds
torch      = the reference's statements (tests/pvrcnn_seg_ref.py) on the same device tensors: what a user runs without this package.
Per side: median and min of 100 hipEvent-timed steps after 20 warm-ups, host glue included, and the kernels one step launches
(torch.profiler).  For the two reweight kernels: their device durations from the same profile against the bytes they must move at the
copy rate measured in this process (the floor of tools/vsa_time.py).
    python tests/perf/pvrcnn_seg_time.py [--out profiles/r14_pvrcnn_seg_time.txt]"""
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
import pvrcnn_seg_ref as ref  # noqa: E402
from mmdet3d_gaussian_amd import _host  # noqa: E402

WARM, ITERS = 20, 100
N, C = 4 * 2048, 128


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(us), 1), round(min(us), 1)


def kernels(fn):
    """[(kernel name, device us)] of one step (memory copies not counted), or a string with the reason when the profiler is unavailable"""
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


def copy_rate():
    """bytes per second of a device-to-device copy of 512 MiB (read + written), as tools/vsa_time.py measures it"""
    big = torch.empty(512 << 20, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(big)
    for _ in range(3):
        dst.copy_(big)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        dst.copy_(big)
    b.record()
    torch.cuda.synchronize()
    return 2 * big.numel() * 10 / (a.elapsed_time(b) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_pvrcnn_seg_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pvrcnn_seg_time.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rate = copy_rate()
    say(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, copy_rate_TBps=round(rate / 1e12, 2), N=N, C=C,
                        warmups=WARM, timed_steps=ITERS)))
    slower = []
    for agnostic in (True, False):
        K = 1 if agnostic else ref.NUM_CLASSES
        g = torch.Generator().manual_seed(K)
        x = ref.gapped_logits(N, K, g).to(dev).requires_grad_(True)
        feats = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
        u = torch.rand(N, generator=g)
        t = torch.full((N,), ref.NUM_CLASSES, dtype=torch.int64)
        t[u < 0.1] = torch.randint(0, ref.NUM_CLASSES, (N,), generator=g)[u < 0.1]
        t[u > 0.95] = -1
        t = t.to(dev)
        ones = torch.ones(N, C, device=dev)
        unit = _host.unit_grad(dev)

        def ours():
            x.grad = feats.grad = None
            loss = amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t, ref.NUM_CLASSES, agnostic)['loss_seg']
            out = amd.keypoint_reweight(feats, x)
            (loss + out.sum()).backward()
            return loss

        def ours_unit():
            x.grad = feats.grad = None
            loss = amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t, ref.NUM_CLASSES, agnostic)['loss_seg']
            out = amd.keypoint_reweight(feats, x)
            torch.autograd.backward([loss, out], grad_tensors=[unit, ones])
            return loss

        def eager():
            x.grad = feats.grad = None
            loss = ref.seg_loss(x, t, ref.NUM_CLASSES, agnostic, ref.LOSS_SEG)[0]
            out = ref.reweight(feats, x)[0]
            (loss + out.sum()).backward()
            return loss

        a = float(ours().detach())
        ga = (x.grad.clone(), feats.grad.clone())
        b = float(ours_unit().detach())
        gb = (x.grad.clone(), feats.grad.clone())
        e = float(eager().detach())
        assert a == b and abs(a - e) <= 1e-5 * abs(e), (a, b, e)
        for got in (ga, gb):
            assert torch.allclose(got[0], x.grad, rtol=1e-4, atol=1e-6) and torch.allclose(got[1], feats.grad, rtol=1e-5, atol=1e-7)
        o_med, o_min = timed(ours)
        u_med, u_min = timed(ours_unit)
        e_med, e_min = timed(eager)
        ko, ku, ke = kernels(ours), kernels(ours_unit), kernels(eager)
        count = lambda k: len(k) if isinstance(k, list) else k      # noqa: E731
        say(json.dumps(dict(what=f'seg loss + reweight + backward of loss + out.sum(), N = {N}, C = {C}, K = {K}, class_agnostic = {agnostic}',
                            ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=count(ko),
                            ours_unit_us_median=u_med, ours_unit_us_min=u_min, ours_unit_kernel_launches=count(ku),
                            torch_restatement_us_median=e_med, torch_restatement_us_min=e_min, torch_restatement_kernel_launches=count(ke),
                            ratio_of_medians=round(e_med / o_med, 2), ratio_of_medians_unit=round(e_med / u_med, 2))))
        if isinstance(ku, list):
            say(json.dumps(dict(what=f'kernels of one ours_unit step, K = {K}', kernels=[[n[:60], round(d, 1)] for n, d in ku])))
            fwd_bytes = 4 * (2 * N * C + N * K) + N                       # feats read, out written, logits read, winners written
            bwd_bytes = 4 * (3 * N * C + 2 * N * K) + N                   # grad_out and feats read, grad_feats written, logits read, grad_seg written, winners read
            for key, nbytes in (('reweight_kernel', fwd_bytes), ('reweight_backward_kernel', bwd_bytes)):
                d = [dur for n, dur in ku if key in n]
                say(json.dumps(dict(kernel=key, K=K, device_us=[round(v, 1) for v in d], bytes_moved=nbytes, floor_us_at_copy_rate=round(nbytes / rate * 1e6, 2))))
        if o_med > e_med:
            slower.append((K, 'ours', o_med, e_med))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    assert not slower, f'our median step is slower than the torch restatement: (K, side, ours us, torch us) {slower}'


if __name__ == '__main__':
    main()
