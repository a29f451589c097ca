#!/usr/bin/env python3
"""PVRCNNBboxHead's training slice (pvrcnn_bbox_head.py:140-351) on the GPU, us per step: targets + the three losses + backward() of
their sum, at R = 4 x 128 and 16 x 128 RoIs with half of them positive (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:240-249).
ours  = pvrcnn_head_get_targets + pvrcnn_head_loss on the reference's per-sample lists, `sum(losses.values()).backward()` (one launch each
        + the concatenations, the sum and the backward's elementwise scales)
ours_stacked_unit = the same two calls on stacked tensors with device-resident counts, backward with `unit_grad` as the upstream
        gradients: the two launches alone
torch = the reference's statements (tests/pvrcnn_train_ref.py) on the same device tensors, its three host syncs included: what a user
        runs without this package.
Per side: median and min of 100 hipEvent-timed steps after 20 warm-ups, and the kernel launches of one step (torch.profiler)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
import pvrcnn_train_ref as ref  # noqa: E402
from mmdet3d_gaussian_amd import _host  # noqa: E402

dev = torch.device('cuda:0')
WARM, ITERS = 20, 100


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


def launches(fn):
    """kernels one step puts on the device (memory copies not counted), or None with the reason when the profiler is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
                 and 'memset' not in e.name.lower()]
        return len(names)
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}'


def main():
    for B in (4, 16):
        shape = ((128, 64),) * B
        pos, gts, ious, rois, cls_score, bbox_pred = ref.draw(shape, seed=B)
        pos, gts, ious = [p.to(dev) for p in pos], [g.to(dev) for g in gts], [i.to(dev) for i in ious]
        rois = rois.to(dev)
        x = cls_score.to(dev).requires_grad_(True)
        p = bbox_pred.to(dev).requires_grad_(True)

        def ours():
            x.grad = p.grad = None
            tg = amd.pvrcnn_head_get_targets(pos, gts, ious, ref.CFG)
            losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, rois, *tg)
            sum(losses.values()).backward()
            return losses

        pb, pg, iu = torch.cat(pos), torch.cat(gts), torch.cat(ious)
        pc = torch.tensor([q.shape[0] for q in pos], dtype=torch.int32, device=dev)
        rc = torch.tensor([i.shape[0] for i in ious], dtype=torch.int32, device=dev)
        unit = [_host.unit_grad(dev)] * 3

        def stacked():
            x.grad = p.grad = None
            tg = amd.pvrcnn_head_get_targets(pb, pg, iu, ref.CFG, pos_batch_cnt=pc, roi_batch_cnt=rc)
            losses = amd.pvrcnn_head_loss(ref.LOSS_CLS, ref.LOSS_BBOX, x, p, rois, *tg)
            torch.autograd.backward([losses[k] for k in ref.LOSS_KEYS], grad_tensors=unit)
            return losses

        def eager():
            x.grad = p.grad = None
            tg = ref.get_targets(pos, gts, ious, ref.CFG)
            losses = ref.loss(x, p, rois, *tg)
            sum(losses.values()).backward()
            return losses

        a = ours()
        ga = (x.grad.clone(), p.grad.clone())
        e = eager()
        for k in ref.LOSS_KEYS:
            assert abs(float(a[k].detach()) - float(e[k].detach())) <= 1e-5 * abs(float(e[k].detach())), (k, float(a[k].detach()), float(e[k].detach()))
        assert torch.allclose(ga[0], x.grad, rtol=1e-4, atol=1e-7) and torch.allclose(ga[1], p.grad, rtol=1e-3, atol=1e-6)
        o_med, o_min = timed(ours)
        s_med, s_min = timed(stacked)
        e_med, e_min = timed(eager)
        print(json.dumps(dict(what=f'PVRCNNBboxHead targets + loss + backward, {B} x 128 rois, {B} x 64 positives',
                              ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=launches(ours),
                              ours_stacked_unit_us_median=s_med, ours_stacked_unit_us_min=s_min, ours_stacked_unit_kernel_launches=launches(stacked),
                              torch_restatement_us_median=e_med, torch_restatement_us_min=e_min, torch_restatement_kernel_launches=launches(eager),
                              ratio_of_medians=round(e_med / o_med, 2), ratio_of_medians_stacked_unit=round(e_med / s_med, 2))), flush=True)


if __name__ == '__main__':
    main()
