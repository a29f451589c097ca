#!/usr/bin/env python3
"""PV-RCNN's RoI assign-and-sample stage (pvrcnn_roi_head.py:225-297) on the GPU, us per call, at 4 x 512 proposals, ~20 gts per sample,
three classes, num = 128 with the shipped thresholds (configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:213-249).
ours   = pvrcnn_assign_and_sample through its wrapper, stacked form with device counts, keys given (two launches)
iou    = bbox_overlaps_3d alone on the 2048 x 80 pairs of the stacked batch (what a per-sample matrix would cost at most)
torch  = the plain-torch restatement (tests/pvrcnn_sample_ref.py) on the same device, its IoU matrices from bbox_overlaps_3d: what a
         user runs without this op; with the kernels and the host syncs of one call.
Per side: device events around 50 back-to-back calls, the median of 5 such batches after a warm-up, divided by 50.  For ours also the
two kernels' own device durations (torch.profiler), which tell the kernels' share of a call from the host glue's."""
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402
import pvrcnn_sample_ref as ref  # noqa: E402

dev = torch.device('cuda:0')
CALLS, BATCHES = 50, 5


def timed(fn, calls=CALLS):
    for _ in range(5):
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


def kernels(fn):
    """(kernel launches of one call, {kernel name: device us}) from torch.profiler, or the reason it is unavailable"""
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
            dur[e.name[:60]] = round(dur.get(e.name[:60], 0.0) + (getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)), 1)
        return len(ev), dur
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}', {}


def syncs(fn):
    """host syncs of one call, counted by torch's sync debug mode"""
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        return sum('synchroniz' in str(x.message) for x in w)
    finally:
        torch.cuda.set_sync_debug_mode('default')


def main():
    samples = [ref.make_sample(100 + b, ref.mixed(512), 18 + b) for b in range(4)]
    case = ref._case(samples, ref.SHIPPED, ref._sampler(128), 77)
    props, plab = torch.cat(case['proposals']).to(dev), torch.cat(case['proposal_labels']).to(dev)
    gts, glab = torch.cat(case['gt_bboxes']).to(dev), torch.cat(case['gt_labels']).to(dev)
    pc = torch.tensor([p.shape[0] for p in case['proposals']], dtype=torch.int32, device=dev)
    gc = torch.tensor([g.shape[0] for g in case['gt_bboxes']], dtype=torch.int32, device=dev)
    keys, fill = case['keys'].to(dev), case['fill_keys'].to(dev)

    def ours():
        return amd.pvrcnn_assign_and_sample(props, plab, gts, glab, case['assigner'], case['sampler'], prop_batch_cnt=pc, gt_batch_cnt=gc,
                                            keys=keys, fill_keys=fill, return_assignment=True)

    def iou():
        return amd.bbox_overlaps_3d(props, gts)

    def eager():
        return ref.restate(case, dev=dev)[0]

    a, e = ours(), eager()
    for k in e:
        assert torch.equal(a[k], e[k]), k
    o_med, o_min = timed(ours)
    i_med, i_min = timed(iou)
    e_med, e_min = timed(eager, calls=5)
    o_n, o_dur = kernels(ours)
    e_n, _ = kernels(eager)
    i_n, i_dur = kernels(iou)
    kernel_us = round(sum(o_dur.values()), 1)
    print(json.dumps(dict(what='PVRCNNROIHead._assign_and_sample, 4 x 512 proposals, 18..21 gts per sample, 3 classes, num 128',
                          ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=o_n, ours_syncs=syncs(ours), ours_kernels_device_us=o_dur,
                          ours_kernels_device_us_sum=kernel_us,
                          dominant=('kernels' if kernel_us > 0.5 * o_med else 'host glue') + ' (kernels\' device time against the per-call time)',
                          iou_us_median=i_med, iou_us_min=i_min, iou_kernel_launches=i_n, iou_kernels_device_us=i_dur,
                          torch_restatement_us_median=e_med, torch_restatement_us_min=e_min, torch_restatement_kernel_launches=e_n,
                          torch_restatement_syncs=syncs(eager), ratio_of_medians=round(e_med / o_med, 2))), flush=True)


if __name__ == '__main__':
    main()
