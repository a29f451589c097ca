#!/usr/bin/env python3
"""PV-RCNN's RPN proposal stage (PartA2RPNHead.get_bboxes) on the GPU, us per call, at the shipped shapes
(configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py): B = 4 samples, a 200 x 176 map, A = 6 anchors per cell (211 200 anchors
per sample), C = 3 classes; the train proposal config (nms_pre 9000, nms_post 512, max_num 512, nms_thr 0.8) and the test one
(1024 / 100 / 100 / 0.7), score_thr 0 and rotated NMS as shipped; on two kinds of maps:
  trained : logits near -5 but for blobs round 40 objects per sample whose deltas point at the object — many duplicates for the NMS;
  random  : N(0, 1.5) logits and N(0, 0.3) deltas everywhere.
ours   = rpn_proposals (a fill, nine launches and the batched NMS, no sync), eager and replayed from a captured graph
torch  = A STAND-IN, not mmdet3d: the reference's statements (get_bboxes_single + class_agnostic_nms of the published 0.x text)
         written out in torch on the same GPU, per sample, over this package's own nms_gpu — what a user runs without the op, with
         its kernels and host syncs.  It favours torch: nms_gpu here is faster than mmdet3d's.
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; kernel launches and the kernels' own
device durations from torch.profiler (a run of its own); host syncs from torch's sync debug mode.  The streaming launch
(key_kernel) reads B A C H W and writes B H W A words; its device time is set against a device-to-device copy that moves the same
number of bytes in the same process."""
import json
import math
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402

dev = torch.device('cuda:0')
B, H, W, A, C, BATCHES = 4, 200, 176, 6, 3, 5
CONFIGS = dict(train=dict(nms_pre=9000, nms_post=512, max_num=512, nms_thr=0.8, score_thr=0.0, use_rotate_nms=True),
               test=dict(nms_pre=1024, nms_post=100, max_num=100, nms_thr=0.7, score_thr=0.0, use_rotate_nms=True))
DIR_OFFSET, DIR_LIMIT_OFFSET = 0.7854, 0.0


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


def kernels(fn, copies=False):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memset' not in e.name.lower()
          and (copies or 'memcpy' not in e.name.lower())]
    dur = {}
    for e in ev:
        name = e.name.split('(')[0][-40:]
        dur[name] = round(dur.get(name, 0.0) + (getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)), 1)
    return len(ev), dur


def syncs(fn):
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        return sum('synchroniz' in str(x.message) for x in w)
    finally:
        torch.cuda.set_sync_debug_mode('default')


def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


def standin_single(cls, bbox, dirp, anchors, cfg):
    """get_bboxes_single + class_agnostic_nms for one sample, statement by statement, on the tensors' device"""
    dir_cls = torch.max(dirp.permute(1, 2, 0).reshape(-1, 2), dim=-1)[1]
    scores = cls.permute(1, 2, 0).reshape(-1, C).sigmoid()
    bbox = bbox.permute(1, 2, 0).reshape(-1, 7)
    nms_pre = cfg['nms_pre']
    if nms_pre > 0 and scores.shape[0] > nms_pre:
        max_scores, _ = scores.max(dim=1)
        _, topk_inds = max_scores.topk(nms_pre)
        anchors, bbox, scores, dir_cls = anchors[topk_inds, :], bbox[topk_inds, :], scores[topk_inds, :], dir_cls[topk_inds]
    xa, ya, za, wa, la, ha, ra = torch.split(anchors, 1, dim=-1)
    xt, yt, zt, wt, lt, ht, rt = torch.split(bbox, 1, dim=-1)
    za = za + ha / 2
    diagonal = torch.sqrt(la ** 2 + wa ** 2)
    xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * ha + za
    lg, wg, hg = torch.exp(lt) * la, torch.exp(wt) * wa, torch.exp(ht) * ha
    zg = zg - hg / 2
    bboxes = torch.cat([xg, yg, zg, wg, lg, hg, rt + ra], dim=-1)
    for_nms = amd.xywhr2xyxyr(bboxes[:, [0, 1, 3, 4, 6]])
    max_scores, labels = torch.max(scores, dim=1)
    mask = max_scores > cfg['score_thr']
    bboxes, for_nms, max_scores, labels, scores, dir_cls = bboxes[mask], for_nms[mask], max_scores[mask], labels[mask], scores[mask], dir_cls[mask]
    keep = amd.nms_gpu(for_nms, max_scores, cfg['nms_thr'], post_max_size=cfg['nms_post'])
    bboxes, max_scores, labels, scores, dir_cls = bboxes[keep], max_scores[keep], labels[keep], scores[keep], dir_cls[keep]
    inds = max_scores.argsort(descending=True)[:cfg['max_num']]
    bboxes, max_scores, labels, scores, dir_cls = bboxes[inds], max_scores[inds], labels[inds], scores[inds], dir_cls[inds]
    dir_rot = limit_period(bboxes[..., 6] - DIR_OFFSET, DIR_LIMIT_OFFSET, math.pi)
    bboxes[..., 6] = dir_rot + DIR_OFFSET + math.pi * dir_cls.to(bboxes.dtype)
    return dict(boxes_3d=bboxes, scores_3d=max_scores, labels_3d=labels, cls_preds=scores)


def make_anchors():
    sizes = np.float32([[1.6, 3.9, 1.56], [0.6, 0.8, 1.73], [0.6, 1.76, 1.73]])
    an = np.zeros((H, W, 3, 2, 7), np.float32)
    an[..., 0] = np.linspace(0, 70.4, W, dtype=np.float32)[None, :, None, None]
    an[..., 1] = np.linspace(-40, 40, H, dtype=np.float32)[:, None, None, None]
    an[..., 2] = np.float32([-1.78, -0.6, -0.6])[None, None, :, None]
    an[..., 3:6] = sizes[None, None, :, None, :]
    an[..., 6] = np.float32([0, 1.57])[None, None, None, :]
    return an.reshape(-1, 7)


def make(kind, seed, anchors):
    rng = np.random.default_rng(seed)
    if kind == 'random':
        cls = rng.normal(0, 1.5, (B, A * C, H, W)).astype(np.float32)
        bbox = rng.normal(0, 0.3, (B, A * 7, H, W)).astype(np.float32)
    else:
        cls = (-5 + rng.normal(0, 0.7, (B, A * C, H, W))).astype(np.float32)
        bbox = rng.normal(0, 0.05, (B, A * 7, H, W)).astype(np.float32)
        an = anchors.reshape(H, W, A, 7)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        for b in range(B):
            for _ in range(40):
                cy, cx, k = rng.integers(4, H - 4), rng.integers(4, W - 4), rng.integers(0, 3)
                near = np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / 8.0).astype(np.float32)
                for rot in range(2):
                    a = k * 2 + rot
                    cls[b, a * C + k] += 8 * near
                    diag = np.sqrt(an[:, :, a, 3] ** 2 + an[:, :, a, 4] ** 2)
                    m = near > 0.05
                    bbox[b, a * 7 + 0][m] = ((an[cy, cx, a, 0] - an[:, :, a, 0]) / diag)[m]
                    bbox[b, a * 7 + 1][m] = ((an[cy, cx, a, 1] - an[:, :, a, 1]) / diag)[m]
    dirp = rng.normal(0, 1, (B, A * 2, H, W)).astype(np.float32)
    return tuple(torch.from_numpy(x).to(dev) for x in (cls, bbox, dirp))


def main():
    anchors_np = make_anchors()
    anchors = torch.from_numpy(anchors_np).to(dev)
    words = B * A * C * H * W + B * H * W * A                       # the streaming launch: read + written
    src = torch.empty(words // 2, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    _, copy_dur = kernels(lambda: dst.copy_(src), copies=True)
    copy_us = sum(copy_dur.values())
    copy_ev, _ = timed(lambda: dst.copy_(src), 50)
    for kind in ('trained', 'random'):
        cls, bbox, dirp = make(kind, 7, anchors_np)
        for cname, cfg in CONFIGS.items():
            def ours():
                return amd.rpn_proposals(cls, bbox, dirp, anchors, cfg, C, dir_offset=DIR_OFFSET, dir_limit_offset=DIR_LIMIT_OFFSET)

            def standin():
                return [standin_single(cls[b], bbox[b], dirp[b], anchors, cfg) for b in range(B)]

            o, e = ours(), standin()
            cnt = o['batch_cnt'].tolist()
            same_counts = cnt == [len(d['scores_3d']) for d in e]
            start, worst = 0, 0.0
            for b, d in enumerate(e):      # informational: the stand-in ranks rounded sigmoids with torch's tie order and libm's exp
                if same_counts and cnt[b]:
                    worst = max(worst, float((o['boxes_3d'][start:start + cnt[b]] - d['boxes_3d']).abs().max()))
                start += max(cnt[b], 0)
            o_med, o_min = timed(ours, 20)
            e_med, e_min = timed(standin, 3)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ours()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ours()
            g_med, g_min = timed(graph.replay, 20)
            o_n, o_dur = kernels(ours)
            e_n, _ = kernels(standin)
            key_us = sum(v for k, v in o_dur.items() if 'key_kernel' in k)
            print(json.dumps(dict(
                what=f'PartA2RPNHead.get_bboxes, {B} x {H} x {W} x {A} anchors, {C} classes, {kind} maps, {cname} config {cfg["nms_pre"]}/'
                     f'{cfg["nms_post"]}/{cfg["max_num"]}/{cfg["nms_thr"]}',
                rows_per_sample=cnt, standin_keeps_the_same_counts=same_counts, worst_box_difference_to_standin=worst,
                ours_us_median=o_med, ours_us_min=o_min, ours_graph_replay_us_median=g_med, ours_graph_replay_us_min=g_min,
                ours_kernel_launches=o_n, ours_syncs=syncs(ours), ours_kernels_device_us=o_dur,
                torch_standin_us_median=e_med, torch_standin_us_min=e_min, torch_standin_kernel_launches=e_n, torch_standin_syncs=syncs(standin),
                ratio_of_medians=round(e_med / o_med, 2), entry_not_slower_than_standin=bool(o_med <= e_med),
                streaming_launch_bytes=words * 4, streaming_launch_us=key_us, copy_of_the_same_bytes_kernel_us=round(copy_us, 1),
                copy_of_the_same_bytes_event_us=copy_ev, streaming_over_copy=round(key_us / max(copy_us, 1e-9), 2))), flush=True)


if __name__ == '__main__':
    main()
