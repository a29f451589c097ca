#!/usr/bin/env python3
"""The SimOTA BEV assigner (sim_ota_3d_assigner.py:34-211) on the GPU, us per call, at the shape tools/pib_time.py names: 468 x 468 =
219 024 shared BEV priors, 64 gts per sample, 3 classes, 4 samples; in two regimes:
  trained : a prior's prediction is the nearest gt's box, jittered, its score high on that gt's class — many pairs overlap;
  random  : random boxes at the priors and random scores — costs clamped to match_init, few overlaps per gt.
ours   = simota_assign, shared-prior stacked form with device counts (a fill and three launches, no sync)
torch  = the reference's statements written out in torch on the same GPU, per sample, over this package's own points_in_boxes_all
         and bbox_overlaps_3d (a stand-in that favours torch: the reference's CUDA ops are not faster): what a user runs without the
         op, with its kernels and host syncs.  Its gt_inds equal ours wherever torch's topk breaks no tie differently (reported).
Per side: device events around back-to-back calls, the median of 5 batches after a warm-up; kernel launches and the kernels' own
device durations from torch.profiler; host syncs from torch's sync debug mode.  The select kernel's time is set against the number
of (candidate, gt) pairs that pass the cheap overlap test, i.e. the full clips it ran (the test restated in torch)."""
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mmdet3d_gaussian_amd as amd  # noqa: E402

dev = torch.device('cuda:0')
SIDE, G, C, B, BATCHES = 468, 64, 3, 4, 5
PRM = dict(center_radius=0.5, candidate_topk=10, iou_weight=3.0, cls_weight=1.0, match_init=2.0)


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


def kernels(fn):
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
            dur[e.name[:48]] = round(dur.get(e.name[:48], 0.0) + (getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)), 1)
        return len(ev), dur
    except Exception as e:      # noqa: BLE001
        return f'profiler unavailable: {e}', {}


def syncs(fn):
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        return sum('synchroniz' in str(x.message) for x in w)
    finally:
        torch.cuda.set_sync_debug_mode('default')


def statements(scores, boxes, priors, gts, labels):
    """sim_ota_3d_assigner.py:60-211 for one sample, statement by statement, on the tensors' device"""
    INF, EPS = 100000000, 0.00000001
    num_gt, num_bboxes = gts.size(0), boxes.size(0)
    assigned = priors.new_full((num_bboxes,), 0, dtype=torch.long)
    xyz = torch.cat([priors[:, :2], priors.new_zeros(priors.size(0), 1)], dim=-1)
    gt_bev = gts.clone()
    gt_bev[..., 2] = -INF
    gt_bev[..., 5] = 2 * INF
    in_gts = amd.points_in_boxes_all(xyz.unsqueeze(0), gt_bev.unsqueeze(0))[0] > 0
    in_cts = (priors[:, :2].unsqueeze(1) - gts[..., :2].unsqueeze(0)).abs().max(-1).values < PRM['center_radius']
    valid = in_gts.any(dim=1) | in_cts.any(dim=1)
    both = in_gts[valid, :] & in_cts[valid, :]
    vbox, vscore = boxes[valid], scores[valid]
    nv = vbox.size(0)
    ious = amd.bbox_overlaps_3d(vbox, gts)
    iou_cost = -torch.log(ious + EPS)
    onehot = F.one_hot(labels.to(torch.int64), scores.shape[-1]).float().unsqueeze(0).repeat(nv, 1, 1)
    vscore = vscore.unsqueeze(1).repeat(1, num_gt, 1)
    cls_cost = F.binary_cross_entropy(vscore.sqrt_(), onehot, reduction='none').sum(-1)
    cost = cls_cost * PRM['cls_weight'] + iou_cost * PRM['iou_weight']
    cost[both] = cost[both].clamp(max=PRM['match_init'])
    matching = torch.zeros_like(cost)
    topk = min(PRM['candidate_topk'], ious.shape[0])
    topk_ious, _ = torch.topk(ious, topk, dim=0)
    ks = torch.clamp(topk_ious.sum(0).int(), min=1)
    for g in range(num_gt):
        _, pos_idx = torch.topk(cost[:, g], k=ks[g].item(), largest=False)
        matching[:, g][pos_idx] = 1.0
    multi = matching.sum(1) > 1
    if multi.sum() > 0:
        _, argmin = torch.min(cost[multi, :], dim=1)
        matching[multi, :] *= 0.0
        matching[multi, argmin] = 1.0
    fg = matching.sum(1) > 0.0
    valid[valid.clone()] = fg
    matched = matching[fg, :].argmax(1)
    assigned[valid] = matched + 1
    return assigned


def make(regime, seed):
    rng = np.random.default_rng(seed)
    lin = np.linspace(-37.44, 37.44, SIDE, dtype=np.float32)
    ys, xs = np.meshgrid(lin, lin, indexing='ij')
    priors = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(SIDE * SIDE, 0.16, np.float32)], 1)
    P = SIDE * SIDE
    sc, bx, gt, lb = [], [], [], []
    for _ in range(B):
        g = np.zeros((G, 7), np.float32)
        g[:, 0:2] = rng.uniform(-35, 35, (G, 2))
        g[:, 2] = rng.uniform(-1.5, -0.5, G)
        g[:, 3], g[:, 4], g[:, 5] = rng.uniform(3.2, 4.8, G), rng.uniform(1.5, 2.1, G), rng.uniform(1.4, 1.8, G)
        g[:, 6] = rng.uniform(-3.1, 3.1, G)
        l = rng.integers(0, C, G)
        if regime == 'trained':
            near = torch.cdist(torch.from_numpy(priors[:, :2]), torch.from_numpy(g[:, :2])).argmin(1).numpy()
            b = (g[near] + rng.normal(0, 0.1, (P, 7))).astype(np.float32)
            s = rng.uniform(0.01, 0.15, (P, C)).astype(np.float32)
            s[np.arange(P), l[near]] = rng.uniform(0.6, 0.98, P)
        else:
            b = np.concatenate([priors[:, :2] + rng.normal(0, 0.5, (P, 2)), rng.uniform(-1.5, -0.5, (P, 1)), rng.uniform(1, 5, (P, 3)),
                                rng.uniform(-3.1, 3.1, (P, 1))], 1).astype(np.float32)
            s = rng.uniform(0, 1, (P, C)).astype(np.float32)
        sc.append(s), bx.append(b), gt.append(g), lb.append(l.astype(np.int64))
    to = lambda xs_: [torch.from_numpy(x).to(dev) for x in xs_]   # noqa: E731
    return to(sc), to(bx), torch.from_numpy(priors).to(dev), to(gt), to(lb)


def full_clips(boxes, gts, valid):
    """pairs (candidate, gt) that pass roi_sample::may_overlap, restated in torch"""
    def lite(b):
        hw, hh = b[:, 3] / 2, b[:, 4] / 2
        x1, y1, x2, y2 = b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh
        return (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1).abs() + (y2 - y1).abs(), b[:, 2], b[:, 2] + b[:, 5]
    a, g = lite(boxes[valid]), lite(gts)
    dd = (a[0][:, None] - g[0][None]) ** 2 + (a[1][:, None] - g[1][None]) ** 2
    reach = 0.5 * (a[2][:, None] + g[2][None]) + 1e-2
    h = (torch.minimum(a[4][:, None], g[4][None]) - torch.maximum(a[3][:, None], g[3][None])).clamp(min=0)
    return int((~(dd > reach * reach * 1.0001) & (h != 0)).sum())


def main():
    pcnt = torch.full((B,), SIDE * SIDE, dtype=torch.int32, device=dev)
    gcnt = torch.full((B,), G, dtype=torch.int32, device=dev)
    for regime in ('trained', 'random'):
        sc, bx, priors, gt, lb = make(regime, 5)
        S, X, T, L = torch.cat(sc), torch.cat(bx), torch.cat(gt), torch.cat(lb)

        def ours():
            return amd.simota_assign(S, X, priors, T, L, prior_batch_cnt=pcnt, gt_batch_cnt=gcnt, shared_priors=True, **PRM)

        def eager():
            return [statements(sc[b], bx[b], priors, gt[b], lb[b]) for b in range(B)]

        o, e = ours(), torch.cat(eager())
        differ = int((o['gt_inds'] != e).sum())
        cands = clips = 0
        for b in range(B):
            xyz = torch.cat([priors[:, :2], priors.new_zeros(priors.size(0), 1)], dim=-1)
            tall = gt[b].clone()
            tall[:, 2], tall[:, 5] = -1e8, 2e8
            v = (amd.points_in_boxes_all(xyz.unsqueeze(0), tall.unsqueeze(0))[0] > 0).any(1) | \
                ((priors[:, None, :2] - gt[b][None, :, :2]).abs().max(-1).values < PRM['center_radius']).any(1)
            cands += int(v.sum())
            clips += full_clips(bx[b], gt[b], v)
        o_med, o_min = timed(ours, 20)
        e_med, e_min = timed(eager, 2)
        o_n, o_dur = kernels(ours)
        e_n, _ = kernels(eager)
        sel = sum(v for k, v in o_dur.items() if 'select_kernel' in k)
        print(json.dumps(dict(what=f'SimOTABEVAssigner.assign, {B} x {SIDE * SIDE} shared priors, {G} gts per sample, {C} classes, {regime} predictions',
                              candidates=cands, positives=int(o['pos_cnt'].sum()), rows_where_torch_topk_broke_a_tie_differently=differ,
                              ours_us_median=o_med, ours_us_min=o_min, ours_kernel_launches=o_n, ours_syncs=syncs(ours), ours_kernels_device_us=o_dur,
                              select_kernel_us=sel, full_clips=clips, select_ns_per_full_clip=round(sel * 1e3 / max(clips, 1), 2),
                              torch_statements_us_median=e_med, torch_statements_us_min=e_min, torch_statements_kernel_launches=e_n,
                              torch_statements_syncs=syncs(eager), ratio_of_medians=round(e_med / o_med, 2))), flush=True)


if __name__ == '__main__':
    main()
