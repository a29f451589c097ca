"""Plain-torch restatement of `PVRCNNROIHead._assign_and_sample` (the reference's models/roi_heads/pvrcnn_roi_head.py:225-297) by
the rules `pvrcnn_assign_and_sample` documents, and the cases of tests/test_{cpu,gpu}_pvrcnn_sample.py.

mmdet's MaxIoUAssigner and mmdet3d's IoUNegPiecewiseSampler / BboxOverlaps3D are third party and absent: nothing here is their
text.  The restatement loops over samples, classes and pieces with nonzero() and a stable argsort of the keys, and takes its IoU
matrix FROM `bbox_overlaps_3d` (the CPU twin), so the package and the restatement decide on the same bits and every output must be
EQUAL.  `exact_iou3d` is the fp64 yardstick of the IoU values themselves.

Each case is built from jittered copies of its gts — a copy lifted by a fraction f of the height has IoU (1 - f) / (1 + f), so all
three regimes of the assigner occur by construction — and the builder ASSERTS that the situation a case is named after arises.
The first sixteen cases spread their gts over 30 m: a proposal meets about one gt.  The `dense_*`, `limits`, `num1024_*`,
`b1024_tiny` and `boundary_pairs` cases reach what only the device has: rounds of the pair queue, chunks of 1024 proposals, the
sort at 4096 entries, every limit, and pairs on the edges of the two cheap overlap tests (`may_overlap_np` counts what is queued).
"""
import functools
import math

import numpy as np
import torch

import mmdet3d_gaussian_amd as amd
from nms_ref import exact_iou_xyxyr
from rbox_inputs import eval_boxes

F32 = torch.float32


def _assigner(pos, neg, low, **kw):
    return dict(type='MaxIoUAssigner', iou_calculator=dict(type='BboxOverlaps3D', coordinate='lidar'), pos_iou_thr=pos, neg_iou_thr=neg,
                min_pos_iou=low, ignore_iof_thr=-1, **kw)


def _sampler(num, pos_fraction=0.5, fractions=(0.8, 0.2), thrs=(0.55, 0.1)):
    return dict(type='IoUNegPiecewiseSampler', num=num, pos_fraction=pos_fraction, neg_piece_fractions=list(fractions),
                neg_iou_piece_thrs=list(thrs), neg_pos_ub=-1, add_gt_as_proposals=False, return_iou=True)


SHIPPED = [_assigner(0.55, 0.55, 0.55)] * 3      # configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:213-249
RPN_STYLE = [_assigner(0.6, 0.45, 0.45)] * 3      # neg_iou_thr < pos_iou_thr: the band between them is ignored


# ---------------------------------------------------------------------------------------------------------------- fp64 IoU
def exact_iou3d(a, b):
    """fp64 3D IoU of two [x, y, z, dx, dy, dz, yaw] rows (fp32 values taken as exact): Sutherland-Hodgman BEV intersection of
    tests/nms_ref.py times the height overlap."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if math.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (math.hypot(a[3], a[4]) + math.hypot(b[3], b[4])) + 1e-6:
        return 0.0
    xa = [a[0] - a[3] / 2, a[1] - a[4] / 2, a[0] + a[3] / 2, a[1] + a[4] / 2, a[6]]
    xb = [b[0] - b[3] / 2, b[1] - b[4] / 2, b[0] + b[3] / 2, b[1] + b[4] / 2, b[6]]
    iou = exact_iou_xyxyr(xa, xb)
    inter = iou * (a[3] * a[4] + b[3] * b[4]) / (1.0 + iou)
    ov = inter * max(0.0, min(a[2] + a[5], b[2] + b[5]) - max(a[2], b[2]))
    return ov / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - ov, 1e-8)


def hand_made_pairs():
    """identical boxes, touching faces, disjoint in z only, one inside the other, yaw at 0, +-pi/2 and pi: (P, 7), (P, 7), pairwise"""
    base = [1.0, 2.0, -1.0, 3.0, 1.5, 1.25, 0.3]
    a, b = [], []

    def pair(x, y):
        a.append(x)
        b.append(y)
    pair(base, base)
    pair(base, [1.0, 2.0, 0.25, 3.0, 1.5, 1.25, 0.3])                    # the faces touch in z
    pair([0.0, 0.0, 0.0, 2.0, 2.0, 1.0, 0.0], [2.0, 0.0, 0.0, 2.0, 2.0, 1.0, 0.0])   # the faces touch in x
    pair(base, [1.0, 2.0, 5.0, 3.0, 1.5, 1.25, 0.3])                     # disjoint in z only
    pair(base, [1.1, 2.05, -0.75, 1.0, 0.5, 0.5, 0.3])                   # one inside the other
    pair(base, [1.1, 2.05, -0.75, 1.0, 0.5, 0.5, 1.1])
    for yaw in (0.0, math.pi / 2, -math.pi / 2, math.pi):
        pair([0.5, 0.5, 0.0, 4.0, 2.0, 1.5, yaw], [1.0, 0.25, 0.5, 4.0, 2.0, 1.5, 0.0])
        pair([0.5, 0.5, 0.0, 4.0, 2.0, 1.5, yaw], [0.5, 0.5, 0.0, 4.0, 2.0, 1.5, yaw])
    return torch.tensor(a, dtype=F32), torch.tensor(b, dtype=F32)


@functools.lru_cache(maxsize=None)
def iou_inputs():
    """(65, 7), (33, 7) random boxes and the hand-made pairs, with the fp64 IoU of each: computed once, shared, never modified"""
    a, b = torch.from_numpy(eval_boxes(65, seed=3)), torch.from_numpy(eval_boxes(33, seed=4))
    exact = torch.tensor([[exact_iou3d(x, y) for y in b.numpy()] for x in a.numpy()], dtype=torch.float64)
    ha, hb = hand_made_pairs()
    hexact = torch.tensor([exact_iou3d(x, y) for x, y in zip(ha.numpy(), hb.numpy())], dtype=torch.float64)
    return a, b, exact, ha, hb, hexact


# ---------------------------------------------------------------------------------------------------------------- the rules
def _f(v):
    return torch.tensor(v, dtype=F32)


def assign_one(iou, plab, glab, assigners):
    """one sample: iou (N, G) fp32 -> gt_inds (N,) int64 into the FULL gt list, max_overlaps (N,) fp32"""
    N = plab.numel()
    gt_inds = torch.zeros(N, dtype=torch.int64, device=plab.device)
    max_overlaps = torch.zeros(N, dtype=F32, device=plab.device)
    iou = torch.where(iou > 0, iou, torch.zeros_like(iou))            # NaN and negative values count as no overlap
    for c, cfg in enumerate(assigners):
        pi = (plab == c).nonzero().view(-1)
        gi = (glab == c).nonzero().view(-1)
        if pi.numel() == 0 or gi.numel() == 0:
            continue
        ov = iou[pi][:, gi].t().contiguous()                          # (gts of the class, proposals of the class)
        mx = ov.max(dim=0).values
        arg = (ov == mx[None]).to(torch.uint8).argmax(dim=0)          # the lowest gt on a tie
        assigned = torch.full((pi.numel(),), -1, dtype=torch.int64, device=plab.device)
        assigned[(mx >= 0) & (mx < _f(cfg['neg_iou_thr']))] = 0
        pos = mx >= _f(cfg['pos_iou_thr'])
        assigned[pos] = arg[pos] + 1
        if cfg.get('match_low_quality', True):
            for g in range(gi.numel()):
                gmax = ov[g].max()
                if gmax >= _f(cfg['min_pos_iou']):
                    ties = (ov[g] == gmax).nonzero().view(-1)
                    if cfg.get('gt_max_assign_all', True):
                        assigned[ties] = g + 1
                    else:
                        assigned[ties[0]] = g + 1
        gt_inds[pi] = torch.where(assigned > 0, gi[(assigned - 1).clamp(min=0)] + 1, assigned)
        max_overlaps[pi] = mx
    return gt_inds, max_overlaps


def _draw(members, k, keys):
    """`members` ascending proposal indices: the k with the smallest (key, index), in that order (all of them when there are fewer)"""
    order = torch.argsort(keys[members], stable=True)
    return members[order][:k]


def sample_one(gt_inds, max_overlaps, keys, fill_keys, sampler):
    """one sample -> (positives in ascending index, negatives in output order, what happened)"""
    num = sampler['num']
    npos = int(num * sampler['pos_fraction'])
    thrs, fracs = sampler['neg_iou_piece_thrs'], sampler['neg_piece_fractions']
    P = (gt_inds > 0).nonzero().view(-1)
    pos = _draw(P, npos, keys).sort().values
    expected = num - pos.numel()
    Q = gt_inds == 0
    chosen = torch.zeros(0, dtype=torch.int64, device=gt_inds.device)
    info = dict(n_pos=P.numel(), n_neg=int(Q.sum()), n_ignored=int((gt_inds < 0).sum()), pieces=[], takes=[], carried=[], fill=0, fill_from=None)
    if Q.any():
        carry = 0
        K = len(thrs)
        for i in range(K):
            lo = _f(thrs[i + 1]) if i + 1 < K else _f(0.0)
            piece = (Q & (max_overlaps >= lo) & (max_overlaps < _f(thrs[i]))).nonzero().view(-1)
            room = expected - chosen.numel()
            want = room if i + 1 == K else int(expected * fracs[i]) + carry
            info['carried'].append(carry)
            if piece.numel() < want:
                take = piece.numel()
                carry += want - piece.numel()
            else:
                take = want
                carry = 0
            take = max(min(take, room), 0)
            chosen = torch.cat([chosen, _draw(piece, take, keys)])
            info['pieces'].append(piece.numel())
            info['takes'].append(take)
        short = expected - chosen.numel()
        source = piece if piece.numel() > 0 else chosen.clone()
        if short > 0 and source.numel() > 0:
            m = source.numel()
            j = pos.numel() + chosen.numel() + torch.arange(short, device=gt_inds.device)
            pick = (fill_keys[j] * m).floor().long().clamp(min=0, max=m - 1)
            chosen = torch.cat([chosen, source[pick]])
            info['fill'], info['fill_from'] = short, 'last' if piece.numel() > 0 else 'chosen'
    return pos, chosen, info


def restate(case, dev='cpu'):
    """the whole stage in plain torch on `dev`: the dict `pvrcnn_assign_and_sample(..., return_assignment=True)` returns, plus `info` per
    sample"""
    kw = dict(device=dev)
    sampler, assigners = case['sampler'], case['assigner']
    assigners = assigners if isinstance(assigners, list) else [assigners]
    num = sampler['num']
    npos = int(num * sampler['pos_fraction'])
    B = len(case['proposals'])
    rois, ious, inds, pb, pg, pgi, all_gi, all_mo, all_lab, infos = [], [], [], [], [], [], [], [], [], []
    pos_cnt, roi_cnt = [], []
    k0 = 0
    for b in range(B):
        prop, plab, gts, glab = (case[k][b].to(dev) for k in ('proposals', 'proposal_labels', 'gt_bboxes', 'gt_labels'))
        keys = case['keys'][k0:k0 + prop.shape[0]].to(dev)
        k0 += prop.shape[0]
        fill = case['fill_keys'][b * num:(b + 1) * num].to(dev)
        iou = amd.bbox_overlaps_3d(prop, gts)
        gi, mo = assign_one(iou, plab, glab, assigners)
        pos, neg, info = sample_one(gi, mo, keys, fill, sampler)
        sel = torch.cat([pos, neg])
        rois.append(torch.cat([torch.full((sel.numel(), 1), float(b), **kw), prop[sel]], 1))
        ious.append(mo[sel])
        inds.append(sel)
        pb.append(prop[pos])
        pg.append(gts[gi[pos] - 1])
        pgi.append(gi[pos] - 1)
        all_gi.append(gi)
        all_mo.append(mo)
        all_lab.append(torch.where(gi > 0, glab[(gi - 1).clamp(min=0)] if glab.numel() else gi, torch.full_like(gi, -1)))
        pos_cnt.append(pos.numel())
        roi_cnt.append(sel.numel())
        infos.append(info)
    R, Q = sum(roi_cnt), sum(pos_cnt)
    pad_roi = torch.zeros(B * num - R, 8, **kw)
    pad_roi[:, 0] = -1
    out = dict(rois=torch.cat(rois + [pad_roi]), ious=torch.cat(ious + [torch.zeros(B * num - R, **kw)]),
               inds=torch.cat(inds + [torch.zeros(B * num - R, dtype=torch.int64, **kw)]),
               pos_bboxes=torch.cat(pb + [torch.zeros(B * npos - Q, 7, **kw)]), pos_gt_bboxes=torch.cat(pg + [torch.zeros(B * npos - Q, 7, **kw)]),
               pos_assigned_gt_inds=torch.cat(pgi + [torch.zeros(B * npos - Q, dtype=torch.int64, **kw)]),
               pos_batch_cnt=torch.tensor(pos_cnt, dtype=torch.int32, **kw), roi_batch_cnt=torch.tensor(roi_cnt, dtype=torch.int32, **kw),
               gt_inds=torch.cat(all_gi), max_overlaps=torch.cat(all_mo), labels=torch.cat(all_lab))
    return out, infos


# ---------------------------------------------------------------------------------------------------------------- the cases
def _jitter(rng, gt, regime):
    """a proposal from a gt row: lifted by a fraction f of the height (IoU ~ (1 - f) / (1 + f)) with a little noise elsewhere"""
    p = gt.copy()
    if regime == 'far':
        p[:2] += rng.uniform(40.0, 60.0, 2)
        return p
    f = dict(tight=rng.uniform(0.0, 0.15), medium=rng.uniform(0.33, 0.7), loose=rng.uniform(0.85, 0.97))[regime]
    p[2] += f * gt[5] * (1 if rng.random() < 0.5 else -1)
    p[:2] += rng.normal(0, 0.01, 2)
    p[3:6] *= rng.uniform(0.99, 1.01, 3)
    p[6] += rng.normal(0, 0.01)
    return p


def make_sample(seed, regimes, n_gt, C=3, gt_classes=None, stray=0.0):
    """`regimes`: [(name, how many proposals)], each proposal a jittered copy of gt (i mod n_gt) with that gt's label; `stray`: the
    share of proposals and gts whose label is replaced by one outside [0, C)"""
    rng = np.random.default_rng(seed)
    gts = eval_boxes(n_gt, seed=seed + 1000, spread=30.0) if n_gt else np.zeros((0, 7), np.float32)
    glab = rng.choice(gt_classes if gt_classes is not None else np.arange(C), n_gt).astype(np.int64)
    props, plab = [], []
    i = 0
    for name, count in regimes:
        for _ in range(count):
            if n_gt:
                g = i % n_gt
                props.append(_jitter(rng, gts[g], name))
                plab.append(glab[g])
            else:
                props.append(eval_boxes(1, seed=seed * 7919 + i)[0])
                plab.append(rng.integers(0, C))
            i += 1
    props = np.asarray(props, np.float32).reshape(-1, 7)
    plab = np.asarray(plab, np.int64).reshape(-1)
    if stray:
        m = rng.random(plab.shape[0]) < stray
        plab[m] = rng.choice([-1, C, C + 5], int(m.sum()))
        m = rng.random(n_gt) < stray
        glab[m] = rng.choice([-1, C], int(m.sum()))
    order = rng.permutation(props.shape[0])
    return torch.from_numpy(props[order]), torch.from_numpy(plab[order]), torch.from_numpy(gts), torch.from_numpy(glab)


def mixed(n):
    """n proposals over all regimes"""
    a = n // 4
    return [('tight', a), ('medium', a), ('loose', a), ('far', n - 3 * a)]


# ---- cases that fill the pair queue: WL_CAP pairs per round and chunk of 1024 proposals (csrc/roi_sample.hip)
CHUNK, WL_CAP = 1024, 4096


def _where_lt(a, b):
    return np.where(a < b, a, b)                                      # rbox::fmin2, also on a NaN


def _where_gt(a, b):
    return np.where(a > b, a, b)                                      # rbox::fmax2


def _lite_np(b):
    """`lite_of` of csrc/roi_sample_common.h on (rows, 7) fp32, one operation at a time"""
    b = np.asarray(b, np.float32)
    two = np.float32(2.0)
    hw, hh = b[:, 3] / two, b[:, 4] / two
    x1, y1, x2, y2 = b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh
    return dict(cx=(x1 + x2) / two, cy=(y1 + y2) / two, ra=np.abs(x2 - x1) + np.abs(y2 - y1), z0=b[:, 2], z1=b[:, 2] + b[:, 5])


def pair_terms_np(props, gts):
    """the quantities `may_overlap` decides on, (proposals, gts) fp32 matrices: squared centre distance, the circle test's bound
    reach^2 * 1.0001 and the height overlap"""
    a, b = _lite_np(props), _lite_np(gts)
    with np.errstate(invalid='ignore', over='ignore'):
        ddx, ddy = a['cx'][:, None] - b['cx'][None], a['cy'][:, None] - b['cy'][None]
        reach = np.float32(0.5) * (a['ra'][:, None] + b['ra'][None]) + np.float32(1e-2)
        d2 = ddx * ddx + ddy * ddy
        bound = reach * reach * np.float32(1.0001)
        top, bottom = _where_lt(a['z1'][:, None], b['z1'][None]), _where_gt(a['z0'][:, None], b['z0'][None])
        ov_h = _where_gt(top - bottom, np.float32(0.0))
    assert d2.dtype == bound.dtype == ov_h.dtype == np.float32
    return d2, bound, ov_h


def may_overlap_np(props, gts):
    """numpy fp32 restatement of `lite_of` / `may_overlap` (csrc/roi_sample_common.h): (proposals, gts) bool, True where the device
    queues the pair for clipping.  Used to COUNT queued pairs, so that a builder can assert the situation; never to decide."""
    d2, bound, ov_h = pair_terms_np(props, gts)
    with np.errstate(invalid='ignore'):
        return ~(d2 > bound) & (ov_h != 0)


def queued_pairs(sample, C):
    """pairs of equal class in [0, C) the device queues, per chunk of 1024 proposals of one sample"""
    props, plab, gts, glab = (t.numpy() for t in sample)
    if props.shape[0] == 0 or gts.shape[0] == 0:
        return [0] * -(-props.shape[0] // CHUNK)
    m = may_overlap_np(props, gts) & (plab[:, None] == glab[None]) & (plab[:, None] >= 0) & (plab[:, None] < C)
    return [int(m[i:i + CHUNK].sum()) for i in range(0, props.shape[0], CHUNK)]


def make_dense(seed, n, n_gt, dup=False):
    """one class, a parked row of cars: n_gt gts with centres in a 6 m x 6 m square, every proposal a tight / medium / loose copy of
    gt (i mod n_gt), so a proposal passes the cheap tests with most gts.  `dup`: the last gt row is a copy of row 0 and the best
    proposal of gt 0 is copied onto two other proposals of gt 0: three proposals tie the maxima of BOTH rows, and rule 4 with
    gt_max_assign_all gives them to the higher index."""
    rng = np.random.default_rng(seed)
    gts = np.zeros((n_gt, 7), np.float32)
    gts[:, :2] = rng.uniform(-3.0, 3.0, (n_gt, 2))
    gts[:, 2] = rng.uniform(-1.2, -0.8, n_gt)
    gts[:, 3:6] = np.array([3.9, 1.6, 1.5]) * rng.uniform(0.9, 1.1, (n_gt, 3))
    gts[:, 6] = rng.uniform(-3.1, 3.1, n_gt)
    if dup:
        gts[-1] = gts[0]
    props = np.asarray([_jitter(rng, gts[i % n_gt], ('tight', 'medium', 'loose')[i % 3]) for i in range(n)], np.float32)
    props = torch.from_numpy(props[rng.permutation(n)])
    gts = torch.from_numpy(gts)
    if dup:
        v = amd.bbox_overlaps_3d(props, gts[:1])[:, 0]
        best = int(v.argmax())
        others = [i for i in (v > 0.2).nonzero().view(-1).tolist() if i != best]
        props[others[0]] = props[best]
        props[others[-1]] = props[best]
    return props, torch.zeros(n, dtype=torch.int64), gts, torch.zeros(n_gt, dtype=torch.int64)


def _dense_check(name, case, chunks, dup=False):
    """`chunks`: what must hold of the queued pairs per chunk"""
    def check(out, infos):
        q = queued_pairs([case[k][0] for k in ('proposals', 'proposal_labels', 'gt_bboxes', 'gt_labels')], 3)
        n_gt = case['gt_bboxes'][0].shape[0]
        FACTS[name] = dict(queued=q, to_last_gt=int((out['gt_inds'] == n_gt).sum()), n_pos=infos[0]['n_pos'])
        ok = chunks(q)
        if dup:     # the duplicate row: the three tied proposals go to the HIGHER index, nobody else does, gt 1 keeps the rest
            v = amd.bbox_overlaps_3d(case['proposals'][0], case['gt_bboxes'][0][:1])[:, 0]
            tied = v == v.max()
            ok = ok and int(tied.sum()) >= 3 and bool((out['gt_inds'][tied] == n_gt).all()) and int((out['gt_inds'] == n_gt).sum()) >= 3 \
                and bool((out['gt_inds'][~tied] != n_gt).all()) and int((out['gt_inds'] == 1).sum()) > 0
        return ok
    return check


FACTS = {}      # what the builders measured, by case: printed by the tests, quoted in DESIGN.md


def make_boundary(seed):
    """one class, 64 gts 40 m apart (a proposal meets its own gt only) and 9 proposals per gt, placed ON the edges of the two cheap
    tests of `may_overlap`:
      a  same BEV rectangle, the bottom face at fp32(z + dz) of the gt: the height overlap is exactly 0.0f -> not queued, IoU 0;
      b  the bottom face 1..8 ulp below that: a height overlap below 1e-6 and an IoU that is tiny and POSITIVE -> must be queued;
      c  the centre at a squared distance of reach^2 * 1.0001 * (1 -+ 5e-4) from the gt's: just inside (queued, clipped to 0) and
         just outside (not queued) the bounding-circle test;
      d  shifted by 0.8 of the length along the gt's long axis: a real overlap whose centre distance is beyond HALF the reach, so a
         circle test with too small a radius loses it;
    and four ordinary copies (tight, tight, medium, loose)."""
    rng = np.random.default_rng(seed)
    n_gt = 64
    gts = np.zeros((n_gt, 7), np.float32)
    gts[:, 0] = (np.arange(n_gt) % 8 - 3.5) * 40.0 + rng.uniform(-2, 2, n_gt)
    gts[:, 1] = (np.arange(n_gt) // 8 - 3.5) * 40.0 + rng.uniform(-2, 2, n_gt)
    gts[:, 2] = rng.uniform(-1.2, -0.8, n_gt)
    gts[:, 3:6] = np.array([3.9, 1.6, 1.5]) * rng.uniform(0.9, 1.1, (n_gt, 3))
    gts[:, 6] = rng.uniform(-3.1, 3.1, n_gt)
    props, kind, own = [], [], []

    def add(p, k, g):
        props.append(np.asarray(p, np.float32))
        kind.append(k)
        own.append(g)
    for g in range(n_gt):
        gt = gts[g]
        top = np.float32(gt[2] + gt[5])                                # the gt's top face as the kernel computes it
        p = gt.copy()
        p[2] = top
        add(p, 'a', g)
        p = gt.copy()
        p[2] = top
        for _ in range(int(rng.integers(1, 9))):
            p[2] = np.nextafter(p[2], np.float32(-np.inf))
        add(p, 'b', g)
        ra = np.float32(gt[3] + gt[4])
        bound = float((np.float32(0.5) * (ra + ra) + np.float32(1e-2)) ** 2 * np.float32(1.0001))
        for k, f in (('c_in', 1.0 - 5e-4), ('c_out', 1.0 + 5e-4)):
            t = rng.uniform(0, 2 * np.pi)
            d = math.sqrt(bound * f)
            p = gt.copy()
            p[0] += d * math.cos(t)
            p[1] += d * math.sin(t)
            add(p, k, g)
        p = gt.copy()                                                  # the rectangle turns clockwise by yaw (rbox::obox_make)
        p[0] += 0.8 * gt[3] * math.cos(gt[6])
        p[1] -= 0.8 * gt[3] * math.sin(gt[6])
        add(p, 'd', g)
        for regime in ('tight', 'tight', 'medium', 'loose'):
            add(_jitter(rng, gt, regime), regime, g)
    order = rng.permutation(len(props))
    props, kind, own = np.stack(props)[order], np.asarray(kind)[order], np.asarray(own)[order]
    sample = (torch.from_numpy(props), torch.zeros(len(props), dtype=torch.int64), torch.from_numpy(gts), torch.zeros(n_gt, dtype=torch.int64))

    def check(out, infos):
        d2, bound, ov_h = pair_terms_np(props, gts)
        may = may_overlap_np(props, gts)
        rows = np.arange(len(props))
        d2, bound, ov_h, mine = d2[rows, own], bound[rows, own], ov_h[rows, own], may[rows, own]
        iou = amd.bbox_overlaps_3d(sample[0], sample[2]).numpy()
        assert not may[iou > 0].size or may[iou > 0].all()             # the cheap tests exclude pairs of IoU 0 only
        assert (may.sum(1) <= 1).all()                                 # the gts are far apart: nobody meets a second one
        own_iou = iou[rows, own]
        inside = d2 <= bound
        near = np.abs(d2.astype(np.float64) / bound.astype(np.float64) - 1.0) < 1e-3
        a = (kind == 'a') & inside & (ov_h == 0) & ~mine & (own_iou == 0)
        b = (kind == 'b') & inside & (ov_h > 0) & (ov_h < 1e-6) & mine & (own_iou > 0) & (own_iou < 1e-6)
        c_in = (kind == 'c_in') & near & inside & mine & (own_iou == 0)
        c_out = (kind == 'c_out') & near & ~inside & ~mine & (own_iou == 0)
        half = (np.float32(0.25) * (_lite_np(props)['ra'] + _lite_np(gts)['ra'][own])) ** 2
        d = (kind == 'd') & (d2 > half) & mine & (own_iou > 0.05)
        FACTS['boundary_pairs'] = dict(a=int(a.sum()), b=int(b.sum()), c_in=int(c_in.sum()), c_out=int(c_out.sum()), d=int(d.sum()),
                                       queued=int(may.sum()))
        # b and d reach the outputs: a proposal whose only overlap is lost would come out with max_overlap 0
        mo = out['max_overlaps'].numpy()
        return min(a.sum(), b.sum(), c_in.sum(), c_out.sum(), d.sum()) >= 32 and (mo[b] > 0).all() and (mo[d] > 0.05).all() \
            and (mo[a | c_in | c_out] == 0).all()
    return sample, check


def make_tiny_batch(seed, B):
    """B samples of 0..5 proposals on 0..2 gts"""
    rng = np.random.default_rng(seed)
    return [make_sample(1000 + b, mixed(int(rng.integers(0, 6))), int(rng.integers(0, 3))) for b in range(B)]


LIMIT_THRS = (0.55, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.01)
LIMIT_FRACS = (0.02, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.38)      # the first piece comes up short and carries; every piece then takes


@functools.lru_cache(maxsize=None)
def clamped_call():
    """a stacked call whose counts pass the limits: sample 0 has 4100 proposals and 1030 gts, sample 1 65 on 5.  Returns the stacked
    operands with the counts [4100, 65] / [1030, 5], and the restatement of the case the kernel must make of it: rows [:4096] and
    [:1024] of sample 0, its keys cut alike.  Shared, never modified."""
    big, small = make_sample(51, mixed(4100), 1030), make_sample(52, mixed(65), 5)
    full = _case([big, small], SHIPPED, _sampler(128), 43)
    cut = dict(full, proposals=[big[0][:4096], small[0]], proposal_labels=[big[1][:4096], small[1]], gt_bboxes=[big[2][:1024], small[2]],
               gt_labels=[big[3][:1024], small[3]], keys=torch.cat([full['keys'][:4096], full['keys'][4100:]]))
    want, infos = restate(cut)
    # the surplus rows would matter if they took part: a proposal past 4096 is a tight copy of a gt, a kept proposal belongs to a gt past 1024
    surplus = amd.bbox_overlaps_3d(big[0][4096:], big[2][:1024]).max(1).values
    lost = amd.bbox_overlaps_3d(big[0][:4096], big[2][1024:]).max(1).values
    assert infos[0]['n_pos'] > 64 and infos[1]['n_pos'] > 0 and infos[1]['n_neg'] > 0 and (surplus > 0.55).any() and (lost > 0.55).any()
    return full, want


def _case(samples, assigner, sampler, seed, keys=None):
    g = torch.Generator().manual_seed(seed)
    n = sum(s[0].shape[0] for s in samples)
    return dict(proposals=[s[0] for s in samples], proposal_labels=[s[1] for s in samples], gt_bboxes=[s[2] for s in samples],
                gt_labels=[s[3] for s in samples], assigner=assigner, sampler=sampler,
                keys=torch.rand(n, generator=g) if keys is None else keys, fill_keys=torch.rand(len(samples) * sampler['num'], generator=g))


def _build(name):
    if name == 'b1_512_33':
        return _case([make_sample(1, mixed(512), 33)], SHIPPED, _sampler(128), 1), None
    if name == 'b3_middle_empty':
        return _case([make_sample(2, mixed(65), 33), make_sample(3, [], 0), make_sample(4, mixed(63), 1)], SHIPPED, _sampler(128), 2), \
            lambda out, infos: out['roi_batch_cnt'][1] == 0 and out['roi_batch_cnt'][0] > 0 and out['roi_batch_cnt'][2] > 0
    if name == 'b1_1025_65':
        return _case([make_sample(5, mixed(1025), 65)], SHIPPED, _sampler(128), 3), None
    if name == 'b4_tiny':      # 1 proposal without a gt, 64 proposals on 65 gts, no proposal on 1 gt, 1 proposal on 1 gt
        return _case([make_sample(6, [('far', 1)], 0), make_sample(7, mixed(64), 65), make_sample(8, [], 1), make_sample(9, [('tight', 1)], 1)],
                     SHIPPED, _sampler(128), 4), None
    if name == 'b3_num8':
        return _case([make_sample(10, mixed(65), 33), make_sample(11, [], 0), make_sample(12, mixed(512), 65)], SHIPPED, _sampler(8), 5), None
    if name == 'single_assigner':     # one config for one class: the dict form
        return _case([make_sample(13, mixed(64), 33, C=1)], SHIPPED[0], _sampler(8), 6), None
    if name == 'stray_labels':       # class 2 has no gt; labels outside [0, C) on both sides
        def check(out, infos):
            c = _build(name)[0]
            return (c['gt_labels'][0] == 2).sum() == 0 and (c['proposal_labels'][0] < 0).any() and (c['proposal_labels'][0] >= 3).any() \
                and (c['gt_labels'][0] < 0).any() and (c['gt_labels'][0] >= 3).any()
        s = make_sample(14, mixed(200), 33, gt_classes=[0, 1], stray=0.15)
        s[1][:7] = 2                                                  # proposals of the class without a gt
        return _case([s], SHIPPED, _sampler(128), 7), check
    if name == 'more_positives_than_npos':
        return _case([make_sample(15, [('tight', 40), ('far', 20)], 5)], SHIPPED, _sampler(8), 8), \
            lambda out, infos: infos[0]['n_pos'] > 4 and out['pos_batch_cnt'][0] == 4
    if name == 'no_negatives':
        return _case([make_sample(16, [('tight', 6)], 3)], SHIPPED, _sampler(8), 9), \
            lambda out, infos: infos[0]['n_neg'] == 0 and out['roi_batch_cnt'][0] == 4
    if name == 'hard_piece_empty':
        return _case([make_sample(17, [('tight', 10), ('far', 300)], 5)], SHIPPED, _sampler(128), 10), \
            lambda out, infos: infos[0]['pieces'][0] == 0 and infos[0]['carried'][1] > 0 and infos[0]['takes'][1] > 0 and infos[0]['fill'] == 0
    if name == 'last_piece_short':
        return _case([make_sample(18, [('tight', 6), ('medium', 12), ('far', 5)], 4)], SHIPPED, _sampler(128), 11), \
            lambda out, infos: infos[0]['fill'] > 0 and infos[0]['fill_from'] == 'last' and infos[0]['takes'][0] > 0
    if name == 'last_piece_empty':
        return _case([make_sample(19, [('tight', 6), ('medium', 12)], 4)], [_assigner(0.6, 0.6, 0.6)] * 3, _sampler(128, thrs=(0.6, 0.1)), 12), \
            lambda out, infos: infos[0]['pieces'][1] == 0 and infos[0]['takes'][0] > 0 and infos[0]['fill_from'] == 'chosen'
    if name == 'rpn_style_ignored':
        return _case([make_sample(20, mixed(256), 33)], RPN_STYLE, _sampler(128), 13), \
            lambda out, infos: infos[0]['n_ignored'] > 0 and (out['gt_inds'][out['inds'][:int(out['roi_batch_cnt'][0])]] >= 0).all()
    if name in ('low_quality_all', 'low_quality_first'):
        # gt 0 meets only medium proposals, two of them identical and its best: below pos_iou_thr, above min_pos_iou
        props, plab, gts, glab = make_sample(21, [('medium', 40), ('far', 20)], 4)
        own = ((plab == glab[0]) & (amd.bbox_overlaps_3d(props, gts[:1])[:, 0] > 0)).nonzero().view(-1)
        best = own[amd.bbox_overlaps_3d(props[own], gts[:1])[:, 0].argmax()]
        twin = own[own != best][-1]
        props[twin] = props[best]
        assigner = [_assigner(0.8, 0.2, 0.25, gt_max_assign_all=name == 'low_quality_all')] * 3

        def check(out, infos):
            v = amd.bbox_overlaps_3d(props, gts[:1])[:, 0]
            both = out['gt_inds'][best] == 1 and out['gt_inds'][twin] == 1
            lone = out['gt_inds'][min(best, twin)] == 1 and out['gt_inds'][max(best, twin)] == -1
            return 0.25 <= v.max() < 0.8 and v[best] == v.max() == v[twin] and (both if name == 'low_quality_all' else lone)
        return _case([(props, plab, gts, glab)], assigner, _sampler(128), 14), check
    if name == 'equal_keys':       # every draw is decided by the index
        s = make_sample(22, [('tight', 40), ('medium', 60), ('loose', 60), ('far', 40)], 7)
        return _case([s], SHIPPED, _sampler(8), 15, keys=torch.full((200,), 0.5)), \
            lambda out, infos: infos[0]['n_pos'] > 4 and infos[0]['pieces'][0] > infos[0]['takes'][0] > 0
    if name in ('dense_two_rounds', 'dense_three_rounds', 'dense_2049', 'dense_4096'):
        n, n_gt, dup, seed = dict(dense_two_rounds=(1024, 8, True, 31), dense_three_rounds=(1024, 12, False, 32), dense_2049=(2049, 6, True, 31),
                                  dense_4096=(4096, 3, False, 31))[name]
        case = _case([make_dense(seed, n, n_gt, dup=dup)], SHIPPED, _sampler(128), 40)
        if name == 'dense_two_rounds':
            return case, _dense_check(name, case, lambda q: len(q) == 1 and WL_CAP < q[0] <= 2 * WL_CAP, dup=True)
        if name == 'dense_three_rounds':
            return case, _dense_check(name, case, lambda q: len(q) == 1 and q[0] > 2 * WL_CAP)
        if name == 'dense_2049':      # two full chunks of two rounds each, and ONE proposal in the third
            return case, _dense_check(name, case, lambda q: len(q) == 3 and q[0] > WL_CAP and q[1] > WL_CAP and 0 < q[2] <= 6, dup=True)
        full = _dense_check(name, case, lambda q: len(q) == 4 and min(q) > CHUNK)      # four full chunks, the sort at 4096 entries
        return case, lambda out, infos: full(out, infos) and infos[0]['n_pos'] > 64 and out['pos_batch_cnt'][0] == 64
    if name == 'limits':      # MAX_PROPS, MAX_GTS, MAX_CLASSES, MAX_NUM and MAX_PIECES at once
        case = _case([make_sample(50, mixed(4096), 1024, C=16)], [_assigner(0.55, 0.55, 0.55)] * 16,
                     _sampler(1024, fractions=LIMIT_FRACS, thrs=LIMIT_THRS), 42)

        def check(out, infos):
            i = infos[0]
            FACTS[name] = dict(n_pos=i['n_pos'], pieces=i['pieces'], takes=i['takes'], carried=i['carried'], fill=i['fill'],
                               to_gt_1024=int((out['gt_inds'] == 1024).sum()), queued=queued_pairs([case[k][0] for k in (
                                   'proposals', 'proposal_labels', 'gt_bboxes', 'gt_labels')], 16))
            return i['n_pos'] >= 512 and out['pos_batch_cnt'][0] == 512 and min(i['pieces']) > 0 and min(i['takes']) > 0 \
                and max(i['carried']) > 0 and (out['gt_inds'] == 1024).any() and len(set(case['gt_labels'][0].tolist())) == 16
        return case, check
    if name == 'num1024_fill_last':
        def check(out, infos):
            FACTS[name] = dict(fill=infos[0]['fill'], fill_from=infos[0]['fill_from'])
            return infos[0]['fill'] > 900 and infos[0]['fill_from'] == 'last' and out['roi_batch_cnt'][0] == 1024
        return _case([make_sample(23, [('tight', 40), ('far', 30)], 5)], SHIPPED, _sampler(1024), 16), check
    if name == 'num1024_fill_chosen':
        def check(out, infos):
            FACTS[name] = dict(fill=infos[0]['fill'], fill_from=infos[0]['fill_from'])
            return infos[0]['fill'] > 900 and infos[0]['fill_from'] == 'chosen' and infos[0]['pieces'][1] == 0 and out['roi_batch_cnt'][0] == 1024
        return _case([make_sample(19, [('tight', 6), ('medium', 12)], 4)], [_assigner(0.6, 0.6, 0.6)] * 3, _sampler(1024, thrs=(0.6, 0.1)), 17), check
    if name == 'b1024_tiny':      # MAX_SAMPLES
        def check(out, infos):
            FACTS[name] = dict(no_roi=int((out['roi_batch_cnt'] == 0).sum()), with_fill=sum(i['fill'] > 0 for i in infos),
                               rows=int(out['roi_batch_cnt'].sum()))
            return FACTS[name]['no_roi'] >= 100 and FACTS[name]['with_fill'] >= 100 and out['roi_batch_cnt'].numel() == 1024
        return _case(make_tiny_batch(5, 1024), SHIPPED, _sampler(8), 18), check
    if name == 'boundary_pairs':
        sample, check = make_boundary(24)
        return _case([sample], SHIPPED, _sampler(128), 19), check
    raise KeyError(name)


CASES = ('b1_512_33', 'b3_middle_empty', 'b1_1025_65', 'b4_tiny', 'b3_num8', 'single_assigner', 'stray_labels', 'more_positives_than_npos',
         'no_negatives', 'hard_piece_empty', 'last_piece_short', 'last_piece_empty', 'rpn_style_ignored', 'low_quality_all',
         'low_quality_first', 'equal_keys', 'dense_two_rounds', 'dense_three_rounds', 'dense_2049', 'dense_4096', 'limits', 'num1024_fill_last',
         'num1024_fill_chosen', 'b1024_tiny', 'boundary_pairs')
NEW_CASES = CASES[16:]
SANITIZED = ('b3_middle_empty', 'last_piece_short', 'low_quality_all', 'dense_two_rounds', 'limits')     # the driver of tests/hostmath/roi_sample_sanitize.cpp runs these


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, expected outputs, per-sample info): computed once per case, shared by every test, never modified"""
    case, check = _build(name)
    out, infos = restate(case)
    assert check is None or bool(check(out, infos)), f'case {name!r} does not produce the situation it is named after: {infos}'
    return case, out, infos
